#!/bin/bash
# The standing validation on one MI355X: the -m gpu suite, the benchmark with --full, and (optionally) the rocprofv3 kernel
# trace of a short bench run.  Everything lands under $OUT (default results/; copied into profiles/ by hand).
#   bash tools/gpu_validate.sh [tag] [pytest|bench|prof ...]
cd "${GRAFT_REPO_ROOT:-.}" || exit 1
export TMPDIR=/tmp
OUT=${OUT:-results}
TAG=${1:-r05}; shift
WHAT=${*:-pytest bench}
mkdir -p $OUT
for w in $WHAT; do
  case $w in
    pytest)
      timeout 1500 python -m pytest tests -m gpu -q -p no:cacheprovider --durations=15 > $OUT/${TAG}_pytest_gpu.log 2>&1
      echo "pytest rc=$?"; tail -n 25 $OUT/${TAG}_pytest_gpu.log ;;
    bench)
      timeout 900 python bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/${TAG}_bench_stdout.log 2> $OUT/${TAG}_bench_stderr.log
      echo "bench rc=$?"; grep '^{' $OUT/${TAG}_bench_stdout.log | tail -n 1 | tee $OUT/${TAG}_bench_line.json | cut -c1-1500
      cp profiles/bench_detail.json $OUT/${TAG}_bench_detail.json 2>/dev/null ;;
    benchshort)
      timeout 600 python bench.py --steps 6 --warmup 3 --full --no-cpu-baseline --no-vae > $OUT/${TAG}_benchshort_stdout.log 2> $OUT/${TAG}_benchshort_stderr.log
      echo "benchshort rc=$?"; grep '^{' $OUT/${TAG}_benchshort_stdout.log | tail -n 1 | tee $OUT/${TAG}_benchshort_line.json | cut -c1-1200
      cp profiles/bench_detail.json $OUT/${TAG}_benchshort_detail.json 2>/dev/null ;;
    prof)
      ( cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats -d "$OLDPWD/$OUT/${TAG}_prof" -o trace -- \
          python "$OLDPWD/bench.py" --full --no-cpu-baseline --no-vae --steps 3 --no-detail > "$OLDPWD/$OUT/${TAG}_prof_bench.log" 2>&1 )
      echo "prof rc=$?"; find $OUT/${TAG}_prof -name '*kernel_stats.csv' | head -n 2
      # keep only the stats tables (the raw trace is hundreds of MB)
      find $OUT/${TAG}_prof -type f ! -name '*stats*.csv' -delete 2>/dev/null ;;
  esac
done
