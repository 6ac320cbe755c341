"""A/B of the launcher's two regimes at BASELINE config 2's shape (16 f x 512^2, 30 DDIM steps of which 18 guided, synthetic
weights): `--lanes 3 --batch 1` - the best a script reached before `--batch` - against `--lanes 2 --batch 5`, the packed
regime bench.py times.  Both through `python -m motionclone_amd.launch ... tools/standin_video_sample.py`, i.e. the script
call sequence (set_all_seed, build the pipeline, per line obtain_motion_representation + sample_video), hipGraph replay.

  python tools/launch_batch_ab.py [--videos 40 --legs 2] [--out profiles/launch_batch_ab]

Every leg is ONE child process (a launcher job over an examples file of --videos lines), started under its own
`timeout -k 10 <seconds>`, one at a time, alternating A B A B; the tool stops at the first non-zero exit status.  Per leg two
rates are recorded: the launcher's own videos/min over the whole job (model construction and the warm-up turns included), and
the steady-state rate - the lines that completed after EVERY script thread had finished its first line (all graphs captured,
all lanes concurrent) over the time from that moment to the last completion, from the stand-in's per-line host timestamps
(taken after the result's copy to the host, which synchronises).  Reserved device memory is the process's at the end of the
job.  A difference is worth quoting only where it exceeds the spread of the repeated legs; both series are written down."""
import argparse
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGIMES = (("A", 3, 1), ("B", 2, 5))


def leg(work, name, lanes, batch, limit):
    out = os.path.join(work, name)
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, "-m", "motionclone_amd.launch", "--lanes", str(lanes), "--batch",
           str(batch), os.path.join(ROOT, "tools", "standin_video_sample.py"), "--examples", os.path.join(work, "examples.jsonl"),
           "--motion-representation-save-dir", os.path.join(out, "mr"), "--generated-videos-save-dir", os.path.join(out, "out")]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT))
    head = [ln for ln in r.stdout.splitlines() if ln.startswith('{"examples"')]
    if r.returncode != 0 or not head:
        print(r.stdout[-4000:])
        raise SystemExit("launch_batch_ab: leg %s failed (exit status %d); nothing written" % (name, r.returncode))
    recs = []
    for path in glob.glob(os.path.join(out, "out", "graphs_*.json")):
        with open(path) as f:
            recs.append(json.load(f))
    firsts = [min(rec["done_at"].values()) for rec in recs if rec["done_at"]]
    every = sorted(t for rec in recs for t in rec["done_at"].values())
    t0 = max(firsts)                                  # the last thread's first line: every warm-up turn is over
    steady = [t for t in every if t > t0]
    res = dict(job=json.loads(head[-1]), steady_videos=len(steady),
               steady_videos_per_min=60.0 * len(steady) / (every[-1] - t0) if steady else None,
               reserved_gib=max(rec["reserved_gib"] for rec in recs), max_reserved_gib=max(rec["max_reserved_gib"] for rec in recs))
    shutil.rmtree(out)                                # the latents and representations of a leg are not kept
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=40, help="lines of the examples file of every leg")
    ap.add_argument("--legs", type=int, default=2, help="A B pairs")
    ap.add_argument("--limit", type=int, default=420, help="seconds one leg may take (timeout -k 10)")
    ap.add_argument("--commit", default=None, help="what to record as the measured commit (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "launch_batch_ab"))
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("launch_batch_ab: no GPU; a rate is measured on the MI355X or not at all")
    device = torch.cuda.get_device_name(0)      # (queried without creating a context that outlives the legs' memory readings)
    commit = args.commit
    if commit is None:
        g = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True)
        commit = g.stdout.strip() if g.returncode == 0 and g.stdout.strip() else "unknown (not a git checkout)"
    work = tempfile.mkdtemp(prefix="launch_batch_ab_")
    series = {name: [] for name, _, _ in REGIMES}
    try:
        with open(os.path.join(work, "examples.jsonl"), "w") as f:
            for i in range(args.videos):        # three reference videos, a prompt and a seed per line
                f.write(json.dumps(dict(video_path="camera_%d.mp4" % (i % 3), new_prompt="prompt number %d" % i, seed=2025 + i)) + "\n")
        for n in range(args.legs):
            for name, lanes, batch in REGIMES:
                res = leg(work, "%s%d" % (name, n), lanes, batch, args.limit)
                series[name].append(res)
                print("leg %s%d: %s" % (name, n, json.dumps(res)), flush=True)
    finally:
        shutil.rmtree(work, ignore_errors=True)
    out = dict(device=device, commit=commit, videos_per_leg=args.videos, legs=series)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out + ".json", "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)

    def mean(xs):
        return sum(xs) / len(xs)
    md = ["# Launcher: `--lanes 3 --batch 1` vs `--lanes 2 --batch 5` (config 2 shape)", "",
          "%s, commit %s.  16 frames x 512^2, 30 DDIM steps (18 guided), synthetic weights, hipGraph replay, %d lines per job through "
          "`python -m motionclone_amd.launch ... tools/standin_video_sample.py` (the scripts' call sequence; no VAE / CLIP); one job "
          "per leg, legs alternated A B A B (`tools/launch_batch_ab.py`)." % (device, commit, args.videos), "",
          "| regime | steady-state videos/min (legs) | mean | whole job videos/min, load and warm-up included (legs) | reserved HBM at the end (GiB) |",
          "|---|---|---|---|---|"]
    means = {}
    for name, lanes, batch in REGIMES:
        legs = series[name]
        st = [x["steady_videos_per_min"] for x in legs]
        means[name] = mean(st)
        md.append("| %s: `--lanes %d --batch %d` (%d script threads) | %s | %.2f | %s | %s |" % (
            name, lanes, batch, lanes * batch, ", ".join("%.2f" % x for x in st), means[name],
            ", ".join("%.2f" % x["job"]["videos_per_min"] for x in legs), ", ".join("%.1f" % x["reserved_gib"] for x in legs)))
    spread = max(max(x["steady_videos_per_min"] for x in series[n]) - min(x["steady_videos_per_min"] for x in series[n]) for n in series)
    md += ["", "Steady state = the lines completed after every script thread had finished its first line (A: %s, B: %s of %d), over the "
           "time from then to the last completion.  B against A: %+.2f %% steady-state videos/min; largest spread between the repeated "
           "legs of one regime: %.2f videos/min." % (", ".join(str(x["steady_videos"]) for x in series["A"]),
                                                      ", ".join(str(x["steady_videos"]) for x in series["B"]), args.videos,
                                                      100.0 * (means["B"] / means["A"] - 1.0), spread), ""]
    with open(args.out + ".md", "w") as f:
        f.write("\n".join(md))
    print("\n".join(md))


if __name__ == "__main__":
    main()
