"""Cost of the region-weighted guidance kernels (motion mask) next to the unweighted entry points, at config 2's up_blocks.1
shape in the packed regime (V = 5 videos: B*HW = 5 x 256 rows, heads 8, F 16, d 160) on cuda:0 -> profiles/masked_tattn.md.

    python tools/masked_tattn_bench.py                      weighted (B) against unweighted (A) entries of this build
    python tools/masked_tattn_bench.py --parent-lib LIB     this build's unweighted entries (B) against those of LIB (A),
                                                            a libmotionclone_hip.so built from the parent commit

Method of topk_tattn_bench.py (warm-up, many launches between two HIP events) in ABAB order: every round times arm A, then
arm B, so drift of the shared machine hits both arms alike.  Per case the medians over the rounds and the A-to-A spread
((max - min) / median of arm A's rounds) are reported: a difference inside that spread is not a difference.  The measurement
runs in a child process under a time limit of its own; without a GPU the record says NOT MEASURED."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "masked_tattn.md")
V, HW, HEADS, F, D = 5, 256, 8, 16, 160
ENTRIES = ("mc_tattn_loss_f16", "mc_tattn_loss_topk_f16", "mc_tattn_bwd_f16", "mc_tattn_bwd_topk_f16")


def worker(parent_lib, rounds, iters):
    import torch
    from motionclone_amd import lib, ops
    dev = torch.device("cuda:0")
    this = lib.load()
    other = None
    if parent_lib:
        other = ctypes.CDLL(parent_lib)
        for name in ENTRIES:
            fn = getattr(other, name)
            fn.argtypes, fn.restype = lib.SIGNATURES[name], ctypes.c_int

    def timeit(fn, warm=20):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / iters

    C = HEADS * D
    gen = torch.Generator(device=dev).manual_seed(1)
    qkv = (torch.randn(V * F * HW, 3 * C, device=dev, generator=gen) * 0.5).half()
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    do = torch.randn(V * F * HW, C, device=dev, generator=gen).half()
    g = torch.empty_like(qkv)
    ul = torch.empty(V * HW * HEADS, device=dev)
    loss = torch.empty(1, device=dev)
    roww = torch.rand(V * HW, F, device=dev, generator=gen) * 2.0
    sc, st = float(D ** -0.5), ops._stream(q)

    def check(rc):
        if rc != 0:
            raise RuntimeError("kernel entry failed: rc = %d" % rc)

    for K in (1, 4):
        idx = torch.topk(torch.rand(V * HW, HEADS, F, F, device=dev, generator=gen), K, -1).indices.to(torch.uint8).contiguous()
        val = torch.rand(V * HW, HEADS, F, K, device=dev, generator=gen) * 0.5
        plain = "mc_tattn_%s_f16" if K == 1 else "mc_tattn_%s_topk_f16"
        kk = () if K == 1 else (K,)

        def loss_call(h, name, extra):
            return lambda: check(getattr(h, name)(q.data_ptr(), k.data_ptr(), q.stride(0), idx.data_ptr(), val.data_ptr(), *extra,
                                                  ul.data_ptr(), loss.data_ptr(), V, F, HW, HEADS, D, sc, st))

        def bwd_call(h, name, extra, dout):
            return lambda: check(getattr(h, name)(q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0),
                                                  None if dout is None else dout.data_ptr(), 0 if dout is None else dout.stride(0),
                                                  g[:, :C].data_ptr(), g[:, C:2 * C].data_ptr(), g[:, 2 * C:].data_ptr(), g.stride(0),
                                                  idx.data_ptr(), val.data_ptr(), *extra, 1.0, V, F, HW, HEADS, D, sc, st))
        wk = (K, roww.data_ptr())
        if other is None:     # A: unweighted, B: weighted, both of this build
            cases = [("loss", loss_call(this, plain % "loss", kk), loss_call(this, "mc_tattn_loss_weighted_f16", wk)),
                     ("bwd", bwd_call(this, plain % "bwd", kk, do), bwd_call(this, "mc_tattn_bwd_weighted_f16", wk, do)),
                     ("bwd_seed_only", bwd_call(this, plain % "bwd", kk, None), bwd_call(this, "mc_tattn_bwd_weighted_f16", wk, None))]
        else:                 # A: the parent build's unweighted entries, B: this build's
            cases = [("loss", loss_call(other, plain % "loss", kk), loss_call(this, plain % "loss", kk)),
                     ("bwd", bwd_call(other, plain % "bwd", kk, do), bwd_call(this, plain % "bwd", kk, do)),
                     ("bwd_seed_only", bwd_call(other, plain % "bwd", kk, None), bwd_call(this, plain % "bwd", kk, None))]
        for what, fa, fb in cases:
            a, b = [], []
            for _ in range(rounds):     # A B A B ...
                a.append(timeit(fa))
                b.append(timeit(fb))
            ma, mb = statistics.median(a), statistics.median(b)
            print(json.dumps(dict(case=what, K=K, a_us=round(ma, 2), b_us=round(mb, 2), b_over_a=round(mb / ma, 4),
                                  a_spread=round((max(a) - min(a)) / ma, 4), b_spread=round((max(b) - min(b)) / mb, 4),
                                  rounds=rounds, iters=iters)), flush=True)


def table(rows, a_name, b_name):
    out = ["| case | K | %s us | %s us | B / A | A-to-A spread | verdict |" % (a_name, b_name), "|---|---|---|---|---|---|---|"]
    for r in rows:
        d = r["b_over_a"] - 1.0
        verdict = "inside the spread" if abs(d) <= r["a_spread"] else ("B slower" if d > 0 else "B faster")
        out.append("| %s | %d | %.2f | %.2f | %.4f | %.2f %% | %s |" % (r["case"], r["K"], r["a_us"], r["b_us"], r["b_over_a"],
                                                                        100 * r["a_spread"], verdict))
    return out


def run_child(args, parent_lib):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--rounds", str(args.rounds), "--iters", str(args.iters)]
    if parent_lib:
        cmd += ["--parent-lib", parent_lib]
    try:
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        return None, "the measurement did not finish within %d s" % args.timeout
    if r.returncode != 0:
        return None, "the measurement failed (exit %d): %s" % (r.returncode, r.stderr.strip().splitlines()[-1:] or "")
    return [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")], None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args.parent_lib, args.rounds, args.iters)
    import torch
    doc = ["# Region-weighted guidance kernels (motion mask): cost", "",
           "`tools/masked_tattn_bench.py`, config 2's `up_blocks.1` shape in the packed regime (B*HW = %d x %d, heads %d, F %d, d %d);"
           % (V, HW, HEADS, F, D),
           "ABAB rounds of warm-up + launches between two HIP events; medians over the rounds; the A-to-A spread is (max - min) / median",
           "of arm A's rounds.  A difference inside the spread is not a difference.", ""]
    doc += ["## Weighted (B) against unweighted (A) entries of this build", ""]
    if not torch.cuda.is_available():
        doc += ["NOT MEASURED: no GPU in this run.", ""]
        doc += ["## Unweighted entries of this build (B) against the parent commit's library (A)", "", "NOT MEASURED: no GPU in this run.", ""]
    else:
        rows, err = run_child(args, None)
        doc += (table(rows, "unweighted", "weighted") if rows else ["NOT MEASURED: %s" % err]) + [""]
        doc += ["## Unweighted entries of this build (B) against the parent commit's library (A)", ""]
        if not args.parent_lib:
            doc += ["NOT MEASURED: no parent library given (--parent-lib).", ""]
        elif not os.path.exists(args.parent_lib):
            doc += ["NOT MEASURED: %s does not exist." % os.path.relpath(args.parent_lib, ROOT), ""]
        else:
            rows, err = run_child(args, os.path.abspath(args.parent_lib))
            doc += (table(rows, "parent", "this build") if rows else ["NOT MEASURED: %s" % err]) + [""]
            doc += ["The unweighted instantiations are the parent's code (the weight is a template flag, no pointer test), so B / A",
                    "is expected at 1 within the spread.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(doc))
    print("\n".join(doc))


if __name__ == "__main__":
    main()
