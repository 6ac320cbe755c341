"""Cost of the video-wide GroupNorm entries (mc_groupnorm_fwd_span_f16 / mc_groupnorm_bwd_span_f16, span = F) next to the
per-frame entries on the same tensors, at the four resolution levels of config 2 (16 frames, 64 x 64 latents: 4096 / 1024 /
256 / 64 tokens per frame at 320 / 640 / 1280 / 1280 channels) for one and for five packed videos, on cuda:0
-> profiles/groupnorm_video_wide.md.

    python tools/gn_span_bench.py [--out FILE]

Both variants read and write the same bytes; the video-wide form adds one finalize launch per norm (32 x videos workgroups).
Method of tools/masked_tattn_bench.py: warm-up, many launches between two HIP events, ABAB rounds in ONE process (A = per
frame, B = video-wide), medians over the rounds and the A-to-A spread ((max - min) / median of arm A's rounds): a difference
inside that spread is not a difference.  The measurement runs in a child process under a time limit of its own; without a
GPU the record says NOT MEASURED."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "groupnorm_video_wide.md")
F = 16
LEVELS = ((4096, 320), (1024, 640), (256, 1280), (64, 1280))     # (tokens per frame, channels)
VIDEOS = (1, 5)


def worker(rounds, iters):
    import torch
    from motionclone_amd import lib, ops
    dev = torch.device("cuda:0")
    h = lib.load()

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

    def check(rc):
        if rc != 0:
            raise RuntimeError("kernel entry failed: rc = %d" % rc)

    gen = torch.Generator(device=dev).manual_seed(1)
    for V in VIDEOS:
        for hw, C in LEVELS:
            frames = V * F
            x = torch.randn(frames * hw, C, device=dev, generator=gen).half()
            dz = torch.randn(frames * hw, C, device=dev, generator=gen).half()
            out = torch.empty_like(x)
            gamma = torch.ones(C, device=dev)
            beta = torch.zeros(C, device=dev)
            partial = ops.workspace("groupnorm", x, frames, hw)
            st_a = torch.empty(frames, 32, 2, device=dev)
            st_b = torch.empty(V, 32, 2, device=dev)
            bs_a = ops.workspace("groupnorm_bwd_stats", x, frames)
            bs_b = ops.workspace("groupnorm_bwd_stats_span", x, frames, F)
            s = ops._stream(x)
            p = lambda t: t.data_ptr()     # noqa: E731

            def fwd_a():
                check(h.mc_groupnorm_fwd_f16(p(x), None, C, 0, C, C, frames, hw, 1e-5, p(partial), p(st_a), p(gamma), p(beta), p(out), C, 1, s))

            def fwd_b():
                check(h.mc_groupnorm_fwd_span_f16(p(x), None, C, 0, C, C, frames, hw, F, 1e-5, p(partial), p(st_b), p(gamma), p(beta),
                                                  p(out), C, 1, s))

            def bwd_a():
                check(h.mc_groupnorm_bwd_f16(p(x), None, C, 0, C, C, frames, hw, p(dz), C, p(st_a), p(gamma), p(beta), 1, p(partial),
                                             p(bs_a), p(out), C, 0, s))

            def bwd_b():
                check(h.mc_groupnorm_bwd_span_f16(p(x), None, C, 0, C, C, frames, hw, F, p(dz), C, p(st_b), p(gamma), p(beta), 1,
                                                  p(partial), p(bs_b), p(out), C, 0, s))
            for what, fa, fb in (("fwd", fwd_a, fwd_b), ("bwd", bwd_a, bwd_b)):
                a, b = [], []
                for _ in range(rounds):     # A B A B ...
                    a.append(timeit(fa))
                    b.append(timeit(fb))
                ma, mb = statistics.median(a), statistics.median(b)
                print(json.dumps(dict(case=what, videos=V, hw=hw, C=C, a_us=round(ma, 2), b_us=round(mb, 2), b_over_a=round(mb / ma, 4),
                                      a_spread=round((max(a) - min(a)) / ma, 4), rounds=rounds, iters=iters)), flush=True)
            del x, dz, out
            torch.cuda.empty_cache()


def table(rows):
    out = ["| pass | videos | tokens / frame | C | per frame us | video-wide us | B / A | B - A us | A-to-A spread | verdict |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        d = r["b_over_a"] - 1.0
        verdict = "inside the spread" if abs(d) <= r["a_spread"] else ("video-wide slower" if d > 0 else "video-wide faster")
        out.append("| %s | %d | %d | %d | %.2f | %.2f | %.4f | %+.2f | %.2f %% | %s |" % (
            r["case"], r["videos"], r["hw"], r["C"], r["a_us"], r["b_us"], r["b_over_a"], r["b_us"] - r["a_us"], 100 * r["a_spread"], verdict))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args.rounds, args.iters)
    import torch
    doc = ["# Video-wide GroupNorm (AnimateDiff v1 layout): cost next to the per-frame entries", "",
           "`tools/gn_span_bench.py`: config 2's four levels (%d frames; tokens per frame x channels %s), one and five packed videos;"
           % (F, ", ".join("%d x %d" % l for l in LEVELS)),
           "A = `mc_groupnorm_fwd_f16` / `mc_groupnorm_bwd_f16`, B = `mc_groupnorm_fwd_span_f16` / `mc_groupnorm_bwd_span_f16` with span = %d," % F,
           "GroupNorm + SiLU, single source.  ABAB rounds of warm-up + launches between two HIP events in one process; medians over",
           "the rounds; the A-to-A spread is (max - min) / median of arm A's rounds.  A difference inside the spread is not a difference.",
           "Both arms move the same bytes; B adds one finalize launch per norm.", ""]
    if not torch.cuda.is_available():
        doc += ["NOT MEASURED: no GPU in this run.", ""]
    else:
        cmd = [sys.executable, os.path.abspath(__file__), "--worker", "--rounds", str(args.rounds), "--iters", str(args.iters)]
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.timeout, cwd=ROOT)
            if r.returncode != 0:
                doc += ["NOT MEASURED: the measurement failed (exit %d): %s" % (r.returncode, r.stderr.strip().splitlines()[-1:] or ""), ""]
            else:
                doc += table([json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]) + [""]
        except subprocess.TimeoutExpired:
            doc += ["NOT MEASURED: the measurement did not finish within %d s." % args.timeout, ""]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(doc))
    print("\n".join(doc))


if __name__ == "__main__":
    main()
