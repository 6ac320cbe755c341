"""What a long video costs: ONE 64-frame video run as sliding context windows (L = 16, overlap 4: five windows per step, one
packed forward + the window gather + the windowed update) against FIVE independent 16-frame videos packed V = 5 into one launch
sequence - the same forward work per step, at BASELINE config 2's resolution and schedule (512^2, 30 DDIM steps of which 18
guided, synthetic weights as bench.py uses them).  The expectation is equal time plus two small launches per step.

  python tools/context_windows_bench.py [--legs 2 --rounds 1] [--out profiles/context_windows]

Both regimes live in ONE process (same engine, same weights, hipGraph replay, a sampler each) and are timed alternately
A B A B around a device synchronise.  The driver starts the measurement as ONE child process under `timeout -k 10 <seconds>` and
stops at the first failure; the child (`--worker`) prints one JSON line, the driver writes <out>.json / <out>.md.  Where no GPU
run happened (`--not-measured`, or no device) the .md says NOT MEASURED and carries no number."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def worker(args):
    import torch
    from motionclone_amd import lib, ops, spec
    from motionclone_amd.engine import UNet3DEngine, default_config
    from motionclone_amd.sampler import MotionCloneSampler
    lib.load()
    dev = torch.device("cuda", 0)
    cfg = default_config()
    sd, _ = spec.synthetic_state_dict(cfg, seed=1234, device=dev)
    eng = UNet3DEngine(sd, cfg, dev)
    F, L, ov, h = args.frames, args.length, args.overlap, args.size // 8
    nW = len(ops.context_windows(F, L, ov))
    ctx = dict(length=L, overlap=ov)

    def sampler():
        return MotionCloneSampler(eng, cfg_scale=7.5, motion_guidance_weight=2000.0, warm_up_steps=10, cool_up_steps=10,
                                  num_inference_steps=args.ddim_steps, guidance_steps=args.guided_steps, guidance_scale=0.4).enable_graphs()

    def tensors(V, frames, seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        lat = torch.randn((V, 4, frames, h, h), generator=g, device=dev, dtype=torch.float16)
        vid = (0.18215 * torch.randn((V, 4, frames, h, h), generator=g, device=dev)).half()
        noise = torch.randn((V, 4, frames, h, h), generator=g, device=dev, dtype=torch.float16)
        return lat, vid, noise
    text = torch.randn((2, 77, 768), generator=torch.Generator(device=dev).manual_seed(7), device=dev).half()
    sa, sb = sampler(), sampler()
    lat_a, vid_a, noise_a = tensors(nW, L, 100)          # A: nW independent L-frame videos, packed
    text_a = torch.cat([text[0:1].expand(nW, -1, -1), text[1:2].expand(nW, -1, -1)], 0).contiguous()
    lat_b, vid_b, noise_b = tensors(1, F, 200)           # B: one F-frame video as nW windows

    def run_a():
        reps = sa.extract(vid_a, noise_a, text[0:1], add_noise_step=400)
        return sa.sample(lat_a, text_a, reps)

    def run_b():
        reps = sb.extract(vid_b, noise_b, text[0:1], add_noise_step=400, context=ctx)
        return sb.sample(lat_b, text, reps, context=ctx)
    count = {}
    orig = lib.call

    def counting(name, *a):
        count[name] = count.get(name, 0) + 1
        return orig(name, *a)
    launches = {}
    for name, smp, fn in (("A", sa, run_a), ("B", sb, run_b)):       # one eager pass each: the launches of one run, counted
        graphs, smp._graphs = smp._graphs, None
        count.clear()
        lib.call = counting
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            lib.call = orig
            smp._graphs = graphs
        launches[name] = sum(count.values())
        if name == "B":
            launches["B_window_launches"] = count.get("mc_latent_windows_f16", 0) + count.get("mc_cfg_ddim_step_windows_f16", 0)
    for fn in (run_a, run_b):                                        # captures every graph: never timed
        out = fn()
        torch.cuda.synchronize()
        assert torch.isfinite(out.float()).all()
    legs = {"A": [], "B": []}
    for _ in range(args.legs):
        for name, fn in (("A", run_a), ("B", run_b)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.rounds):
                fn()
            torch.cuda.synchronize()
            legs[name].append((time.perf_counter() - t0) / args.rounds)
    res = dict(shape=dict(frames=F, length=L, overlap=ov, windows=nW, size=args.size, ddim_steps=args.ddim_steps,
                          guided_steps=args.guided_steps, device=torch.cuda.get_device_name(0)),
               launches=launches)
    for name in ("A", "B"):
        s = legs[name]
        res[name] = dict(seconds_legs=[round(x, 3) for x in s], seconds=round(sum(s) / len(s), 3), spread=round(max(s) - min(s), 3))
    res["extra_percent"] = round(100.0 * (res["B"]["seconds"] / res["A"]["seconds"] - 1.0), 2)
    res["exceeds_spread_of_A"] = bool(abs(res["B"]["seconds"] - res["A"]["seconds"]) > res["A"]["spread"])
    print("CONTEXT_WINDOWS " + json.dumps(res), flush=True)


HEAD = "# One long video as context windows vs the same windows as independent packed videos"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--length", type=int, default=16)
    ap.add_argument("--overlap", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ddim-steps", type=int, default=30)
    ap.add_argument("--guided-steps", type=int, default=18)
    ap.add_argument("--legs", type=int, default=2, help="A B pairs")
    ap.add_argument("--rounds", type=int, default=1, help="runs per leg")
    ap.add_argument("--limit", type=int, default=540, help="seconds the measurement may take (timeout -k 10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "context_windows"))
    ap.add_argument("--not-measured", action="store_true", help="write the .md without a GPU run")
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    setup = ("%d frames as windows of %d with overlap %d at %d^2, %d DDIM steps (%d guided), synthetic weights, hipGraph replay; A = "
             "the windows' count of independent %d-frame videos packed into one launch sequence, B = the long video; one process, "
             "legs alternated A B A B (`tools/context_windows_bench.py`)." % (args.frames, args.length, args.overlap, args.size,
                                                                             args.ddim_steps, args.guided_steps, args.length))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    if args.not_measured:
        with open(args.out + ".md", "w") as f:
            f.write("\n".join([HEAD, "", setup, "", "NOT MEASURED: no GPU run of this tool has happened yet.  The expectation - the same "
                               "forward work per step plus two small launches (the window gather and the windowed update) - is an "
                               "expectation, not a result.", ""]))
        return
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker"]
    for k in ("frames", "length", "overlap", "size", "ddim_steps", "guided_steps", "legs", "rounds"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("CONTEXT_WINDOWS ")]
    if r.returncode != 0 or not line:
        print(r.stdout[-4000:])
        raise SystemExit("context_windows_bench: the measurement failed (exit status %d); nothing written" % r.returncode)
    res = json.loads(line[-1][len("CONTEXT_WINDOWS "):])
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    s, la = res["shape"], res["launches"]
    md = [HEAD, "", s["device"] + ": " + setup, "",
          "| regime | seconds per run (legs) | mean | launches per run (eager pass) |", "|---|---|---|---|",
          "| A: %d packed videos of %d frames | %s | %.3f | %d |" % (s["windows"], s["length"], ", ".join("%.3f" % x for x in res["A"]["seconds_legs"]),
                                                                     res["A"]["seconds"], la["A"]),
          "| B: one video of %d frames, %d windows | %s | %.3f | %d (%d of them the gather / windowed update) |" % (
              s["frames"], s["windows"], ", ".join("%.3f" % x for x in res["B"]["seconds_legs"]), res["B"]["seconds"], la["B"],
              la["B_window_launches"]),
          "", "The long video against the packed videos: %+.2f %% time per run; spread of the repeated A legs %.3f s - the difference %s "
          "it." % (res["extra_percent"], res["A"]["spread"], "exceeds" if res["exceeds_spread_of_A"] else "does NOT exceed"), ""]
    with open(args.out + ".md", "w") as f:
        f.write("\n".join(md))
    print("\n".join(md))


if __name__ == "__main__":
    main()
