"""A/B at BASELINE config 4's shape (i2v_rgb + SparseCtrl, 16 f x 512^2, 30 DDIM steps of which 12 guided, synthetic weights
as bench.py uses them): three lanes of ONE video each - all the packed path could do for image-to-video before SparseCtrl
batches - against L lanes of V videos per launch sequence, every video with its own condition image.  Both regimes live in
ONE process (same engine, same weights, hipGraph replay, their own samplers and GEMM lane hint) and are timed alternately
A B A B; reported per regime: videos/min of every leg, reserved HBM, kernel launches per video (counted on an eager pass).

  python tools/i2v_packed_ab.py [--lanes 2 --batch 3 --legs 2 --rounds 2] [--out profiles/i2v_packed_ab]

The driver starts the measurement as ONE child process under `timeout -k 10 <seconds>` (a GPU step never outlives its
limit) and stops at the first failure; the child (`--worker`) prints one JSON line, the driver writes <out>.json / <out>.md.
A gain is worth quoting only where it exceeds the spread of the repeated A legs; both numbers are written down either way."""
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
    from motionclone_amd import lib, spec
    from motionclone_amd.engine import ControlNetEngine, UNet3DEngine, default_config
    from motionclone_amd.sampler import MotionCloneSampler, sample_interleaved
    lib.load()
    dev = torch.device("cuda", 0)
    cfg = default_config()
    sd, _ = spec.synthetic_state_dict(cfg, seed=1234, device=dev)
    eng = UNet3DEngine(sd, cfg, dev)
    ceng = ControlNetEngine(spec.synthetic_controlnet_state_dict(cfg, seed=4321, device=dev), cfg, dev)
    F, h = args.frames, args.size // 8

    def video(seed):
        g = torch.Generator(device=dev).manual_seed(seed)
        lat = torch.randn((1, 4, F, h, h), generator=g, device=dev, dtype=torch.float16)
        text = torch.randn((2, 77, 768), generator=g, device=dev).half()
        vid = (0.18215 * torch.randn((1, 4, F, h, h), generator=g, device=dev)).half()
        noise = torch.randn((1, 4, F, h, h), generator=g, device=dev, dtype=torch.float16)
        cond, mask = torch.zeros_like(vid), torch.zeros_like(vid[:, :1])
        cond[:, :, 0] = 0.18215 * torch.randn((1, 4, h, h), generator=g, device=dev).half()   # its own condition image
        mask[:, :, 0] = 1
        return (lat, text, vid, noise), dict(cond=cond, mask=mask, scale=1.0)

    def sampler(lanes, graphs=True):
        s = MotionCloneSampler(eng, cfg_scale=7.5, motion_guidance_weight=2000.0, warm_up_steps=10, cool_up_steps=10,
                               num_inference_steps=args.ddim_steps, guidance_steps=args.guided_steps, guidance_scale=0.4,
                               controlnet=ceng)
        s.gemm_lanes = lanes          # the tile / split-K choice assumes this many launch sequences in flight
        return s.enable_graphs() if graphs else s

    def regime(lanes, batch, seed0):
        vids = [video(seed0 + k) for k in range(lanes * batch)]
        if batch == 1:
            jobs, ctrls = [v[0] for v in vids], [v[1] for v in vids]
        else:
            jobs = [[v[0] for v in vids[k * batch:(k + 1) * batch]] for k in range(lanes)]
            ctrls = [[v[1] for v in vids[k * batch:(k + 1) * batch]] for k in range(lanes)]
        smps = [sampler(lanes) for _ in range(lanes)]
        streams = [torch.cuda.Stream(device=dev) for _ in range(lanes)]

        def run(rounds):
            for _ in range(rounds):
                sample_interleaved(smps, jobs, streams, add_noise_step=400, ctrl=ctrls)
            torch.cuda.synchronize()
        # launches per video: one job on a sampler without graphs, every C-ABI call counted
        count = [0]
        orig = lib.call

        def counting(name, *a):
            count[0] += 1
            return orig(name, *a)
        lib.call = counting
        try:
            sample_interleaved([sampler(lanes, graphs=False)], jobs[:1], None, add_noise_step=400, ctrl=ctrls[:1])
            torch.cuda.synchronize()
        finally:
            lib.call = orig
        torch.cuda.empty_cache()
        before = torch.cuda.memory_reserved(dev)
        run(1)                        # captures every lane's graphs, fills its pool: never timed
        torch.cuda.empty_cache()
        return dict(lanes=lanes, batch=batch, run=run, videos_per_round=lanes * batch, launches_per_video=count[0] / batch,
                    reserved_gib=(torch.cuda.memory_reserved(dev) - before) / 2 ** 30, legs=[])

    A = regime(3, 1, 100)
    B = regime(args.lanes, args.batch, 200)
    for _ in range(args.legs):
        for r, rounds in ((A, args.rounds * max(1, B["videos_per_round"] // 3)), (B, args.rounds)):
            t0 = time.perf_counter()
            r["run"](rounds)
            dt = time.perf_counter() - t0
            r["legs"].append(60.0 * rounds * r["videos_per_round"] / dt)
    out = {}
    for name, r in (("A", A), ("B", B)):
        legs = r["legs"]
        out[name] = dict(regime="%d lanes x %d video%s" % (r["lanes"], r["batch"], "" if r["batch"] == 1 else "s"),
                         videos_per_min_legs=[round(x, 2) for x in legs], videos_per_min=round(sum(legs) / len(legs), 2),
                         spread=round(max(legs) - min(legs), 2), reserved_gib=round(r["reserved_gib"], 1),
                         launches_per_video=round(r["launches_per_video"]))
    out["gain_percent"] = round(100.0 * (out["B"]["videos_per_min"] / out["A"]["videos_per_min"] - 1.0), 2)
    out["gain_exceeds_spread_of_A"] = bool(abs(out["B"]["videos_per_min"] - out["A"]["videos_per_min"]) > out["A"]["spread"])
    out["shape"] = dict(frames=F, size=args.size, ddim_steps=args.ddim_steps, guided_steps=args.guided_steps,
                        device=torch.cuda.get_device_name(0), total_reserved_gib=round(torch.cuda.memory_reserved(dev) / 2 ** 30, 1))
    print("I2V_PACKED_AB " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--batch", type=int, default=3)
    ap.add_argument("--legs", type=int, default=2, help="A B pairs")
    ap.add_argument("--rounds", type=int, default=2, help="rounds of the packed regime per leg (A runs as many videos)")
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--ddim-steps", type=int, default=30)
    ap.add_argument("--guided-steps", type=int, default=12)
    ap.add_argument("--limit", type=int, default=840, help="seconds the measurement may take (timeout -k 10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "i2v_packed_ab"))
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--worker"]
    for k in ("lanes", "batch", "legs", "rounds", "frames", "size", "ddim_steps", "guided_steps"):
        cmd += ["--" + k.replace("_", "-"), str(getattr(args, k))]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("I2V_PACKED_AB ")]
    if r.returncode != 0 or not line:
        print(r.stdout[-4000:])
        raise SystemExit("i2v_packed_ab: the measurement failed (exit status %d); nothing written" % r.returncode)
    res = json.loads(line[-1][len("I2V_PACKED_AB "):])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out + ".json", "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    a, b, s = res["A"], res["B"], res["shape"]
    md = ["# Image-to-video (config 4 shape): three lanes of one video vs packed lanes", "",
          "%s, %d frames x %d^2, %d DDIM steps (%d guided), SparseCtrl encoder every step, synthetic weights, hipGraph replay; "
          "one process, legs alternated A B A B (`tools/i2v_packed_ab.py`)." % (s["device"], s["frames"], s["size"], s["ddim_steps"],
                                                                                  s["guided_steps"]), "",
          "| regime | videos/min (legs) | mean | reserved HBM (GiB, this regime's graphs and buffers) | launches per video |",
          "|---|---|---|---|---|"]
    for r_ in (a, b):
        md.append("| %s | %s | %.2f | %.1f | %d |" % (r_["regime"], ", ".join("%.2f" % x for x in r_["videos_per_min_legs"]),
                                                       r_["videos_per_min"], r_["reserved_gib"], r_["launches_per_video"]))
    md += ["", "Packed against three lanes of one: %+.2f %% videos/min; spread of the repeated A legs %.2f videos/min - the "
           "difference %s it." % (res["gain_percent"], a["spread"], "exceeds" if res["gain_exceeds_spread_of_A"] else "does NOT exceed"), ""]
    with open(args.out + ".md", "w") as f:
        f.write("\n".join(md))
    print("\n".join(md))


if __name__ == "__main__":
    main()
