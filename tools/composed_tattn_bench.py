"""Cost of the slot-weighted guidance kernels (motion composition: several references per video) at the shape of config 2's
hooked modules (up_blocks.1: 256 positions, heads 8, F 16, d 160), one video and the packed regime (V = 5), on cuda:0
-> profiles/composed_tattn.md.

    python tools/composed_tattn_bench.py                     slot-weighted (B) against row-weighted (A) entries of this build, K = 2, 4, 8
    python tools/composed_tattn_bench.py --parent-lib LIB    also this build's unweighted and row-weighted entries (B) against
                                                             those of LIB (A), a libmotionclone_hip.so built from the parent commit

Method of masked_tattn_bench.py (warm-up, many launches between two HIP events) in ABAB order inside one process: every round
times arm A, then arm B, so drift of the shared machine hits both arms alike.  Per case the medians over the rounds and the
A-to-A spread ((max - min) / median of arm A's rounds) are reported: a difference inside that spread is not a difference, and
the spread of the same run is the margin of the parent comparison.  The measurement runs in a child process under a time limit
of its own; without a GPU the record says NOT MEASURED.  The register / scratch figures of the new instantiations come from
the compiler's kernel-resource-usage remarks (no GPU needed).  No videos/min is claimed for composed runs."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "composed_tattn.md")
HW, HEADS, F, D = 256, 8, 16, 160
VS = (1, 5)
ENTRIES = ("mc_tattn_loss_f16", "mc_tattn_loss_topk_f16", "mc_tattn_bwd_f16", "mc_tattn_bwd_topk_f16",
           "mc_tattn_loss_weighted_f16", "mc_tattn_bwd_weighted_f16")


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

    def check(rc):
        if rc != 0:
            raise RuntimeError("kernel entry failed: rc = %d" % rc)

    C = HEADS * D
    sc = float(D ** -0.5)
    for V in VS:
        gen = torch.Generator(device=dev).manual_seed(1)
        qkv = (torch.randn(V * F * HW, 3 * C, device=dev, generator=gen) * 0.5).half()
        q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
        do = torch.randn(V * F * HW, C, device=dev, generator=gen).half()
        g = torch.empty_like(qkv)
        ul = torch.empty(V * HW * HEADS, device=dev)
        loss = torch.empty(1, device=dev)
        roww = torch.rand(V * HW, F, device=dev, generator=gen) * 2.0
        st = ops._stream(q)
        for K in ((1, 4) if other is not None else (2, 4, 8)):
            idx = torch.topk(torch.rand(V * HW, HEADS, F, F, device=dev, generator=gen), K, -1).indices.to(torch.uint8).contiguous()
            val = torch.rand(V * HW, HEADS, F, K, device=dev, generator=gen) * 0.5
            slotw = (roww / K).unsqueeze(-1).expand(-1, -1, K).contiguous()      # one reference: the row-weighted loss itself
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
            wk, sk = (K, roww.data_ptr()), (K, slotw.data_ptr())
            if other is None:     # A: row-weighted, B: slot-weighted, both of this build
                cases = [("loss", loss_call(this, "mc_tattn_loss_weighted_f16", wk), loss_call(this, "mc_tattn_loss_slotw_f16", sk)),
                         ("bwd", bwd_call(this, "mc_tattn_bwd_weighted_f16", wk, do), bwd_call(this, "mc_tattn_bwd_slotw_f16", sk, do)),
                         ("bwd_seed_only", bwd_call(this, "mc_tattn_bwd_weighted_f16", wk, None),
                          bwd_call(this, "mc_tattn_bwd_slotw_f16", sk, None))]
            else:                 # A: the parent build's entries, B: this build's
                cases = []
                for tag, lname, bname, extra in (("unweighted", plain % "loss", plain % "bwd", kk),
                                                 ("row-weighted", "mc_tattn_loss_weighted_f16", "mc_tattn_bwd_weighted_f16", wk)):
                    cases += [(tag + " loss", loss_call(other, lname, extra), loss_call(this, lname, extra)),
                              (tag + " bwd", bwd_call(other, bname, extra, do), bwd_call(this, bname, extra, do)),
                              (tag + " bwd_seed_only", bwd_call(other, bname, extra, None), bwd_call(this, bname, extra, None))]
            for what, fa, fb in cases:
                a, b = [], []
                for _ in range(rounds):     # A B A B ...
                    a.append(timeit(fa))
                    b.append(timeit(fb))
                ma, mb = statistics.median(a), statistics.median(b)
                print(json.dumps(dict(case=what, V=V, K=K, a_us=round(ma, 2), b_us=round(mb, 2), b_over_a=round(mb / ma, 4),
                                      a_spread=round((max(a) - min(a)) / ma, 4), b_spread=round((max(b) - min(b)) / mb, 4),
                                      rounds=rounds, iters=iters)), flush=True)


def resources():
    """VGPR / AGPR / scratch / occupancy of the slot-weighted instantiations (KM = 8, W = 2) from hipcc's remarks"""
    import re
    import tempfile
    from motionclone_amd import build
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    if not os.path.exists(hipcc):
        return ["NOT RECORDED: no hipcc in this run.", ""]
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([hipcc] + build.HIP_FLAGS + ["-Rpass-analysis=kernel-resource-usage", "-c",
                                                        os.path.join(build.CSRC, "temporal.hip"), "-o", os.path.join(tmp, "t.o")],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        return ["NOT RECORDED: the compile with remarks failed.", ""]
    kern, cur = {}, None
    for line in r.stdout.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = kern.setdefault(m.group(1), {})
        for key, tag in (("VGPRs", "v"), ("AGPRs", "a"), ("ScratchSize [bytes/lane]", "s"), ("Occupancy [waves/SIMD]", "o")):
            m = re.search(r" " + re.escape(key) + r": (\d+)", line)
            if m and cur is not None:
                cur[tag] = int(m.group(1))
    rows = []
    for name, f in sorted(kern.items()):
        m = re.match(r"_ZN2mc16tattn_(fwd|bwd)_kernelILi(\d+)ELi(\d+)E(?:Li0EL[bi]([01])E)?Li8ELi2EE", name)
        if m:
            rows.append((m.group(1), int(m.group(2)), int(m.group(3)), int(m.group(4) or 0), f))
    if not rows:
        return ["NOT RECORDED: no slot-weighted instantiation in the remarks.", ""]
    out = ["%d kernels in the file, %d of them slot-weighted (KM = 8, W = 2); scratch is %d bytes / lane at most over these."
           % (len(kern), len(rows), max(f["s"] for *_, f in rows)), "",
           "| kernel | F tiles | d tiles | 16-byte loads | VGPRs | AGPRs | scratch B/lane | waves/SIMD |", "|---|---|---|---|---|---|---|---|"]
    for kind, nt, dt, vec, f in rows:
        out.append("| %s | %d | %d | %s | %d | %d | %d | %d |" % (kind, nt, dt, "yes" if vec else "no", f["v"], f["a"], f["s"], f["o"]))
    return out + [""]


def table(rows, a_name, b_name):
    out = ["| case | V | K | %s us | %s us | B / A | A-to-A spread | verdict |" % (a_name, b_name), "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        d = r["b_over_a"] - 1.0
        verdict = "inside the spread" if abs(d) <= r["a_spread"] else ("B slower" if d > 0 else "B faster")
        out.append("| %s | %d | %d | %.2f | %.2f | %.4f | %.2f %% | %s |" % (r["case"], r["V"], r["K"], r["a_us"], r["b_us"], r["b_over_a"],
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
    ap.add_argument("--timeout", type=int, default=300)
    ap.add_argument("--out", default=OUT)
    ap.add_argument("--worker", action="store_true")
    args = ap.parse_args()
    if args.worker:
        return worker(args.parent_lib, args.rounds, args.iters)
    import torch
    doc = ["# Slot-weighted guidance kernels (motion composition): cost", "",
           "`tools/composed_tattn_bench.py`, the shape of config 2's hooked modules (`up_blocks.1`: B*HW = V x %d, heads %d, F %d, d %d),"
           % (HW, HEADS, F, D),
           "V = 1 and the packed regime V = 5; ABAB rounds of warm-up + launches between two HIP events in one process; medians over",
           "the rounds; the A-to-A spread is (max - min) / median of arm A's rounds.  A difference inside the spread is not a",
           "difference.  No videos/min is claimed for composed runs: only these kernels were timed.", ""]
    doc += ["## Slot-weighted (B) against row-weighted (A) entries of this build, same K", "",
            "One reference with slot_w = row_w / K, so both arms compute the same loss and seeds.", ""]
    parent_title = "## Unweighted and row-weighted entries of this build (B) against the parent commit's library (A)"
    if not torch.cuda.is_available():
        doc += ["NOT MEASURED: no GPU in this run.", "", parent_title, "", "NOT MEASURED: no GPU in this run.", ""]
    else:
        rows, err = run_child(args, None)
        doc += (table(rows, "row-weighted", "slot-weighted") if rows else ["NOT MEASURED: %s" % err]) + [""]
        doc += [parent_title, ""]
        if not args.parent_lib:
            doc += ["NOT MEASURED: no parent library given (--parent-lib).", ""]
        elif not os.path.exists(args.parent_lib):
            doc += ["NOT MEASURED: %s does not exist." % os.path.relpath(args.parent_lib, ROOT), ""]
        else:
            rows, err = run_child(args, os.path.abspath(args.parent_lib))
            doc += (table(rows, "parent", "this build") if rows else ["NOT MEASURED: %s" % err]) + [""]
            if rows:
                worst = [r for r in rows if r["b_over_a"] - 1.0 > r["a_spread"]]
                doc += ["The margin is the A-to-A spread of the same run.  %s" % (
                    "Every case is inside it or faster." if not worst else
                    "SLOWER THAN THE PARENT BEYOND THE SPREAD: %s." % ", ".join("%s V=%d K=%d" % (r["case"], r["V"], r["K"]) for r in worst)), ""]
    doc += ["## Registers and scratch of the new instantiations", "",
            "`-Rpass-analysis=kernel-resource-usage` on `csrc/temporal.hip` with the library's flags:", ""] + resources()
    doc += ["## What was and was not run on hardware", ""]
    if torch.cuda.is_available():
        doc += ["Run on %s: the kernel timings above (the parent comparison only where a table is shown)." % torch.cuda.get_device_name(0),
                "Not run for speed: a composed video end to end - no videos/min is claimed for composed runs.  Correctness on",
                "hardware is the gpu-marked half of `tests/test_composed_kernels.py` / `tests/test_composed_engine.py`.", ""]
    else:
        doc += ["Nothing: this record was written without a GPU.", ""]
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(doc))
    print("\n".join(doc))


if __name__ == "__main__":
    main()
