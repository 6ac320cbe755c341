"""Cost of the top-k guidance kernels next to the k = 1 entry points on the same build, at config 2's up_blocks.1 shape in
the packed regime (V = 5 videos: B*HW = 5 x 256 rows, heads 8, F 16, d 160) on cuda:0 -> JSON lines.  Method of
tattn_bench.py: warm-up, many launches between two HIP events.  K = 1 goes through the *_topk entries directly (ops
dispatches K = 1 to the k = 1 entries)."""
import json
import sys

import torch

sys.path.insert(0, ".")
from motionclone_amd import lib, ops  # noqa: E402

dev = torch.device("cuda:0")


def timeit(fn, iters=200, warm=20):
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


V, HW, heads, F, d = 5, 256, 8, 16, 160
C = heads * d
qkv = (torch.randn(V * F * HW, 3 * C, device=dev) * 0.5).half()
q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
do = torch.randn(V * F * HW, C, device=dev).half()
g = torch.empty_like(qkv)
ul = torch.empty(V * HW * heads, device=dev)
loss = torch.empty(1, device=dev)
sc, st = float(d ** -0.5), ops._stream(q)
for K in (1, 4):
    idx = torch.topk(torch.rand(V * HW, heads, F, F, device=dev), K, -1).indices.to(torch.uint8).contiguous()
    val = torch.rand(V * HW, heads, F, K, device=dev) * 0.5
    kk = (K,)
    for entry, extra in (("mc_tattn_%s_topk_f16", kk),) + ((("mc_tattn_%s_f16", ()),) if K == 1 else ()):
        def bwd(dout):
            lib.call(entry % "bwd", q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), None if dout is None else dout.data_ptr(),
                     0 if dout is None else dout.stride(0), g[:, :C].data_ptr(), g[:, C:2 * C].data_ptr(), g[:, 2 * C:].data_ptr(),
                     g.stride(0), idx.data_ptr(), val.data_ptr(), *extra, 1.0, V, F, HW, heads, d, sc, st)

        def lossf():
            lib.call(entry % "loss", q.data_ptr(), k.data_ptr(), q.stride(0), idx.data_ptr(), val.data_ptr(), *extra,
                     ul.data_ptr(), loss.data_ptr(), V, F, HW, heads, d, sc, st)
        print(json.dumps(dict(K=K, entries=entry % "*", bwd_us=round(timeit(lambda: bwd(do)), 2),
                              bwd_seed_only_us=round(timeit(lambda: bwd(None)), 2), loss_us=round(timeit(lossf), 2))), flush=True)
for K in (1, 4):
    print(json.dumps(dict(K=K, topk_us=round(timeit(lambda: ops.tattn_topk(q, k, V, F, HW, heads, d, K)), 2),
                          top1_us=round(timeit(lambda: ops.tattn_top1(q, k, V, F, HW, heads, d)), 2))), flush=True)
