"""Top-k motion representation, kernel level: mc_tattn_topk_f16 / mc_tattn_loss_topk_f16 / mc_tattn_bwd_topk_f16.

Extraction is checked exactly against torch.topk / a stable sort of the library's own fp16 probabilities (the tie rule:
equal probabilities by ascending frame) and, with the k = 1 test's bounds, against fp32 torch on the same q / k.  Loss and
backward are checked against gather + mse_loss + autograd with the tolerances tests/test_kernels.py uses for k = 1, for
index rows that are distinct (topk) and for rows that may repeat a frame (randint).  K = 1 through the new entry points is
bit-identical to the k = 1 entry points.  Runs on the host simulator and, marked gpu, on the gfx950 library.
"""
import pytest
import torch
import torch.nn.functional as Fn

from motionclone_amd import lib, ops

B, HW, HEADS = 2, 6, 2
CASES = [(5, 16, 1), (5, 16, 2), (5, 16, 5),        # K = F, masked key slots
         (16, 40, 1), (16, 40, 2), (16, 40, 4),     # one score tile, vector-load backward
         (24, 32, 3),                               # two tiles, ragged second tile
         (32, 80, 2), (32, 80, 8),                  # winners that cross tiles
         (32, 160, 4)]


def rnd(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.float16).to(dev)


def close(a, b, atol, rtol, what=""):
    a = a.float().cpu()
    b = b.float().cpu()
    err = (a - b).abs()
    tol = atol + rtol * b.abs()
    bad = (err > tol).float().mean().item()
    assert torch.isfinite(a).all(), what + ": non-finite output"
    assert bad == 0.0, "%s: %.4f%% elements off, max err %.4g (ref max %.3g)" % (
        what, 100 * bad, err.max().item(), b.abs().max().item())


def _temporal_ref(qkv, F_, d):
    t = qkv.float().reshape(B, F_, HW, 3, HEADS, d).permute(3, 0, 2, 4, 1, 5)  # [3, B, HW, heads, F, d]
    return t[0].reshape(-1, HEADS, F_, d), t[1].reshape(-1, HEADS, F_, d), t[2].reshape(-1, HEADS, F_, d)


def _temporal_unref(t, F_, d):  # [B*HW, heads, F, d] -> [(b f hw), heads*d]
    return t.reshape(B, HW, HEADS, F_, d).permute(0, 3, 1, 2, 4).reshape(B * F_ * HW, HEADS * d)


def _qkv(dev, F_, d):
    return rnd((B * F_ * HW, 3 * HEADS * d), dev, 1, 0.8)   # as test_kernels.py::test_temporal_attention_and_guidance


def _check_extraction(q, k, F_, d, K, qkv):
    Ph = ops.tattn_prob(q, k, B, F_, HW, HEADS, d).float().cpu()
    val, idx = ops.tattn_topk(q, k, B, F_, HW, HEADS, d, K)
    assert val.shape == idx.shape == (B * HW, HEADS, F_, K) and val.dtype == torch.float16 and idx.dtype == torch.uint8
    # exact, nothing excluded: values of torch.topk, indices of a stable descending sort (ties: lower frame first)
    assert torch.equal(val.float().cpu(), torch.topk(Ph, K, -1).values), "top-k values differ from torch.topk(P_fp16)"
    order = torch.sort(Ph, dim=-1, descending=True, stable=True).indices[..., :K]
    assert torch.equal(idx.long().cpu(), order), "top-k indices differ from the stable descending order"
    # against fp32 torch on the same q / k, nothing excluded
    Q, Kt, _ = _temporal_ref(qkv.cpu(), F_, d)
    P = ((Q @ Kt.transpose(-1, -2)) * d ** -0.5).softmax(-1)
    rv = torch.topk(P, K, -1).values
    close(val, rv, 2e-3, 2e-3, "top-k value")
    assert ((torch.gather(P, -1, idx.long().cpu()) - rv).abs() < 1e-3).all(), "top-k index beyond a numerical tie"
    return Ph, val, idx


@pytest.mark.parametrize("F_,d,K", CASES)
def test_topk_extraction(backend, F_, d, K):
    dev = backend
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    _, val, idx = _check_extraction(q, k, F_, d, K, qkv)
    if K == 1:
        v1, i1 = ops.tattn_top1(q, k, B, F_, HW, HEADS, d)
        assert torch.equal(val.view(torch.int16), v1.view(torch.int16)) and torch.equal(idx, i1)


@pytest.mark.parametrize("F_,d,K", [(24, 32, 3), (16, 40, 4)])
def test_topk_constructed_ties(backend, F_, d, K):
    """two key frames are copies of two others (one pair inside a tile / lane, one across tiles or lanes): their
    probabilities are equal in every row, and the rows where a pair reaches the top K pin the lower-index-first rule"""
    dev = backend
    C = HEADS * d
    qkv = _qkv(dev, F_, d).clone()
    rows = qkv.view(B, F_, HW, 3 * C)
    pairs = [(2, 3), (1, F_ - 3)]
    for a, b in pairs:
        rows[:, b, :, C:2 * C] = rows[:, a, :, C:2 * C]
    # the duplicated keys are made large so that they reach the top K of many rows
    for a, b in pairs:
        rows[:, a, :, C:2 * C] *= 2.0
        rows[:, b, :, C:2 * C] *= 2.0
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    Ph, val, idx = _check_extraction(q, k, F_, d, K, qkv)
    for a, b in pairs:
        assert torch.equal(Ph[..., a], Ph[..., b])
    idx = idx.long().cpu()
    hit = 0
    for a, b in pairs:
        both = (idx == a).any(-1) & (idx == b).any(-1)
        hit += int(both.sum())
        pa = (idx == a).float().argmax(-1)
        pb = (idx == b).float().argmax(-1)
        assert (pb[both] > pa[both]).all(), "tied frames %d / %d not in ascending order" % (a, b)
    assert hit >= 20, "the construction put a tied pair into the top %d of only %d rows" % (K, hit)


def _seeds(P, F_, K, distinct, dev):
    shape = tuple(P.shape[:-1]) + (K,)
    if distinct:   # torch.topk of a random map: K distinct frames per row
        ref_idx = torch.topk(torch.rand(P.shape, generator=torch.Generator().manual_seed(7)), K, -1).indices
    else:          # may name a frame twice in a row
        ref_idx = torch.randint(0, F_, shape, generator=torch.Generator().manual_seed(7))
    ref_val = torch.rand(shape, generator=torch.Generator().manual_seed(8)) * 0.5
    return ref_idx.to(torch.uint8).to(dev).contiguous(), ref_val.to(dev)


@pytest.mark.parametrize("distinct", [True, False], ids=["topk_idx", "randint_idx"])
@pytest.mark.parametrize("F_,d,K", CASES)
def test_topk_loss_and_backward(backend, F_, d, K, distinct):
    dev = backend
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    Q, Kt, V = (t.to(dev).requires_grad_() for t in _temporal_ref(qkv, F_, d))
    P = ((Q @ Kt.transpose(-1, -2)) * d ** -0.5).softmax(-1)
    ref = P @ V
    ref_idx, ref_val = _seeds(P, F_, K, distinct, dev)
    if not distinct and K > 1:
        srt = ref_idx.sort(-1).values
        assert (srt[..., 1:] == srt[..., :-1]).any(), "randint drew no repeated frame"

    loss = ops.tattn_loss(q, k, ref_idx, ref_val, B, F_, HW, HEADS, d)
    gathered = torch.gather(P, -1, ref_idx.long())
    loss_ref = Fn.mse_loss(gathered, ref_val)
    print("loss %.6g ref %.6g" % (loss.item(), loss_ref.item()))
    assert abs(loss.item() - loss_ref.item()) < 2e-3 * max(1.0, abs(loss_ref.item())) + 1e-5

    weight = 300.0
    do = rnd((B * F_ * HW, C), dev, 3)
    dO = _temporal_ref(torch.cat([do, do, do], 1), F_, d)[0]
    total = (ref * dO).sum() + weight * loss_ref
    gq, gk, gv = torch.autograd.grad(total, (Q, Kt, V), retain_graph=True)
    dqkv = torch.zeros_like(qkv)
    coef = weight * 2.0 / gathered.numel()
    ops.tattn_bwd(q, k, v, do, dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:], B, F_, HW, HEADS, d,
                  ref_idx=ref_idx, ref_val=ref_val, seed_coef=coef)
    close(dqkv[:, :C], _temporal_unref(gq, F_, d), 1e-2, 2e-2, "tattn dq")
    close(dqkv[:, C:2 * C], _temporal_unref(gk, F_, d), 1e-2, 2e-2, "tattn dk")
    close(dqkv[:, 2 * C:], _temporal_unref(gv, F_, d), 1e-2, 2e-2, "tattn dv")

    # seed only (dO = NULL)
    gq2, gk2 = torch.autograd.grad(weight * Fn.mse_loss(torch.gather(P, -1, ref_idx.long()), ref_val), (Q, Kt))
    d2 = torch.ones_like(qkv)
    ops.tattn_bwd(q, k, v, None, d2[:, :C], d2[:, C:2 * C], d2[:, 2 * C:], B, F_, HW, HEADS, d,
                  ref_idx=ref_idx, ref_val=ref_val, seed_coef=coef)
    close(d2[:, :C], _temporal_unref(gq2, F_, d), 2e-3, 2e-2, "seed dq")
    close(d2[:, C:2 * C], _temporal_unref(gk2, F_, d), 2e-3, 2e-2, "seed dk")
    assert d2[:, 2 * C:].abs().max() == 0


def _raw_loss(name, q, k, ref_idx, ref_val, F_, d, K=None):
    ul = torch.zeros(B * HW * HEADS, dtype=torch.float32, device=q.device)
    loss = torch.zeros(1, dtype=torch.float32, device=q.device)
    kk = () if K is None else (K,)
    lib.call(name, q.data_ptr(), k.data_ptr(), q.stride(0), ref_idx.data_ptr(), ref_val.data_ptr(), *kk, ul.data_ptr(),
             loss.data_ptr(), B, F_, HW, HEADS, d, float(d ** -0.5), ops._stream(q))
    return loss


def _raw_bwd(name, qkv, do, ref_idx, ref_val, coef, F_, d, K=None):
    C = HEADS * d
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    g = torch.full_like(qkv, 7.0)
    kk = () if K is None else (K,)
    lib.call(name, q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), None if do is None else do.data_ptr(),
             0 if do is None else do.stride(0), g[:, :C].data_ptr(), g[:, C:2 * C].data_ptr(), g[:, 2 * C:].data_ptr(),
             g.stride(0), ref_idx.data_ptr(), ref_val.data_ptr(), *kk, float(coef), B, F_, HW, HEADS, d, float(d ** -0.5),
             ops._stream(q))
    return g


@pytest.mark.parametrize("F_,d", [(5, 16), (16, 40), (24, 32), (32, 80), (32, 160)])
def test_k1_through_topk_entries_is_bit_identical(backend, F_, d):
    """K = 1 through mc_tattn_*_topk_f16 (ops dispatches K = 1 to the k = 1 entries, so this goes through lib.call)"""
    dev = backend
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    v1, i1 = ops.tattn_top1(q, k, B, F_, HW, HEADS, d)
    vk, ik = ops.tattn_topk(q, k, B, F_, HW, HEADS, d, 1)
    assert torch.equal(vk.view(torch.int16), v1.view(torch.int16)) and torch.equal(ik, i1)
    ref_idx, ref_val = _seeds(torch.empty(B * HW, HEADS, F_, F_), F_, 1, False, dev)
    l1 = _raw_loss("mc_tattn_loss_f16", q, k, ref_idx, ref_val, F_, d)
    lk = _raw_loss("mc_tattn_loss_topk_f16", q, k, ref_idx, ref_val, F_, d, K=1)
    assert torch.equal(l1.view(torch.int32), lk.view(torch.int32)) and l1.item() > 0
    do = rnd((B * F_ * HW, C), dev, 3)
    coef = 300.0 * 2.0 / ref_idx.numel()
    for dout in (do, None):
        g1 = _raw_bwd("mc_tattn_bwd_f16", qkv, dout, ref_idx, ref_val, coef, F_, d)
        gk = _raw_bwd("mc_tattn_bwd_topk_f16", qkv, dout, ref_idx, ref_val, coef, F_, d, K=1)
        assert torch.equal(g1.view(torch.int16), gk.view(torch.int16))
        assert g1[:, :C].float().abs().max() > 0


@pytest.mark.parametrize("F_,K", [(5, 0), (5, 6), (32, 9), (32, 0), (16, -1)])
def test_topk_range_errors_launch_nothing(backend, F_, K):
    dev = backend
    d = 16
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    n = B * HW * HEADS * F_ * 16
    val = torch.full((n,), 3.0, dtype=torch.float16, device=dev)
    idx = torch.full((n,), 77, dtype=torch.uint8, device=dev)
    sc = float(d ** -0.5)
    with pytest.raises(RuntimeError):
        lib.call("mc_tattn_topk_f16", q.data_ptr(), k.data_ptr(), q.stride(0), val.data_ptr(), idx.data_ptr(), K, B, F_, HW,
                 HEADS, d, sc, ops._stream(q))
    assert (val == 3.0).all() and (idx == 77).all()
    ref_idx = torch.zeros(n, dtype=torch.uint8, device=dev)
    ref_val = torch.zeros(n, dtype=torch.float32, device=dev)
    ul = torch.full((B * HW * HEADS,), 5.0, dtype=torch.float32, device=dev)
    loss = torch.full((1,), 5.0, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError):
        lib.call("mc_tattn_loss_topk_f16", q.data_ptr(), k.data_ptr(), q.stride(0), ref_idx.data_ptr(), ref_val.data_ptr(), K,
                 ul.data_ptr(), loss.data_ptr(), B, F_, HW, HEADS, d, sc, ops._stream(q))
    assert (ul == 5.0).all() and (loss == 5.0).all()
    g = torch.full_like(qkv, 7.0)
    with pytest.raises(RuntimeError):
        lib.call("mc_tattn_bwd_topk_f16", q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), None, 0, g[:, :C].data_ptr(),
                 g[:, C:2 * C].data_ptr(), g[:, 2 * C:].data_ptr(), g.stride(0), ref_idx.data_ptr(), ref_val.data_ptr(), K,
                 300.0, B, F_, HW, HEADS, d, sc, ops._stream(q))
    assert (g == 7.0).all()
    if K >= 0:
        with pytest.raises(RuntimeError):
            ops.tattn_topk(q, k, B, F_, HW, HEADS, d, K)
