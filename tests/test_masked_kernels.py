"""Region-weighted guidance, kernel level: mc_tattn_loss_weighted_f16 / mc_tattn_bwd_weighted_f16.

The weighted loss is restated here in fp32 torch: sum(w[bn, f] * (gather(P, idx) - ref)^2) over the UNWEIGHTED element count;
its autograd gradient is the reference of the backward.  Tolerances are those of tests/test_kernels.py::
test_temporal_attention_and_guidance and tests/test_topk_kernels.py for the unweighted kernels; nothing is excluded.
Weights of ones through the weighted entries give the unweighted entries' bits (K = 1: mc_tattn_*_f16, K > 1:
mc_tattn_*_topk_f16); rows of weight 0 contribute nothing.  Runs on the host simulator and, marked gpu, on the gfx950 library.
"""
import pytest
import torch

from motionclone_amd import lib, ops

B, HW, HEADS = 2, 6, 2
CASES = [(5, 16, 1), (5, 16, 5),        # masked key slots
         (16, 40, 1), (16, 40, 4),      # one score tile, vector-load backward
         (24, 32, 3),                   # ragged second tile
         (32, 80, 8),                   # winners across tiles
         (32, 160, 2)]                  # widest head dimension of the list


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
    return rnd((B * F_ * HW, 3 * HEADS * d), dev, 1, 0.8)


def _seeds(F_, K, dev):
    """K distinct frames per row (torch.topk of a random map), references in [0, 0.5)"""
    shape = (B * HW, HEADS, F_, K)
    ref_idx = torch.topk(torch.rand((B * HW, HEADS, F_, F_), generator=torch.Generator().manual_seed(7)), K, -1).indices
    ref_val = torch.rand(shape, generator=torch.Generator().manual_seed(8)) * 0.5
    return ref_idx.to(torch.uint8).to(dev).contiguous(), ref_val.to(dev)


def _weights(F_, dev):
    """[BN, F] in [0, 2], about a quarter of the rows exactly 0"""
    g = torch.Generator().manual_seed(11)
    w = torch.rand((B * HW, F_), generator=g) * 2.0
    w[torch.rand((B * HW, F_), generator=g) < 0.25] = 0.0
    assert 0.1 < (w == 0).float().mean() < 0.45
    return w.to(dev).contiguous()


def _weighted_loss(P, ref_idx, ref_val, w):
    """the issue's L_m: 1 / (BN heads F K) * sum w[bn, f] (P[.., idx] - ref)^2"""
    err = (torch.gather(P, -1, ref_idx.long()) - ref_val) ** 2
    return (w[:, None, :, None] * err).sum() / err.numel()


@pytest.mark.parametrize("F_,d,K", CASES)
def test_weighted_loss_and_backward(backend, F_, d, K):
    dev = backend
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    Q, Kt, V = (t.to(dev).requires_grad_() for t in _temporal_ref(qkv, F_, d))
    P = ((Q @ Kt.transpose(-1, -2)) * d ** -0.5).softmax(-1)
    ref = P @ V
    ref_idx, ref_val = _seeds(F_, K, dev)
    w = _weights(F_, dev)

    loss = ops.tattn_loss(q, k, ref_idx, ref_val, B, F_, HW, HEADS, d, row_w=w)
    loss_ref = _weighted_loss(P, ref_idx, ref_val, w)
    plain_ref = _weighted_loss(P, ref_idx, ref_val, torch.ones_like(w))
    print("loss %.6g ref %.6g (unweighted %.6g)" % (loss.item(), loss_ref.item(), plain_ref.item()))
    assert abs(loss.item() - loss_ref.item()) < 2e-3 * max(1.0, abs(loss_ref.item())) + 1e-5
    assert abs(loss_ref.item() - plain_ref.item()) > 1e-3   # the weights matter at this tolerance

    weight = 300.0
    do = rnd((B * F_ * HW, C), dev, 3)
    dO = _temporal_ref(torch.cat([do, do, do], 1), F_, d)[0]
    total = (ref * dO).sum() + weight * loss_ref
    gq, gk, gv = torch.autograd.grad(total, (Q, Kt, V), retain_graph=True)
    dqkv = torch.zeros_like(qkv)
    coef = weight * 2.0 / ref_idx.numel()
    # dO + seed
    ops.tattn_bwd(q, k, v, do, dqkv[:, :C], dqkv[:, C:2 * C], dqkv[:, 2 * C:], B, F_, HW, HEADS, d,
                  ref_idx=ref_idx, ref_val=ref_val, seed_coef=coef, row_w=w)
    close(dqkv[:, :C], _temporal_unref(gq, F_, d), 1e-2, 2e-2, "tattn dq")
    close(dqkv[:, C:2 * C], _temporal_unref(gk, F_, d), 1e-2, 2e-2, "tattn dk")
    close(dqkv[:, 2 * C:], _temporal_unref(gv, F_, d), 1e-2, 2e-2, "tattn dv")

    # seed only (dO = NULL)
    gq2, gk2 = torch.autograd.grad(weight * loss_ref, (Q, Kt))
    d2 = torch.ones_like(qkv)
    ops.tattn_bwd(q, k, v, None, d2[:, :C], d2[:, C:2 * C], d2[:, 2 * C:], B, F_, HW, HEADS, d,
                  ref_idx=ref_idx, ref_val=ref_val, seed_coef=coef, row_w=w)
    close(d2[:, :C], _temporal_unref(gq2, F_, d), 2e-3, 2e-2, "seed dq")
    close(d2[:, C:2 * C], _temporal_unref(gk2, F_, d), 2e-3, 2e-2, "seed dk")
    assert d2[:, 2 * C:].abs().max() == 0
    # a query row of weight 0 gets no seed: its dq is exactly zero (dq of row f depends on dS of row f only)
    dq_rows = d2[:, :C].reshape(B, F_, HW, C).permute(0, 2, 1, 3).reshape(B * HW, F_, C)
    assert (w == 0).any() and dq_rows[w == 0].abs().max() == 0
    assert dq_rows[w > 0.5].abs().max() > 0


def _raw_loss(name, q, k, ref_idx, ref_val, F_, d, extra=()):
    ul = torch.zeros(B * HW * HEADS, dtype=torch.float32, device=q.device)
    loss = torch.zeros(1, dtype=torch.float32, device=q.device)
    lib.call(name, q.data_ptr(), k.data_ptr(), q.stride(0), ref_idx.data_ptr(), ref_val.data_ptr(), *extra, ul.data_ptr(),
             loss.data_ptr(), B, F_, HW, HEADS, d, float(d ** -0.5), ops._stream(q))
    return loss


def _raw_bwd(name, qkv, do, ref_idx, ref_val, coef, F_, d, extra=()):
    C = HEADS * d
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    g = torch.full_like(qkv, 7.0)
    lib.call(name, q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), None if do is None else do.data_ptr(),
             0 if do is None else do.stride(0), g[:, :C].data_ptr(), g[:, C:2 * C].data_ptr(), g[:, 2 * C:].data_ptr(),
             g.stride(0), ref_idx.data_ptr(), ref_val.data_ptr(), *extra, float(coef), B, F_, HW, HEADS, d, float(d ** -0.5),
             ops._stream(q))
    return g


@pytest.mark.parametrize("F_,d,K", CASES)
def test_weights_of_one_are_bit_identical_to_the_unweighted_entries(backend, F_, d, K):
    dev = backend
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    ref_idx, ref_val = _seeds(F_, K, dev)
    ones = torch.ones((B * HW, F_), dtype=torch.float32, device=dev)
    plain, kk = ("mc_tattn_%s_f16", ()) if K == 1 else ("mc_tattn_%s_topk_f16", (K,))
    l0 = _raw_loss(plain % "loss", q, k, ref_idx, ref_val, F_, d, kk)
    l1 = _raw_loss("mc_tattn_loss_weighted_f16", q, k, ref_idx, ref_val, F_, d, (K, ones.data_ptr()))
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and l0.item() > 0
    do = rnd((B * F_ * HW, C), dev, 3)
    coef = 300.0 * 2.0 / ref_idx.numel()
    for dout in (do, None):
        g0 = _raw_bwd(plain % "bwd", qkv, dout, ref_idx, ref_val, coef, F_, d, kk)
        g1 = _raw_bwd("mc_tattn_bwd_weighted_f16", qkv, dout, ref_idx, ref_val, coef, F_, d, (K, ones.data_ptr()))
        assert torch.equal(g0.view(torch.int16), g1.view(torch.int16))
        assert g0[:, :C].float().abs().max() > 0


@pytest.mark.parametrize("F_,d,K", [(5, 16, 5), (16, 40, 1), (16, 40, 4), (32, 80, 8)])
def test_zero_weights_give_zero_loss_and_zero_gradient(backend, F_, d, K):
    dev = backend
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    ref_idx, ref_val = _seeds(F_, K, dev)
    zeros = torch.zeros((B * HW, F_), dtype=torch.float32, device=dev)
    loss = _raw_loss("mc_tattn_loss_weighted_f16", q, k, ref_idx, ref_val, F_, d, (K, zeros.data_ptr()))
    assert loss.item() == 0.0
    g = _raw_bwd("mc_tattn_bwd_weighted_f16", qkv, None, ref_idx, ref_val, 300.0, F_, d, (K, zeros.data_ptr()))
    assert (g == 0).all()      # dq, dk, dv all written, all exactly zero
    # with dO the zero weights leave the plain attention backward (no seed): the k = 1 entry with ref_idx = NULL
    do = rnd((B * F_ * HW, C), dev, 3)
    g1 = _raw_bwd("mc_tattn_bwd_weighted_f16", qkv, do, ref_idx, ref_val, 300.0, F_, d, (K, zeros.data_ptr()))
    v = qkv[:, 2 * C:]
    g0 = torch.full_like(qkv, 7.0)
    lib.call("mc_tattn_bwd_f16", q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), do.data_ptr(), do.stride(0),
             g0[:, :C].data_ptr(), g0[:, C:2 * C].data_ptr(), g0[:, 2 * C:].data_ptr(), g0.stride(0), None, None, 0.0,
             B, F_, HW, HEADS, d, float(d ** -0.5), ops._stream(q))
    assert torch.equal(g0, g1)     # as values: a seed of 0 * (P - ref) may turn a -0 of dP into +0


@pytest.mark.parametrize("F_,K,null_w", [(5, 0, False), (32, 9, False), (5, 6, False), (16, 2, True), (16, 1, True)])
def test_weighted_range_errors_launch_nothing(backend, F_, K, null_w):
    dev = backend
    d = 16
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    n = B * HW * HEADS * F_ * 16
    sc = float(d ** -0.5)
    ref_idx = torch.zeros(n, dtype=torch.uint8, device=dev)
    ref_val = torch.zeros(n, dtype=torch.float32, device=dev)
    w = torch.ones((B * HW, F_), dtype=torch.float32, device=dev)
    wp = None if null_w else w.data_ptr()
    ul = torch.full((B * HW * HEADS,), 5.0, dtype=torch.float32, device=dev)
    loss = torch.full((1,), 5.0, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError):
        lib.call("mc_tattn_loss_weighted_f16", q.data_ptr(), k.data_ptr(), q.stride(0), ref_idx.data_ptr(), ref_val.data_ptr(),
                 K, wp, ul.data_ptr(), loss.data_ptr(), B, F_, HW, HEADS, d, sc, ops._stream(q))
    assert (ul == 5.0).all() and (loss == 5.0).all()
    g = torch.full_like(qkv, 7.0)
    with pytest.raises(RuntimeError):
        lib.call("mc_tattn_bwd_weighted_f16", q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), None, 0,
                 g[:, :C].data_ptr(), g[:, C:2 * C].data_ptr(), g[:, 2 * C:].data_ptr(), g.stride(0), ref_idx.data_ptr(),
                 ref_val.data_ptr(), K, wp, 300.0, B, F_, HW, HEADS, d, sc, ops._stream(q))
    assert (g == 7.0).all()


def test_ops_check_the_weights(backend):
    dev = backend
    F_, d, K = 5, 16, 1
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    ref_idx, ref_val = _seeds(F_, K, dev)
    good = torch.ones((B * HW, F_), dtype=torch.float32, device=dev)
    for bad, what in ((good.half(), "float32"), (good.t().contiguous().t(), "contiguous"), (good[:, :4].contiguous(), "row_w")):
        with pytest.raises(ValueError, match=what):
            ops.tattn_loss(q, k, ref_idx, ref_val, B, F_, HW, HEADS, d, row_w=bad)
    dq = torch.zeros_like(qkv)
    with pytest.raises(ValueError, match="ref_idx"):
        ops.tattn_bwd(q, k, qkv[:, 2 * C:], None, dq[:, :C], dq[:, C:2 * C], dq[:, 2 * C:], B, F_, HW, HEADS, d, row_w=good)
