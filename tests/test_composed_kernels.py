"""Motion composition, kernel level: mc_tattn_loss_slotw_f16 / mc_tattn_bwd_slotw_f16.

A query row carries the entries of R references concatenated (K = sum K_r <= 8 slots) and one weight per slot,
slot_w[bn, f, s] = lambda_r * w_r[bn, f] / K_r.  The loss is restated here in fp32 torch per reference,
    L = sum_r lambda_r / (BN heads F K_r) * sum w_r[bn, f] (P[.., idx_r] - val_r)^2,
and its autograd gradient is the reference of the backward.  Tolerances are those of tests/test_masked_kernels.py::
test_weighted_loss_and_backward, unchanged; nothing is excluded.  Runs on the host simulator and, marked gpu, on the gfx950
library.
"""
import pytest
import torch

from motionclone_amd import lib, ops

B, HW, HEADS = 2, 6, 2
BN = B * HW
CASES = [(5, 16, (1, 1)),
         (5, 16, (3, 5)),                      # more slots than frames: duplicates are forced
         (16, 40, (2, 2)),                     # one 16-byte weight read, vector-load backward
         (16, 40, (1, 3)),
         (24, 32, (3, 1, 2)),                  # ragged second tile, slot by slot weight reads
         (32, 80, (4, 4)),                     # two 16-byte weight reads
         (32, 160, (1, 1, 1, 1, 1, 1, 1, 1))]
LAMBDAS = (1.0, 0.5, 2.0, 0.75, 1.5, 0.25, 1.25, 0.6)
WEIGHT = 300.0


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


def _reference(F_, K, r, dev):
    """reference r: K distinct frames per row (torch.topk of a random map), values in [0, 0.5)"""
    idx = torch.topk(torch.rand((BN, HEADS, F_, F_), generator=torch.Generator().manual_seed(7 + 10 * r)), K, -1).indices
    val = torch.rand((BN, HEADS, F_, K), generator=torch.Generator().manual_seed(8 + 10 * r)) * 0.5
    return idx.to(torch.uint8).to(dev).contiguous(), val.to(dev)


def _weights(F_, dev, r=0):
    """[BN, F] in [0, 2], about a quarter of the rows exactly 0 (r = 0: the weights of test_masked_kernels.py)"""
    g = torch.Generator().manual_seed(11 + 10 * r)
    w = torch.rand((BN, F_), generator=g) * 2.0
    w[torch.rand((BN, F_), generator=g) < 0.25] = 0.0
    assert 0.1 < (w == 0).float().mean() < 0.45
    return w.to(dev).contiguous()


def _merge(refs, ws, lams):
    """the merged form of the kernels: entries concatenated in reference order, slot_w = lambda_r w_r / K_r (float64 -> f32)"""
    idx = torch.cat([r[0] for r in refs], -1).contiguous()
    val = torch.cat([r[1] for r in refs], -1).contiguous()
    sw = torch.cat([(lam * w.double() / r[0].shape[-1])[:, :, None].expand(-1, -1, r[0].shape[-1])
                    for r, w, lam in zip(refs, ws, lams)], -1).float().contiguous()
    return idx, val, sw


def _composed_loss(P, refs, ws, lams):
    """the issue's L_m: every reference keeps its own unweighted mean"""
    total = 0.0
    for (idx, val), w, lam in zip(refs, ws, lams):
        err = (torch.gather(P, -1, idx.long()) - val) ** 2
        total = total + lam * (w[:, None, :, None] * err).sum() / err.numel()
    return total


def _setup(dev, F_, d, ks, same_w=False):
    qkv = _qkv(dev, F_, d)
    Q, Kt, V = (t.to(dev).requires_grad_() for t in _temporal_ref(qkv, F_, d))
    P = ((Q @ Kt.transpose(-1, -2)) * d ** -0.5).softmax(-1)
    refs = [_reference(F_, K, r, dev) for r, K in enumerate(ks)]
    ws = [_weights(F_, dev, 0 if same_w else r) for r in range(len(ks))]
    lams = LAMBDAS[:len(ks)]
    return qkv, (Q, Kt, V), P, refs, ws, lams


def _bwd(qkv, do, idx, val, coef, F_, d, fill=0.0, **kw):
    C = HEADS * d
    g = torch.full_like(qkv, fill)
    ops.tattn_bwd(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], do, g[:, :C], g[:, C:2 * C], g[:, 2 * C:], B, F_, HW, HEADS, d,
                  ref_idx=idx, ref_val=val, seed_coef=coef, **kw)
    return g


def _check_against_autograd(dev, F_, d, qkv, QKV, P, refs, ws, lams):
    C = HEADS * d
    Q, Kt, V = QKV
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    idx, val, sw = _merge(refs, ws, lams)
    assert idx.shape[-1] == sum(r[0].shape[-1] for r in refs) <= 8 and tuple(sw.shape) == (BN, F_, idx.shape[-1])
    loss = ops.tattn_loss(q, k, idx, val, B, F_, HW, HEADS, d, slot_w=sw)
    loss_ref = _composed_loss(P, refs, ws, lams)
    print("loss %.6g ref %.6g" % (loss.item(), loss_ref.item()))
    assert abs(loss.item() - loss_ref.item()) < 2e-3 * max(1.0, abs(loss_ref.item())) + 1e-5

    do = rnd((B * F_ * HW, C), dev, 3)
    dO = _temporal_ref(torch.cat([do, do, do], 1), F_, d)[0]
    total = ((P @ V) * dO).sum() + WEIGHT * loss_ref
    gq, gk, gv = torch.autograd.grad(total, (Q, Kt, V), retain_graph=True)
    coef = WEIGHT * 2.0 / (BN * HEADS * F_)       # the new denominator: the K_r live in the weights
    g = _bwd(qkv, do, idx, val, coef, F_, d, slot_w=sw)
    close(g[:, :C], _temporal_unref(gq, F_, d), 1e-2, 2e-2, "tattn dq")
    close(g[:, C:2 * C], _temporal_unref(gk, F_, d), 1e-2, 2e-2, "tattn dk")
    close(g[:, 2 * C:], _temporal_unref(gv, F_, d), 1e-2, 2e-2, "tattn dv")
    # seed only (dO = NULL)
    gq2, gk2 = torch.autograd.grad(WEIGHT * loss_ref, (Q, Kt), retain_graph=True)
    g2 = _bwd(qkv, None, idx, val, coef, F_, d, fill=1.0, slot_w=sw)
    close(g2[:, :C], _temporal_unref(gq2, F_, d), 2e-3, 2e-2, "seed dq")
    close(g2[:, C:2 * C], _temporal_unref(gk2, F_, d), 2e-3, 2e-2, "seed dk")
    assert g2[:, 2 * C:].abs().max() == 0
    assert g2[:, :C].float().abs().max() > 0
    return loss_ref, g2


@pytest.mark.parametrize("F_,d,ks", CASES)
def test_composed_loss_and_backward(backend, F_, d, ks):
    dev = backend
    qkv, QKV, P, refs, ws, lams = _setup(dev, F_, d, ks)
    loss_ref, _ = _check_against_autograd(dev, F_, d, qkv, QKV, P, refs, ws, lams)
    # the second reference matters at this tolerance
    without = _composed_loss(P, refs[:1] + refs[2:], ws[:1] + ws[2:], lams[:1] + lams[2:])
    print("without the second reference %.6g" % without.item())
    assert abs(loss_ref.item() - without.item()) > 1e-3


@pytest.mark.parametrize("F_,d", [(5, 16), (16, 40), (32, 80)])
def test_a_frame_named_by_two_references_gets_both_seeds(backend, F_, d):
    dev = backend
    qkv, QKV, P, refs, ws, lams = _setup(dev, F_, d, (1, 1))
    refs[1] = (refs[0][0].clone(), refs[1][1])           # reference 1 repeats reference 0's index, with its own values
    _check_against_autograd(dev, F_, d, qkv, QKV, P, refs, ws, lams)


@pytest.mark.parametrize("F_,d,ks", [(5, 16, (3, 5)), (16, 40, (2, 2)), (24, 32, (3, 1, 2))])
def test_rows_whose_slots_all_weigh_zero_get_no_seed(backend, F_, d, ks):
    dev = backend
    C = HEADS * d
    qkv, QKV, P, refs, ws, lams = _setup(dev, F_, d, ks, same_w=True)
    _, g2 = _check_against_autograd(dev, F_, d, qkv, QKV, P, refs, ws, lams)
    w = ws[0]
    # dq of row f depends on dS of row f only
    dq_rows = g2[:, :C].reshape(B, F_, HW, C).permute(0, 2, 1, 3).reshape(BN, F_, C)
    assert (w == 0).any() and dq_rows[w == 0].abs().max() == 0
    assert dq_rows[w > 0.5].abs().max() > 0


@pytest.mark.parametrize("F_,d,ks", [(5, 16, (1, 1)), (16, 40, (2, 3)), (24, 32, (3, 1, 2)), (32, 80, (4,))])
def test_zero_weight_padding_to_eight_slots_changes_no_bit(backend, F_, d, ks):
    dev = backend
    C = HEADS * d
    qkv, _, _, refs, ws, lams = _setup(dev, F_, d, ks)
    idx, val, sw = _merge(refs, ws, lams)
    K = idx.shape[-1]
    pad = 8 - K
    idx8 = torch.cat([idx, torch.zeros(idx.shape[:-1] + (pad,), dtype=torch.uint8, device=dev)], -1).contiguous()
    val8 = torch.cat([val, torch.zeros(val.shape[:-1] + (pad,), dtype=torch.float32, device=dev)], -1).contiguous()
    sw8 = torch.cat([sw, torch.zeros(sw.shape[:-1] + (pad,), dtype=torch.float32, device=dev)], -1).contiguous()
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    l0 = ops.tattn_loss(q, k, idx, val, B, F_, HW, HEADS, d, slot_w=sw)
    l1 = ops.tattn_loss(q, k, idx8, val8, B, F_, HW, HEADS, d, slot_w=sw8)
    assert torch.equal(l0.view(torch.int32), l1.view(torch.int32)) and l0.item() > 0
    do = rnd((B * F_ * HW, C), dev, 3)
    coef = WEIGHT * 2.0 / (BN * HEADS * F_)
    for dout in (do, None):
        g0 = _bwd(qkv, dout, idx, val, coef, F_, d, fill=7.0, slot_w=sw)
        g1 = _bwd(qkv, dout, idx8, val8, coef, F_, d, fill=7.0, slot_w=sw8)
        assert torch.equal(g0.view(torch.int16), g1.view(torch.int16))
        assert g0[:, :C].float().abs().max() > 0


@pytest.mark.parametrize("F_,d,K", [(5, 16, 1), (16, 40, 4), (24, 32, 3), (32, 80, 8)])
def test_one_reference_agrees_with_the_row_weighted_entries(backend, F_, d, K):
    dev = backend
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k = qkv[:, :C], qkv[:, C:2 * C]
    idx, val = _reference(F_, K, 0, dev)
    w = _weights(F_, dev)
    _, _, sw = _merge([(idx, val)], [w], [1.0])
    l_row = ops.tattn_loss(q, k, idx, val, B, F_, HW, HEADS, d, row_w=w)
    l_slot = ops.tattn_loss(q, k, idx, val, B, F_, HW, HEADS, d, slot_w=sw)
    assert abs(l_slot.item() - l_row.item()) < 2e-3 * max(1.0, abs(l_row.item())) + 1e-5 and l_row.item() > 0
    do = rnd((B * F_ * HW, C), dev, 3)
    # row-weighted: coefficient over BN heads F K entries; slot-weighted: over BN heads F rows, 1 / K in the weights
    c_row, c_slot = WEIGHT * 2.0 / idx.numel(), WEIGHT * 2.0 / (BN * HEADS * F_)
    for dout, atol in ((do, 1e-2), (None, 2e-3)):
        g_row = _bwd(qkv, dout, idx, val, c_row, F_, d, row_w=w)
        g_slot = _bwd(qkv, dout, idx, val, c_slot, F_, d, slot_w=sw)
        for n, sl in (("dq", slice(0, C)), ("dk", slice(C, 2 * C)), ("dv", slice(2 * C, 3 * C))):
            close(g_slot[:, sl], g_row[:, sl], atol, 2e-2, "slot- vs row-weighted " + n)
        assert g_row[:, :C].float().abs().max() > 0


@pytest.mark.parametrize("F_,d,ks", [(16, 40, (2, 2)), (32, 80, (3, 5))])
def test_two_launches_give_the_same_bits(backend, F_, d, ks):
    dev = backend
    C = HEADS * d
    qkv, _, _, refs, ws, lams = _setup(dev, F_, d, ks)
    idx, val, sw = _merge(refs, ws, lams)
    do = rnd((B * F_ * HW, C), dev, 3)
    runs = []
    for _ in range(2):
        loss = ops.tattn_loss(qkv[:, :C], qkv[:, C:2 * C], idx, val, B, F_, HW, HEADS, d, slot_w=sw).clone()
        runs.append((loss, _bwd(qkv, do, idx, val, 0.01, F_, d, slot_w=sw)))
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32))
    assert torch.equal(runs[0][1].view(torch.int16), runs[1][1].view(torch.int16))


@pytest.mark.parametrize("F_,K,null", [(5, 0, ""), (32, 9, ""), (16, 2, "slot_w"), (16, 2, "ref_idx"), (16, 2, "ref_val")])
def test_slot_range_errors_launch_nothing(backend, F_, K, null):
    dev = backend
    d = 16
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    n = BN * HEADS * F_ * 16
    sc = float(d ** -0.5)
    ptr = dict(ref_idx=torch.zeros(n, dtype=torch.uint8, device=dev), ref_val=torch.zeros(n, dtype=torch.float32, device=dev),
               slot_w=torch.ones(BN * F_ * 16, dtype=torch.float32, device=dev))
    ip, vp, wp = (None if null == name else ptr[name].data_ptr() for name in ("ref_idx", "ref_val", "slot_w"))
    ul = torch.full((BN * HEADS,), 5.0, dtype=torch.float32, device=dev)
    loss = torch.full((1,), 5.0, dtype=torch.float32, device=dev)
    with pytest.raises(RuntimeError):
        lib.call("mc_tattn_loss_slotw_f16", q.data_ptr(), k.data_ptr(), q.stride(0), ip, vp, K, wp, ul.data_ptr(),
                 loss.data_ptr(), B, F_, HW, HEADS, d, sc, ops._stream(q))
    assert (ul == 5.0).all() and (loss == 5.0).all()
    g = torch.full_like(qkv, 7.0)
    with pytest.raises(RuntimeError):
        lib.call("mc_tattn_bwd_slotw_f16", q.data_ptr(), k.data_ptr(), v.data_ptr(), q.stride(0), None, 0,
                 g[:, :C].data_ptr(), g[:, C:2 * C].data_ptr(), g[:, 2 * C:].data_ptr(), g.stride(0), ip, vp, K, wp, 300.0,
                 B, F_, HW, HEADS, d, sc, ops._stream(q))
    assert (g == 7.0).all()


def test_ops_check_the_slot_weights(backend):
    dev = backend
    F_, d = 5, 16
    C = HEADS * d
    qkv = _qkv(dev, F_, d)
    q, k, v = qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:]
    idx, val = _reference(F_, 2, 0, dev)
    good = torch.ones((BN, F_, 2), dtype=torch.float32, device=dev)
    row = torch.ones((BN, F_), dtype=torch.float32, device=dev)
    dq = torch.full_like(qkv, 7.0)
    for bad, what in ((good.half(), "float32"), (good.transpose(0, 1).contiguous().transpose(0, 1), "contiguous"),
                      (good[:, :, :1].contiguous(), "slot_w"), (row, "slot_w")):
        with pytest.raises(ValueError, match=what):
            ops.tattn_loss(q, k, idx, val, B, F_, HW, HEADS, d, slot_w=bad)
        with pytest.raises(ValueError, match=what):
            ops.tattn_bwd(q, k, v, None, dq[:, :C], dq[:, C:2 * C], dq[:, 2 * C:], B, F_, HW, HEADS, d, ref_idx=idx,
                          ref_val=val, seed_coef=1.0, slot_w=bad)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.tattn_loss(q, k, idx, val, B, F_, HW, HEADS, d, row_w=row, slot_w=good)
    with pytest.raises(ValueError, match="mutually exclusive"):
        ops.tattn_bwd(q, k, v, None, dq[:, :C], dq[:, C:2 * C], dq[:, 2 * C:], B, F_, HW, HEADS, d, ref_idx=idx, ref_val=val,
                      seed_coef=1.0, row_w=row, slot_w=good)
    with pytest.raises(ValueError, match="ref_idx"):
        ops.tattn_bwd(q, k, v, None, dq[:, :C], dq[:, C:2 * C], dq[:, 2 * C:], B, F_, HW, HEADS, d, slot_w=good)
    assert (dq == 7.0).all()
