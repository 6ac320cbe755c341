"""Sliding context windows, kernel level: the window rule (ops.context_windows), the gather (mc_latent_windows_f16) and the
blended CFG + DDIM update of the long latent (mc_cfg_ddim_step_windows_f16) against an fp64 restatement, bit-identity with the
existing update wherever one window covers a frame, and a negative control on the frames that several cover."""
import pytest
import torch

from motionclone_amd import lib, ops

from context_util import blend_update_f64, cover, tokens_to_latent, weights64

A_T, A_PREV, CFG = 0.61, 0.72, 7.5


def test_window_rule():
    assert ops.context_windows(7, 4, 2) == [0, 2, 3]
    assert ops.context_windows(8, 4, 0) == [0, 4]
    assert ops.context_windows(4, 4, 1) in ([], [0])
    assert ops.context_windows(3, 4, 1) == []
    assert ops.context_windows(64, 16, 4) == [0, 12, 24, 36, 48]
    for F, L, ov in [(7, 4, 2), (8, 4, 0), (64, 16, 4), (36, 16, 6), (33, 32, 31), (9, 4, 3), (5, 1, 0), (100, 32, 5)]:
        starts = ops.context_windows(F, L, ov)
        S = L - ov
        assert len(starts) == -(-(F - L) // S) + 1 and starts == sorted(starts)
        assert all(0 <= s and s + L <= F for s in starts) and starts[-1] == F - L
        assert all(cover(f, starts, L) for f in range(F))
        assert starts[:-1] == [w * S for w in range(len(starts) - 1)]
    for bad in [(8, 0, 0), (40, 33, 1), (8, 4, 4), (8, 4, -1), (64, 2, 1)]:      # L, overlap, nW = 63 > 32
        with pytest.raises(ValueError):
            ops.context_windows(*bad)
    with pytest.raises(ValueError, match="33"):
        ops.context_windows(36, 4, 3)


def _inputs(F, L, ov, CL, H, W, ld, dev, seed):
    g = torch.Generator().manual_seed(seed)
    nW = len(ops.context_windows(F, L, ov))
    T = nW * L * H * W
    ec = torch.randn(T, ld, generator=g).half().to(dev)
    eu = torch.randn(T, ld, generator=g).half().to(dev)
    x = torch.randn(1, CL, F, H, W, generator=g).half().to(dev)
    score = torch.randn(nW, CL, L, H, W, generator=g).float().to(dev)
    return ec, eu, x, score


@pytest.mark.parametrize("F,L,ov", [(7, 4, 2), (8, 4, 0), (9, 4, 3), (5, 1, 0)])
@pytest.mark.parametrize("CL", [4, 3])
def test_gather_equals_slicing(backend, F, L, ov, CL):
    x = torch.randn(1, CL, F, 2, 3, generator=torch.Generator().manual_seed(F + CL)).half().to(backend)
    got = ops.latent_windows(x, L, ov)
    want = torch.cat([x[:, :, s:s + L] for s in ops.context_windows(F, L, ov)], 0)
    assert got.shape == want.shape and torch.equal(got, want)
    with pytest.raises(ValueError):
        ops.latent_windows(x[:, :, :L], L, ov)
    with pytest.raises(ValueError):
        ops.latent_windows(torch.cat([x, x], 0), L, ov)


def _check(got, want):
    got = got.double().cpu()
    want = want.cpu()
    max_abs, rel = (got - want).abs().max().item(), ((got - want).norm() / want.norm()).item()
    print("windowed update: max abs %.3e  rel L2 %.3e" % (max_abs, rel))
    assert rel < 1e-3 and max_abs < 2e-2


@pytest.mark.parametrize("weights", ["triangular", "uniform"])
@pytest.mark.parametrize("with_score", [False, True])
@pytest.mark.parametrize("want_eps", [False, True])
@pytest.mark.parametrize("sigma", [0.0, 0.02])
@pytest.mark.parametrize("CL,ld,shift", [(4, 4, 0), (4, 8, 0), (4, 6, 0), (3, 5, 0), (4, 8, 1)])
def test_update_against_the_fp64_restatement(backend, weights, with_score, want_eps, sigma, CL, ld, shift):
    """F = 7, L = 4, S = 2: starts [0, 2, 3] - the last window is clamped; frame 3 lies in three windows, frames 0, 1 and 6
    in one.  (4, 8, shift 1): a one-column-shifted eps window, rows not 8-byte aligned, takes the scalar path."""
    dev = backend
    F, L, ov, H, W = 7, 4, 2, 2, 3
    starts = ops.context_windows(F, L, ov)
    assert [len(cover(f, starts, L)) for f in range(F)] == [1, 1, 2, 3, 2, 2, 1]
    ec, eu, x, score = _inputs(F, L, ov, CL, H, W, ld, dev, seed=100 + ld + shift)
    ecw, euw = ec[:, shift:shift + CL], eu[:, shift:shift + CL]
    sc = score if with_score else None
    coef = 0.9 * (1 - A_T) ** 0.5 if with_score else 0.0
    wt = ops.context_weights(L, weights, device=dev)
    got = ops.cfg_ddim_step_windows(ecw, euw, x, sc, wt, L, ov, CFG, A_T, A_PREV, coef, want_eps=want_eps, sigma=sigma)
    nW = len(starts)
    want, want_e = blend_update_f64(tokens_to_latent(ecw.cpu(), nW, CL, L, H, W), tokens_to_latent(euw.cpu(), nW, CL, L, H, W),
                                    x.cpu(), None if sc is None else sc.cpu(), starts, L, weights64(L, weights), CFG, A_T, A_PREV,
                                    coef, sigma)
    if want_eps:
        _check(got[0], want)
        _check(got[1], want_e)
    else:
        _check(got, want)


@pytest.mark.parametrize("weights", ["triangular", "uniform"])
@pytest.mark.parametrize("with_score", [False, True])
@pytest.mark.parametrize("CL,ld", [(4, 8), (3, 5)])
def test_single_cover_is_the_existing_update_bit_for_bit(backend, weights, with_score, CL, ld):
    """48 x 48 pixels, not the 2 x 3 of the other tests: two kernels that round an intermediate product differently still agree
    on all but about one fp16 output in 2^12 (an fp32 ulp only shows where the value sits next to an fp16 rounding boundary),
    so a bit-for-bit statement needs some 10^5 elements to mean anything"""
    dev = backend
    H, W = 48, 48
    a = dict(cfg=CFG, a_t=A_T, a_prev=A_PREV, score_coef=0.9 * (1 - A_T) ** 0.5 if with_score else 0.0)
    # F = 7, L = 4, S = 2: frames 0, 1 (window 0) and 6 (window 2) have one cover
    F, L, ov = 7, 4, 2
    starts = ops.context_windows(F, L, ov)
    ec, eu, x, score = _inputs(F, L, ov, CL, H, W, ld, dev, seed=7 + ld)
    ec, eu = ec[:, :CL], eu[:, :CL]
    sc = score if with_score else None
    wt = ops.context_weights(L, weights, device=dev)
    got, got_e = ops.cfg_ddim_step_windows(ec, eu, x, sc, wt, L, ov, want_eps=True, sigma=0.02, **a)
    T1 = L * H * W
    seen = 0
    for f in range(F):
        ws = cover(f, starts, L)
        if len(ws) != 1:
            continue
        w = ws[0]
        s = starts[w]
        one, one_e = ops.cfg_ddim_step(ec[w * T1:(w + 1) * T1], eu[w * T1:(w + 1) * T1], x[:, :, s:s + L].contiguous(),
                                       None if sc is None else sc[w:w + 1], want_eps=True, sigma=0.02, **a)
        assert torch.equal(got[:, :, f], one[:, :, f - s]) and torch.equal(got_e[:, :, f], one_e[:, :, f - s])
        seen += 1
    assert seen == 3
    # F = 8, L = 4, S = 4: two disjoint windows - the whole output is the V = 2 batched update
    F, L, ov = 8, 4, 0
    ec, eu, x, score = _inputs(F, L, ov, CL, H, W, ld, dev, seed=11 + ld)
    ec, eu = ec[:, :CL], eu[:, :CL]
    sc = score if with_score else None
    got, got_e = ops.cfg_ddim_step_windows(ec, eu, x, sc, wt, L, ov, want_eps=True, **a)
    x2 = torch.cat([x[:, :, :4], x[:, :, 4:]], 0).contiguous()
    two, two_e = ops.cfg_ddim_step(ec, eu, x2, sc, want_eps=True, **a)
    assert torch.equal(got, torch.cat([two[0:1], two[1:2]], 2)) and torch.equal(got_e, torch.cat([two_e[0:1], two_e[1:2]], 2))


def test_negative_control_multiply_covered_frames_are_a_blend(backend):
    """with random per-window eps, a frame that several windows cover differs from EVERY single window's update by O(1): a
    kernel that took one window (first, last, heaviest) instead of the blend cannot pass the fp64 test above"""
    dev = backend
    F, L, ov, CL, H, W = 7, 4, 2, 4, 2, 3
    starts = ops.context_windows(F, L, ov)
    ec, eu, x, score = _inputs(F, L, ov, CL, H, W, 4, dev, seed=3)
    wt = ops.context_weights(L, "triangular", device=dev)
    coef = 0.9 * (1 - A_T) ** 0.5
    got = ops.cfg_ddim_step_windows(ec, eu, x, score, wt, L, ov, CFG, A_T, A_PREV, coef)
    T1 = L * H * W
    multi = 0
    for f in range(F):
        ws = cover(f, starts, L)
        if len(ws) < 2:
            continue
        for w in ws:
            s = starts[w]
            one = ops.cfg_ddim_step(ec[w * T1:(w + 1) * T1], eu[w * T1:(w + 1) * T1], x[:, :, s:s + L].contiguous(),
                                    score[w:w + 1], CFG, A_T, A_PREV, coef)
            d = (got[:, :, f].float() - one[:, :, f - s].float())
            assert d.abs().max() > 50 * 2e-2 and d.norm() / one[:, :, f - s].float().norm() > 0.1
        multi += 1
    assert multi == 4


def test_entries_reject_bad_shapes(emu_device):
    h = lib.load() if lib._lib is None else lib._lib
    z = torch.zeros(4096, dtype=torch.float16)
    wt = torch.ones(32, dtype=torch.float32)
    p = z.data_ptr()

    def upd(nW, CL, F, L, S, HW, ld, wtp=wt.data_ptr()):
        return h.mc_cfg_ddim_step_windows_f16(p, p, ld, p, None, wtp, p, None, 1.0, 1.0, 0.0, 1.0, 0.0, 0.0, nW, CL, F, L, S, HW, None)

    def gat(nW, CL, F, L, S, HW):
        return h.mc_latent_windows_f16(p, p, nW, CL, F, L, S, HW, None)
    assert upd(3, 4, 7, 4, 2, 6, 4) == 0 and gat(3, 4, 7, 4, 2, 6) == 0
    assert upd(2, 4, 7, 4, 2, 6, 4) == -1 and gat(2, 4, 7, 4, 2, 6) == -1          # nW does not follow from (F, L, S)
    assert upd(3, 4, 7, 4, 2, 6, 3) == -1                                          # ld < CL
    assert upd(3, 4, 7, 4, 2, 6, 4, None) == -1                                    # no weight table
    assert upd(3, 0, 7, 4, 2, 6, 4) == -1 and gat(3, 0, 7, 4, 2, 6) == -1
    assert upd(3, 4, 7, 4, 2, 0, 4) == -1 and gat(3, 4, 7, 4, 2, 0) == -1
    assert upd(1, 4, 3, 4, 2, 6, 4) == -1 and gat(1, 4, 3, 4, 2, 6) == -1          # F < L
    assert upd(3, 4, 7, 4, 0, 6, 4) == -1 and gat(3, 4, 7, 4, 0, 6) == -1          # stride 0
    assert upd(2, 4, 7, 4, 5, 6, 4) == -1 and gat(2, 4, 7, 4, 5, 6) == -1          # stride > L leaves frames uncovered
    assert upd(2, 4, 34, 33, 1, 1, 4) == -1 and gat(2, 4, 34, 33, 1, 1) == -1      # L > 32
    assert upd(34, 4, 34, 1, 1, 1, 4) == -1 and gat(34, 4, 34, 1, 1, 1) == -1      # nW > 32
    with pytest.raises(ValueError):
        ops.cfg_ddim_step_windows(z[:16].reshape(4, 4), z[:16].reshape(4, 4), z[:7 * 4 * 6].reshape(1, 4, 7, 2, 3), None,
                                  wt[:4], 4, 2, 7.5, 0.5, 0.6, 0.0)
    with pytest.raises(ValueError):
        ops.context_weights(4, "gaussian")
