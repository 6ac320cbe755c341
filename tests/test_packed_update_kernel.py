"""mc_cfg_ddim_step_batched_f16: the fused CFG + DDIM update for V videos in ONE launch.  For every video the batched call
must be BIT-IDENTICAL to the one-video entry (mc_cfg_ddim_step_f16) on that video's rows: same coefficients, same
per-element arithmetic and order, only the indexing differs."""
import ctypes

import pytest
import torch

from motionclone_amd import lib, ops


def _inputs(V, CL, F, H, W, ld, dev, seed):
    g = torch.Generator().manual_seed(seed)
    T = V * F * H * W
    ec = torch.randn(T, ld, generator=g).half().to(dev)
    eu = torch.randn(T, ld, generator=g).half().to(dev)
    x = torch.randn(V, CL, F, H, W, generator=g).half().to(dev)
    score = (1e-3 * torch.randn(V, CL, F, H, W, generator=g)).float().to(dev)
    return ec, eu, x, score


@pytest.mark.parametrize("V", [1, 2, 5])
@pytest.mark.parametrize("with_score", [False, True])
@pytest.mark.parametrize("want_eps", [False, True])
@pytest.mark.parametrize("sigma", [0.0, 0.02])
@pytest.mark.parametrize("CL,ld", [(4, 4), (4, 8), (4, 6), (3, 5)])   # vector rows, wider vector rows, unaligned rows, CL != 4
def test_batched_update_equals_the_one_video_update_bit_for_bit(backend, V, with_score, want_eps, sigma, CL, ld):
    dev = backend
    F, H, W = 3, 4, 5
    ec, eu, x, score = _inputs(V, CL, F, H, W, ld, dev, seed=1000 + 7 * V + ld)
    ec, eu = ec[:, :CL], eu[:, :CL]            # column windows of the wider rows
    sc = score if with_score else None
    a_t, a_prev, cfg = 0.61, 0.72, 7.5
    coef = 0.9 * (1 - a_t) ** 0.5 if with_score else 0.0
    got = ops.cfg_ddim_step(ec, eu, x, sc, cfg, a_t, a_prev, coef, want_eps=want_eps, sigma=sigma)
    T1 = F * H * W
    for v in range(V):
        one = ops.cfg_ddim_step(ec[v * T1:(v + 1) * T1], eu[v * T1:(v + 1) * T1], x[v:v + 1],
                                None if sc is None else sc[v:v + 1], cfg, a_t, a_prev, coef, want_eps=want_eps, sigma=sigma)
        if want_eps:
            assert torch.equal(got[0][v:v + 1], one[0]) and torch.equal(got[1][v:v + 1], one[1])
        else:
            assert torch.equal(got[v:v + 1], one)
    out = got[0] if want_eps else got
    assert out.shape == x.shape and torch.isfinite(out.float()).all()
    if sigma:      # sigma changes the direction coefficient: not the eta = 0 update
        plain = ops.cfg_ddim_step(ec, eu, x, sc, cfg, a_t, a_prev, coef)
        assert not torch.equal(out, plain)


def test_batched_entry_against_the_formula_and_the_unaligned_pointer_path(backend):
    """fp32 restatement of the update (the batched entry is not only self-consistent), and eps rows that start at an address
    that is not 8-byte aligned (a one-column-shifted window) take the scalar loads: same values"""
    dev = backend
    V, CL, F, H, W, ld = 2, 4, 2, 3, 3, 8
    ec, eu, x, score = _inputs(V, CL, F, H, W, ld, dev, seed=5)
    a_t, a_prev, cfg, coef = 0.5, 0.8, 7.5, 0.3
    al = ops.cfg_ddim_step(ec[:, :CL], eu[:, :CL], x, score, cfg, a_t, a_prev, coef)
    un = ops.cfg_ddim_step(ec[:, 1:1 + CL], eu[:, 1:1 + CL], x, score, cfg, a_t, a_prev, coef)
    for win, got in ((slice(0, CL), al), (slice(1, 1 + CL), un)):
        c = ec[:, win].float().reshape(V, F, H, W, CL).permute(0, 4, 1, 2, 3)
        u = eu[:, win].float().reshape(V, F, H, W, CL).permute(0, 4, 1, 2, 3)
        eps = c + cfg * (c - u)
        x0 = (x.float() - (1 - a_t) ** 0.5 * eps) / a_t ** 0.5
        want = a_prev ** 0.5 * x0 + (1 - a_prev) ** 0.5 * (eps - coef * score)
        assert (got.float() - want).abs().max() < 2e-2
        assert ((got.float() - want).norm() / want.norm()) < 1e-3
    with pytest.raises(ValueError):
        ops.cfg_ddim_step(ec[:-1, :CL], eu[:-1, :CL], x, None, cfg, a_t, a_prev, 0.0)
    with pytest.raises(ValueError):
        ops.cfg_ddim_step(ec[:, :CL], eu[:, :CL], x, score[:1], cfg, a_t, a_prev, coef)


def test_batched_entry_rejects_bad_shapes(emu_device):
    h = lib.load() if lib._lib is None else lib._lib
    fn = h.mc_cfg_ddim_step_batched_f16
    z = torch.zeros(64, dtype=torch.float16)
    args = lambda V, CL, F, HW, ld: (z.data_ptr(), z.data_ptr(), ld, z.data_ptr(), None, z.data_ptr(), None,   # noqa: E731
                                     1.0, 1.0, 0.0, 1.0, 0.0, 0.0, V, CL, F, HW, None)
    assert fn(*args(0, 4, 1, 1, 4)) == -1 and fn(*args(1, 4, 1, 1, 3)) == -1 and fn(*args(1, 4, 0, 1, 4)) == -1
    assert fn(*args(2, 4, 2, 2, 4)) == 0


def test_index_arithmetic_is_64_bit():
    """A shape whose element count crosses 2^31 (V * CL * F * HW = 2^32 halfs = 8 GiB per operand) does not fit the
    simulator's time or memory budget, so the kernel's index arithmetic is restated on the host: token tok = (v F + f) HW + p
    reads row tok (offset tok * ld) and writes (v, c, f, p) at ((v CL + c) F + f) HW + p.  Python integers do not wrap; the
    kernel computes the same expressions in long / size_t, and the launch wrapper forms V * F * HW in long."""
    V, CL, F, HW, ld = 40, 4, 32, 128 * 128, 320     # 40 videos of config-5 size inside a 320-wide token matrix
    tokens = V * F * HW
    assert tokens * ld > 2 ** 31 and V * CL * F * HW > 2 ** 26
    for tok in (0, 1, HW - 1, HW, F * HW - 1, F * HW, tokens // 2 + 12345, tokens - 1):
        p, r = tok % HW, tok // HW
        f, v = r % F, r // F
        dst = ((v * CL) * F + f) * HW + p
        assert 0 <= dst < V * CL * F * HW
        assert dst + (CL - 1) * F * HW < V * CL * F * HW
        # the one-video entry on video v's rows addresses the same element
        src_one = (f * HW + p) * ld
        assert v * F * HW * ld + src_one == tok * ld
        for c in range(CL):
            idx_one = (c * F + f) * HW + p           # cfg_ddim_kernel's idx for (c, f, p)
            assert v * CL * F * HW + idx_one == dst + c * F * HW
    # the widest intermediate of the wrapper and the kernel fits 63 bits with room to spare
    assert tokens * ld * 2 < 2 ** 62
    assert ctypes.sizeof(ctypes.c_long) == 8 and ctypes.sizeof(ctypes.c_size_t) == 8
