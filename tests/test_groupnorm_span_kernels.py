"""Video-wide GroupNorm(32)(+SiLU): mc_groupnorm_fwd_span_f16 / _fwd_partial_span_ / _bwd_span_ - the statistics of one
(video, group) span the F frames of the video, as torch.nn.GroupNorm on [B, C, F, H, W] does (reference resnet.py:143-165 with
use_inflated_groupnorm = false).  Reference: torch.nn.functional.group_norm on the 5-D fp32 tensor and its autograd; bounds are
those of tests/test_kernels.py::test_groupnorm_fwd_bwd for the per-frame entries.

The frames of a video get different scales and offsets, so per-frame statistics are wrong by far more than the bound: every
case asserts that negative control (the per-frame entry on the same input misses the reference by more than 5 x the bound)."""
import pytest
import torch
import torch.nn.functional as Fn

from motionclone_amd import lib, ops

FWD_TOL = (1e-2, 5e-3)
BWD_TOL = (1e-2, 1e-2)
SIZES = {"5x7": (5, 7), "32x24": (32, 24)}     # ragged last chunk; several chunks per frame, 144 per video (GPU only)
B_VID, F_VID = 2, 3
FRAME_SCALE = (0.5, 1.0, 2.0)
FRAME_SHIFT = (-1.0, 0.25, 1.5)


def big(dev):
    return dev.type == "cuda"


def rnd(shape, dev, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.float16).to(dev)


def worst(a, b, atol, rtol):
    """largest error in units of the bound atol + rtol |b|"""
    a, b = a.float().cpu(), b.float().cpu()
    assert torch.isfinite(a).all()
    return ((a - b).abs() / (atol + rtol * b.abs())).max().item()


def close(a, b, atol, rtol, what=""):
    w = worst(a, b, atol, rtol)
    print("%s: worst error %.3f of the bound" % (what, w))
    assert w <= 1.0, "%s: worst error %.3f x the bound" % (what, w)


def to_rows(x5):      # [B, C, F, H, W] -> [(b f y x), C]
    return x5.permute(0, 2, 3, 4, 1).reshape(-1, x5.shape[1]).contiguous()


def from_rows(t, B, F, H, W):
    return t.reshape(B, F, H, W, -1).permute(0, 4, 1, 2, 3)


def video(C, H, W, dev, seed):
    """fp16 [B, C, F, H, W] whose frames differ in scale and offset"""
    x = torch.randn((B_VID, C, F_VID, H, W), generator=torch.Generator().manual_seed(seed))
    x = x * torch.tensor(FRAME_SCALE).view(1, 1, F_VID, 1, 1) + torch.tensor(FRAME_SHIFT).view(1, 1, F_VID, 1, 1)
    return x.to(torch.float16).to(dev)


def affine(C, dev):
    gamma = (1 + 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(2))).to(dev)
    beta = (0.1 * torch.randn(C, generator=torch.Generator().manual_seed(3))).to(dev)
    return gamma, beta


_REF = {}


def reference(C, H, W, silu, dev):
    """(x fp16, gamma, beta, dz fp16, fp32 reference output, fp32 reference dx), computed once per (shape, device)"""
    key = (C, H, W, silu, str(dev))
    if key not in _REF:
        x = video(C, H, W, dev, 1)
        gamma, beta = affine(C, dev)
        dz = rnd((B_VID, C, F_VID, H, W), dev, 4)
        xr = x.float().requires_grad_()
        ref = Fn.group_norm(xr, 32, gamma, beta, 1e-5)
        if silu:
            ref = Fn.silu(ref)
        (dref,) = torch.autograd.grad(ref, xr, dz.float())
        _REF[key] = (x, gamma, beta, dz, ref.detach(), dref.detach())
    return _REF[key]


@pytest.mark.parametrize("accumulate", [False, True], ids=["write", "accumulate"])
@pytest.mark.parametrize("C1,C2,silu", [(64, 0, True), (320, 0, False), (64, 128, True), (960, 0, True)])
@pytest.mark.parametrize("size", list(SIZES))
def test_groupnorm_span_fwd_bwd(backend, size, C1, C2, silu, accumulate):
    dev = backend
    if size == "32x24" and not big(dev):
        pytest.skip("32 x 24 tokens per frame (144 chunks per video) is the GPU-sized case")
    H, W = SIZES[size]
    C, hw, frames = C1 + C2, H * W, B_VID * F_VID
    x, gamma, beta, dz, ref, dref = reference(C, H, W, silu, dev)
    xa = to_rows(x[:, :C1])
    xb = to_rows(x[:, C1:]) if C2 else None
    y, stats = ops.gn_fwd(xa, xb, gamma, beta, silu, frames, hw, 1e-5, span=F_VID)
    assert tuple(stats.shape) == (B_VID, 32, 2)
    close(from_rows(y, B_VID, F_VID, H, W), ref, *FWD_TOL, "video-wide gn fwd")
    # the statistics themselves, against fp64 on the stored fp16 values
    xg = x.double().cpu().reshape(B_VID, 32, -1)
    mean, var = xg.mean(-1), xg.var(-1, unbiased=False)
    assert torch.allclose(stats[..., 0].double().cpu(), mean, rtol=1e-4, atol=1e-4)
    assert torch.allclose(stats[..., 1].double().cpu(), (var + 1e-5).rsqrt(), rtol=1e-3, atol=1e-5)
    # negative control: per-frame statistics on the same input are wrong by far more than the bound
    y_pf, st_pf = ops.gn_fwd(xa, xb, gamma, beta, silu, frames, hw, 1e-5)
    miss = worst(from_rows(y_pf, B_VID, F_VID, H, W), ref, *FWD_TOL)
    print("per-frame entry misses the video-wide reference by %.1f x the bound" % miss)
    assert miss > 5.0, miss
    # two runs: identical bits
    y2, stats2 = ops.gn_fwd(xa, xb, gamma, beta, silu, frames, hw, 1e-5, span=F_VID)
    assert torch.equal(y, y2) and torch.equal(stats, stats2)
    # backward
    dzr = to_rows(dz)
    if accumulate:
        base = rnd((frames * hw, C), dev, 5)
        dx = base.clone()
        ops.gn_bwd(xa, xb, dzr, stats, gamma, beta, silu, frames, hw, out=dx, accumulate=True, span=F_VID)
        want = dref + from_rows(base, B_VID, F_VID, H, W).float()
        dx_b = base.clone()
        ops.gn_bwd(xa, xb, dzr, stats, gamma, beta, silu, frames, hw, out=dx_b, accumulate=True, span=F_VID)
        pf = base.clone()
        ops.gn_bwd(xa, xb, dzr, st_pf, gamma, beta, silu, frames, hw, out=pf, accumulate=True)
    else:
        dx = ops.gn_bwd(xa, xb, dzr, stats, gamma, beta, silu, frames, hw, span=F_VID)
        want = dref
        dx_b = ops.gn_bwd(xa, xb, dzr, stats, gamma, beta, silu, frames, hw, span=F_VID)
        pf = ops.gn_bwd(xa, xb, dzr, st_pf, gamma, beta, silu, frames, hw)
    close(from_rows(dx, B_VID, F_VID, H, W), want, *BWD_TOL, "video-wide gn bwd")
    assert torch.equal(dx, dx_b)
    miss = worst(from_rows(pf, B_VID, F_VID, H, W), want, *BWD_TOL)
    print("per-frame backward misses the video-wide reference by %.1f x the bound" % miss)
    assert miss > 5.0, miss


def _p(t):
    return None if t is None else t.data_ptr()


def _ld(t):
    return 0 if t is None else t.stride(0)


def _span_fwd(xa, xb, gamma, beta, silu, frames, hw, span, eps=1e-5):
    """mc_groupnorm_fwd_span_f16 itself (ops.gn_fwd routes span == 1 to the per-frame entry)"""
    c1 = xa.shape[1]
    ctot = c1 + (xb.shape[1] if xb is not None else 0)
    partial = ops.workspace("groupnorm", xa, frames, hw)
    stats = torch.empty((frames // max(span, 1), 32, 2), dtype=torch.float32, device=xa.device)
    out = torch.empty((frames * hw, ctot), dtype=torch.float16, device=xa.device)
    lib.call("mc_groupnorm_fwd_span_f16", _p(xa), _p(xb), _ld(xa), _ld(xb), c1, ctot, frames, hw, span, eps, _p(partial),
             _p(stats), _p(gamma), _p(beta), _p(out), _ld(out), int(silu), ops._stream(xa))
    return out, stats


def _span_bwd(xa, xb, dz, stats, gamma, beta, silu, frames, hw, span):
    c1 = xa.shape[1]
    ctot = c1 + (xb.shape[1] if xb is not None else 0)
    partial = ops.workspace("groupnorm", xa, frames, hw)
    bstats = ops.workspace("groupnorm_bwd_stats_span", xa, frames, span)
    out = torch.empty((frames * hw, ctot), dtype=torch.float16, device=xa.device)
    lib.call("mc_groupnorm_bwd_span_f16", _p(xa), _p(xb), _ld(xa), _ld(xb), c1, ctot, frames, hw, span, _p(dz), _ld(dz),
             _p(stats), _p(gamma), _p(beta), int(silu), _p(partial), _p(bstats), _p(out), _ld(out), 0, ops._stream(xa))
    return out


@pytest.mark.parametrize("C1,C2,silu", [(64, 128, True), (320, 0, False)])
def test_span_one_is_the_per_frame_entry_bit_for_bit(backend, C1, C2, silu):
    dev = backend
    H, W = SIZES["32x24" if big(dev) else "5x7"]
    C, hw, frames = C1 + C2, H * W, B_VID * F_VID
    x, gamma, beta, dz, _, _ = reference(C, H, W, silu, dev)
    xa = to_rows(x[:, :C1])
    xb = to_rows(x[:, C1:]) if C2 else None
    y0, st0 = ops.gn_fwd(xa, xb, gamma, beta, silu, frames, hw, 1e-5)
    y1, st1 = _span_fwd(xa, xb, gamma, beta, silu, frames, hw, 1)
    assert torch.equal(y0, y1) and torch.equal(st0, st1)
    assert lib.workspace_bytes("groupnorm_bwd_stats_span", frames, 1) == lib.workspace_bytes("groupnorm_bwd_stats", frames)
    dx0 = ops.gn_bwd(xa, xb, to_rows(dz), st0, gamma, beta, silu, frames, hw)
    dx1 = _span_bwd(xa, xb, to_rows(dz), st1, gamma, beta, silu, frames, hw, 1)
    assert torch.equal(dx0, dx1)
    # and ops routes span == 1 to the per-frame entries
    y2, st2 = ops.gn_fwd(xa, xb, gamma, beta, silu, frames, hw, 1e-5, span=1)
    assert torch.equal(y0, y2) and torch.equal(st0, st2)


@pytest.mark.parametrize("cfg", [11, 0], ids=["ring64", "library_choice"])
def test_partial_entry_fed_by_the_conv_epilogue(backend, cfg):
    """mc_groupnorm_fwd_partial_span_f16 on the per-(frame, chunk, group) partials that mc_gemm_gnstats_f16 leaves (they are
    per frame: the producer does not know the span) against the statistics-pass entry on the same tensor"""
    dev = backend
    if cfg == 0 and not big(dev):
        pytest.skip("library_choice: at simulator sizes the library's own kernel choice leaves no epilogue statistics")
    span = 3
    frames, hw, N, K = (6, 64, 320, 128) if cfg == 11 else (24, 1024, 320, 640)
    M = frames * hw
    a, w = rnd((M, K), dev, 1), rnd((N, K), dev, 2, 0.1)
    # rows of the frames of a video at different offsets, through the residual
    f_of_row = (torch.arange(M) // hw) % span
    R = (torch.tensor([-2.0, 0.5, 3.0])[f_of_row].view(M, 1) + torch.zeros(M, N)).half().to(dev)
    out, gnp = ops.gemm(a, w, residual=R, cfg=cfg, tileloop=False, gn_hw=hw)
    if gnp is None:
        pytest.skip("library_choice: the library's kernel for this problem leaves no epilogue statistics")
    gamma, beta = affine(N, dev)
    y0, st0 = ops.gn_fwd(out, None, gamma, beta, True, frames, hw, 1e-5, span=span)
    y1, st1 = ops.gn_fwd(out, None, gamma, beta, True, frames, hw, 1e-5, span=span, gnp=gnp)
    assert tuple(st1.shape) == (frames // span, 32, 2)
    close(st1, st0, 1e-5, 1e-5, "statistics from the epilogue vs the statistics pass")
    close(y1, y0, 2e-3, 2e-3, "normalised output")
    x5 = out.float().reshape(frames // span, span, hw, N).permute(0, 3, 1, 2)
    ref = Fn.silu(Fn.group_norm(x5, 32, gamma, beta, 1e-5)).permute(0, 2, 3, 1).reshape(M, N)
    close(y1, ref, *FWD_TOL, "video-wide GroupNorm + SiLU from epilogue statistics vs fp32 torch")
    y_pf, _ = ops.gn_fwd(out, None, gamma, beta, True, frames, hw, 1e-5, gnp=gnp)
    assert worst(y_pf, ref, *FWD_TOL) > 5.0
    y2, st2 = ops.gn_fwd(out, None, gamma, beta, True, frames, hw, 1e-5, span=span, gnp=gnp)
    assert torch.equal(y1, y2) and torch.equal(st1, st2)


def test_bad_span_is_a_shape_error(backend):
    dev = backend
    H, W = SIZES["5x7"]
    x, gamma, beta, dz, _, _ = reference(64, H, W, True, dev)
    xa, frames, hw = to_rows(x), B_VID * F_VID, H * W
    fns = lib.load()
    for span in (0, -1, 4, 5, 7):
        partial = ops.workspace("groupnorm", xa, frames, hw)
        stats = torch.full((frames, 32, 2), 7.0, dtype=torch.float32, device=dev)
        out = torch.full((frames * hw, 64), 3.0, dtype=torch.float16, device=dev)
        st = ops._stream(xa)
        rc = fns.mc_groupnorm_fwd_span_f16(_p(xa), None, 64, 0, 64, 64, frames, hw, span, 1e-5, _p(partial), _p(stats), _p(gamma),
                                           _p(beta), _p(out), 64, 1, st)
        assert rc == -1, (span, rc)
        rc = fns.mc_groupnorm_fwd_partial_span_f16(_p(xa), 64, 64, frames, hw, span, 1e-5, _p(partial), 1, _p(stats), _p(gamma),
                                                   _p(beta), _p(out), 64, 1, st)
        assert rc == -1, (span, rc)
        rc = fns.mc_groupnorm_bwd_span_f16(_p(xa), None, 64, 0, 64, 64, frames, hw, span, _p(to_rows(dz)), 64, _p(stats), _p(gamma),
                                           _p(beta), 1, _p(partial), _p(stats), _p(out), 64, 0, st)
        assert rc == -1, (span, rc)
        assert fns.mc_workspace_bytes_groupnorm_bwd_stats_span(frames, span) == -1
        if big(dev):
            torch.cuda.synchronize()
        assert bool((out == 3.0).all()) and bool((stats == 7.0).all()), "nothing may be launched"
    with pytest.raises(ValueError, match="span"):
        ops.gn_fwd(xa, None, gamma, beta, True, frames, hw, 1e-5, span=4)
    with pytest.raises(ValueError, match="span"):
        ops.gn_bwd(xa, None, to_rows(dz), torch.zeros(1, 32, 2, device=dev), gamma, beta, True, frames, hw, span=4)
