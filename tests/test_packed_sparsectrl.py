"""Several videos per step with SparseCtrl (image-to-video) and with batch_guided=False: the packed encoder, the packed
guided / plain / last step, the batched extraction and the interleaved loop with one condition per video - each video against
its own V = 1 run and against the fp32 oracle.

Bounds (none chosen here): encoder / step against the oracle 2e-2 (latents, residuals) and 5e-2 (gradient) as in
tests/test_sparsectrl.py; batched against alone 2e-3 (latents, residuals) and 2e-2 (gradient) as in
tests/test_engine_parity.py::test_videos_batched_in_one_launch_sequence_match_their_separate_steps; the loop 5e-3 as there."""
import pytest
import torch

from motionclone_amd import lib
from motionclone_amd.engine import ControlNetEngine, UNet3DEngine, split_residuals
from motionclone_amd.sampler import MotionCloneSampler, batch_ctrl, sample_interleaved
from oracle import guidance_ref as G
from oracle import unet3d_ref as U
from parity_util import MAX_FLIP_FRACTION, TIE_GAP

HP = dict(cfg_scale=7.5, motion_guidance_weight=2000.0, warm_up_steps=10, cool_up_steps=10)
TOL_ORACLE, TOL_ORACLE_GRAD = 2e-2, 5e-2        # tests/test_sparsectrl.py
TOL_ALONE, TOL_ALONE_GRAD, TOL_LOOP = 2e-3, 2e-2, 5e-3   # tests/test_engine_parity.py


def rel(a, b):
    return ((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm().clamp_min(1e-12)).item()


def tok(t):  # [B, C, F, H, W] -> tokens
    return t.permute(0, 2, 3, 4, 1).reshape(-1, t.shape[1])


def rows(t, b, B):
    n = t.shape[0] // B
    return t[b * n:(b + 1) * n]


def latent_conds(V, F, H, W):
    """one condition image per video (its VAE latent, synthetic) on frame 0 - and on the last frame too for odd videos"""
    cond = torch.zeros(V, 4, F, H, W)
    mask = torch.zeros(V, 1, F, H, W)
    for v in range(V):
        g = torch.Generator().manual_seed(40 + v)
        cond[v, :, 0] = 0.18215 * torch.randn(4, H, W, generator=g)
        mask[v, :, 0] = 1
        if v % 2:
            cond[v, :, F - 1] = 0.18215 * torch.randn(4, H, W, generator=g)
            mask[v, :, F - 1] = 1
    return cond.half().float(), mask


def pixel_conds(V, F, H, W):
    cond = torch.zeros(V, 3, F, H, W)
    mask = torch.zeros(V, 1, F, H, W)
    for v in range(V):
        cond[v, :, 0] = torch.rand(3, H, W, generator=torch.Generator().manual_seed(50 + v))
        mask[v, :, 0] = 1
    return cond.half().float(), mask


def videos(cfg, V, F, H, W, dev):
    out = []
    for v in range(V):
        g = torch.Generator().manual_seed(200 + v)
        lat = torch.randn(1, 4, F, H, W, generator=g).half()
        text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=g).half()
        vid = (0.18215 * torch.randn(1, 4, F, H, W, generator=g)).half()
        noise = torch.randn(1, 4, F, H, W, generator=g).half()
        out.append(tuple(t.to(dev) for t in (lat, text, vid, noise)))
    return out


def pack_text(vids):
    return torch.cat([v[1][0:1] for v in vids] + [v[1][1:2] for v in vids], 0)


@pytest.fixture(scope="module")
def tiny():
    cfg = dict(U.TINY_CONFIG)
    sd = {k: v.half().float() for k, v in U.random_state_dict(cfg, seed=1234).items()}
    csd = {k: v.half().float() for k, v in U.random_controlnet_state_dict(cfg).items()}
    return cfg, sd, csd


# ---- 2. encoder ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pixel", [False, True])
@pytest.mark.parametrize("share_prefix", [True, False])
def test_packed_encoder_matches_oracle_and_its_own_one_video_runs(backend, tiny, pixel, share_prefix):
    dev = backend
    cfg, _, csd = tiny
    V, F, H, W = 2, 2, 8, 8
    if pixel:
        csd = {k: v.half().float() for k, v in U.random_controlnet_state_dict(cfg, conditioning_channels=3,
                                                                                simplified=False).items()}
        cond, mask = pixel_conds(V, F, 8 * H, 8 * W)
    else:
        cond, mask = latent_conds(V, F, H, W)
    assert not torch.equal(cond[0], cond[1])
    vids = videos(cfg, V, F, H, W, dev)
    text = pack_text(vids)
    ceng = ControlNetEngine(csd, cfg, dev)
    ceng.share_prefix = share_prefix
    scale, t = 0.8, 500
    down, mid = ceng.forward((2 * V, 4, F, H, W), t, text, cond.half().to(dev), mask.half().to(dev), scale)
    assert len(down) == 12
    worst_o = worst_a = 0.0
    for v in range(V):
        tv = vids[v][1]
        with torch.no_grad():
            d_ref, m_ref = U.controlnet_forward(csd, cfg, (2, 4, F, H, W), t, tv.float().cpu(), cond[v:v + 1], mask[v:v + 1], scale)
        d1, m1 = ceng.forward((2, 4, F, H, W), t, tv, cond[v:v + 1].half().to(dev), mask[v:v + 1].half().to(dev), scale)
        for half, b in ((0, v), (1, V + v)):          # [u_1 .. u_V | c_1 .. c_V]
            for a, r, o in zip(down + [mid], d_ref + [m_ref], d1 + [m1]):
                e_o, e_a = rel(rows(a, b, 2 * V), tok(r[[half]])), rel(rows(a, b, 2 * V), rows(o, half, 2))
                worst_o, worst_a = max(worst_o, e_o), max(worst_a, e_a)
                assert e_o < TOL_ORACLE, (v, half, e_o)
                assert e_a < TOL_ALONE, (v, half, e_a)
    print("packed encoder pixel=%s share=%s: worst vs oracle %.3e, vs alone %.3e" % (pixel, share_prefix, worst_o, worst_a))
    # the u half [0, V) and the c half [V, 2 V) as ranges
    du, mu = split_residuals(down, mid, 0, 2 * V, V)
    dc, mc = split_residuals(down, mid, V, 2 * V, V)
    assert all(torch.equal(torch.cat([a, b], 0), d) for a, b, d in zip(du, dc, down)) and torch.equal(torch.cat([mu, mc], 0), mid)
    assert torch.equal(split_residuals(down, mid, 1, 2 * V)[1], rows(mid, 1, 2 * V))
    # [1, ...] condition with V > 1 = the same condition for every video
    b1, bm = ceng.forward((2 * V, 4, F, H, W), t, text, cond[:1].half().to(dev), mask[:1].half().to(dev), scale)
    r1, rm = ceng.forward((2 * V, 4, F, H, W), t, text, cond[:1].expand(V, -1, -1, -1, -1).half().to(dev),
                          mask[:1].half().to(dev), scale)
    assert all(torch.equal(a, b) for a, b in zip(b1 + [bm], r1 + [rm]))
    with pytest.raises(ValueError, match="conditions for a batch"):
        ceng.forward((6, 4, F, H, W), t, torch.cat([text, text[:2]], 0), cond.half().to(dev), mask.half().to(dev), scale)


# ---- 3. steps ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch_guided", [True, False])
def test_packed_steps_with_one_condition_per_video(backend, tiny, batch_guided):
    """Guided step, plain step and last step of V = 2 videos with their own condition images in ONE launch sequence: each
    video against its separate V = 1 step (2e-3 latents, 2e-2 gradient), one video against the oracle with injected residuals
    (2e-2 / 5e-2), and the negative control: with the two conditions swapped the result moves away by more than the bound."""
    dev = backend
    cfg, sd, csd = tiny
    V, F, H, W = 2, 4, 8, 8
    N, Gs, gs = 4, 2, 0.3
    ts = G.uneven_timesteps(N, Gs, gs)
    eng = UNet3DEngine(sd, cfg, dev)
    ceng = ControlNetEngine(csd, cfg, dev)
    smp = MotionCloneSampler(eng, num_inference_steps=N, guidance_steps=Gs, guidance_scale=gs, controlnet=ceng,
                             batch_guided=batch_guided, **HP)
    vids = videos(cfg, V, F, H, W, dev)
    cond, mask = latent_conds(V, F, H, W)
    scale = 0.8
    ctrls = [dict(cond=cond[v:v + 1].half().to(dev), mask=mask[v:v + 1].half().to(dev), scale=scale) for v in range(V)]
    ctrl2 = batch_ctrl(ctrls, V)
    swapped = batch_ctrl(ctrls[::-1], V)
    assert ctrl2["cond"].shape[0] == V and ctrl2["scale"] == scale
    reps = [smp.extract(vid, noise, text[0:1], ctrl=ctrls[v]) for v, (_, text, vid, noise) in enumerate(vids)]
    rep_devs = [eng.prepare_representation(r) for r in reps]
    rep_cat = eng.prepare_representation(reps)
    lat2 = torch.cat([v[0] for v in vids], 0)
    text2 = pack_text(vids)
    for i in (0, Gs, N - 1):                      # guided, plain, last
        aux2 = {}
        nxt2 = smp.step(lat2, i, text2, rep_cat, aux=aux2, ctrl=ctrl2)
        assert nxt2.shape == lat2.shape
        nxt_sw = smp.step(lat2, i, text2, rep_cat, ctrl=swapped)
        for v, (lat, text, _, _) in enumerate(vids):
            aux1 = {}
            nxt1 = smp.step(lat, i, text, rep_devs[v], aux=aux1, ctrl=ctrls[v])
            e = rel(nxt2[v:v + 1], nxt1)
            print("step %d video %d batch_guided=%s: latents vs alone %.3e" % (i, v, batch_guided, e), end="")
            assert e < TOL_ALONE, (i, v, e)
            if i < Gs:
                eg = rel(aux2["grad"][v:v + 1], aux1["grad"])
                print("  gradient vs alone %.3e" % eg, end="")
                assert eg < TOL_ALONE_GRAD, (i, v, eg)
            moved = rel(nxt_sw[v:v + 1], nxt1)
            print("  swapped conditions %.3e" % moved)
            assert moved > TOL_ALONE, "the conditions are ignored: swapped result %.3e from the right one" % moved
            if v == 1:    # against the oracle, residuals of this video's own condition injected
                with torch.no_grad():
                    d, m = U.controlnet_forward(csd, cfg, (2, 4, F, H, W), int(ts[i]), text.float().cpu(), cond[v:v + 1],
                                                mask[v:v + 1], scale)
                if i < Gs:
                    rep_cpu = {k: [a.float().cpu(), b.cpu()] for k, (a, b) in reps[v].items()}
                    ref, ref_aux = G.guided_step(sd, cfg, lat.float().cpu(), i, ts, text.float().cpu(), rep_cpu,
                                                 dict(HP, guidance_steps=Gs), res_u=([t[[0]] for t in d], m[[0]]),
                                                 res_c=([t[[1]] for t in d], m[[1]]))
                    assert rel(aux2["grad"][v:v + 1], ref_aux["grad"]) < TOL_ORACLE_GRAD
                else:
                    ref, _ = G.plain_step_full(sd, cfg, lat.float().cpu(), i, ts, text.float().cpu(), HP["cfg_scale"], res=(d, m))
                assert rel(nxt2[v:v + 1], ref) < TOL_ORACLE
    # shape errors stay errors
    with pytest.raises(ValueError, match="text must hold"):
        smp.step(lat2, 0, text2[:2], rep_cat, ctrl=ctrl2, aux={})
    bad = dict(cond=torch.cat([ctrl2["cond"], ctrl2["cond"][:1]], 0), mask=torch.cat([ctrl2["mask"], ctrl2["mask"][:1]], 0))
    with pytest.raises(ValueError, match="condition batch must be 1"):
        smp.step(lat2, 0, text2, rep_cat, ctrl=bad, aux={})
    with pytest.raises(ValueError, match="one conditioning scale"):
        batch_ctrl([ctrls[0], dict(ctrls[1], scale=0.5)], V)


# ---- 4. extraction ----------------------------------------------------------------------------------------------------------
def test_batched_extraction_equals_the_per_video_extraction(backend, tiny):
    """ONE partial forward + one top-1 launch per hooked attention for V videos against V separate extractions.

    Which case applies: the GEMM tile / split-K choice follows the row count, so the q / k rows of the batched forward may
    differ from the one-video forward in fp32 summation order - bit equality of the values is NOT derivable.  The check
    therefore is: values within 2 fp16 ulps of the V = 1 run; indices may differ only on rows whose top-2 gap in the fp32
    oracle's P is below the 5e-4 tie bound of the full-size tests, and on no more than the share those tolerate (0.5 %).
    Measured (tiny UNet, V = 2, with and without SparseCtrl) on the host simulator: 0 of 192 rows differ in index, largest
    value deviation 0 ulps (the tiny shapes take the same tiles at V times the rows, so the result is bit-identical
    there).  The test prints the share it finds on every run."""
    dev = backend
    cfg, sd, csd = tiny
    V, F, H, W = 2, 2 if dev.type == "cpu" else 4, 8, 8
    eng = UNet3DEngine(sd, cfg, dev)
    ceng = ControlNetEngine(csd, cfg, dev)
    smp = MotionCloneSampler(eng, num_inference_steps=4, guidance_steps=2, guidance_scale=0.3, controlnet=ceng, **HP)
    vids = videos(cfg, V, F, H, W, dev)
    cond, mask = latent_conds(V, F, H, W)
    ctrls = [dict(cond=cond[v:v + 1].half().to(dev), mask=mask[v:v + 1].half().to(dev), scale=0.8) for v in range(V)]
    for ctrl_list in (None, ctrls):
        launches = []
        orig = lib.call
        lib.call = lambda name, *a: (launches.append(name), orig(name, *a))[1]
        try:
            got = smp.extract(torch.cat([v[2] for v in vids], 0), torch.cat([v[3] for v in vids], 0),
                              torch.cat([v[1][0:1] for v in vids], 0), ctrl=None if ctrl_list is None else batch_ctrl(ctrl_list, V))
        finally:
            lib.call = orig
        assert isinstance(got, list) and len(got) == V
        assert launches.count("mc_tattn_top1_f16") == len(eng.hooked_names())       # one launch per hooked attention, not V
        diff_rows = total_rows = worst_ulp = 0
        for v, (_, text, vid, noise) in enumerate(vids):
            c = None if ctrl_list is None else ctrl_list[v]
            one = smp.extract(vid, noise, text[0:1], ctrl=c)
            noisy = smp.add_noise(400, vid, noise).float().cpu()
            with torch.no_grad():
                dr = mr = None
                if c is not None:
                    dr, mr = U.controlnet_forward(csd, cfg, noisy.shape, 400, text[0:1].float().cpu(), cond[v:v + 1], mask[v:v + 1], 0.8)
                rec = {}
                U.unet_forward(sd, cfg, noisy, 400, text[0:1].float().cpu(), only_motion_feature=True, record=rec,
                               down_residuals=dr, mid_residual=mr)
                prob = G.temp_attn_prob(rec, cfg["motion_heads"])
            assert list(got[v]) == list(one) == eng.hooked_names()
            for k in one:
                (bv, bi), (ov, oi) = got[v][k], one[k]
                assert bv.shape == ov.shape and bi.dtype == torch.uint8 and bi.shape == oi.shape
                ulp = (bv.cpu().view(torch.int16).int() - ov.cpu().view(torch.int16).int()).abs()   # positive fp16: ordered bits
                mism = (bi != oi).cpu()
                worst_ulp = max(worst_ulp, int(ulp[~mism].max()))
                assert int(ulp[~mism].max()) <= 2, (k, int(ulp.max()))
                if mism.any():     # a differing index must be a tie in the oracle's P: its top-2 gap below the tie bound
                    top2 = torch.topk(prob[k], k=2, dim=-1).values
                    gap = (top2[..., 0:1] - top2[..., 1:2])[mism]
                    assert float(gap.max()) < TIE_GAP, (k, float(gap.max()))
                diff_rows += int(mism.sum())
                total_rows += mism.numel()
                assert (bv.float().cpu() - prob[k].max(-1, keepdim=True).values).abs().max() < 5e-3   # and against the oracle
        print("batched extraction ctrl=%s: %d of %d rows differ in index, largest value deviation %d ulps"
              % (ctrl_list is not None, diff_rows, total_rows, worst_ulp))
        assert diff_rows <= MAX_FLIP_FRACTION * total_rows, (diff_rows, total_rows)


# ---- 5. loop ----------------------------------------------------------------------------------------------------------------
def test_interleaved_loop_with_one_condition_per_video(backend, tiny):
    dev = backend
    cfg, sd, csd = tiny
    V, F, H, W = 2, 2 if dev.type == "cpu" else 4, 8, 8
    eng = UNet3DEngine(sd, cfg, dev)
    ceng = ControlNetEngine(csd, cfg, dev)

    def mk():
        return MotionCloneSampler(eng, num_inference_steps=2, guidance_steps=1, guidance_scale=0.3, controlnet=ceng, **HP)
    vids = videos(cfg, V, F, H, W, dev)
    cond, mask = latent_conds(V, F, H, W)
    c0, c1 = [dict(cond=cond[v:v + 1].half().to(dev), mask=mask[v:v + 1].half().to(dev), scale=0.8) for v in range(V)]
    s = mk()
    a = sample_interleaved([s], [list(vids)], ctrl=[[c0, c1]])[0]
    b = sample_interleaved([mk(), mk()], vids, ctrl=[c0, c1])
    a2 = sample_interleaved([s], [list(vids)], ctrl=[batch_ctrl([c0, c1], V)])[0]      # an already batched dict
    assert a.shape[0] == V and torch.equal(a, a2)
    for v in range(V):
        e = rel(a[v:v + 1], b[v])
        print("loop video %d: %.3e" % (v, e))
        assert e < TOL_LOOP, (v, e)
    # one dict for every job still means the same condition everywhere (a batched job broadcasts it)
    same = sample_interleaved([s], [list(vids)], ctrl=c0)[0]
    alone = sample_interleaved([mk()], [vids[1]], ctrl=c0)[0]
    assert rel(same[1:2], alone) < TOL_LOOP
    assert rel(same[1:2], a[1:2]) > TOL_LOOP          # ... which is not video 1's own condition
    with pytest.raises(ValueError, match="ctrl entries"):
        sample_interleaved([s], [list(vids)], ctrl=[c0, c1])
    with pytest.raises(ValueError, match="per-video conditions"):
        sample_interleaved([s], [list(vids)], ctrl=[[c0]])


# ---- 7. V = 1 unchanged -------------------------------------------------------------------------------------------------
def test_one_video_sparsectrl_step_keeps_the_one_video_update_entry(backend, tiny, monkeypatch):
    dev = backend
    cfg, sd, csd = tiny
    F, H, W = 2, 8, 8
    eng = UNet3DEngine(sd, cfg, dev)
    ceng = ControlNetEngine(csd, cfg, dev)
    smp = MotionCloneSampler(eng, num_inference_steps=4, guidance_steps=2, guidance_scale=0.3, controlnet=ceng, **HP)
    (lat, text, vid, noise), = videos(cfg, 1, F, H, W, dev)
    cond, mask = latent_conds(1, F, H, W)
    ctrl = dict(cond=cond.half().to(dev), mask=mask.half().to(dev), scale=0.8)
    rep_dev = eng.prepare_representation(smp.extract(vid, noise, text[0:1], ctrl=ctrl))
    names = []
    orig = lib.call
    monkeypatch.setattr(lib, "call", lambda name, *a: (names.append(name), orig(name, *a))[1])
    for i in (0, 2):
        smp.step(lat, i, text, rep_dev, ctrl=ctrl, aux={})
    assert names.count("mc_cfg_ddim_step_f16") == 2 and "mc_cfg_ddim_step_batched_f16" not in names
    names.clear()
    lat2 = torch.cat([lat, lat], 0)
    smp.step(lat2, 2, torch.cat([text[0:1]] * 2 + [text[1:2]] * 2, 0), {}, ctrl=ctrl, aux={})
    assert names.count("mc_cfg_ddim_step_batched_f16") == 1 and "mc_cfg_ddim_step_f16" not in names
