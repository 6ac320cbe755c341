"""BASELINE config 4's shape (i2v_rgb + SparseCtrl, 16 f x 512^2, schedule (30, 12, 0.3)) with V = 3 videos in ONE launch
sequence, every video with its own condition image, against the fp32 oracle run per video ON THE MI355X: the batched
extraction, one guided step, the switch step (first plain one) and the last step.  Bounds: those of the one-video config-4
cases of tests/test_fullsize_parity.py (parity_util: latents / eps TOL_FWD, gradient TOL_GRAD_FULLSIZE, arg-max flips ties at
TIE_GAP on at most MAX_FLIP_FRACTION of the rows, values 5e-3)."""
import pytest
import torch

import parity_util as PU
from motionclone_amd import spec
from motionclone_amd.engine import ControlNetEngine, UNet3DEngine, default_config
from motionclone_amd.sampler import MotionCloneSampler
from oracle import guidance_ref as G
from oracle import unet3d_ref as U

pytestmark = pytest.mark.gpu


def test_three_videos_packed_config4_against_the_oracle():
    from motionclone_amd import lib
    lib._lib = None
    lib._is_emulated = False
    lib.load()
    dev = torch.device("cuda:0")
    cfg = default_config()
    sd, _ = spec.synthetic_state_dict(cfg, seed=1234, device=dev)
    csd = spec.synthetic_controlnet_state_dict(cfg, seed=4321, device=dev)
    eng, ceng = UNet3DEngine(sd, cfg, dev), ControlNetEngine(csd, cfg, dev)
    sdo, csdo = PU.oracle_weights(sd, dev), PU.oracle_weights(csd, dev)
    V, F, H, W = 3, 16, 64, 64
    N, Gs, gs = 30, 12, 0.3
    smp = MotionCloneSampler(eng, num_inference_steps=N, guidance_steps=Gs, guidance_scale=gs, controlnet=ceng, **PU.HP)
    ts = G.uneven_timesteps(N, Gs, gs)
    hp = dict(PU.HP, guidance_steps=Gs)
    scale = 1.0
    vids = []
    for v in range(V):
        g = torch.Generator(device=dev).manual_seed(3000 + v)
        lat = torch.randn((1, 4, F, H, W), generator=g, device=dev).half()
        text = torch.randn((2, 77, cfg["cross_attention_dim"]), generator=g, device=dev).half()
        vid = (0.18215 * torch.randn((1, 4, F, H, W), generator=g, device=dev)).half()
        noise = torch.randn((1, 4, F, H, W), generator=g, device=dev).half()
        cond, mask = torch.zeros_like(vid), torch.zeros_like(vid[:, :1])
        cond[:, :, 0] = (0.18215 * torch.randn((1, 4, H, W), generator=g, device=dev)).half()
        mask[:, :, 0] = 1
        vids.append((lat, text, vid, noise, cond, mask))
    ctrl = dict(cond=torch.cat([v[4] for v in vids], 0), mask=torch.cat([v[5] for v in vids], 0), scale=scale)
    lat3 = torch.cat([v[0] for v in vids], 0)
    text3 = torch.cat([v[1][0:1] for v in vids] + [v[1][1:2] for v in vids], 0)

    def residuals(v, shape, t, text):
        with torch.no_grad(), PU.oracle_mode(dev):
            return U.controlnet_forward(csdo, cfg, shape, t, text.float(), vids[v][4].float(), vids[v][5].float(), scale)

    # ---- batched extraction: every video's top-1 against ITS oracle maps --------------------------------------------------
    reps = smp.extract(torch.cat([v[2] for v in vids], 0), torch.cat([v[3] for v in vids], 0),
                       torch.cat([v[1][0:1] for v in vids], 0), add_noise_step=400, ctrl=ctrl)
    assert len(reps) == V
    rep_refs = []
    for v, (lat, text, vid, noise, _, _) in enumerate(vids):
        noisy = smp.add_noise(400, vid, noise).float()
        dr, mr = residuals(v, noisy.shape, 400, text[0:1])
        rec = {}
        with torch.no_grad(), PU.oracle_mode(dev):
            U.unet_forward(sdo, cfg, noisy, 400, text[0:1].float(), only_motion_feature=True, record=rec, down_residuals=dr,
                           mid_residual=mr)
            prob = G.temp_attn_prob(rec, cfg["motion_heads"])
        rep_refs.append(G.motion_representation(prob))
        flips = total = 0
        worst_gap = worst_val = 0.0
        for k in rep_refs[v]:
            n, tot, gap, dv = PU.flip_stats(reps[v][k][1], reps[v][k][0], prob[k])
            flips, total, worst_gap, worst_val = flips + n, total + tot, max(worst_gap, gap), max(worst_val, dv)
        PU.report("cfg4_packed_v%d" % v, extraction_flips=flips, extraction_rows=total, extraction_flip_max_gap=worst_gap,
                  extraction_value_abs_max_err=worst_val)
        assert worst_gap <= PU.TIE_GAP and worst_val < 5e-3 and flips <= PU.MAX_FLIP_FRACTION * total, (v, flips, total, worst_gap)
        del rec, prob, dr, mr
    rep_cat = eng.prepare_representation(rep_refs)

    # ---- one guided step, the switch step, the last step -------------------------------------------------------------------
    aux = {}
    nxt = smp.step(lat3, 0, text3, rep_cat, aux=aux, ctrl=ctrl)
    T1 = F * H * W
    for v, (lat, text, _, _, _, _) in enumerate(vids):
        d, m = residuals(v, (2, 4, F, H, W), int(ts[0]), text)
        with PU.oracle_mode(dev):
            ref, ref_aux = G.guided_step(sdo, cfg, lat.float(), 0, ts, text.float(), rep_refs[v], hp,
                                         res_u=([t[[0]] for t in d], m[[0]]), res_c=([t[[1]] for t in d], m[[1]]))
        e = dict(latents=PU.rel(nxt[v:v + 1], ref), grad=PU.rel(aux["grad"][v:v + 1], ref_aux["grad"]),
                 eps_c=PU.rel(PU.to_lat(aux["eps_c"][v * T1:(v + 1) * T1], 1, F, H, W), ref_aux["eps_c"]),
                 eps_u=PU.rel(PU.to_lat(aux["eps_u"][v * T1:(v + 1) * T1], 1, F, H, W), ref_aux["eps_u"]))
        PU.report("cfg4_packed_v%d" % v, **{"guided_" + k: x for k, x in e.items()})
        assert e["eps_c"] < PU.TOL_FWD and e["eps_u"] < PU.TOL_FWD and e["latents"] < PU.TOL_FWD, (v, e)
        assert e["grad"] < PU.TOL_GRAD_FULLSIZE, (v, e)
        del d, m, ref, ref_aux
    del aux
    x = nxt
    for i in (Gs, N - 1):
        nx = smp.step(x, i, text3, {}, ctrl=ctrl)
        for v, (_, text, _, _, _, _) in enumerate(vids):
            d, m = residuals(v, (2, 4, F, H, W), int(ts[i]), text)
            with PU.oracle_mode(dev):
                ref, _ = G.plain_step_full(sdo, cfg, x[v:v + 1].float(), i, ts, text.float(), PU.HP["cfg_scale"], res=(d, m))
            e = PU.rel(nx[v:v + 1], ref)
            PU.report("cfg4_packed_v%d" % v, **{"plain_step_%d_latents" % i: e})
            assert e < PU.TOL_FWD, (i, v, e)
            del d, m, ref
        x = nx
    torch.cuda.empty_cache()
