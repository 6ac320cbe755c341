"""Motion composition - several motion references guide one video - through the engine, the sampler, the drop-in API and the
launcher on the tiny UNet3D.

The composed loss is restated here in fp32 torch on top of the oracle's own pieces (oracle/unet3d_ref.py forward,
guidance_ref.temp_attn_prob / ddim_step): per module
    sum_r lambda_r / numel_r * sum(w_r[bn, f] (gather(P, idx_r) - val_r)^2)
with w_r the area mean of reference r's mask (ones without one).  Bounds are those of tests/test_masked_engine.py:
test_guided_step_with_a_half_plane_mask_matches_oracle for the guided step, test_packed_step_with_one_masked_video_equals_the_
separate_steps for packed batches."""
import glob
import json
import os

import pytest
import torch

from motionclone_amd import lanes
from motionclone_amd.engine import UNet3DEngine
from motionclone_amd.sampler import MotionCloneSampler
from oracle import guidance_ref as G
from oracle import reference_shim as shim
from oracle import unet3d_ref as U
from test_dropin_api import build_pipeline
from test_engine_parity import HP, make_inputs, rel_err, to_lat
from test_masked_engine import GRAD_BOUND, oracle_weights

F_, H_, W_ = 4, 8, 8
LAM_B = 0.5


@pytest.fixture
def tiny():
    cfg = dict(U.TINY_CONFIG)
    sd = {k: v.half().float() for k, v in U.random_state_dict(cfg, seed=1234).items()}
    return cfg, sd


def left_mask():
    m = torch.zeros(F_, H_, W_)
    m[:, :, :W_ // 2] = 1.0
    return m


def right_mask():
    return 1.0 - left_mask()


def oracle_rep(sd, cfg, vid, noise, uncond, k):
    """guidance_ref.extract_representation with torch.topk(k) in place of its k = 1"""
    noisy = G.add_noise(G.alphas_cumprod(), 400, vid, noise)
    rec = {}
    with torch.no_grad():
        U.unet_forward(sd, cfg, noisy, 400, uncond, guidance_block=1, only_motion_feature=True, record=rec, hooked=("up_blocks.1",))
        out = {}
        for name, p in G.temp_attn_prob(rec, cfg["motion_heads"]).items():
            v, i = torch.topk(p, k=k, dim=-1)
            out[name] = [v, i.to(torch.uint8)]
    return out


def composed_temp_loss(prob, refs):
    """refs: [(representation, lambda, mask or None)]; every reference keeps its own unweighted mean"""
    total = 0.0
    for name, p in prob.items():
        for rep, lam, mask in refs:
            ref_v, ref_i = rep[name]
            err = (torch.gather(p, index=ref_i.to(torch.int64), dim=-1) - ref_v.to(p.dtype)) ** 2
            w = oracle_weights(mask, p.shape[0]) if mask is not None else torch.ones(p.shape[0], F_)
            total = total + lam * (w[:, None, :, None] * err).sum() / err.numel()
    return total


def oracle_composed_step(sd, cfg, latents, step_index, timesteps, text, refs, hp):
    """guidance_ref.guided_step with the composed loss in place of temp_loss"""
    acp = G.alphas_cumprod()
    t = int(timesteps[step_index])
    control = latents.clone().detach().requires_grad_(True)
    with torch.no_grad():
        eps_u = U.unet_forward(sd, cfg, latents, t, text[[0]])
    rec = {}
    eps_c = U.unet_forward(sd, cfg, control, t, text[[1]], record=rec, hooked=("up_blocks.1",))
    loss = hp["motion_guidance_weight"] * composed_temp_loss(G.temp_attn_prob(rec, cfg["motion_heads"]), refs)
    loss = loss * G.guidance_scale_factor(step_index, hp["guidance_steps"], hp["warm_up_steps"], hp["cool_up_steps"])
    (grad,) = torch.autograd.grad(loss, control)
    eps = eps_c + hp["cfg_scale"] * (eps_c - eps_u)
    nxt = G.ddim_step(acp, timesteps, step_index, eps.detach(), control.detach(), score=grad.detach())
    return nxt.detach(), dict(eps_u=eps_u.detach(), eps_c=eps_c.detach(), loss=loss.detach(), grad=grad.detach())


_ORACLE = {}


def oracle_case(tiny):
    """computed once: reference A (top-1, the example's own) and B (top-2, from other latents), the oracle steps with A on the
    left half alone and with {A on the left half, B on the right half at lambda 0.5}"""
    if not _ORACLE:
        cfg, sd = tiny
        lat, text, vid, noise = make_inputs(cfg)
        lat16, text16 = lat.half(), text.half()
        N, Gs, gscale = 4, 2, 0.3
        hp = dict(HP, guidance_steps=Gs)
        uncond = text16[[0]].float()
        rep_a = oracle_rep(sd, cfg, vid, noise, uncond, 1)
        g = torch.Generator().manual_seed(77)
        vid_b = 0.18215 * torch.randn(1, 4, F_, H_, W_, generator=g)
        rep_b = oracle_rep(sd, cfg, vid_b, torch.randn(1, 4, F_, H_, W_, generator=g), uncond, 2)
        ts = G.uneven_timesteps(N, Gs, gscale)
        a = (sd, cfg, lat16.float(), 0, ts, text16.float())
        _ORACLE.update(rep_a=rep_a, rep_b=rep_b, lat16=lat16, text16=text16, N=N, Gs=Gs, gscale=gscale,
                       only_a=oracle_composed_step(*a, [(rep_a, 1.0, left_mask())], hp),
                       both=oracle_composed_step(*a, [(rep_a, 1.0, left_mask()), (rep_b, LAM_B, right_mask())], hp))
    return _ORACLE


def _sampler(eng, o):
    return MotionCloneSampler(eng, num_inference_steps=o["N"], guidance_steps=o["Gs"], guidance_scale=o["gscale"], **HP)


def _refs_b(o, **kw):
    return [dict(dict(representation=o["rep_b"], weight=LAM_B, mask=right_mask()), **kw)]


def _prepare_both(eng, o):
    return eng.prepare_representation(o["rep_a"], frames=F_, mask=left_mask(), grid=(H_, W_), references=_refs_b(o))


def test_the_second_reference_moves_the_oracle_gradient_well_beyond_the_bound(tiny):
    """a condition on the chosen case, on the CPU: adding B moves the oracle gradient by more than 10 bounds, so a step that
    ignored the second reference could not pass the comparison below; and one reference restated is the oracle's own step"""
    o = oracle_case(tiny)
    apart = rel_err(o["only_a"][1]["grad"], o["both"][1]["grad"])
    print("REFERENCE_SEPARATION %.3f" % apart)
    assert apart > 10 * GRAD_BOUND
    cfg, sd = tiny
    hp = dict(HP, guidance_steps=o["Gs"])
    ts = G.uneven_timesteps(o["N"], o["Gs"], o["gscale"])
    _, plain = G.guided_step(sd, cfg, o["lat16"].float(), 0, ts, o["text16"].float(), o["rep_a"], hp)
    _, again = oracle_composed_step(sd, cfg, o["lat16"].float(), 0, ts, o["text16"].float(), [(o["rep_a"], 1.0, None)], hp)
    assert rel_err(again["grad"], plain["grad"]) < 1e-5


def test_guided_step_with_two_references_matches_oracle(backend, tiny):
    dev = backend
    cfg, sd = tiny
    o = oracle_case(tiny)
    eng = UNet3DEngine(sd, cfg, dev)
    smp = _sampler(eng, o)
    rep_dev = _prepare_both(eng, o)
    for e in rep_dev.values():       # the merged form: K = 1 + 2 slots, weights lambda_r w_r / K_r
        assert len(e) == 3 and e[0].shape[-1] == 3 and e[2].shape == (e[0].shape[0], F_, 3) and e[2].dtype == torch.float32
        wl, wr = oracle_weights(left_mask(), e[0].shape[0]), oracle_weights(right_mask(), e[0].shape[0])
        want = torch.stack([wl, LAM_B * wr / 2, LAM_B * wr / 2], -1)
        assert torch.equal(e[2].cpu(), want)
    aux = {}
    nxt = smp.step(o["lat16"].to(dev), 0, o["text16"].to(dev), rep_dev, aux=aux)
    ref_nxt, ref_aux = o["both"]
    e = dict(eps_c=rel_err(to_lat(aux["eps_c"], 1, F_, H_, W_), ref_aux["eps_c"]),
             eps_u=rel_err(to_lat(aux["eps_u"], 1, F_, H_, W_), ref_aux["eps_u"]),
             loss=abs(aux["loss"].item() - ref_aux["loss"].item()) / abs(ref_aux["loss"].item()),
             grad=rel_err(aux["grad"], ref_aux["grad"]), latents=rel_err(nxt, ref_nxt))
    print("COMPOSED_GUIDED_STEP %s" % e)
    assert e["eps_c"] < 2e-2 and e["eps_u"] < 2e-2
    assert e["loss"] < 3e-2
    assert e["grad"] < GRAD_BOUND, e
    assert e["latents"] < 2e-2


def test_composed_gradient_is_the_sum_of_the_single_reference_gradients(backend, tiny):
    dev = backend
    cfg, sd = tiny
    o = oracle_case(tiny)
    eng = UNet3DEngine(sd, cfg, dev)
    smp = _sampler(eng, o)
    lat, text = o["lat16"].to(dev), o["text16"].to(dev)
    both, only_a, only_b = {}, {}, {}
    smp.step(lat, 0, text, _prepare_both(eng, o), aux=both)
    # the existing masked path, one reference each
    smp.step(lat, 0, text, eng.prepare_representation(o["rep_a"], frames=F_, mask=left_mask(), grid=(H_, W_)), aux=only_a)
    smp.step(lat, 0, text, eng.prepare_representation(o["rep_b"], frames=F_, mask=right_mask(), grid=(H_, W_)), aux=only_b)
    want = only_a["grad"].float() + LAM_B * only_b["grad"].float()
    err = rel_err(both["grad"], want)
    print("LINEARITY %.3e" % err)
    assert err < GRAD_BOUND
    assert rel_err(both["grad"], only_a["grad"]) > 10 * GRAD_BOUND
    l_want = float(only_a["loss"]) + LAM_B * float(only_b["loss"])
    assert abs(float(both["loss"]) - l_want) < 3e-2 * abs(l_want)


def test_a_reference_of_weight_zero_is_the_run_without_it(backend, tiny):
    dev = backend
    cfg, sd = tiny
    o = oracle_case(tiny)
    eng = UNet3DEngine(sd, cfg, dev)
    smp = _sampler(eng, o)
    lat, text = o["lat16"].to(dev), o["text16"].to(dev)
    for kw in (dict(), dict(mask=left_mask(), grid=(H_, W_))):
        plain = eng.prepare_representation(o["rep_a"], frames=F_, **kw)
        zero = eng.prepare_representation(o["rep_a"], frames=F_, references=_refs_b(o, weight=0.0), **kw)
        none = eng.prepare_representation(o["rep_a"], frames=F_, references=[], **kw)
        for other in (zero, none):
            assert list(other) == list(plain)
            for name in plain:
                assert len(other[name]) == len(plain[name]) == (3 if kw else 2)
                assert all(torch.equal(a, b) and a.dtype == b.dtype for a, b in zip(other[name], plain[name]))
        a0, a1 = {}, {}
        x0 = smp.step(lat, 0, text, plain, aux=a0)
        x1 = smp.step(lat, 0, text, zero, aux=a1)
        assert torch.equal(x0, x1) and torch.equal(a0["grad"], a1["grad"]) and torch.equal(a0["loss"], a1["loss"])
    # two references of which one weighs 0: the slots of the other alone
    two = eng.prepare_representation(o["rep_a"], frames=F_, grid=(H_, W_),
                                     references=_refs_b(o, weight=0.0) + _refs_b(o))
    one = eng.prepare_representation(o["rep_a"], frames=F_, grid=(H_, W_), references=_refs_b(o))
    assert all(all(torch.equal(a, b) for a, b in zip(two[n], one[n])) for n in one)


def _packed_videos(dev, cfg, smp, topks):
    vids = []
    for v, k in enumerate(topks):
        g = torch.Generator().manual_seed(100 + v)
        lat = torch.randn(1, 4, F_, H_, W_, generator=g).half().to(dev)
        text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=g).half().to(dev)
        vid = (0.18215 * torch.randn(1, 4, F_, H_, W_, generator=g)).half().to(dev)
        noise = torch.randn(1, 4, F_, H_, W_, generator=g).half().to(dev)
        vids.append((lat, text, smp.extract(vid, noise, text[0:1], topk=k)))
    return vids


def _extra(dev, cfg, smp, seed, k):
    g = torch.Generator().manual_seed(seed)
    vid = (0.18215 * torch.randn(1, 4, F_, H_, W_, generator=g)).half().to(dev)
    noise = torch.randn(1, 4, F_, H_, W_, generator=g).half().to(dev)
    uncond = torch.randn(1, 7, cfg["cross_attention_dim"], generator=g).half().to(dev)
    return smp.extract(vid, noise, uncond, topk=k)


def _check_packed_against_separate(eng, smp, vids, masks, refs):
    reps = [v[2] for v in vids]
    rep_cat = eng.prepare_representation(reps, frames=F_, mask=masks, grid=(H_, W_), references=refs)
    lat2 = torch.cat([v[0] for v in vids], 0)
    text2 = torch.cat([v[1][0:1] for v in vids] + [v[1][1:2] for v in vids], 0)
    aux2 = {}
    nxt2 = smp._step_eager(lat2, 0, text2, rep_cat, aux=aux2)
    l_sep, ones = 0.0, []
    for v, (lat, text, rep) in enumerate(vids):
        aux1 = {}
        one = eng.prepare_representation(rep, frames=F_, mask=masks[v], grid=(H_, W_), references=refs[v])
        ones.append(one)
        nxt1 = smp._step_eager(lat, 0, text, one, aux=aux1)
        l_sep += float(aux1["loss"])
        assert rel_err(nxt2[v:v + 1], nxt1) < 2e-3, (v, rel_err(nxt2[v:v + 1], nxt1))
        assert rel_err(aux2["grad"][v:v + 1], aux1["grad"]) < 2e-2
        assert aux1["grad"].abs().max() > 0
    assert abs(float(aux2["loss"]) - l_sep) < 2e-3 * abs(l_sep)
    return rep_cat, ones


def test_packed_step_with_one_composed_video_equals_the_separate_steps(backend, tiny):
    dev = backend
    cfg, sd = tiny
    eng = UNet3DEngine(sd, cfg, dev)
    smp = MotionCloneSampler(eng, num_inference_steps=3, guidance_steps=2, guidance_scale=0.3, **HP)
    vids = _packed_videos(dev, cfg, smp, (1, 1))
    refs = [[dict(representation=_extra(dev, cfg, smp, 300, 2), weight=LAM_B, mask=right_mask())], None]
    masks = [left_mask(), None]
    rep_cat, ones = _check_packed_against_separate(eng, smp, vids, masks, refs)
    assert len(next(iter(ones[0].values()))) == 3 and len(next(iter(ones[1].values()))) == 2     # alone, video 1 is the plain path
    for e in rep_cat.values():
        n = e[0].shape[0] // 2
        # video 1 has no references: w_0 / K_0 = 1 in its one slot, the rest is padding of weight 0, index 0, value 0
        assert len(e) == 3 and e[0].shape[-1] == 3 and e[2].shape == (2 * n, F_, 3)
        assert (e[2][n:, :, 0] == 1).all() and (e[2][n:, :, 1:] == 0).all()
        assert (e[0][n:, :, :, 1:] == 0).all() and (e[1][n:, :, :, 1:] == 0).all()
    # no references anywhere: today's entries, and today's error for differing top-k
    plain = eng.prepare_representation([v[2] for v in vids], frames=F_, references=[None, None])
    assert all(len(e) == 2 for e in plain.values())
    other = smp.extract(torch.zeros(1, 4, F_, H_, W_).half().to(dev), torch.ones(1, 4, F_, H_, W_).half().to(dev), vids[0][1][0:1], topk=2)
    with pytest.raises(ValueError, match="differ in their top-k"):
        eng.prepare_representation([vids[0][2], other], frames=F_, references=[None, []])


def test_packed_videos_of_two_and_five_slots_are_padded(backend, tiny):
    dev = backend
    cfg, sd = tiny
    eng = UNet3DEngine(sd, cfg, dev)
    smp = MotionCloneSampler(eng, num_inference_steps=3, guidance_steps=2, guidance_scale=0.3, **HP)
    vids = _packed_videos(dev, cfg, smp, (1, 2))
    refs = [[dict(representation=_extra(dev, cfg, smp, 300, 1), weight=2.0)],
            [dict(representation=_extra(dev, cfg, smp, 301, 3), weight=LAM_B, mask=right_mask(), mask_normalize=True)]]
    rep_cat, ones = _check_packed_against_separate(eng, smp, vids, [None, left_mask()], refs)
    assert next(iter(ones[0].values()))[0].shape[-1] == 2 and next(iter(ones[1].values()))[0].shape[-1] == 5
    for name, e in rep_cat.items():
        n = e[0].shape[0] // 2
        assert e[0].shape[-1] == 5 and e[2].shape == (2 * n, F_, 5)
        assert (e[2][:n, :, 2:] == 0).all() and (e[0][:n, :, :, 2:] == 0).all() and (e[1][:n, :, :, 2:] == 0).all()
        assert torch.equal(e[2][:n, :, :2], ones[0][name][2]) and torch.equal(e[2][n:], ones[1][name][2])
        assert (e[2][:n, :, 0] == 1).all() and (e[2][:n, :, 1] == 2).all()


def test_reference_validation_names_the_problem(backend, tiny):
    dev = backend
    cfg, sd = tiny
    o = oracle_case(tiny)
    eng = UNet3DEngine(sd, cfg, dev)
    a, b = o["rep_a"], o["rep_b"]

    def widen(rep, k):
        return {n: [v.expand(-1, -1, -1, k).contiguous(), i.expand(-1, -1, -1, k).contiguous()] for n, (v, i) in rep.items()}
    prep = lambda refs, rep=a, **kw: eng.prepare_representation(rep, frames=F_, grid=(H_, W_), references=refs, **kw)   # noqa: E731
    prep([dict(representation=widen(a, 3)), dict(representation=widen(a, 4))])          # 1 + 3 + 4 = 8 slots fit
    with pytest.raises(ValueError, match=r"sum to 9 slots"):
        prep([dict(representation=widen(a, 4)), dict(representation=widen(a, 4))])
    prep([dict(representation=widen(a, 4)), dict(representation=widen(a, 4), weight=0)])  # dropped before the slots are counted
    foreign = dict(b)
    foreign["down_blocks.0.motion_modules.0.temporal_transformer.transformer_blocks.0.attention_blocks.0"] = foreign.pop(next(iter(b)))
    with pytest.raises(ValueError, match=r"motion reference 1: its modules differ.*foreign \['down_blocks.0"):
        prep([dict(representation=foreign)])
    longer = {n: [torch.cat([v, v], 2), torch.cat([i, i], 2)] for n, (v, i) in b.items()}
    with pytest.raises(ValueError, match="holds 8 frames, the run has 4"):
        prep([dict(representation=longer)])
    with pytest.raises(ValueError, match=r"motion reference 1, .*\[BN = \d+, heads = \d+, F = 4, K\]"):
        eng.prepare_representation(a, references=[dict(representation=longer)])       # the run's F not given: against reference 0
    fewer = {n: [v[:-1], i[:-1]] for n, (v, i) in b.items()}
    with pytest.raises(ValueError, match="motion reference 2, "):
        prep([dict(representation=b), dict(representation=fewer)])
    for w in (-0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="motion reference 1: weight .* negative or not finite"):
            prep([dict(representation=b, weight=w)])
    with pytest.raises(ValueError, match="frames"):
        prep([dict(representation=b, mask=torch.ones(F_ + 1, H_, W_))])
    with pytest.raises(ValueError, match="representation"):
        prep([dict(weight=1.0)])
    with pytest.raises(ValueError, match="reference lists"):
        eng.prepare_representation([a, a], frames=F_, references=[dict(representation=b)])


@pytest.mark.gpu
def test_graph_replay_with_new_references_and_separate_entries(gpu_device, tiny):
    """references of the same shapes but other contents replay the captured graph (a copy into the static buffers) and equal the
    eager step bit for bit; composed, masked and plain guided steps are separate graph entries"""
    dev = gpu_device
    cfg, sd = tiny
    eng = UNet3DEngine(sd, cfg, dev)
    N, Gs = 3, 2
    lat, text, vid, noise = [t.half().to(dev) for t in make_inputs(cfg)]
    eager = MotionCloneSampler(eng, num_inference_steps=N, guidance_steps=Gs, guidance_scale=0.3, **HP)
    graphed = MotionCloneSampler(eng, num_inference_steps=N, guidance_steps=Gs, guidance_scale=0.3, **HP).enable_graphs()
    rep = eager.extract(vid, noise, text[0:1])
    b1, b2 = _extra(dev, cfg, eager, 300, 2), _extra(dev, cfg, eager, 301, 2)
    runs = [dict(references=[dict(representation=b1, weight=LAM_B, mask=right_mask())], mask=left_mask()),
            dict(references=[dict(representation=b2, weight=2.0)]),            # same shapes: a copy, not a capture
            dict(mask=left_mask()), dict(),
            dict(references=[dict(representation=b1, weight=LAM_B, mask=right_mask())], mask=left_mask())]
    counts, finals = [], []
    for kw in runs:
        rep_dev = eng.prepare_representation(rep, frames=F_, grid=(H_, W_), **kw)
        xe, xg = lat, lat
        for i in range(N):
            xe = eager.step(xe, i, text, rep_dev)
            xg = graphed.step(xg, i, text, rep_dev).clone()
            assert torch.equal(xe, xg), i
        counts.append(len(graphed._graphs))
        finals.append(xe)
    assert counts == [N, N, N + Gs, N + 2 * Gs, N + 2 * Gs], counts
    assert not torch.equal(finals[0], finals[1]) and not torch.equal(finals[0], finals[2]) and torch.equal(finals[0], finals[4])
    kinds = sorted({(sig[0][2], sig[0][3], sig[0][1][-1]) for key in graphed._graphs for sig in [key[3]] if sig})
    assert kinds == [(False, False, 1), (True, False, 1), (True, True, 3)], kinds


def test_dropin_motion_references_key_and_overrides(backend, tiny, tmp_path):
    from motionclone_amd.utils import motionclone_functions as mf
    dev = backend
    cfg, sd = tiny
    N, Gs, gscale = 2, 1, 0.3
    pipe = build_pipeline(dev, cfg, sd, N, Gs, gscale)
    pipe.sample_video_batch = mf.sample_video_batch.__get__(pipe)
    text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=torch.Generator().manual_seed(7)).half().to(dev)
    lat0 = torch.randn(1, 4, F_, H_, W_, generator=torch.Generator().manual_seed(2025)).half().to(dev)

    def video(seed):
        return (0.18215 * torch.randn(1, 4, F_, H_, W_, generator=torch.Generator().manual_seed(seed))).half().to(dev)
    # further references: .pt files written by obtain_motion_representation with motion_topk 3 and 1
    p3, p1, p_mask = str(tmp_path / "b_top3.pt"), str(tmp_path / "c_top1.pt"), str(tmp_path / "right.pt")
    for path, seed, k in ((p3, 21, 3), (p1, 22, 1)):
        pipe.obtain_motion_representation(generator=torch.Generator(device=dev).manual_seed(seed), video_latents=video(seed),
                                          uncond_embeddings=text[0:1], motion_representation_path=path, motion_topk=k)
    assert next(iter(torch.load(p3).values()))[0].shape[-1] == 3 and next(iter(torch.load(p1).values()))[0].shape[-1] == 1
    torch.save(right_mask(), p_mask)
    pipe.obtain_motion_representation(generator=torch.Generator(device=dev).manual_seed(5), video_latents=video(11),
                                      uncond_embeddings=text[0:1])
    rep = pipe.motion_representation_dict

    def run(**kw):
        return pipe.sample_video(noisy_latents=lat0, text_embeddings=text, decode=False, **kw).clone()

    smp = mf._sampler(pipe)

    def loop(**kw):
        x = lat0
        rep_dev = smp.engine.prepare_representation(rep, frames=F_, **kw)
        for i in range(N):
            x = smp._step_eager(x, i, text, rep_dev)
        return x
    base = run()
    assert torch.equal(base, loop())                 # the key absent: the parent path's latents, bit for bit
    refs3 = [dict(representation=torch.load(p3), weight=LAM_B, mask=right_mask())]
    want3 = loop(grid=(H_, W_), references=refs3)
    want1 = loop(grid=(H_, W_), references=[dict(representation=torch.load(p1))])
    assert not torch.equal(want3, base) and not torch.equal(want1, base) and not torch.equal(want1, want3)
    # the yaml key
    pipe.input_config.motion_references = [dict(representation_path=p3, weight=LAM_B, mask_path=p_mask)]
    assert torch.equal(run(), want3)
    # ... overridden per example: the examples-file line of a launcher thread, and the per-call argument
    lanes.set_example(dict(video_path="x.mp4", motion_references=[dict(representation_path=p1)]))
    try:
        assert torch.equal(run(), want1)
    finally:
        lanes.set_example(None)
    assert torch.equal(run(), want3)
    assert torch.equal(run(motion_references=[dict(representation=torch.load(p1), weight=1.0)]), want1)
    # the example's own reference keeps motion_mask_path
    pipe.input_config.motion_mask_path = str(tmp_path / "left.pt")
    torch.save(left_mask(), pipe.input_config.motion_mask_path)
    assert torch.equal(run(), loop(mask=left_mask(), grid=(H_, W_), references=refs3))
    del pipe.input_config.motion_mask_path
    with pytest.raises(ValueError, match="unknown keys"):
        run(motion_references=[dict(representation_path=p1, lambda_=2.0)])
    with pytest.raises(ValueError, match="negative"):
        run(motion_references=[dict(representation_path=p1, weight=-1.0)])
    del pipe.input_config.motion_references
    assert torch.equal(run(), base)                  # key gone: the plain latents again, bit for bit

    # sample_video_batch: V = 1 (the two functions themselves) and V = 2 (one composed example, one plain)
    def example(s, **kw):
        g = torch.Generator().manual_seed(s)
        return dict(video_latents=(0.18215 * torch.randn(1, 4, F_, H_, W_, generator=g)).half().to(dev),
                    uncond_embeddings=torch.randn(1, 7, cfg["cross_attention_dim"], generator=g).half().to(dev),
                    text_embeddings=torch.randn(2, 7, cfg["cross_attention_dim"], generator=g).half().to(dev),
                    noisy_latents=torch.randn(1, 4, F_, H_, W_, generator=g).half().to(dev),
                    generator=torch.Generator(device=dev).manual_seed(s), **kw)
    composed = [dict(representation_path=p3, weight=LAM_B, mask_path=p_mask)]
    one_c = pipe.sample_video_batch([example(1, motion_references=composed)], decode=False)[0].clone()
    one_p = pipe.sample_video_batch([example(1)], decode=False)[0].clone()
    two_p = pipe.sample_video_batch([example(2)], decode=False)[0].clone()
    assert not torch.equal(one_c, one_p)
    got = pipe.sample_video_batch([example(1, motion_references=composed), example(2)], decode=False)
    assert rel_err(got[0], one_c) < 5e-3 and rel_err(got[1], two_p) < 5e-3      # the packed tests' loop tolerance
    assert rel_err(got[0], one_p) > rel_err(got[0], one_c)      # the packed run did use the first example's references


# ---- launcher --batch 2 with one composed example (host simulator, the harness of tests/test_launcher_batch.py) ---------------
needs_reference = pytest.mark.skipif(not shim.available(), reason="reference tree not present")


@needs_reference
def test_launcher_batch_of_two_with_one_composed_example(tmp_path):
    """line 0 carries `motion_references` (line 1's representation file of the serial run, weight 1), line 1 nothing: the packed
    group of two equals the same file run one example at a time, to the packed-versus-alone bound; line 0 has moved away from
    its serial (one reference) result, line 1 has not"""
    from test_launcher_batch import TIMEOUT, child, clean_env, rel
    from test_packed_dropin_api import TOL_LOOP
    from motionclone_amd import build
    build.build_emu()
    work = str(tmp_path)
    env = clean_env()
    p = child("t2v", work, "serial", "--lines", 2, env=env)
    out = p.communicate(timeout=TIMEOUT)[0]
    assert p.returncode == 0 and "ENTRY_OK" in out, out[-4000:]
    with open(os.path.join(work, "examples.jsonl")) as f:
        lines = [json.loads(ln) for ln in f]
    lines[0]["motion_references"] = [dict(representation_path=os.path.join(work, "mr_serial", "clip1.pt"), weight=1.0)]
    composed = os.path.join(work, "composed.jsonl")
    with open(composed, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    procs = {tag: child("t2v", work, "launch", "--lanes", 1, "--batch", b, "--examples", composed, "--tag", tag, env=env)
             for tag, b in (("packed", 2), ("alone", 1))}
    sizes = {}
    try:
        for tag, p in procs.items():
            out = p.communicate(timeout=TIMEOUT)[0]
            assert p.returncode == 0 and "ENTRY_OK" in out, out[-4000:]
            sizes[tag] = [json.loads(ln.split(" ", 1)[1]) for ln in out.splitlines() if ln.startswith("JOB_SIZES")][0]
    finally:
        for p in procs.values():
            if p.poll() is None:
                p.kill()
    assert sizes == dict(packed=[2], alone=[1, 1]), sizes

    def latents(tag, i):
        (path,) = glob.glob(os.path.join(work, "videos_%s*" % tag, "clip%d.latents.pt" % i))
        return torch.load(path)
    e0, e1 = rel(latents("packed", 0), latents("alone", 0)), rel(latents("packed", 1), latents("alone", 1))
    moved, kept = rel(latents("alone", 0), latents("serial", 0)), rel(latents("alone", 1), latents("serial", 1))
    print("COMPOSED_LAUNCH packed vs alone %.3e %.3e; composed vs serial %.3e, plain vs serial %.3e" % (e0, e1, moved, kept))
    assert e0 < TOL_LOOP and e1 < TOL_LOOP
    assert kept < TOL_LOOP < moved
