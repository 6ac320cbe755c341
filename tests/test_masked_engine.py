"""Region-weighted motion guidance (motion mask) through the engine, the sampler and the drop-in API on the tiny UNet3D.

The weighted loss is restated here in fp32 torch on top of the oracle's own pieces (oracle/unet3d_ref.py forward,
guidance_ref.temp_attn_prob / ddim_step): per module  sum(w[bn, f] (gather(P, idx) - ref)^2) / numel  with w the area mean of
the mask over the block of the picture a position covers.  Bounds are those of tests/test_topk_engine.py (guided step) and
of the packed-against-alone tests."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from motionclone_amd.engine import UNet3DEngine, check_motion_mask, reduce_motion_mask
from motionclone_amd.sampler import MotionCloneSampler
from oracle import guidance_ref as G
from oracle import unet3d_ref as U
from test_dropin_api import build_pipeline
from test_engine_parity import HP, make_inputs, rel_err, to_lat

F_, H_, W_ = 4, 8, 8
GRAD_BOUND = 5e-2        # tests/test_topk_engine.py: guided step gradient against the oracle


@pytest.fixture
def tiny():
    cfg = dict(U.TINY_CONFIG)
    sd = {k: v.half().float() for k, v in U.random_state_dict(cfg, seed=1234).items()}
    return cfg, sd


def half_plane_mask():
    """[F, H, W]: the left half of the picture guided with weight 2 in its upper and 1 in its lower part, the right half
    free; the last two frames not guided at all"""
    m = torch.zeros(F_, H_, W_)
    m[:, :, :W_ // 2] = 1.0
    m[:, :H_ // 2, :W_ // 2] = 2.0
    m[F_ - 2:] = 0.0
    return m


def oracle_weights(mask, hw):
    """[hw, F]: area mean of the mask [F, H', W'] (or [H', W']) over the block each of the hw positions covers, in fp32 torch"""
    m = mask.float()
    if m.dim() == 2:
        m = m.unsqueeze(0).expand(F_, -1, -1)
    side = int(round((hw * H_ / W_) ** 0.5))
    pooled = Fn.adaptive_avg_pool2d(m.unsqueeze(0), (side, hw // side))[0]
    return pooled.reshape(F_, hw).t()


def weighted_temp_loss(prob, rep, mask, normalize=False):
    losses = []
    for name, p in prob.items():
        ref_v, ref_i = rep[name]
        err = (torch.gather(p, index=ref_i.to(torch.int64), dim=-1) - ref_v.to(p.dtype)) ** 2
        if mask is None:
            losses.append(err.mean())
            continue
        w = oracle_weights(mask, p.shape[0])
        if normalize:
            w = w / w.mean()
        losses.append((w[:, None, :, None] * err).sum() / err.numel())
    return torch.stack(losses).sum()


def oracle_guided_step(sd, cfg, latents, step_index, timesteps, text, rep, hp, mask, normalize=False, hooked=("up_blocks.1",)):
    """guidance_ref.guided_step with the weighted loss in place of temp_loss"""
    acp = G.alphas_cumprod()
    t = int(timesteps[step_index])
    control = latents.clone().detach().requires_grad_(True)
    with torch.no_grad():
        eps_u = U.unet_forward(sd, cfg, latents, t, text[[0]])
    rec = {}
    eps_c = U.unet_forward(sd, cfg, control, t, text[[1]], record=rec, hooked=hooked)
    loss = hp["motion_guidance_weight"] * weighted_temp_loss(G.temp_attn_prob(rec, cfg["motion_heads"]), rep, mask, normalize)
    loss = loss * G.guidance_scale_factor(step_index, hp["guidance_steps"], hp["warm_up_steps"], hp["cool_up_steps"])
    (grad,) = torch.autograd.grad(loss, control)
    eps = eps_c + hp["cfg_scale"] * (eps_c - eps_u)
    nxt = G.ddim_step(acp, timesteps, step_index, eps.detach(), control.detach(), score=grad.detach())
    return nxt.detach(), dict(eps_u=eps_u.detach(), eps_c=eps_c.detach(), loss=loss.detach(), grad=grad.detach())


_ORACLE = {}


def oracle_case(tiny):
    """the reference of the guided-step tests, computed once: representation, unmasked / masked / normalised oracle steps"""
    if not _ORACLE:
        cfg, sd = tiny
        lat, text, vid, noise = make_inputs(cfg)
        lat16, text16 = lat.half(), text.half()
        N, Gs, gscale = 4, 2, 0.3
        hp = dict(HP, guidance_steps=Gs)
        rep = G.extract_representation(sd, cfg, vid, noise, text16[[0]].float())
        ts = G.uneven_timesteps(N, Gs, gscale)
        mask = half_plane_mask()
        a = (sd, cfg, lat16.float(), 0, ts, text16.float(), rep, hp)
        _ORACLE.update(rep=rep, lat16=lat16, text16=text16, mask=mask, N=N, Gs=Gs, gscale=gscale,
                       plain=G.guided_step(*a), masked=oracle_guided_step(*a, mask),
                       normed=oracle_guided_step(*a, mask, normalize=True))
    return _ORACLE


def _sampler(eng, o):
    return MotionCloneSampler(eng, num_inference_steps=o["N"], guidance_steps=o["Gs"], guidance_scale=o["gscale"], **HP)


def test_the_mask_moves_the_oracle_gradient_well_beyond_the_bound(tiny):
    """a condition on the chosen mask, on the CPU: the masked oracle gradient is at least 10 bounds away from the unmasked one,
    so a step that ignored the mask could not pass the comparison below; and the restatement with mask = None is the oracle"""
    o = oracle_case(tiny)
    apart = rel_err(o["plain"][1]["grad"], o["masked"][1]["grad"])
    print("MASK_SEPARATION %.3f" % apart)
    assert apart >= 10 * GRAD_BOUND
    cfg, sd = tiny
    hp = dict(HP, guidance_steps=o["Gs"])
    _, again = oracle_guided_step(sd, cfg, o["lat16"].float(), 0, G.uneven_timesteps(o["N"], o["Gs"], o["gscale"]),
                                  o["text16"].float(), o["rep"], hp, None)
    assert rel_err(again["grad"], o["plain"][1]["grad"]) < 1e-5


def test_guided_step_with_a_half_plane_mask_matches_oracle(backend, tiny):
    dev = backend
    cfg, sd = tiny
    o = oracle_case(tiny)
    eng = UNet3DEngine(sd, cfg, dev)
    smp = _sampler(eng, o)
    rep_dev = eng.prepare_representation(o["rep"], frames=F_, mask=o["mask"], grid=(H_, W_))
    assert all(len(e) == 3 and e[2].shape == (e[0].shape[0], F_) and e[2].dtype == torch.float32 for e in rep_dev.values())
    aux = {}
    nxt = smp.step(o["lat16"].to(dev), 0, o["text16"].to(dev), rep_dev, aux=aux)
    ref_nxt, ref_aux = o["masked"]
    e = dict(eps_c=rel_err(to_lat(aux["eps_c"], 1, F_, H_, W_), ref_aux["eps_c"]),
             eps_u=rel_err(to_lat(aux["eps_u"], 1, F_, H_, W_), ref_aux["eps_u"]),
             loss=abs(aux["loss"].item() - ref_aux["loss"].item()) / abs(ref_aux["loss"].item()),
             grad=rel_err(aux["grad"], ref_aux["grad"]), latents=rel_err(nxt, ref_nxt))
    print("MASKED_GUIDED_STEP %s" % e)
    assert e["eps_c"] < 2e-2 and e["eps_u"] < 2e-2
    assert e["loss"] < 3e-2
    assert e["grad"] < GRAD_BOUND, e
    assert e["latents"] < 2e-2


def test_pixel_mask_and_its_latent_area_mean_give_identical_weights(backend, tiny):
    """two hooked blocks on different grids; values are multiples of 1 / 4, so every block sum and mean is exact"""
    dev = backend
    cfg, sd = tiny
    blocks = ["down_blocks.1", "up_blocks.1"]      # 4 x 4 and 2 x 2 positions on the 8 x 8 latent grid
    eng = UNet3DEngine(sd, cfg, dev, guidance_blocks=blocks)
    smp = MotionCloneSampler(eng, num_inference_steps=4, guidance_steps=2, guidance_scale=0.3, **HP)
    _, text, vid, noise = make_inputs(cfg)
    rep = smp.extract(vid.half().to(dev), noise.half().to(dev), text[[0]].half().to(dev))
    g = torch.Generator().manual_seed(3)
    pixel = torch.randint(0, 9, (F_, 8 * H_, 8 * W_), generator=g).float() / 4.0
    latent = Fn.avg_pool2d(pixel.unsqueeze(0), 8)[0]
    assert latent.shape == (F_, H_, W_)
    a = eng.prepare_representation(rep, frames=F_, mask=pixel, grid=(H_, W_))
    b = eng.prepare_representation(rep, frames=F_, mask=latent, grid=(H_, W_))
    grids = set()
    for name in eng.hooked_names():
        assert torch.equal(a[name][2], b[name][2]), name
        hw = a[name][0].shape[0]
        grids.add(hw)
        assert torch.equal(a[name][2].cpu(), oracle_weights(latent, hw)), name
    assert grids == {16, 4}, grids
    # a 2-D mask is the same mask in every frame
    c = eng.prepare_representation(rep, frames=F_, mask=latent[0], grid=(H_, W_))
    d = eng.prepare_representation(rep, frames=F_, mask=latent[0].unsqueeze(0).expand(F_, -1, -1), grid=(H_, W_))
    assert all(torch.equal(c[n][2], d[n][2]) for n in c)


def test_mask_of_ones_is_the_unmasked_step_and_zero_mask_gives_zero(backend, tiny):
    dev = backend
    cfg, sd = tiny
    o = oracle_case(tiny)
    eng = UNet3DEngine(sd, cfg, dev)
    smp = _sampler(eng, o)
    lat, text = o["lat16"].to(dev), o["text16"].to(dev)
    plain = eng.prepare_representation(o["rep"], frames=F_)
    assert all(len(e) == 2 for e in plain.values())
    ones = eng.prepare_representation(o["rep"], frames=F_, mask=torch.ones(H_, W_), grid=(H_, W_))
    zero = eng.prepare_representation(o["rep"], frames=F_, mask=torch.zeros(F_, 2 * H_, 2 * W_), grid=(H_, W_))
    a0, a1, az = {}, {}, {}
    x0 = smp.step(lat, 0, text, plain, aux=a0)
    x1 = smp.step(lat, 0, text, ones, aux=a1)
    assert torch.equal(x0, x1) and torch.equal(a0["grad"], a1["grad"]) and torch.equal(a0["loss"], a1["loss"])
    assert torch.equal(a0["eps_c"], a1["eps_c"]) and a0["grad"].abs().max() > 0
    smp.step(lat, 0, text, zero, aux=az)
    assert az["grad"].abs().max() == 0 and float(az["loss"]) == 0.0


def test_normalised_mask_divides_by_the_mean_weight(backend, tiny):
    dev = backend
    cfg, sd = tiny
    o = oracle_case(tiny)
    eng = UNet3DEngine(sd, cfg, dev)
    smp = _sampler(eng, o)
    lat, text = o["lat16"].to(dev), o["text16"].to(dev)
    rep_n = eng.prepare_representation(o["rep"], frames=F_, mask=o["mask"], mask_normalize=True, grid=(H_, W_))
    aux = {}
    smp.step(lat, 0, text, rep_n, aux=aux)
    ref = o["normed"][1]
    assert rel_err(aux["grad"], ref["grad"]) < GRAD_BOUND
    assert abs(aux["loss"].item() - ref["loss"].item()) < 3e-2 * abs(ref["loss"].item())
    # the oracle's normalised gradient is the un-normalised one over mean(w); one hooked grid, so one mean for all modules
    means = {float(oracle_weights(o["mask"], e[0].shape[0]).mean()) for e in rep_n.values()}
    assert len(means) == 1
    mean = means.pop()
    assert 0 < mean < 1
    assert rel_err(ref["grad"] * mean, o["masked"][1]["grad"]) < 1e-4
    assert rel_err(aux["grad"] * mean, o["masked"][1]["grad"]) < GRAD_BOUND
    with pytest.raises(ValueError, match="mean"):
        eng.prepare_representation(o["rep"], frames=F_, mask=torch.zeros(H_, W_), mask_normalize=True, grid=(H_, W_))
    eng.prepare_representation(o["rep"], frames=F_, mask=torch.zeros(H_, W_), grid=(H_, W_))       # legal without normalisation


def test_packed_step_with_one_masked_video_equals_the_separate_steps(backend, tiny):
    dev = backend
    cfg, sd = tiny
    eng = UNet3DEngine(sd, cfg, dev)
    smp = MotionCloneSampler(eng, num_inference_steps=3, guidance_steps=2, guidance_scale=0.3, **HP)
    vids = []
    for v in range(2):
        g = torch.Generator().manual_seed(100 + v)
        lat = torch.randn(1, 4, F_, H_, W_, generator=g).half().to(dev)
        text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=g).half().to(dev)
        vid = (0.18215 * torch.randn(1, 4, F_, H_, W_, generator=g)).half().to(dev)
        noise = torch.randn(1, 4, F_, H_, W_, generator=g).half().to(dev)
        vids.append((lat, text, vid, noise))
    reps = smp.extract(torch.cat([v[2] for v in vids], 0), torch.cat([v[3] for v in vids], 0),
                       torch.cat([v[1][0:1] for v in vids], 0))
    masks = [half_plane_mask(), None]
    rep_cat = eng.prepare_representation(reps, frames=F_, mask=masks, grid=(H_, W_))
    for e in rep_cat.values():
        n = e[0].shape[0] // 2
        assert len(e) == 3 and e[2].shape == (2 * n, F_) and (e[2][n:] == 1).all() and (e[2][:n] != 1).any()
    lat2 = torch.cat([v[0] for v in vids], 0)
    text2 = torch.cat([v[1][0:1] for v in vids] + [v[1][1:2] for v in vids], 0)
    aux2 = {}
    nxt2 = smp._step_eager(lat2, 0, text2, rep_cat, aux=aux2)
    l_sep = 0.0
    for v, (lat, text, _, _) in enumerate(vids):
        aux1 = {}
        one = eng.prepare_representation(reps[v], frames=F_, mask=masks[v], grid=(H_, W_))
        assert len(next(iter(one.values()))) == (3 if masks[v] is not None else 2)
        nxt1 = smp._step_eager(lat, 0, text, one, aux=aux1)
        l_sep += float(aux1["loss"])
        assert rel_err(nxt2[v:v + 1], nxt1) < 2e-3, (v, rel_err(nxt2[v:v + 1], nxt1))
        assert rel_err(aux2["grad"][v:v + 1], aux1["grad"]) < 2e-2
    assert abs(float(aux2["loss"]) - l_sep) < 2e-3 * abs(l_sep)
    # a list of masks where none is set: the two-tuples of the unmasked path
    assert all(len(e) == 2 for e in eng.prepare_representation(reps, frames=F_, mask=[None, None], grid=(H_, W_)).values())


def test_mask_validation_names_the_problem(tiny):
    good = torch.ones(F_, H_, W_)
    check_motion_mask(good, F_, (H_, W_))
    check_motion_mask(torch.ones(3 * H_, 2 * W_), F_, (H_, W_))
    for bad, what in ((torch.ones(F_ + 1, H_, W_), "frames"),
                      (torch.ones(F_, H_ + 4, W_), "multiple"),
                      (torch.ones(F_, H_ // 2, W_ // 2), "multiple"),
                      (-good, "negative"),
                      (good * float("nan"), "NaN"),
                      (good * float("inf"), "NaN or infinite"),
                      (torch.ones(1, F_, H_, W_), "dimensions")):
        with pytest.raises(ValueError, match=what):
            check_motion_mask(bad, F_, (H_, W_))
    with pytest.raises(ValueError, match="positions"):
        reduce_motion_mask(check_motion_mask(good, F_, (H_, W_)), (H_, W_), 5)


def test_prepare_representation_validates_the_mask(backend, tiny):
    dev = backend
    cfg, sd = tiny
    o = oracle_case(tiny)
    eng = UNet3DEngine(sd, cfg, dev)
    rep = o["rep"]
    good = torch.ones(F_, H_, W_)
    for bad, what in ((torch.ones(F_ + 1, H_, W_), "frames"), (torch.ones(F_, H_ + 4, W_), "multiple"), (-good, "negative"),
                      (good * float("nan"), "NaN"), (torch.ones(1, F_, H_, W_), "dimensions")):
        with pytest.raises(ValueError, match=what):
            eng.prepare_representation(rep, frames=F_, mask=bad, grid=(H_, W_))
    with pytest.raises(ValueError, match="list of 3 masks for 2"):
        eng.prepare_representation([rep, rep], frames=F_, mask=[good, None, None], grid=(H_, W_))
    with pytest.raises(ValueError, match="grid"):
        eng.prepare_representation(rep, frames=F_, mask=good)


@pytest.mark.gpu
def test_graph_replay_with_a_new_mask_and_separate_entries(gpu_device, tiny):
    """masks of the same shape but other contents replay the captured graph (a copy into the static weights) and equal the
    eager step bit for bit; masked and unmasked guided steps are separate graph entries"""
    dev = gpu_device
    cfg, sd = tiny
    eng = UNet3DEngine(sd, cfg, dev)
    N, Gs = 3, 2
    lat, text, vid, noise = [t.half().to(dev) for t in make_inputs(cfg)]
    eager = MotionCloneSampler(eng, num_inference_steps=N, guidance_steps=Gs, guidance_scale=0.3, **HP)
    graphed = MotionCloneSampler(eng, num_inference_steps=N, guidance_steps=Gs, guidance_scale=0.3, **HP).enable_graphs()
    rep = eager.extract(vid, noise, text[0:1])
    other = torch.rand(F_, H_, W_, generator=torch.Generator().manual_seed(9)) * 2.0
    counts, finals = [], []
    for mask in (half_plane_mask(), other, None, half_plane_mask()):
        rep_dev = eng.prepare_representation(rep, frames=F_, mask=mask, grid=(H_, W_))
        xe, xg = lat, lat
        for i in range(N):
            xe = eager.step(xe, i, text, rep_dev)
            xg = graphed.step(xg, i, text, rep_dev).clone()
            assert torch.equal(xe, xg), i
        counts.append(len(graphed._graphs))
        finals.append(xe)
    assert counts == [N, N, N + Gs, N + Gs], counts       # the second mask replays; the unmasked video adds its guided steps
    assert not torch.equal(finals[0], finals[1]) and not torch.equal(finals[0], finals[2]) and torch.equal(finals[0], finals[3])
    weighted = sorted({sig[0][2] for key in graphed._graphs for sig in [key[3]] if sig})
    assert weighted == [False, True]


def test_dropin_mask_keys_and_per_example_override(backend, tiny, tmp_path):
    from motionclone_amd.utils import motionclone_functions as mf
    dev = backend
    cfg, sd = tiny
    N, Gs, gscale = 2, 1, 0.3
    pipe = build_pipeline(dev, cfg, sd, N, Gs, gscale)
    pipe.sample_video_batch = mf.sample_video_batch.__get__(pipe)
    text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=torch.Generator().manual_seed(7)).half().to(dev)
    vid = (0.18215 * torch.randn(1, 4, F_, H_, W_, generator=torch.Generator().manual_seed(11))).half().to(dev)
    lat0 = torch.randn(1, 4, F_, H_, W_, generator=torch.Generator().manual_seed(2025)).half().to(dev)
    pipe.obtain_motion_representation(generator=torch.Generator(device=dev).manual_seed(5), video_latents=vid,
                                      uncond_embeddings=text[0:1])
    rep = pipe.motion_representation_dict

    def run(**kw):
        return pipe.sample_video(noisy_latents=lat0, text_embeddings=text, decode=False, **kw).clone()
    base = run()
    # the engine's own loop without any mask: the keys absent change nothing
    smp = mf._sampler(pipe)
    x = lat0
    rep_dev = smp.engine.prepare_representation(rep, frames=F_)
    for i in range(N):
        x = smp._step_eager(x, i, text, rep_dev)
    assert torch.equal(base, x)
    mask = half_plane_mask()
    want = lat0
    rep_m = smp.engine.prepare_representation(rep, frames=F_, mask=mask, grid=(H_, W_))
    for i in range(N):
        want = smp._step_eager(want, i, text, rep_m)
    assert not torch.equal(want, base)
    # yaml key motion_mask_path: .pt and .npy
    p_pt, p_npy = str(tmp_path / "mask.pt"), str(tmp_path / "mask.npy")
    torch.save(mask, p_pt)
    np.save(p_npy, mask.numpy())
    for path in (p_pt, p_npy):
        pipe.input_config.motion_mask_path = path
        assert torch.equal(run(), want), path
    # motion_mask_normalize
    pipe.input_config.motion_mask_normalize = True
    normed = run()
    rep_n = smp.engine.prepare_representation(rep, frames=F_, mask=mask, mask_normalize=True, grid=(H_, W_))
    y = lat0
    for i in range(N):
        y = smp._step_eager(y, i, text, rep_n)
    assert torch.equal(normed, y) and not torch.equal(normed, want)
    del pipe.input_config.motion_mask_normalize
    del pipe.input_config.motion_mask_path
    assert torch.equal(run(), base)                       # keys gone: the unmasked latents again, bit for bit
    assert torch.equal(run(motion_mask=mask), want)       # per-call override
    with pytest.raises(ValueError, match="frames"):
        run(motion_mask=torch.ones(F_ + 1, H_, W_))

    # per-example override in sample_video_batch: V = 1 (the two functions themselves) and V = 2 (one masked, one not)
    def example(s, **kw):
        g = torch.Generator().manual_seed(s)
        return dict(video_latents=(0.18215 * torch.randn(1, 4, F_, H_, W_, generator=g)).half().to(dev),
                    uncond_embeddings=torch.randn(1, 7, cfg["cross_attention_dim"], generator=g).half().to(dev),
                    text_embeddings=torch.randn(2, 7, cfg["cross_attention_dim"], generator=g).half().to(dev),
                    noisy_latents=torch.randn(1, 4, F_, H_, W_, generator=g).half().to(dev),
                    generator=torch.Generator(device=dev).manual_seed(s), **kw)
    one_m = pipe.sample_video_batch([example(1, motion_mask=mask)], decode=False)[0].clone()
    one_p = pipe.sample_video_batch([example(1)], decode=False)[0].clone()
    two_p = pipe.sample_video_batch([example(2)], decode=False)[0].clone()
    assert not torch.equal(one_m, one_p)
    got = pipe.sample_video_batch([example(1, motion_mask=p_pt), example(2)], decode=False)
    assert rel_err(got[0], one_m) < 5e-3 and rel_err(got[1], two_p) < 5e-3      # the packed tests' loop tolerance
    assert rel_err(got[0], one_p) > rel_err(got[0], one_m)      # the packed run did use the first example's mask
