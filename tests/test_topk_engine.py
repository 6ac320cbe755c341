"""Top-k motion representation through the engine, the sampler and the drop-in API on the tiny UNet3D.

The oracle (oracle/guidance_ref.py) gathers with an index tensor [.., K] of any K, as the reference's compute_temp_loss does;
only its producer is k = 1, so the representation is built here from its probabilities with torch.topk(k = K).  Bounds are
those of tests/test_engine_parity.py for the k = 1 guided step and the packed step."""
import pytest
import torch

from motionclone_amd import ops
from motionclone_amd.engine import UNet3DEngine
from motionclone_amd.sampler import MotionCloneSampler
from oracle import guidance_ref as G
from oracle import unet3d_ref as U
from test_dropin_api import build_pipeline
from test_engine_parity import HP, make_inputs, rel_err, to_lat


@pytest.fixture
def tiny():
    cfg = dict(U.TINY_CONFIG)
    sd = {k: v.half().float() for k, v in U.random_state_dict(cfg, seed=1234).items()}
    return cfg, sd


def oracle_rep(sd, cfg, vid, noise, uncond, K, add_noise_step=400, noisy=None):
    """G.extract_representation with torch.topk(k = K) in place of its k = 1 producer"""
    if noisy is None:
        noisy = G.add_noise(G.alphas_cumprod(), add_noise_step, vid, noise)
    rec = {}
    with torch.no_grad():
        U.unet_forward(sd, cfg, noisy, add_noise_step, uncond, only_motion_feature=True, record=rec)
        prob = G.temp_attn_prob(rec, cfg["motion_heads"])
    rep = {}
    for name, p in prob.items():
        v, i = torch.topk(p, k=K, dim=-1)
        rep[name] = [v, i.to(torch.uint8)]
    return rep


@pytest.mark.parametrize("K", [2, 4])
def test_guided_step_with_topk_representation_matches_oracle(backend, tiny, K):
    """also the bad-input case of a [BN, heads, F, K > 1] file in the reference's layout: before top-k support it was
    accepted and read with the k = 1 stride (wrong guidance, no error)"""
    dev = backend
    cfg, sd = tiny
    lat, text, vid, noise = make_inputs(cfg)
    lat16, text16 = lat.half(), text.half()
    N, Gs, gscale = 4, 2, 0.3
    hp = dict(HP, guidance_steps=Gs)
    rep = oracle_rep(sd, cfg, vid, noise, text16[[0]].float(), K)
    assert all(v.shape[-1] == K for v, _ in rep.values())
    ts = G.uneven_timesteps(N, Gs, gscale)
    eng = UNet3DEngine(sd, cfg, dev)
    smp = MotionCloneSampler(eng, num_inference_steps=N, guidance_steps=Gs, guidance_scale=gscale, **HP)
    rep_dev = eng.prepare_representation(rep, frames=4)
    aux = {}
    nxt = smp.step(lat16.to(dev), 0, text16.to(dev), rep_dev, aux=aux)
    ref_nxt, ref_aux = G.guided_step(sd, cfg, lat16.float(), 0, ts, text16.float(), rep, hp)
    e = dict(eps_c=rel_err(to_lat(aux["eps_c"], 1, 4, 8, 8), ref_aux["eps_c"]),
             eps_u=rel_err(to_lat(aux["eps_u"], 1, 4, 8, 8), ref_aux["eps_u"]),
             loss=abs(aux["loss"].item() - ref_aux["loss"].item()) / abs(ref_aux["loss"].item()),
             grad=rel_err(aux["grad"], ref_aux["grad"]), latents=rel_err(nxt, ref_nxt))
    print("TOPK_GUIDED_STEP K=%d %s" % (K, e))
    assert e["eps_c"] < 2e-2 and e["eps_u"] < 2e-2
    assert e["loss"] < 3e-2
    assert e["grad"] < 5e-2, e
    assert e["latents"] < 2e-2


def test_extract_topk_is_the_topk_of_the_engine_probabilities(backend, tiny):
    dev = backend
    cfg, sd = tiny
    _, text, vid, noise = make_inputs(cfg)
    eng = UNet3DEngine(sd, cfg, dev)
    smp = MotionCloneSampler(eng, num_inference_steps=4, guidance_steps=2, guidance_scale=0.3, **HP)
    a = [t.half().to(dev) for t in (vid, noise, text[[0]])]
    rep1, rep3 = smp.extract(*a), smp.extract(*a, topk=3)
    ref = oracle_rep(sd, cfg, None, None, text[[0]].half().float(), 3, noisy=smp.add_noise(400, vid.half(), noise.half()).float())
    for k in rep1:
        assert rep1[k][0].shape[-1] == 1 and rep3[k][0].shape == rep1[k][0].shape[:-1] + (3,)
        assert torch.equal(rep3[k][0][..., :1], rep1[k][0]) and torch.equal(rep3[k][1][..., :1], rep1[k][1])
        assert (rep3[k][0].float().cpu() - ref[k][0]).abs().max() < 5e-3     # the bound of the k = 1 extraction test
    for bad in (0, 5, 9):
        with pytest.raises(ValueError):
            smp.extract(*a, topk=bad)


def test_prepare_representation_rejects_bad_files(backend, tiny):
    dev = backend
    cfg, sd = tiny
    _, text, vid, noise = make_inputs(cfg)
    eng = UNet3DEngine(sd, cfg, dev)
    rep = oracle_rep(sd, cfg, vid, noise, text[[0]].half().float(), 2)
    name = next(iter(rep))
    eng.prepare_representation(rep)
    eng.prepare_representation(rep, frames=4)
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):      # values / indices of different shape
        eng.prepare_representation(dict(rep, **{name: [rep[name][0], rep[name][1][..., :1]]}))
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):      # K > min(F, 8): F = 4
        v = rep[name][0]
        eng.prepare_representation(dict(rep, **{name: [torch.cat([v, v, v], -1), torch.cat([rep[name][1]] * 3, -1)]}))
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):      # not 4-D
        eng.prepare_representation(dict(rep, **{name: [rep[name][0][..., 0], rep[name][1][..., 0]]}))
    with pytest.raises(ValueError, match=name.replace(".", r"\.")):      # another video length
        eng.prepare_representation(rep, frames=16)
    big = {k: [torch.zeros(4, 2, 16, 9), torch.zeros(4, 2, 16, 9, dtype=torch.uint8)] for k in rep}
    with pytest.raises(ValueError):                                     # K = 9 > 8 at F = 16
        eng.prepare_representation(big)
    rep1 = oracle_rep(sd, cfg, vid, noise, text[[0]].half().float(), 1)
    with pytest.raises(ValueError, match="top-k"):                       # entries of one representation differ in K
        eng.prepare_representation(dict(rep, **{name: rep1[name]}))
    with pytest.raises(ValueError, match="top-k"):                       # mixed K in one packed list
        eng.prepare_representation([rep, rep1])
    with pytest.raises(ValueError):                                      # the step itself checks F as well
        lat = torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16, device=dev)
        eng.guided_eps_and_grad(lat, 701, text[[1]].half().to(dev), eng.prepare_representation(rep), 2000.0)


def test_packed_step_with_topk_equals_the_one_video_steps(backend, tiny):
    dev = backend
    cfg, sd = tiny
    eng = UNet3DEngine(sd, cfg, dev)
    smp = MotionCloneSampler(eng, num_inference_steps=3, guidance_steps=2, guidance_scale=0.3, **HP)
    vids = []
    for v in range(2):
        g = torch.Generator().manual_seed(100 + v)
        lat = torch.randn(1, 4, 4, 8, 8, generator=g).half().to(dev)
        text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=g).half().to(dev)
        vid = (0.18215 * torch.randn(1, 4, 4, 8, 8, generator=g)).half().to(dev)
        noise = torch.randn(1, 4, 4, 8, 8, generator=g).half().to(dev)
        vids.append((lat, text, vid, noise))
    # one batched extraction: a list of V representations [BN, heads, F, 2]
    reps = smp.extract(torch.cat([v[2] for v in vids], 0), torch.cat([v[3] for v in vids], 0),
                       torch.cat([v[1][0:1] for v in vids], 0), topk=2)
    assert len(reps) == 2 and all(val.shape == idx.shape == (4, cfg["motion_heads"], 4, 2) for r in reps for val, idx in r.values())
    rep_cat = eng.prepare_representation(reps)
    lat2 = torch.cat([v[0] for v in vids], 0)
    text2 = torch.cat([v[1][0:1] for v in vids] + [v[1][1:2] for v in vids], 0)
    aux2 = {}
    nxt2 = smp._step_eager(lat2, 0, text2, rep_cat, aux=aux2)
    l_sep = 0.0
    for v, (lat, text, _, _) in enumerate(vids):
        aux1 = {}
        nxt1 = smp._step_eager(lat, 0, text, eng.prepare_representation(reps[v]), aux=aux1)
        l_sep += float(aux1["loss"])
        assert rel_err(nxt2[v:v + 1], nxt1) < 2e-3, (v, rel_err(nxt2[v:v + 1], nxt1))
        assert rel_err(aux2["grad"][v:v + 1], aux1["grad"]) < 2e-2
    assert abs(float(aux2["loss"]) - l_sep) < 2e-3 * abs(l_sep)


def test_obtain_motion_representation_with_motion_topk(backend, tiny, tmp_path):
    dev = backend
    cfg, sd = tiny
    N, Gs, gscale = 2, 1, 0.3
    pipe = build_pipeline(dev, cfg, sd, N, Gs, gscale)
    text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=torch.Generator().manual_seed(7)).half().to(dev)
    vid = (0.18215 * torch.randn(1, 4, 4, 8, 8, generator=torch.Generator().manual_seed(11))).half().to(dev)
    lat0 = torch.randn(1, 4, 4, 8, 8, generator=torch.Generator().manual_seed(2025)).half().to(dev)

    def extract(path):
        return pipe.obtain_motion_representation(generator=torch.Generator(device=dev).manual_seed(5),
                                                 motion_representation_path=path, video_latents=vid,
                                                 uncond_embeddings=text[0:1])
    # key absent: the reference's k = 1 file, the bits of the k = 1 read-out
    p1 = str(tmp_path / "rep1.pt")
    rep1 = extract(p1)
    saved1 = torch.load(p1)
    for name, module in pipe.unet.named_modules():
        if name in rep1:
            r = module.processor.key
            C, g = r["C"], r["geo"]
            v, i = ops.tattn_top1(r["qkv"][:, :C], r["qkv"][:, C:2 * C], g.B, g.F, g.hw, module.heads, r["d"])
            assert v.shape == (g.B * g.hw, module.heads, 4, 1) == tuple(saved1[name][0].shape)
            assert torch.equal(saved1[name][0].view(torch.int16), v.cpu().view(torch.int16)) and torch.equal(saved1[name][1], i.cpu())
            assert saved1[name][0].dtype == torch.float16 and saved1[name][1].dtype == torch.uint8
    # motion_topk = 3 in the inference config
    pipe.input_config.motion_topk = 3
    p3 = str(tmp_path / "rep3.pt")
    rep3 = extract(p3)
    saved3 = torch.load(p3)
    assert list(saved3) == list(saved1)
    for name in saved3:
        assert tuple(saved3[name][0].shape) == tuple(saved1[name][0].shape[:-1]) + (3,) == tuple(saved3[name][1].shape)
        assert torch.equal(saved3[name][0][..., :1], saved1[name][0]) and saved3[name][1].dtype == torch.uint8
    loss = pipe.compute_temp_loss(pipe.get_temp_attn_prob())
    assert loss.item() < 1e-5        # the extraction's own q / k against its own top-3: zero loss
    # sampling from the file (torch.load inside sample_video) == sampling from the in-memory representation
    del pipe.input_config.motion_topk            # sampling infers K from the representation, never from the config
    from_file = pipe.sample_video(noisy_latents=lat0, text_embeddings=text, decode=False).clone()
    assert pipe.motion_representation_dict is not rep3 and pipe.motion_representation_dict[name][0].shape[-1] == 3
    pipe.motion_representation_path = None
    pipe.motion_representation_dict = rep3
    in_memory = pipe.sample_video(noisy_latents=lat0, text_embeddings=text, decode=False)
    assert torch.equal(from_file, in_memory)
    pipe.motion_representation_dict = rep1
    assert not torch.equal(pipe.sample_video(noisy_latents=lat0, text_embeddings=text, decode=False), in_memory)
    # per-call override and range check
    assert next(iter(pipe.obtain_motion_representation(video_latents=vid, uncond_embeddings=text[0:1],
                                                       motion_topk=2).values()))[0].shape[-1] == 2
    pipe.input_config.motion_topk = 5
    with pytest.raises(ValueError):
        extract(None)


def test_sample_video_batch_takes_motion_topk_per_example(backend, tiny):
    from motionclone_amd.utils import motionclone_functions as mf
    dev = backend
    cfg, sd = tiny
    pipe = build_pipeline(dev, cfg, sd, 2, 1, 0.3)
    pipe.sample_video_batch = mf.sample_video_batch.__get__(pipe)

    def example(s, **kw):
        g = torch.Generator().manual_seed(s)
        return dict(video_latents=(0.18215 * torch.randn(1, 4, 4, 8, 8, generator=g)).half().to(dev),
                    uncond_embeddings=torch.randn(1, 7, cfg["cross_attention_dim"], generator=g).half().to(dev),
                    text_embeddings=torch.randn(2, 7, cfg["cross_attention_dim"], generator=g).half().to(dev),
                    noisy_latents=torch.randn(1, 4, 4, 8, 8, generator=g).half().to(dev),
                    generator=torch.Generator(device=dev).manual_seed(s), **kw)
    with pytest.raises(ValueError, match="top-k"):
        pipe.sample_video_batch([example(1, motion_topk=2), example(2)], decode=False)
    got = pipe.sample_video_batch([example(1, motion_topk=2), example(2, motion_topk=2)], decode=False)
    pipe.input_config.motion_topk = 2
    want = pipe.sample_video_batch([example(1), example(2)], decode=False)
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    one = pipe.sample_video_batch([example(1)], decode=False)[0]          # V = 1: the two functions themselves, K = 2
    assert pipe.motion_representation_dict[next(iter(pipe.motion_representation_dict))][0].shape[-1] == 2
    assert rel_err(got[0], one) < 5e-3       # the packed tests' loop tolerance


@pytest.mark.gpu
def test_graphs_hold_separate_entries_per_topk(gpu_device, tiny):
    """a K = 1 video then a K = 2 video on ONE sampler with hipGraph replay: every step equals its eager result bit for bit,
    and the K = 2 video captures new graphs for the guided steps instead of replaying the K = 1 ones"""
    dev = gpu_device
    cfg, sd = tiny
    eng = UNet3DEngine(sd, cfg, dev)
    N, Gs = 3, 2
    lat, text, vid, noise = [t.half().to(dev) for t in make_inputs(cfg)]
    eager = MotionCloneSampler(eng, num_inference_steps=N, guidance_steps=Gs, guidance_scale=0.3, **HP)
    graphed = MotionCloneSampler(eng, num_inference_steps=N, guidance_steps=Gs, guidance_scale=0.3, **HP).enable_graphs()
    counts = []
    for K in (1, 2, 1, 2):          # the second round replays
        rep_dev = eng.prepare_representation(eager.extract(vid, noise, text[0:1], topk=K), frames=4)
        xe, xg = lat, lat
        for i in range(N):
            xe = eager.step(xe, i, text, rep_dev)
            xg = graphed.step(xg, i, text, rep_dev).clone()
            assert torch.equal(xe, xg), (K, i)
        counts.append(len(graphed._graphs))
    assert counts == [N, N + Gs, N + Gs, N + Gs], counts
    ks = sorted({sig[0][1][-1] for key in graphed._graphs for sig in [key[3]] if sig})
    assert ks == [1, 2]
