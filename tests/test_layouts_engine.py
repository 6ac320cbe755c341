"""The AnimateDiff v1 / v2 model layouts in the engine - video-wide GroupNorm (`inflated_groupnorm = False`), the mid-block motion
module (`motion_mid_block`), decoder-only motion modules and a subset of resolutions - against what the UNMODIFIED reference
UNet3DConditionModel computes for them (tests/golden/reference_layouts.pt, recorded by tests/golden/make_layout_records.py;
the tests do not read the reference tree).  Bounds are those tests/test_engine_parity.py applies to the same quantities.

The golden's inputs give every frame its own scale and offset, and the mid-block module's proj_out is scaled, so that a
per-frame GroupNorm misses the recorded eps by 0.57 and a missing mid-block module by 0.12 relative L2 (the file's metadata):
both far outside the 2e-2 bound."""
import os

import pytest
import torch

import layout_util as LU
from motionclone_amd import ops
from motionclone_amd.engine import ControlNetEngine, UNet3DEngine
from motionclone_amd.sampler import MotionCloneSampler
from oracle import unet3d_ref as U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_layouts.pt")
TOL_EPS, TOL_VAL, TOL_LOSS, TOL_GRAD = 2e-2, 5e-3, 3e-2, 5e-2
_CACHE = {}


def golden():
    if "g" not in _CACHE:
        _CACHE["g"] = torch.load(GOLDEN)
    return _CACHE["g"]


def weights(keys):
    k = repr(sorted(keys.items()))
    if k not in _CACHE:
        _CACHE[k] = LU.layout_state_dict(keys, golden()["meta"]["mid_proj_out_scale"])
    return _CACHE[k]


def engine(name, dev, **kw):
    _, keys, hooks = LU.LAYOUTS[name]
    return UNet3DEngine(weights(keys), LU.engine_config(keys), dev, guidance_blocks=hooks, **kw)


def sampler(eng, **kw):
    return MotionCloneSampler(eng, num_inference_steps=LU.N_STEPS, guidance_steps=LU.G_STEPS, guidance_scale=LU.G_SCALE, **LU.HP, **kw)


def to_lat(eps, B, F=LU.F):
    return ops.cl_to_latent(eps, B, 4, F, LU.H, LU.W).float().cpu()


def test_the_golden_is_sensitive_to_what_the_layouts_change():
    meta = golden()["meta"]
    assert meta["eps_moved_by_video_wide_groupnorm"] >= 5 * TOL_EPS and meta["eps_moved_by_mid_module"] >= 5 * TOL_EPS
    assert tuple(meta["first_mid_attention_index"]) == (40, 42)     # named_modules(): down blocks, up blocks, then the mid block


@pytest.mark.parametrize("name", list(LU.LAYOUTS))
def test_layout_matches_the_reference(backend, name):
    dev = backend
    G = golden()["layouts"][name]
    lat, text, vid, noise = [t.half().to(dev) for t in LU.inputs()]
    eng = engine(name, dev)
    assert eng.hooked_names() == G["hooked"]
    e = LU.rel(to_lat(eng.forward(lat.expand(2, -1, -1, -1, -1), golden()["meta"]["t_forward"], text), 2), G["eps"])
    print(name, "eps", e)
    assert e < TOL_EPS, e
    smp = sampler(eng)
    rep = smp.extract(vid, noise, text[0:1])
    assert list(rep) == list(G["rep"]) == G["hooked"]
    for k in rep:
        v, i = rep[k]
        gv, gi = G["rep"][k]
        assert v.shape == gv.shape and i.dtype == torch.uint8
        assert (v.float().cpu() - gv.float()).abs().max() < TOL_VAL
        mism = i.cpu() != gi
        if mism.any():      # an index differs only where the reference's two best probabilities are within fp16 noise
            assert (G["gap"][k].float()[mism] < TOL_VAL).all(), (k, G["gap"][k].float()[mism].max())
    ref_rep = {k: [v[0].float(), v[1]] for k, v in G["rep"].items()}
    aux = {}
    nxt = smp.step(lat, 0, text, eng.prepare_representation(ref_rep), aux=aux)
    el = abs(float(aux["loss"]) - float(G["loss"])) / abs(float(G["loss"]))
    eg, ex = LU.rel(aux["grad"], G["grad"]), LU.rel(nxt, G["guided"])
    print(name, "loss", el, "grad", eg, "guided latents", ex)
    assert el < TOL_LOSS and eg < TOL_GRAD and ex < TOL_EPS, (el, eg, ex)
    p = smp.step(G["guided"].to(dev), LU.G_STEPS, text, {})
    ep = LU.rel(p, G["plain"])
    print(name, "plain latents", ep)
    assert ep < TOL_EPS, ep


def _two_videos(dev):
    """two videos whose values differ by a factor and an offset: statistics that leak from one video of a packed batch into
    the other would show"""
    lat, text, vid, noise = LU.inputs()
    g = torch.Generator().manual_seed(100)
    lat2 = 2.0 * torch.randn(lat.shape, generator=g) - 0.7
    text2 = torch.randn(text.shape, generator=g)
    vid2 = (vid * 0.5 + 0.05).flip(2).contiguous()
    return [tuple(t.half().to(dev) for t in v) for v in ((lat, text, vid, noise), (lat2, text2, vid2, noise))]


def test_packed_step_equals_the_separate_steps_with_video_wide_groupnorm(backend):
    dev = backend
    eng = engine("a", dev)
    smp = sampler(eng)
    vids = _two_videos(dev)
    reps = [smp.extract(vid, noise, text[0:1]) for (_, text, vid, noise) in vids]
    rep_devs = [eng.prepare_representation(r) for r in reps]
    rep_cat = eng.prepare_representation(reps)
    lat2 = torch.cat([v[0] for v in vids], 0)
    text2 = torch.cat([v[1][0:1] for v in vids] + [v[1][1:2] for v in vids], 0)
    for i in (0,):                      # one guided step (the plain step runs the same forward without the tape)
        aux2 = {}
        nxt2 = smp.step(lat2, i, text2, rep_cat, aux=aux2)
        l_sep = 0.0
        for v, (lat, text, _, _) in enumerate(vids):
            aux1 = {}
            nxt1 = smp.step(lat, i, text, rep_devs[v], aux=aux1)
            assert LU.rel(nxt2[v:v + 1], nxt1) < 2e-3, (i, v, LU.rel(nxt2[v:v + 1], nxt1))
            if i < LU.G_STEPS:
                l_sep += float(aux1["loss"])
                assert LU.rel(aux2["grad"][v:v + 1], aux1["grad"]) < 2e-2
        if i < LU.G_STEPS:
            assert abs(float(aux2["loss"]) - l_sep) < 2e-3 * abs(l_sep)


@pytest.mark.parametrize("name", ["a"])
def test_shared_prefix_equals_the_duplicated_batch(backend, name):
    """forward(dup=True): the first ResnetBlock3D runs once on V videos - video-wide statistics of V, not 2 V, videos"""
    dev = backend
    eng = engine(name, dev)
    vids = _two_videos(dev)
    lats = torch.cat([v[0] for v in vids], 0)
    text2 = torch.cat([v[1][0:1] for v in vids] + [v[1][1:2] for v in vids], 0)
    shared = to_lat(eng.forward(lats, 701, text2, dup=True), 4)
    full = to_lat(eng.forward(torch.cat([lats, lats], 0), 701, text2), 4)
    assert LU.rel(shared, full) < 4e-3, LU.rel(shared, full)
    # and the taped path through the junction: same gradient with and without the shared prefix
    smp = sampler(eng)
    reps = [smp.extract(vid, noise, text[0:1]) for (_, text, vid, noise) in vids]
    rep_dev = eng.prepare_representation(reps)
    tu, tc = text2[:2], text2[2:]
    _, g1, l1, _ = eng.guided_eps_and_grad(lats, 701, tc, rep_dev, 2000.0, want_loss=True, text_uncond=tu)
    eng.share_prefix = False
    _, g0, l0, _ = eng.guided_eps_and_grad(lats, 701, tc, rep_dev, 2000.0, want_loss=True, text_uncond=tu)
    assert LU.rel(g1, g0) < 2e-2 and abs(float(l1) - float(l0)) < 2e-3 * abs(float(l0))


def test_context_windows_with_a_v1_layout_equal_the_packed_step(backend):
    """F = 4 as two disjoint windows of 2: every window is one video of 2 frames for the video-wide statistics, bit for bit
    the packed V = 2 step on the gathered windows (one guided step)"""
    dev = backend
    eng = engine("a", dev)
    smp = sampler(eng)
    g = torch.Generator().manual_seed(5)
    sc = torch.tensor(LU.FRAME_SCALE).view(1, 1, 4, 1, 1)
    lat = (torch.randn(1, 4, 4, LU.H, LU.W, generator=g) * sc + sc - 1).half().to(dev)
    vid = (0.18215 * torch.randn(1, 4, 4, LU.H, LU.W, generator=g) * sc).half().to(dev)
    noise = torch.randn(1, 4, 4, LU.H, LU.W, generator=g).half().to(dev)
    text = LU.inputs()[1].half().to(dev)
    ctx = dict(length=2, overlap=0)

    def halves(t):
        return torch.cat([t[:, :, :2], t[:, :, 2:]], 0).contiguous()
    reps = smp.extract(vid, noise, text[0:1], context=ctx)
    rep_long = smp.prepare_windows(reps, smp.windows(ctx, 4), 4)
    rep_packed = eng.prepare_representation(reps)
    text2 = torch.cat([text[0:1], text[0:1], text[1:2], text[1:2]], 0)
    for i in (0,):
        got = smp.step(lat, i, text, rep_long, context=ctx)
        want = smp.step(halves(lat), i, text2, rep_packed)
        assert torch.equal(got, torch.cat([want[0:1], want[1:2]], 2))
    # and the halves are NOT what one video of 8 frames gives (the statistics follow the window)
    whole = to_lat(eng.forward(lat, 701, text[1:2]), 1, 4)
    parts = to_lat(eng.forward(halves(lat), 701, torch.cat([text[1:2], text[1:2]], 0)), 2, 2)
    assert LU.rel(torch.cat([parts[0:1], parts[1:2]], 2), whole) > 5 * TOL_EPS


@pytest.mark.gpu
def test_graph_replay_equals_eager(gpu_device):
    dev = gpu_device
    eng = engine("c", dev)
    lat, text, vid, noise = [t.half().to(dev) for t in LU.inputs()]
    lat2 = (lat * 0.5 + 0.3).contiguous()
    eager, graphed = sampler(eng), sampler(eng)
    rep = eager.extract(vid, noise, text[0:1])
    want = [eager.sample(x, text, rep).clone() for x in (lat, lat2)]
    graphed.enable_graphs()
    got = [graphed.sample(x, text, rep).clone() for x in (lat, lat2)]      # capture, then replay
    torch.cuda.synchronize()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    assert not torch.equal(got[0], got[1])


def test_resolution_subset_is_structurally_the_reference_layout(backend):
    """motion_module_resolutions = [1, 2] has no recorded results: parameter set and hooked names equal the reference model's,
    and eps does not move when the weights of a module the layout does not have are perturbed (it does for one it has)"""
    dev = backend
    _, keys, hooks = LU.RES12
    from motionclone_amd import spec
    cfg = LU.engine_config(keys)
    want_keys = LU.unpack_keys(golden()["keys"]["res12"])
    assert set(spec.param_shapes(cfg)) == set(want_keys)
    sd_full = LU.layout_state_dict({})                 # every module's weights: the layout must ignore the ones it lacks
    eng = UNet3DEngine(sd_full, cfg, dev, guidance_blocks=hooks)
    assert eng.hooked_names() == golden()["layouts"]["res12"]["hooked"]
    lat, text, _, _ = [t.half().to(dev) for t in LU.inputs()]
    lat = lat[:, :, :2].contiguous()
    base = to_lat(eng.forward(lat, 701, text[1:2]), 1, 2)

    def perturbed(prefix):
        sd = dict(sd_full)
        hit = [k for k in sd if k.startswith(prefix) and k.endswith("proj_out.weight")]
        assert hit
        for k in hit:
            sd[k] = sd[k] * 50.0 + 0.5
        return to_lat(UNet3DEngine(sd, cfg, dev, guidance_blocks=hooks).forward(lat, 701, text[1:2]), 1, 2)
    for absent in ("down_blocks.2.motion_modules.", "up_blocks.1.motion_modules."):
        assert torch.equal(perturbed(absent), base), absent
    for present in ("down_blocks.1.motion_modules.", "up_blocks.2.motion_modules."):
        assert LU.rel(perturbed(present), base) > 1e-2, present
    # decoder-only: the parameter set of layout c
    for name in LU.LAYOUTS:
        assert set(spec.param_shapes(LU.engine_config(LU.LAYOUTS[name][1]))) == set(LU.unpack_keys(golden()["keys"][name])), name


def test_errors_are_named(backend):
    dev = backend
    _, keys_b, _ = LU.LAYOUTS["b"]
    sd_b, cfg_b = weights(keys_b), LU.engine_config(keys_b)
    with pytest.raises(ValueError, match="last entry"):
        UNet3DEngine(sd_b, cfg_b, dev, guidance_blocks=["up_blocks.1", "mid_block"])
    with pytest.raises(ValueError, match="last entry"):
        UNet3DEngine(weights({}), LU.engine_config({}), dev, guidance_blocks=["mid_block"])
    # hooks that hook nothing raise at construction: no mid-block module and none at up block 1's resolution ...
    with pytest.raises(ValueError, match="hook no temporal attention"):
        UNet3DEngine(weights({}), LU.engine_config(dict(motion_resolutions=(1, 2))), dev, guidance_blocks=["mid_block", "up_blocks.1"])
    # ... no module in the down blocks of a decoder-only layout, none at up block 0's resolution
    with pytest.raises(ValueError, match="hook no temporal attention"):
        UNet3DEngine(weights({}), LU.engine_config(dict(motion_decoder_only=True, motion_resolutions=(1, 2))), dev,
                     guidance_blocks=["down_blocks.1", "up_blocks.0"])
    # while v3 with 'mid_block' in front still hooks up block 1 (the entry matches no temporal attention there, as in the reference)
    assert len(UNet3DEngine(weights({}), LU.engine_config({}), dev, guidance_blocks=["mid_block", "up_blocks.1"]).hooked_names()) == 6
    # the position table: v1 modules have 24 positions
    cfg24 = LU.engine_config(dict(inflated_groupnorm=False, motion_pe_max_len=24))
    eng = UNet3DEngine(weights({}), cfg24, dev)
    lat = torch.zeros(1, 4, 25, LU.H, LU.W, dtype=torch.float16, device=dev)
    text = LU.inputs()[1].half().to(dev)
    with pytest.raises(ValueError, match="25.*24"):
        eng.forward(lat, 701, text[1:2])
    # SparseCtrl's encoder stays per frame whatever the layout keys say
    assert ControlNetEngine._span(None, None) == 1
