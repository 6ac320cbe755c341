"""Sliding context windows through the drop-in API: the yaml keys context_length / context_overlap / context_weights carry a
video longer than one window from obtain_motion_representation (windows folded into the row axis, a motion_context entry in
the .pt file) through sample_video; without the keys nothing changes; what is out of scope says so."""
import pytest
import torch

from motionclone_amd.sampler import MotionCloneSampler
from motionclone_amd.utils import motionclone_functions as mf
from oracle import unet3d_ref as U

from test_dropin_api import build_pipeline

HP = dict(cfg_scale=7.5, motion_guidance_weight=2000.0, warm_up_steps=10, cool_up_steps=10)
N, Gs, GSCALE = 2, 1, 0.3


def _pipe(dev, frames, **keys):
    cfg = dict(U.TINY_CONFIG)
    sd = {k: v.half().float() for k, v in U.random_state_dict(cfg, seed=1234).items()}
    pipe = build_pipeline(dev, cfg, sd, N, Gs, GSCALE)
    pipe.input_config.video_length = frames
    for k, v in keys.items():
        setattr(pipe.input_config, k, v)
    return pipe, cfg


def _inputs(cfg, F, dev):
    text = torch.randn(2, 7, cfg["cross_attention_dim"], generator=torch.Generator().manual_seed(7)).half().to(dev)
    vid = (0.18215 * torch.randn(1, 4, F, 8, 8, generator=torch.Generator().manual_seed(11))).half().to(dev)
    lat = torch.randn(1, 4, F, 8, 8, generator=torch.Generator().manual_seed(2025)).half().to(dev)
    return text, vid, lat


def test_round_trip_through_the_representation_file(backend, tmp_path):
    dev = backend
    F, L, ov = 6, 4, 2
    pipe, cfg = _pipe(dev, F, context_length=L, context_overlap=ov)
    text, vid, lat = _inputs(cfg, F, dev)
    path = str(tmp_path / "rep.pt")
    rep = pipe.obtain_motion_representation(generator=torch.Generator(device=dev).manual_seed(5), motion_representation_path=path,
                                            video_latents=vid, uncond_embeddings=text[0:1])
    saved = torch.load(path)
    assert saved["motion_context"] == dict(frames=F, length=L, overlap=ov) == rep["motion_context"]
    names = [k for k in saved if k != "motion_context"]
    assert len(names) == 6 and all(saved[k][0].shape == (2 * 4, cfg["motion_heads"], L, 1) for k in names)   # 2 windows x (2 x 2) positions
    out = pipe.sample_video(noisy_latents=lat, text_embeddings=text, decode=False)       # reads the file back
    assert out.shape == lat.shape and "motion_context" in pipe.motion_representation_dict
    # the sampler-level run on the same noise
    smp = MotionCloneSampler(pipe.unet.engine(), num_inference_steps=N, guidance_steps=Gs, guidance_scale=GSCALE, **HP)
    ctx = dict(length=L, overlap=ov)
    noise = torch.randn(vid.shape, generator=torch.Generator(device=dev).manual_seed(5), device=dev, dtype=vid.dtype)
    reps = smp.extract(vid, noise, text[0:1], context=ctx)
    for w in range(2):
        assert all(torch.equal(reps[w][k][0].cpu(), saved[k][0][w * 4:(w + 1) * 4]) and
                   torch.equal(reps[w][k][1].cpu(), saved[k][1][w * 4:(w + 1) * 4]) for k in names)
    assert torch.equal(out, smp.sample(lat, text, reps, context=ctx))

    # a representation that disagrees with the run, or has no motion_context, is refused by name
    pipe.motion_representation_path = None
    pipe.motion_representation_dict = dict(saved, motion_context=dict(frames=F, length=L, overlap=1))
    with pytest.raises(ValueError, match="motion_context"):
        pipe.sample_video(noisy_latents=lat, text_embeddings=text, decode=False)
    pipe.motion_representation_dict = {k: saved[k] for k in names}
    with pytest.raises(ValueError, match="no motion_context"):
        pipe.sample_video(noisy_latents=lat, text_embeddings=text, decode=False)
    # ... and so is a windowed representation in a run without windows
    pipe.input_config.context_length = None
    pipe.input_config.context_overlap = None
    pipe.motion_representation_dict = dict(saved)
    with pytest.raises(ValueError, match="motion_context"):
        pipe.sample_video(noisy_latents=lat, text_embeddings=text, decode=False)


def test_absent_keys_and_short_videos_change_nothing(backend):
    dev = backend
    F = 4
    pipe, cfg = _pipe(dev, F)
    text, vid, lat = _inputs(cfg, F, dev)

    def run():
        rep = pipe.obtain_motion_representation(generator=torch.Generator(device=dev).manual_seed(5), motion_representation_path=None,
                                                video_latents=vid, uncond_embeddings=text[0:1])
        return rep, pipe.sample_video(noisy_latents=lat, text_embeddings=text, decode=False).clone()
    rep0, out0 = run()
    assert "motion_context" not in rep0
    smp = MotionCloneSampler(pipe.unet.engine(), num_inference_steps=N, guidance_steps=Gs, guidance_scale=GSCALE, **HP)
    assert torch.equal(out0, smp.sample(lat, text, rep0))                    # today's path
    pipe.input_config.context_length = 4                                     # the video fits one window: no windows
    rep1, out1 = run()
    assert "motion_context" not in rep1 and torch.equal(out1, out0)
    assert all(torch.equal(rep0[k][0], rep1[k][0]) and torch.equal(rep0[k][1], rep1[k][1]) for k in rep0)


def test_out_of_scope_combinations_raise_by_name(backend):
    dev = backend
    F, L = 6, 4
    pipe, cfg = _pipe(dev, F, context_length=L, context_overlap=2)
    text, vid, lat = _inputs(cfg, F, dev)
    with pytest.raises(NotImplementedError, match="context_length.*SparseCtrl"):
        pipe.obtain_motion_representation(video_latents=vid, uncond_embeddings=text[0:1], use_controlnet=True)
    rep = {"m": [torch.zeros(8, 2, L, 1), torch.zeros(8, 2, L, 1, dtype=torch.uint8)], "motion_context": dict(frames=F, length=L, overlap=2)}
    pipe.motion_representation_path = None
    pipe.motion_representation_dict = rep
    with pytest.raises(NotImplementedError, match="context_length.*SparseCtrl"):
        pipe.sample_video(noisy_latents=lat, text_embeddings=text, decode=False, add_controlnet=True, controlnet_images=lat)
    with pytest.raises(NotImplementedError, match="context_length.*motion_references"):
        pipe.sample_video(noisy_latents=lat, text_embeddings=text, decode=False,
                          motion_references=[dict(representation={"m": rep["m"]})])
    pipe.sample_video_batch = mf.sample_video_batch.__get__(pipe)
    ex = dict(video_latents=vid, uncond_embeddings=text[0:1], noisy_latents=lat, text_embeddings=text)
    with pytest.raises(NotImplementedError, match="context_length.*sample_video_batch"):
        pipe.sample_video_batch([ex, ex], decode=False)
    from motionclone_amd import lanes
    lanes.begin(0, 1, dev, slot=0, group=lanes.Group(2))       # a launcher lane that packs two examples (--batch 2)
    try:
        with pytest.raises(NotImplementedError, match="context_length.*--batch"):
            pipe.sample_video(noisy_latents=lat, text_embeddings=text, decode=False)
    finally:
        lanes.end()
    for key, val, pat in [("context_overlap", 4, "overlap"), ("context_weights", "gaussian", "context_weights"), ("context_length", 33, "33")]:
        old = getattr(pipe.input_config, key, None)
        setattr(pipe.input_config, key, val)
        with pytest.raises(ValueError, match=pat):
            pipe.obtain_motion_representation(video_latents=torch.cat([vid] * 6, 2) if key == "context_length" else vid,
                                              uncond_embeddings=text[0:1])
        setattr(pipe.input_config, key, old)
    pipe.input_config.context_length = None
    with pytest.raises(ValueError, match="context_overlap is set without context_length"):
        pipe.obtain_motion_representation(video_latents=vid, uncond_embeddings=text[0:1])
