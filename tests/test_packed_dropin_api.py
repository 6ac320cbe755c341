"""`sample_video_batch`: V examples of the pipeline API through one packed launch sequence.  Each example must come out as its
own `obtain_motion_representation` + `sample_video` calls give it (5e-3, the bound of the interleaved-loop test in
tests/test_engine_parity.py), and the generators must end where V sequential calls leave them."""
import pytest
import torch

from motionclone_amd.utils import motionclone_functions as mf
from oracle import unet3d_ref as U
from test_dropin_api import build_pipeline

TOL_LOOP = 5e-3


def rel(a, b):
    return ((a.float().cpu() - b.float().cpu()).norm() / b.float().cpu().norm().clamp_min(1e-12)).item()


def i2v_pipeline(dev, N=3, Gs=2, gscale=0.3, frames=4):
    from motionclone_amd.models.sparse_controlnet import SparseControlNetModel
    cfg = dict(U.TINY_CONFIG)
    sd = {k: v.half().float() for k, v in U.random_state_dict(cfg, seed=1234).items()}
    csd = {k: v.half().float() for k, v in U.random_controlnet_state_dict(cfg).items()}
    pipe = build_pipeline(dev, cfg, sd, N, Gs, gscale)
    ckw = dict(set_noisy_sample_input_to_zero=True, use_simplified_condition_embedding=True, conditioning_channels=4,
               use_motion_module=True, motion_module_resolutions=[1, 2, 4, 8], motion_module_mid_block=False,
               motion_module_type="Vanilla",
               motion_module_kwargs=dict(num_attention_heads=cfg["motion_heads"], num_transformer_block=1,
                                         attention_block_types=["Temporal_Self"], temporal_position_encoding=True,
                                         temporal_position_encoding_max_len=32, temporal_attention_dim_div=1))
    controlnet = SparseControlNetModel.from_unet(pipe.unet, controlnet_additional_kwargs=ckw)
    controlnet.load_state_dict(csd)
    pipe.controlnet = controlnet.to(dev).to(dtype=torch.float16)
    pipe.input_config.image_index = [0]
    pipe.input_config.controlnet_scale = 0.8
    pipe.input_config.video_length = frames
    pipe.sample_video_batch = mf.sample_video_batch.__get__(pipe)       # bound like the other functions of the module
    return pipe, cfg


def make_examples(cfg, dev, frames, seeds, shared_generator=False):
    """different 'prompts' (text embeddings), reference videos, condition images and generators per example"""
    exs = []
    shared = torch.Generator(device=dev).manual_seed(900) if shared_generator else None
    for s in seeds:
        g = torch.Generator().manual_seed(s)
        exs.append(dict(text_embeddings=torch.randn(2, 7, cfg["cross_attention_dim"], generator=g).half().to(dev),
                        video_latents=(0.18215 * torch.randn(1, 4, frames, 8, 8, generator=g)).half().to(dev),
                        uncond_embeddings=torch.randn(1, 7, cfg["cross_attention_dim"], generator=g).half().to(dev),
                        controlnet_images=(0.18215 * torch.randn(1, 4, 1, 8, 8, generator=g)).half().to(dev),
                        generator=shared if shared_generator else torch.Generator(device=dev).manual_seed(500 + s)))
    return exs


def sequential(pipe, exs, eta=0.0):
    outs = []
    for ex in exs:
        pipe.obtain_motion_representation(generator=ex["generator"], use_controlnet=True, video_latents=ex["video_latents"],
                                          uncond_embeddings=ex["uncond_embeddings"])
        outs.append(pipe.sample_video(eta=eta, generator=ex["generator"], text_embeddings=ex["text_embeddings"], decode=False,
                                      add_controlnet=True, controlnet_images=ex["controlnet_images"]).clone())
    return outs


@pytest.mark.parametrize("shared_generator,eta", [(False, 0.0), (True, 0.0), (False, 0.5)])
def test_sample_video_batch_equals_sequential_sample_video_calls(backend, shared_generator, eta):
    dev = backend
    frames = 2 if dev.type == "cpu" else 4
    pipe, cfg = i2v_pipeline(dev, frames=frames)
    assert pipe.sample_video_batch([]) == []
    ref = make_examples(cfg, dev, frames, (1, 2), shared_generator)
    want = sequential(pipe, ref, eta)
    exs = make_examples(cfg, dev, frames, (1, 2), shared_generator)
    got = pipe.sample_video_batch(exs, eta=eta, decode=False)
    assert isinstance(got, list) and len(got) == 2
    for v in range(2):
        assert got[v].shape == want[v].shape == (1, 4, frames, 8, 8) and got[v].dtype == want[v].dtype
        e = rel(got[v], want[v])
        print("sample_video_batch example %d (shared generator %s, eta %g): %.3e" % (v, shared_generator, eta, e))
        assert e < TOL_LOOP, (v, e)
    assert rel(got[0], want[1]) > TOL_LOOP             # the examples are different videos
    # the generators end where the two sequential calls leave them
    for a, b in zip(exs, ref):
        assert torch.equal(a["generator"].get_state(), b["generator"].get_state())
    # one example = the two functions themselves; mixed i2v / t2v examples are refused
    one = pipe.sample_video_batch(make_examples(cfg, dev, frames, (2,)), decode=False)
    if eta == 0.0 and not shared_generator:
        assert torch.equal(one[0], want[1])
        bad = make_examples(cfg, dev, frames, (1, 2))
        del bad[1]["controlnet_images"]
        with pytest.raises(ValueError, match="every example carries a condition image or none"):
            pipe.sample_video_batch(bad, decode=False)


def test_sample_video_batch_text_to_video_and_the_pipeline_method(backend):
    """no condition images: the packed text-to-video path; and the method of the pipeline class (no binding needed)"""
    dev = backend
    frames = 2 if dev.type == "cpu" else 4
    pipe, cfg = i2v_pipeline(dev, frames=frames)
    del pipe.sample_video_batch
    exs = make_examples(cfg, dev, frames, (3, 4))
    for ex in exs:
        del ex["controlnet_images"]
    want = []
    for ex in make_examples(cfg, dev, frames, (3, 4)):
        pipe.obtain_motion_representation(generator=ex["generator"], video_latents=ex["video_latents"],
                                          uncond_embeddings=ex["uncond_embeddings"])
        want.append(pipe.sample_video(generator=ex["generator"], text_embeddings=ex["text_embeddings"], decode=False).clone())
    got = pipe.sample_video_batch(exs, decode=False)
    for v in range(2):
        assert rel(got[v], want[v]) < TOL_LOOP, (v, rel(got[v], want[v]))


@pytest.mark.gpu
def test_second_group_replays_the_captured_graphs_with_new_conditions(gpu_device):
    """hipGraph replay: the first group of two examples captures the packed steps; the second group brings new latents, texts,
    representations and condition images through the static buffers and must still match its sequential calls"""
    dev = gpu_device
    frames = 4
    pipe, cfg = i2v_pipeline(dev, frames=frames)
    first = pipe.sample_video_batch(make_examples(cfg, dev, frames, (1, 2)), decode=False)
    smp = mf._sampler(pipe)
    assert smp._graphs, "the packed steps were not captured"
    packed_keys = {k for k in smp._graphs if k[1][0] == 2}
    assert len(packed_keys) == len(smp.timesteps)
    second = pipe.sample_video_batch(make_examples(cfg, dev, frames, (3, 4)), decode=False)
    assert {k for k in smp._graphs if k[1][0] == 2} == packed_keys       # replayed, nothing captured anew
    want1 = sequential(pipe, make_examples(cfg, dev, frames, (1, 2)))
    want2 = sequential(pipe, make_examples(cfg, dev, frames, (3, 4)))
    for got, want in ((first, want1), (second, want2)):
        for v in range(2):
            e = rel(got[v], want[v])
            print("graph replay example: %.3e" % e)
            assert e < TOL_LOOP, e
    assert rel(second[0], first[0]) > TOL_LOOP
