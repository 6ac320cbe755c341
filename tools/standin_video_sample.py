"""Stand-in for the reference's t2v_video_sample.py where neither the reference tree nor real checkpoints exist (the GPU box):
the same call sequence - `set_all_seed(42)`, build the pipeline and bind the guidance functions onto it, then per line of the
examples file `obtain_motion_representation` (writes `<stem>.pt`) and `sample_video` - over SYNTHETIC inputs, so that
`motionclone_amd.launch [--lanes L] [--batch V] tools/standin_video_sample.py ...` exercises the launcher exactly as the real
script does (tools/launch_batch_ab.py, tests/test_launcher_batch_gpu.py).

There is no VAE and no CLIP: the "VAE posterior" of the reference video is a fixed mean (seeded by the video's name) plus a draw
of the reference's shape [L, 4, H/8, W/8] from the serial RNG stream (the stream the real VAE draws from and the launcher burns
for skipped lines), the "prompt embedding" is seeded by the prompt, and the result written per example is the final latent
(`sample_video(decode=False)`), `<stem>_<prompt>_<seed>.pt` under --generated-videos-save-dir.  Next to them every script thread
writes `graphs_<thread name>.json`: the (step index, latent batch) keys of the hipGraphs its sampler holds after each line, the
wall-clock time at which each line's result was on the host, and the process's reserved device memory at the end.

--checkpoint FILE: torch file with dict(config=<UNet3DEngine config>, state_dict=...); without it the full-size network of
BASELINE config 2 with synthetic weights."""
import argparse
import json
import os
import threading
import time
import types
import zlib

import torch

from motionclone_amd import lanes, spec
from motionclone_amd.engine import default_config
from motionclone_amd.models.unet import UNet3DConditionModel
from motionclone_amd.pipelines.pipeline_animation import AnimationPipeline
from motionclone_amd.scheduler import DDIMSchedulerState
from motionclone_amd.utils import motionclone_functions as mf
from motionclone_amd.utils.util import set_all_seed


def seed_of(text):
    return zlib.crc32(text.encode())


def main(args):
    device = torch.device("cuda" if torch.cuda.is_available() else "cpu")
    set_all_seed(42)
    if args.checkpoint:
        ckpt = torch.load(args.checkpoint)
        cfg, sd = ckpt["config"], ckpt["state_dict"]
    else:
        cfg = default_config()
        sd, _ = spec.synthetic_state_dict(cfg, seed=1234, device=device)
    unet = UNet3DConditionModel(in_channels=4, out_channels=4, block_out_channels=cfg["block_out_channels"], layers_per_block=2,
                                cross_attention_dim=cfg["cross_attention_dim"], attention_head_dim=cfg["attention_heads"],
                                use_motion_module=True, motion_module_resolutions=[1, 2, 4, 8], motion_module_mid_block=False,
                                motion_module_kwargs=dict(num_attention_heads=cfg["motion_heads"], num_transformer_block=1,
                                                          attention_block_types=["Temporal_Self", "Temporal_Self"],
                                                          temporal_position_encoding=True))
    unet.load_state_dict(dict(sd), strict=False)
    unet = unet.to(device).to(dtype=torch.float16)
    pipeline = AnimationPipeline(vae=None, text_encoder=None, tokenizer=None, unet=unet, controlnet=None,
                                 scheduler=DDIMSchedulerState(beta_start=0.00085, beta_end=0.012, beta_schedule="linear",
                                                              steps_offset=1, clip_sample=False))
    pipeline.scheduler.customized_step = mf.schedule_customized_step.__get__(pipeline.scheduler)
    pipeline.scheduler.customized_set_timesteps = mf.schedule_set_timesteps.__get__(pipeline.scheduler)
    pipeline.unet.forward = mf.unet_customized_forward.__get__(pipeline.unet)
    for name in ("sample_video", "single_step_video", "get_temp_attn_prob", "add_noise", "compute_temp_loss",
                 "obtain_motion_representation"):
        setattr(pipeline, name, getattr(mf, name).__get__(pipeline))
    for param in pipeline.unet.parameters():
        param.requires_grad = False
    config = types.SimpleNamespace(cfg_scale=7.5, negative_prompt="", inference_steps=args.steps, guidance_scale=args.guidance_scale,
                                   guidance_steps=args.guidance_steps, warm_up_steps=10, cool_up_steps=10,
                                   motion_guidance_weight=2000, motion_guidance_blocks=["up_blocks.1"], add_noise_step=400,
                                   video_length=args.L, height=args.H, width=args.W, new_prompt="")
    pipeline.input_config, pipeline.unet.input_config = config, config
    pipeline.unet = mf.prep_unet_attention(pipeline.unet, config.motion_guidance_blocks)
    pipeline.unet = mf.prep_unet_conv(pipeline.unet)
    pipeline.scheduler.customized_set_timesteps(config.inference_steps, config.guidance_steps, config.guidance_scale, device=device,
                                                timestep_spacing_type="uneven")
    os.makedirs(args.generated_videos_save_dir, exist_ok=True)
    shape = (args.L, 4, args.H // 8, args.W // 8)
    graphs, done_at = {}, {}

    def graph_keys():
        held = getattr(getattr(pipeline, "_mc_sampler", None), "_graphs", None) or {}
        return sorted([k[0], k[1][0]] for k in held)

    with open(args.examples, "r") as files:
        for line in files:
            example = json.loads(line)
            config.video_path = example["video_path"]
            config.new_prompt = example["new_prompt"]
            stem = os.path.splitext(os.path.basename(config.video_path))[0]
            seed = example.get("seed", args.default_seed)
            # the stand-in for VAE encode + posterior sample: the draw comes from the serial stream, as the real VAE's does
            mean = torch.randn(shape, generator=torch.Generator(device=device).manual_seed(seed_of(stem)), device=device,
                               dtype=torch.float16)
            draw = torch.randn(shape, generator=lanes.serial_generator(), device=device, dtype=torch.float16)
            video_latents = (0.18215 * (mean + 0.1 * draw)).unsqueeze(0).permute(0, 2, 1, 3, 4).contiguous()
            text = torch.randn((2, args.tokens, cfg["cross_attention_dim"]),
                               generator=torch.Generator(device=device).manual_seed(seed_of(config.new_prompt)), device=device).half()

            generator = torch.Generator(device=device)
            generator.manual_seed(seed)
            os.makedirs(args.motion_representation_save_dir, exist_ok=True)
            pipeline.obtain_motion_representation(generator=generator,
                                                  motion_representation_path=os.path.join(args.motion_representation_save_dir, stem + ".pt"),
                                                  video_latents=video_latents, uncond_embeddings=text[0:1])
            generator = torch.Generator(device=device)
            generator.manual_seed(seed)
            config.seed = seed
            latents = pipeline.sample_video(generator=generator, text_embeddings=text, decode=False)
            name = "%s_%s_%d" % (stem, config.new_prompt.strip().replace(" ", "_"), seed)
            torch.save(latents.cpu(), os.path.join(args.generated_videos_save_dir, name + ".pt"))
            graphs[name] = graph_keys()
            done_at[name] = time.time()       # (the copy to the host above has synchronised the stream)
            print(name, "is done")
    with open(os.path.join(args.generated_videos_save_dir, "graphs_%s.json" % threading.current_thread().name), "w") as f:
        gib = (lambda b: round(b / 2 ** 30, 2)) if device.type == "cuda" else (lambda b: None)
        json.dump(dict(lane=lanes.lane_index(), slot=lanes.slot_index(), after_line=graphs, final=graph_keys(), done_at=done_at,
                       reserved_gib=gib(torch.cuda.memory_reserved() if device.type == "cuda" else 0),
                       max_reserved_gib=gib(torch.cuda.max_memory_reserved() if device.type == "cuda" else 0)), f)


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("--examples", type=str, required=True)
    parser.add_argument("--checkpoint", type=str, default=None)
    parser.add_argument("--motion-representation-save-dir", type=str, default="motion_representation/")
    parser.add_argument("--generated-videos-save-dir", type=str, default="generated_videos")
    parser.add_argument("--visible_gpu", type=str, default=None)
    parser.add_argument("--default-seed", type=int, default=2025)
    parser.add_argument("--L", type=int, default=16)
    parser.add_argument("--W", type=int, default=512)
    parser.add_argument("--H", type=int, default=512)
    parser.add_argument("--steps", type=int, default=30)
    parser.add_argument("--guidance-steps", type=int, default=18)
    parser.add_argument("--guidance-scale", type=float, default=0.4)
    parser.add_argument("--tokens", type=int, default=77)
    main(parser.parse_args())
