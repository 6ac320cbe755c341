"""The AnimateDiff v1 / v2 model layouts of the tests: reference switches, engine-config keys, hooks and seeded weights.
Shared by tests/golden/make_layout_records.py (which runs the unmodified reference) and the layout tests (which read only
the recorded results).  Test infrastructure only."""
import math
import zlib
from collections import OrderedDict

import torch

from oracle import unet3d_ref as U

HP = dict(cfg_scale=7.5, motion_guidance_weight=2000.0, warm_up_steps=10, cool_up_steps=10)
N_STEPS, G_STEPS, G_SCALE = 4, 2, 0.3
F, H, W, N_TEXT = 4, 8, 8, 7
FRAME_SCALE = (0.5, 1.0, 1.5, 2.0)       # the frames differ in scale and offset: per-frame statistics are then far from
FRAME_SHIFT = (-0.5, 0.0, 0.5, 1.0)      # video-wide ones (0.57 relative L2 of eps on the tiny config)
MID = "mid_block.motion_modules.0."
MID_SEED = 4321

# name -> (reference constructor switches, engine-config keys, motion_guidance_blocks)
LAYOUTS = OrderedDict([
    ("a", (dict(use_inflated_groupnorm=False),
           dict(inflated_groupnorm=False),
           ["up_blocks.1"])),
    ("b", (dict(motion_module_mid_block=True),
           dict(motion_mid_block=True),
           ["mid_block", "up_blocks.1"])),
    ("c", (dict(use_inflated_groupnorm=False, motion_module_mid_block=True, motion_module_decoder_only=True),
           dict(inflated_groupnorm=False, motion_mid_block=True, motion_decoder_only=True),
           ["mid_block", "up_blocks.1"])),
])
# structural only (no recorded results): motion modules at the two finest resolutions
RES12 = (dict(motion_module_resolutions=[1, 2]), dict(motion_resolutions=(1, 2)), ["up_blocks.3"])


def engine_config(keys):
    return dict(U.TINY_CONFIG, **keys)


def mid_motion_tensors(cfg, proj_out_scale=1.0, seed=MID_SEED):
    """seeded tensors of mid_block.motion_modules.0 (the rule of oracle.unet3d_ref.random_state_dict, own generator);
    `proj_out_scale` multiplies the N(0, 0.02) proj_out weight and bias"""
    g = torch.Generator().manual_seed(seed)
    shapes = U._motion_shapes(MID, cfg["block_out_channels"][-1])
    out = OrderedDict()
    for name, shape in shapes.items():
        if "norm" in name and len(shape) == 1:
            t = (torch.ones(shape) if name.endswith("weight") else torch.zeros(shape)) + 0.05 * torch.randn(shape, generator=g)
        elif "temporal_transformer.proj_out" in name:
            t = 0.02 * proj_out_scale * torch.randn(shape, generator=g)
        else:
            wshape = shapes[name[:-4] + "weight"] if name.endswith("bias") else shape
            fan_in = 1
            for d in wshape[1:]:
                fan_in *= d
            t = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
        out[name] = t
    return out


def has_motion(keys, where, level):
    """does the layout carry motion modules in `where` ('down' / 'up') at resolution level `level` (0 = finest)?"""
    if where == "down" and keys.get("motion_decoder_only", False):
        return False
    return (2 ** level) in tuple(keys.get("motion_resolutions", (1, 2, 4, 8)))


def layout_state_dict(keys, proj_out_scale=1.0, seed=1234):
    """fp16-rounded fp32 weights of a layout: the tiny UNet's seeded weights, plus the mid-block module where the layout has
    one, minus the motion modules it does not have"""
    cfg = U.TINY_CONFIG
    sd = OrderedDict((k, v.half().float()) for k, v in U.random_state_dict(dict(cfg), seed=seed).items())
    if keys.get("motion_mid_block", False):
        sd.update((k, v.half().float()) for k, v in mid_motion_tensors(cfg, proj_out_scale).items())
    out = OrderedDict()
    for k, v in sd.items():
        if ".motion_modules." in k and not k.startswith("mid_block."):
            where, idx = k.split(".")[0], int(k.split(".")[1])
            level = idx if where == "down_blocks" else 3 - idx
            if not has_motion(keys, "down" if where == "down_blocks" else "up", level):
                continue
        out[k] = v
    return out


def inputs():
    """latents / text / reference-video latents / extraction noise; the frames of both latents scaled and shifted"""
    cfg = U.TINY_CONFIG
    lat = torch.randn(1, 4, F, H, W, generator=torch.Generator().manual_seed(2025))
    text = torch.randn(2, N_TEXT, cfg["cross_attention_dim"], generator=torch.Generator().manual_seed(7))
    vid = 0.18215 * torch.randn(1, 4, F, H, W, generator=torch.Generator().manual_seed(11))
    noise = torch.randn(1, 4, F, H, W, generator=torch.Generator().manual_seed(2025))
    sc = torch.tensor(FRAME_SCALE).view(1, 1, F, 1, 1)
    sh = torch.tensor(FRAME_SHIFT).view(1, 1, F, 1, 1)
    lat = lat * sc + sh
    vid = vid * sc + 0.18215 * sh
    return lat.half().float(), text.half().float(), vid.half().float(), noise.half().float()


def rel(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def pack_keys(keys):
    """a state-dict key list as zlib-compressed text (the ~700 names of a layout are 50 KB of repetitive strings)"""
    return zlib.compress("\n".join(keys).encode())


def unpack_keys(blob):
    return zlib.decompress(blob).decode().split("\n")
