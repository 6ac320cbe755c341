"""The AnimateDiff v1 / v2 layouts through the public surface: `UNet3DConditionModel(...)` maps the reference's switches onto
the engine config, the module tree / state-dict keys equal the reference model's (key lists recorded in
tests/golden/reference_layouts.pt), a motion-module checkpoint with mid_block.motion_modules.0.* loads through
`load_weights`, what is still unbuilt raises by name, and the UNMODIFIED t2v_video_sample.py runs `main(args)` with a v2
`model_config` (tests/layout_entry_harness.py, a child process; only where the reference tree exists)."""
import os
import subprocess
import sys
import types

import pytest
import torch

import layout_util as LU
from motionclone_amd.models.unet import UNet3DConditionModel
from motionclone_amd.utils.util import load_weights
from oracle import reference_shim as shim
from oracle import unet3d_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "reference_layouts.pt")
MK = dict(num_attention_heads=U.TINY_CONFIG["motion_heads"], num_transformer_block=1,
          attention_block_types=["Temporal_Self", "Temporal_Self"], temporal_position_encoding=True,
          temporal_position_encoding_max_len=32, temporal_attention_dim_div=1, zero_initialize=True)


def model(**switches):
    cfg = U.TINY_CONFIG
    kw = dict(in_channels=4, out_channels=4, block_out_channels=cfg["block_out_channels"], layers_per_block=2,
              cross_attention_dim=cfg["cross_attention_dim"], attention_head_dim=cfg["attention_heads"], use_motion_module=True,
              motion_module_resolutions=[1, 2, 4, 8], motion_module_mid_block=False, motion_module_type="Vanilla",
              use_inflated_groupnorm=True, motion_module_kwargs=dict(MK), unet_use_cross_frame_attention=False,
              unet_use_temporal_attention=False)
    kw.update(switches)
    return UNet3DConditionModel(**kw)


def test_constructor_maps_the_switches_onto_the_engine_config():
    v3 = model().engine_config
    assert (v3["inflated_groupnorm"], v3["motion_mid_block"], v3["motion_decoder_only"], v3["motion_resolutions"]) == \
        (True, False, False, (1, 2, 4, 8))
    v1 = model(use_inflated_groupnorm=False, motion_module_kwargs=dict(MK, temporal_position_encoding_max_len=24)).engine_config
    assert v1["inflated_groupnorm"] is False and v1["motion_pe_max_len"] == 24 and v1["motion_mid_block"] is False
    v2 = model(motion_module_mid_block=True).engine_config
    assert v2["motion_mid_block"] is True and v2["inflated_groupnorm"] is True
    other = model(motion_module_decoder_only=True, motion_module_resolutions=[1, 2]).engine_config
    assert other["motion_decoder_only"] is True and other["motion_resolutions"] == (1, 2)


def test_state_dict_keys_and_module_order_equal_the_reference_models():
    g = torch.load(GOLDEN)
    for name, (sw, _, hooks) in list(LU.LAYOUTS.items()) + [("res12", LU.RES12)]:
        m = model(**sw)
        assert set(m.state_dict()) == set(LU.unpack_keys(g["keys"][name])), name
        hooked = [n for n, _ in m.temporal_attentions() if any(b in n for b in hooks)]
        assert hooked == g["layouts"][name]["hooked"], name
    names = [n for n, _ in model(motion_module_mid_block=True).temporal_attentions()]
    first, total = g["meta"]["first_mid_attention_index"]
    assert len(names) == total and names.index(LU.MID + "temporal_transformer.transformer_blocks.0.attention_blocks.0") == first


def test_what_is_still_unbuilt_raises_by_name():
    for kw, word in ((dict(motion_module_kwargs=dict(MK, attention_block_types=["Temporal_Self"])), "attention_block_types"),
                     (dict(motion_module_kwargs=dict(MK, attention_block_types=["Temporal_Self", "Temporal_Cross"])), "attention_block_types"),
                     (dict(motion_module_kwargs=dict(MK, num_transformer_block=2)), "num_transformer_block"),
                     (dict(motion_module_kwargs=dict(MK, temporal_position_encoding=False)), "temporal_position_encoding"),
                     (dict(motion_module_kwargs=dict(MK, temporal_attention_dim_div=2)), "temporal_attention_dim_div"),
                     (dict(unet_use_cross_frame_attention=True), "unet_use_cross_frame_attention"),
                     (dict(unet_use_temporal_attention=True), "unet_use_temporal_attention")):
        with pytest.raises(NotImplementedError, match=word):
            model(**kw)


def test_checkpoint_round_trip_with_the_mid_block_module(emu_device, tmp_path):
    """a v2 motion-module checkpoint through load_weights: the mid-block tensors arrive in the model and in its engine (eps
    equals the engine built from the same state dict); a v3 model tolerates the extra keys like the reference"""
    dev = emu_device
    g = torch.load(GOLDEN)
    sw, keys, hooks = LU.LAYOUTS["b"]
    sd = LU.layout_state_dict(keys, g["meta"]["mid_proj_out_scale"])
    ckpt = tmp_path / "mm_v2.ckpt"
    torch.save({"state_dict": {k: v for k, v in sd.items() if "motion_modules." in k}}, str(ckpt))
    m = model(**sw)
    m.load_state_dict({k: v for k, v in sd.items() if "motion_modules." not in k}, strict=False)
    pipe = types.SimpleNamespace(unet=m)
    load_weights(pipe, motion_module_path=str(ckpt))
    got = m.state_dict()
    assert all(torch.equal(got[k].float(), sd[k]) for k in sd), "a tensor did not arrive"
    m.input_config = types.SimpleNamespace(motion_guidance_blocks=hooks)
    assert m.engine().hooked_names() == g["layouts"]["b"]["hooked"]
    lat, text, _, _ = LU.inputs()
    out = m(lat.half().expand(2, -1, -1, -1, -1), g["meta"]["t_forward"], text.half()).sample
    assert LU.rel(out, g["layouts"]["b"]["eps"]) < 2e-2
    v3 = model()
    load_weights(types.SimpleNamespace(unet=v3), motion_module_path=str(ckpt))      # mid-block keys: unexpected, ignored
    assert not any(k.startswith("mid_block.motion_modules") for k in v3.state_dict())


@pytest.mark.skipif(not shim.available(), reason="reference tree not present")
def test_unmodified_t2v_script_runs_with_a_v2_model_config(tmp_path):
    g = torch.load(GOLDEN)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.path.join(ROOT, "tests"))
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "layout_entry_harness.py"), str(tmp_path),
                        str(g["meta"]["mid_proj_out_scale"])], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env,
                       cwd=str(tmp_path), timeout=1500)
    assert p.returncode == 0 and "ENTRY_OK v2" in p.stdout, p.stdout[-4000:]
    import entry_harness as EH
    rec = torch.load(os.path.join(str(tmp_path), "record.pt"))
    pt = torch.load(os.path.join(str(tmp_path), "motion_representation", "clip.pt"))
    assert list(pt) == g["layouts"]["b"]["hooked"] and len(pt) == 8       # the .pt's keys: up block 1, then the mid block
    assert rec["loop"]["steps_run"] == EH.STEPS and rec["loop"]["G"] == EH.GUIDED
    assert torch.isfinite(rec["loop"]["last"].float()).all() and len(rec["videos"]) == 1
    # the extraction the script ran IS the engine's on the same noisy latents (the mid-block module included)
    from motionclone_amd import build, lib
    from motionclone_amd.engine import UNet3DEngine
    lib.use_library_for_tests(build.build_emu())
    try:
        sw, keys, hooks = LU.LAYOUTS["b"]
        eng = UNet3DEngine(LU.layout_state_dict(keys, g["meta"]["mid_proj_out_scale"]), LU.engine_config(keys), "cpu", guidance_blocks=hooks)
        ex = rec["extract"]
        rep = eng.extract_representation(ex["noisy"].half().cpu(), ex["t"], ex["text"].half().cpu())
        for k in pt:
            assert (pt[k][0].float() - rep[k][0].float()).abs().max() < 5e-3, k
    finally:
        lib._lib = None
        lib._is_emulated = False
