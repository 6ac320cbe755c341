"""TEST INFRASTRUCTURE.  tests/entry_harness.py's machinery (imported, not edited) with an AnimateDiff v2 `model_config`:
the UNMODIFIED reference t2v_video_sample.py runs `main(args)` against this repo's drop-in package with
motion_module_mid_block = true, a motion-module checkpoint that holds mid_block.motion_modules.0.* and
motion_guidance_blocks = ["mid_block", "up_blocks.1"], in a child process:

    python tests/layout_entry_harness.py WORKDIR [proj_out scale of the mid-block module]"""
import argparse
import os
import runpy
import sys

import torch
import yaml

import entry_harness as EH
import layout_util as LU

HOOKS = ["mid_block", "up_blocks.1"]


def main():
    work = os.path.abspath(sys.argv[1])
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    os.makedirs(work, exist_ok=True)
    sys.path.insert(0, EH.ROOT)
    assert not any(os.path.abspath(p) == EH.REFERENCE_ROOT for p in sys.path)
    if not torch.cuda.is_available():
        from motionclone_amd import build, lib
        lib.use_library_for_tests(build.build_emu())
        EH.map_cuda_to_cpu()
    written = EH.install_stubs(work)
    EH.write_assets(work, "t2v", 1)
    # the v2 layout on top of the assets: model_config switches, the motion-module checkpoint, the hooks
    switches, keys, _ = LU.LAYOUTS["b"]
    mc_path = os.path.join(work, "model_config.yaml")
    mc = yaml.safe_load(open(mc_path))
    mc["unet_additional_kwargs"].update(switches)
    yaml.safe_dump(mc, open(mc_path, "w"))
    sd = LU.layout_state_dict(keys, scale)
    torch.save({"state_dict": {k: v for k, v in sd.items() if "motion_modules." in k}}, os.path.join(work, "mm.ckpt"))
    inf_path = os.path.join(work, "infer.yaml")
    infer = yaml.safe_load(open(inf_path))
    infer["motion_guidance_blocks"] = list(HOOKS)
    yaml.safe_dump(infer, open(inf_path, "w"))
    rec = {}
    EH.install_recorders(rec)
    ns = runpy.run_path(os.path.join(EH.REFERENCE_ROOT, "t2v_video_sample.py"), run_name="entry_script_under_test")
    import motionclone.models.unet as mu
    assert os.path.abspath(mu.__file__).startswith(EH.ROOT), mu.__file__
    args = argparse.Namespace(motion_representation_save_dir=os.path.join(work, "motion_representation"),
                              generated_videos_save_dir=os.path.join(work, "generated_videos"), visible_gpu=None,
                              default_seed=2025, L=EH.F, W=EH.PX, H=EH.PX, without_xformers=False,
                              pretrained_model_path=os.path.join(work, "sd"), inference_config=inf_path,
                              examples=os.path.join(work, "examples.jsonl"))
    ns["main"](args)
    rec["videos"] = written
    torch.save(rec, os.path.join(work, "record.pt"))
    print("ENTRY_OK v2", written)


if __name__ == "__main__":
    main()
