"""TEST INFRASTRUCTURE for tests/test_launcher_batch.py: the UNMODIFIED reference entry scripts through
`motionclone_amd.launch --lanes L --batch V`, in a child process, on the stubs / tiny assets of tests/entry_harness.py:

    python tests/launcher_batch_harness.py {t2v|i2v} WORKDIR serial  --lines N
    python tests/launcher_batch_harness.py {t2v|i2v} WORKDIR launch  --lanes L --batch V [--examples FILE] [--tag NAME]

`serial` writes the assets and an examples file of N lines - every line with its own reference video, prompt, seed and (i2v)
condition image - and runs the script's `main(args)` in one process: the run everything else is compared with.  `launch` runs
the launcher (under the torchrun environment's ranks) on the same assets.  Both record, per example, the latents that entered
`decode_latents` next to the videos: `<stem>.latents.pt`; `launch` prints the number of videos of every launch sequence
(JOB_SIZES).  2 frames, 8 x 8 latents, 3 DDIM steps of which 2 are guided."""
import argparse
import json
import os
import runpy
import sys

import numpy as np
import torch

import entry_harness as EH

FRAMES = 2


def write_examples(work, kind, n):
    rng = np.random.RandomState(11)
    px = EH.px_of(kind)
    with open(os.path.join(work, "examples.jsonl")) as f:
        base = json.loads(f.readline())
    with open(os.path.join(work, "examples.jsonl"), "w") as f:
        for i in range(n):
            np.save(os.path.join(work, "clip%d.mp4.npy" % i), rng.randint(0, 256, size=(9, 20, 24, 3)).astype(np.uint8))
            ex = dict(base, video_path=os.path.join(work, "clip%d.mp4" % i), new_prompt="a dog walks %d" % i, seed=2026 + i)
            if kind == "i2v":
                from PIL import Image
                img = os.path.join(work, "cond%d.png" % i)
                Image.fromarray(rng.randint(0, 256, size=(px, px, 3)).astype(np.uint8)).save(img)
                ex["condition_image_paths"] = [img]
            f.write(json.dumps(ex) + "\n")


def record_latents(written_dir_of):
    """every decode_latents call leaves its input next to the video the script is about to write"""
    from motionclone_amd.pipelines.pipeline_animation import AnimationPipeline
    decode = AnimationPipeline.decode_latents

    def decode_latents(self, latents):
        c = self.input_config
        stem = os.path.splitext(os.path.basename(c.video_path))[0]
        os.makedirs(written_dir_of(), exist_ok=True)
        torch.save(latents.detach().cpu().clone(), os.path.join(written_dir_of(), stem + ".latents.pt"))
        return decode(self, latents)
    AnimationPipeline.decode_latents = decode_latents


def record_job_sizes(sizes):
    """the number of videos of every launch sequence that starts (step 0 of MotionCloneSampler.step)"""
    from motionclone_amd.sampler import MotionCloneSampler
    step = MotionCloneSampler.step

    def rstep(self, latents, i, *a, **k):
        if i == 0:
            sizes.append(int(latents.shape[0]))
        return step(self, latents, i, *a, **k)
    MotionCloneSampler.step = rstep


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("kind", choices=["t2v", "i2v"])
    ap.add_argument("work")
    ap.add_argument("mode", choices=["serial", "launch"])
    ap.add_argument("--lines", type=int, default=4)
    ap.add_argument("--lanes", default="1")
    ap.add_argument("--batch", default="1")
    ap.add_argument("--examples", default=None)
    ap.add_argument("--tag", default="run")
    a = ap.parse_args()
    kind, work = a.kind, os.path.abspath(a.work)
    os.makedirs(work, exist_ok=True)
    sys.path.insert(0, EH.ROOT)
    if not torch.cuda.is_available():
        from motionclone_amd import build, lib
        lib.use_library_for_tests(build.build_emu())
        EH.map_cuda_to_cpu()
    written = EH.install_stubs(work)
    script = os.path.join(EH.REFERENCE_ROOT, "t2v_video_sample.py" if kind == "t2v" else "i2v_video_sample.py")
    px = EH.px_of(kind)
    sd_path, infer = os.path.join(work, "sd"), os.path.join(work, "infer.yaml")
    if a.mode == "serial":
        EH.write_assets(work, kind, 1)
        write_examples(work, kind, a.lines)
        out = os.path.join(work, "videos_serial")
        record_latents(lambda: out)
        ns = runpy.run_path(script, run_name="entry_script_under_test")
        ns["main"](argparse.Namespace(motion_representation_save_dir=os.path.join(work, "mr_serial"), generated_videos_save_dir=out,
                                      visible_gpu=None, default_seed=2025, L=FRAMES, W=px, H=px, without_xformers=False,
                                      pretrained_model_path=sd_path, inference_config=infer,
                                      examples=os.path.join(work, "examples.jsonl")))
    else:
        from motionclone_amd import launch as L
        rank = int(os.environ.get("RANK", 0))
        out = os.path.join(work, "videos_%s_rank%d" % (a.tag, rank))
        record_latents(lambda: out)
        sizes = []
        record_job_sizes(sizes)
        L.main([script, "--pretrained-model-path", sd_path, "--inference_config", infer, "--examples",
                a.examples or os.path.join(work, "examples.jsonl"), "--motion-representation-save-dir",
                os.path.join(work, "mr_" + a.tag), "--generated-videos-save-dir", out, "--L", str(FRAMES), "--W", str(px), "--H", str(px),
                "--vae-scale", "2", "--lanes", a.lanes, "--batch", a.batch])
        print("JOB_SIZES", json.dumps(sorted(sizes)))
    print("ENTRY_OK", kind, written)


if __name__ == "__main__":
    main()
