"""`motionclone_amd.launch --batch V` where the packed steps replay from hipGraphs: on the GPU.  The reference tree is not there,
so the launcher runs tools/standin_video_sample.py (the reference script's call sequence over synthetic inputs) on a tiny
checkpoint written here: TINY_CONFIG, 4 frames, 8 x 8 latents, 3 DDIM steps of which 2 are guided.  And, in process, the packed
loop factored out of `sample_video_batch` (what a group's leader runs) against `sample_video_batch` itself."""
import glob
import json
import os
import subprocess
import sys

import pytest
import torch

from motionclone_amd.launch import assign
from motionclone_amd.utils import motionclone_functions as mf
from oracle import unet3d_ref as U
from test_packed_dropin_api import TOL_LOOP, i2v_pipeline, make_examples, rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS, GUIDED, FRAMES, N_LINES = 3, 2, 4, 6


def launch(work, tag, n_lanes, batch):
    """ONE child process with the GPU open; a fault, an abort or a timeout fails the test right here"""
    out_dir = os.path.join(work, tag)
    cmd = [sys.executable, "-m", "motionclone_amd.launch", "--lanes", str(n_lanes), "--batch", str(batch),
           os.path.join(ROOT, "tools", "standin_video_sample.py"), "--examples", os.path.join(work, "examples.jsonl"),
           "--checkpoint", os.path.join(work, "tiny.pt"), "--motion-representation-save-dir", os.path.join(out_dir, "mr"),
           "--generated-videos-save-dir", os.path.join(out_dir, "out"), "--L", str(FRAMES), "--H", "64", "--W", "64",
           "--steps", str(STEPS), "--guidance-steps", str(GUIDED), "--guidance-scale", "0.3", "--tokens", "7"]
    env = dict(os.environ, PYTHONPATH=ROOT)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, env=env, cwd=ROOT, timeout=300)
    assert p.returncode == 0, "launcher exited with %s\n%s" % (p.returncode, p.stdout[-4000:])
    head = [json.loads(ln) for ln in p.stdout.splitlines() if ln.startswith('{"examples"')][0]
    assert head["examples"] == N_LINES and head["lanes"] == n_lanes and head["batch"] == batch
    return out_dir


@pytest.mark.gpu
def test_launcher_groups_replay_packed_graphs_and_match_the_serial_run(gpu_device, tmp_path):
    work = str(tmp_path)
    cfg = dict(U.TINY_CONFIG)
    sd = {k: v.half().float() for k, v in U.random_state_dict(cfg, seed=1234).items()}
    torch.save(dict(config=cfg, state_dict=sd), os.path.join(work, "tiny.pt"))
    with open(os.path.join(work, "examples.jsonl"), "w") as f:
        for i in range(N_LINES):
            f.write(json.dumps(dict(video_path="clip%d.mp4" % i, new_prompt="a dog walks %d" % i, seed=2026 + i)) + "\n")
    packed = launch(work, "packed", 2, 2)
    names = ["clip%d_a_dog_walks_%d_%d" % (i, i, 2026 + i) for i in range(N_LINES)]
    assert sorted(os.path.basename(p) for p in glob.glob(os.path.join(packed, "out", "clip*.pt"))) == [n + ".pt" for n in names]

    # lines 0, 1 and 4, 5 are lane 0's two groups, lines 2, 3 lane 1's only one; the leader is slot 0
    assert [assign(i, 1, 2, 2)[1:] for i in range(N_LINES)] == [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1), (0, 1, 1)]
    per_step = [[i, 2] for i in range(STEPS)]
    for lane in range(2):
        with open(os.path.join(packed, "out", "graphs_lane%d_slot0.json" % lane)) as f:
            g = json.load(f)
        assert (g["lane"], g["slot"]) == (lane, 0)
        assert g["final"] == per_step, g         # one packed graph per step index, latent batch 2, and no one-video graph
        first = names[0] if lane == 0 else names[2]
        assert g["after_line"][first] == per_step
        with open(os.path.join(packed, "out", "graphs_lane%d_slot1.json" % lane)) as f:
            assert json.load(f)["final"] == []                           # members that never lead capture nothing
    with open(os.path.join(packed, "out", "graphs_lane0_slot0.json")) as f:
        g = json.load(f)
    assert g["after_line"][names[4]] == g["after_line"][names[0]]        # the second group replayed: nothing captured anew

    serial = launch(work, "serial", 1, 1)        # started after the first child has exited with status 0
    lat = {}
    for i, name in enumerate(names):
        _, lane, slot, _ = assign(i, 1, 2, 2)
        got = torch.load(os.path.join(packed, "mr", "rank0_lane%d_slot%d" % (lane, slot), "clip%d.pt" % i))
        want = torch.load(os.path.join(serial, "mr", "clip%d.pt" % i))
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][1], want[k][1]), (i, k)
        lat[i] = torch.load(os.path.join(packed, "out", name + ".pt"))
        e = rel(lat[i], torch.load(os.path.join(serial, "out", name + ".pt")))
        print("line %d packed in its group vs the serial run: %.3e" % (i, e))
        assert e < TOL_LOOP, (i, e)
    assert rel(lat[0], lat[1]) > TOL_LOOP and rel(lat[0], lat[4]) > TOL_LOOP


def test_packed_loop_on_prepared_inputs_equals_sample_video_batch(backend):
    """what a group's leader runs - `_packed_sample` on per-video inputs prepared by sequential one-video calls - gives what
    `sample_video_batch` gives for the same examples, bit for bit"""
    dev = backend
    frames = 2 if dev.type == "cpu" else 4
    pipe, cfg = i2v_pipeline(dev, frames=frames)
    want = pipe.sample_video_batch(make_examples(cfg, dev, frames, (1, 2)), decode=False)
    exs = make_examples(cfg, dev, frames, (1, 2))
    c = pipe.input_config
    reps, lats, ctrls = [], [], []
    for ex in exs:
        reps.append(pipe.obtain_motion_representation(generator=ex["generator"], use_controlnet=True,
                                                      video_latents=ex["video_latents"], uncond_embeddings=ex["uncond_embeddings"]))
        lats.append(pipe.prepare_latents(1, 4, frames, c.height, c.width, torch.float16, dev, ex["generator"], None))
        cond, mask = mf._placed(ex["controlnet_images"].to(dev, torch.float16), c.image_index, frames=frames)
        ctrls.append(dict(cond=cond, mask=mask, scale=c.controlnet_scale))
    got = mf._packed_sample(pipe, lats, [ex["text_embeddings"] for ex in exs], reps, ctrls)
    assert got.shape == (2, 4, frames, 8, 8)
    for v in range(2):
        print("packed loop on prepared inputs, example %d: %.3e" % (v, rel(got[v:v + 1], want[v])))
        assert torch.equal(got[v:v + 1], want[v]), v
    with pytest.raises(ValueError, match="every example carries a condition image or none"):
        mf._packed_sample(pipe, lats, [ex["text_embeddings"] for ex in exs], reps, [ctrls[0], None])
    with pytest.raises(ValueError, match="share one conditioning scale"):
        mf._packed_sample(pipe, lats, [ex["text_embeddings"] for ex in exs], reps, [ctrls[0], dict(ctrls[1], scale=0.5)])
