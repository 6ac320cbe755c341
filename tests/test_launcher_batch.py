"""`motionclone_amd.launch --batch V`: the UNMODIFIED reference entry scripts, V examples per packed launch sequence.

The launcher cases run the scripts on the host simulator (tests/launcher_batch_harness.py over the stubs and tiny assets of
tests/entry_harness.py: 2 frames, 8 x 8 latents, 3 DDIM steps of which 2 are guided) and compare every example with ONE serial
run of the same script over the same lines: the motion representations bit for bit (extraction and RNG stay per thread), the
videos and the latents they were decoded from within TOL_LOOP = 5e-3 relative L2, the packed-versus-alone bound of
tests/test_packed_dropin_api.py.  They run only where the reference tree exists.  The line-assignment rule and the group object
are tested without any model."""
import glob
import json
import os
import socket
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

from motionclone_amd import lanes
from motionclone_amd.launch import assign
from oracle import reference_shim as shim
from test_packed_dropin_api import TOL_LOOP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
needs_reference = pytest.mark.skipif(not shim.available(), reason="reference tree not present")
HARNESS = os.path.join(ROOT, "tests", "launcher_batch_harness.py")
LINES = {"t2v": 5, "i2v": 2}
TIMEOUT = 1500


def rel(a, b):
    a, b = torch.as_tensor(a).float(), torch.as_tensor(b).float()
    return ((a - b).norm() / b.norm().clamp_min(1e-12)).item()


def child(kind, work, *args, env=None):
    env = dict(os.environ if env is None else env, PYTHONPATH=ROOT)
    return subprocess.Popen([sys.executable, HARNESS, kind, str(work)] + [str(a) for a in args], stdout=subprocess.PIPE,
                            stderr=subprocess.STDOUT, text=True, env=env, cwd=str(work))


def clean_env():
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return env


def prefix_file(work, n, name, edit=None):
    """the first n lines of the serial run's examples file (their serial results are those of the longer file)"""
    with open(os.path.join(str(work), "examples.jsonl")) as f:
        lines = [json.loads(ln) for ln in f.readlines()[:n]]
    if edit:
        edit(lines)
    path = os.path.join(str(work), name)
    with open(path, "w") as f:
        for ln in lines:
            f.write(json.dumps(ln) + "\n")
    return path


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """One serial run per kind, then every launcher job of this module, started together on first use (each takes minutes on
    the host simulator) and waited for - with a timeout - by the case that checks it."""
    state = {}

    def start():
        from motionclone_amd import build
        build.build_emu()          # once, here: the children would otherwise race to rebuild a stale simulator library
        works = {k: tmp_path_factory.mktemp("batch_" + k) for k in LINES}
        serial = {k: child(k, works[k], "serial", "--lines", LINES[k], env=clean_env()) for k in LINES}
        for k, p in serial.items():
            out = p.communicate(timeout=TIMEOUT)[0]
            assert p.returncode == 0 and "ENTRY_OK" in out, out[-4000:]
        t2v, i2v = works["t2v"], works["i2v"]
        four = prefix_file(t2v, 4, "four.jsonl")

        def missing(lines):
            lines[1]["video_path"] = os.path.join(str(t2v), "no_such_clip.mp4")
        bad = prefix_file(t2v, 2, "bad.jsonl", missing)
        env = clean_env()
        procs = {
            "one_lane": [child("t2v", t2v, "launch", "--lanes", 1, "--batch", 2, "--examples", four, "--tag", "one_lane", env=env)],
            "two_lanes": [child("t2v", t2v, "launch", "--lanes", 2, "--batch", 2, "--tag", "two_lanes", env=env)],
            "i2v": [child("i2v", i2v, "launch", "--lanes", 1, "--batch", 2, "--tag", "i2v", env=env)],
            "raises": [child("t2v", t2v, "launch", "--lanes", 1, "--batch", 2, "--examples", bad, "--tag", "raises", env=env)],
        }
        with socket.socket() as s:
            s.bind(("127.0.0.1", 0))
            port = s.getsockname()[1]
        procs["two_ranks"] = [child("t2v", t2v, "launch", "--lanes", 1, "--batch", 2, "--examples", four, "--tag", "two_ranks",
                                    env=dict(env, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                                             MASTER_PORT=str(port))) for r in range(2)]
        state.update(works=works, procs=procs, outs={})

    def get(name):
        if not state:
            start()
        if name not in state["outs"]:
            # a stuck meeting point is a failure, not a hang: TimeoutExpired fails the case, the teardown kills the child
            state["outs"][name] = [(p.communicate(timeout=TIMEOUT)[0], p.returncode) for p in state["procs"][name]]
        return state["works"]["i2v" if name == "i2v" else "t2v"], state["outs"][name]
    yield get
    for ps in state.get("procs", {}).values():
        for p in ps:
            if p.poll() is None:
                p.kill()


def check_against_serial(work, tag, outs, n_lines, world, n_lanes, batch, job_sizes):
    work = str(work)
    for out, code in outs:
        assert code == 0 and "ENTRY_OK" in out, out[-4000:]
    head = [json.loads(ln) for ln in outs[0][0].splitlines() if ln.startswith('{"examples"')][0]
    assert head["batch"] == batch and head["lanes"] == n_lanes and head["world"] == world and head["examples"] == n_lines
    # the launch sequences that ran: full groups of `batch` videos, the rest of a lane alone
    for r, (out, _) in enumerate(outs):
        got = [json.loads(ln.split(" ", 1)[1]) for ln in out.splitlines() if ln.startswith("JOB_SIZES")][0]
        assert got == sorted(job_sizes[r]), (r, got)
    videos = sorted(glob.glob(os.path.join(work, "videos_%s_rank*" % tag, "*.mp4.npy")))
    assert len(videos) == n_lines, videos                         # every line ran exactly once ...
    lat = {}
    for i in range(n_lines):
        rank, lane, slot, _ = assign(i, world, n_lanes, batch)
        mine = [v for v in videos if os.path.basename(v).startswith("clip%d_" % i)]
        assert len(mine) == 1 and os.sep + "videos_%s_rank%d" % (tag, rank) + os.sep in mine[0], (i, mine)    # ... on its rank
        reps = glob.glob(os.path.join(work, "mr_" + tag, "*", "clip%d.pt" % i))
        assert [os.path.basename(os.path.dirname(p)) for p in reps] == ["rank%d_lane%d_slot%d" % (rank, lane, slot)], (i, reps)
        got, want = torch.load(reps[0]), torch.load(os.path.join(work, "mr_serial", "clip%d.pt" % i))
        assert list(got) == list(want)
        for k in want:
            assert torch.equal(got[k][0], want[k][0]) and torch.equal(got[k][1], want[k][1]), (i, k)
        serial_video = glob.glob(os.path.join(work, "videos_serial", "clip%d_*.mp4.npy" % i))[0]
        assert os.path.basename(serial_video) == os.path.basename(mine[0])
        lat[i] = torch.load(os.path.join(os.path.dirname(mine[0]), "clip%d.latents.pt" % i))
        want_lat = torch.load(os.path.join(work, "videos_serial", "clip%d.latents.pt" % i))
        e_lat = rel(lat[i], want_lat)
        e_vid = rel(np.load(mine[0]).astype(np.float32), np.load(serial_video).astype(np.float32))
        print("%s line %d: latents %.3e, video %.3e" % (tag, i, e_lat, e_vid))
        assert e_lat < TOL_LOOP and e_vid < TOL_LOOP, (i, e_lat, e_vid)
    assert rel(lat[0], lat[1]) > TOL_LOOP              # different lines are different videos: the comparison is not vacuous


@needs_reference
def test_one_lane_of_two_slots_reproduces_the_serial_run(runs):
    work, outs = runs("one_lane")
    check_against_serial(work, "one_lane", outs, 4, 1, 1, 2, [[2, 2]])


@needs_reference
def test_two_lanes_of_two_slots_with_a_lone_last_member(runs):
    """lines 0, 1 -> lane 0; 2, 3 -> lane 1; line 4 -> lane 0 again, slot 0, alone: the plain one-video path"""
    assert [assign(i, 1, 2, 2)[1:] for i in range(5)] == [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0), (0, 0, 1)]
    work, outs = runs("two_lanes")
    check_against_serial(work, "two_lanes", outs, 5, 1, 2, 2, [[1, 2, 2]])


@needs_reference
def test_image_to_video_with_one_condition_image_per_member(runs):
    """latent-condition SparseCtrl: slot 1 skips line 0 and must burn its reference-video AND condition-image draws to extract
    line 1's representation bit for bit"""
    work, outs = runs("i2v")
    check_against_serial(work, "i2v", outs, 2, 1, 1, 2, [[2]])


@needs_reference
def test_two_ranks_times_two_slots(runs):
    """rank 0 groups lines 0 and 2, rank 1 lines 1 and 3"""
    work, outs = runs("two_ranks")
    check_against_serial(work, "two_ranks", outs, 4, 2, 1, 2, [[2], [2]])


@needs_reference
def test_a_member_that_raises_ends_the_launcher(runs):
    """line 1 names a reference video that does not exist: slot 1 raises while slot 0 waits for it at the meeting point"""
    _, outs = runs("raises")                 # (the fixture's timeout is the check that nobody waits for ever)
    (out, code), = outs
    assert code not in (0, None), out[-4000:]
    assert "ENTRY_OK" not in out and "no_such_clip.mp4" in out and "FileNotFoundError" in out, out[-4000:]
    assert "TimeoutError" not in out and "deadlock" not in out.lower(), out[-4000:]


@pytest.mark.parametrize("world", [1, 2])
@pytest.mark.parametrize("n_lanes", [1, 2, 3])
@pytest.mark.parametrize("batch", [1, 2, 5])
def test_line_assignment_rule(world, n_lanes, batch):
    for n_lines in range(24):
        owners = {}
        for i in range(n_lines):
            rank, lane, slot, grp = assign(i, world, n_lanes, batch)
            assert 0 <= rank < world and 0 <= lane < n_lanes and 0 <= slot < batch
            owners.setdefault((rank, lane, grp), []).append((slot, i))
            if batch == 1:       # today's rule: virtual rank = rank + world * lane of world * n_lanes
                assert i % (world * n_lanes) == rank + world * lane and slot == 0
        # owned exactly once: `assign` is a function of i, and no two lines share (rank, lane, group, slot)
        assert sum(len(v) for v in owners.values()) == n_lines
        for (rank, lane, grp), members in owners.items():
            slots = [s for s, _ in members]
            assert slots == list(range(len(slots)))                      # filled from slot 0, every slot once
            mine = [i for i in range(n_lines) if i % world == rank]      # the rank's lines, in order
            at = mine.index(members[0][1])
            assert [i for _, i in members] == mine[at:at + len(members)]  # a run of consecutive lines of the rank
            assert at % batch == 0 and (len(members) == batch or mine[at + len(members):] == [])   # only the last is short


def run_threads(targets):
    errors, threads = [], []
    for t in targets:
        def guarded(t=t):
            try:
                t()
            except BaseException as e:   # noqa: BLE001
                errors.append(e)
        threads.append(threading.Thread(target=guarded))
        threads[-1].start()
    for th in threads:
        th.join(timeout=30)
        assert not th.is_alive(), "a group member is stuck at the meeting point"
    return errors


def test_group_members_meet_leave_and_the_lowest_live_slot_leads():
    grp = lanes.Group(3)
    assert grp.leader() == 0 and grp.live() == [0, 1, 2]
    log, got = [], {}

    def run(items):
        log.append((threading.current_thread().name, list(items)))
        return [10 * it for it in items]

    def member(slot, rounds):
        def go():
            threading.current_thread().name = "slot%d" % slot
            for r in range(rounds):
                got[(slot, r)] = grp.meet(slot, 100 * r + slot, run)
            grp.leave(slot)
        return go
    # slot 0 has one line, slot 1 two, slot 2 three: the group shrinks, the leadership moves up
    assert run_threads([member(0, 1), member(1, 2), member(2, 3)]) == []
    assert log == [("slot0", [0, 1, 2]), ("slot1", [101, 102]), ("slot2", [202])]
    assert got == {(0, 0): 0, (1, 0): 10, (2, 0): 20, (1, 1): 1010, (2, 1): 1020, (2, 2): 2020}
    assert grp.live() == [] and grp.leader() is None


def test_group_error_is_reraised_in_every_member():
    # a member that fails elsewhere (its script raised): the two that wait for it re-raise its error
    grp = lanes.Group(3)
    boom = FileNotFoundError("no such reference video")
    waiting = threading.Barrier(3)

    def waits(slot):
        def go():
            waiting.wait(timeout=30)
            grp.meet(slot, slot, lambda items: items)
        return go

    def fails():
        waiting.wait(timeout=30)
        grp.fail(boom)
        grp.leave(2)
    errors = run_threads([waits(0), waits(1), fails])
    assert len(errors) == 2 and all(e is boom for e in errors)
    with pytest.raises(FileNotFoundError):       # and whoever comes later
        grp.meet(0, 0, lambda items: items)
    # the leader's packed run raises (a mixed group): every member gets that error
    grp = lanes.Group(2)

    def run(items):
        raise ValueError("either every example carries a condition image or none does")
    errors = run_threads([lambda: grp.meet(0, "a", run), lambda: grp.meet(1, "b", run)])
    assert len(errors) == 2 and all(isinstance(e, ValueError) and "condition image" in str(e) for e in errors)
