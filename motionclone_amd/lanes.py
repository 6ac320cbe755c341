"""Several examples in flight inside ONE process / GPU ("lanes"): what `motionclone_amd.launch --lanes K` runs on.

A lane is a host thread with its own HIP stream that executes the UNMODIFIED entry script on its share of the examples file.
Independent (prompt, reference-video) examples are the unit of parallelism of this workload; K of them on one
GPU fill each other's kernel tails and under-filled launches (bench.py: +14-20 % videos/min for three in flight).

The one piece of shared state the scripts rely on is torch's GLOBAL generator: `set_all_seed(42)` once, then every example's
VAE posterior draw comes from it, so an example's result depends on how many examples ran before it.
Threads would interleave those draws, so inside a lane the "global" stream is a LANE-PRIVATE generator: `set_all_seed` seeds
it, the drop-in VAE draws from it, and the launcher burns the draws of the examples the lane skips - each lane reproduces the
serial run's stream position for every example it owns, and the results stay bit-identical to the single-process run.

`--batch V` puts V script threads ("slots") on one lane.  Each slot is a thread like the above - its own lines, its own private
serial stream, its own models - but the V of them bring their examples to the lane's `Group`, where the member with the lowest
live slot runs ONE packed launch sequence for all of them (utils/motionclone_functions.py, `sample_video`)."""
import threading

import torch

_LOCAL = threading.local()


class Group:
    """The meeting point of the script threads of one lane.  Every live member brings one item to `meet`; when all of them
    have, the member with the lowest live slot (the leader) calls its `run` on the items in slot order and every member gets its
    own entry of the list `run` returns.  A member whose script has no further line `leave`s: the others then wait for the
    members still alive only, so a group that does not fill runs short.  A member that fails publishes the exception with
    `fail`; every member that waits, or meets later, re-raises it - nobody waits for a member that will not come."""

    def __init__(self, size):
        self.size = size
        self.stream = None         # the lane's HIP stream for the packed steps (opened by the first leader)
        self._cv = threading.Condition()
        self._live = set(range(size))
        self._pending, self._results = {}, {}
        self._running = False
        self._error = None

    def live(self):
        with self._cv:
            return sorted(self._live)

    def leader(self):
        """the lowest live slot (None once every member has left)"""
        with self._cv:
            return min(self._live) if self._live else None

    def leave(self, slot):
        with self._cv:
            self._live.discard(slot)
            self._pending.pop(slot, None)
            self._cv.notify_all()

    def fail(self, exc):
        with self._cv:
            if self._error is None:
                self._error = exc
            self._cv.notify_all()

    def meet(self, slot, item, run):
        with self._cv:
            if self._error is not None:
                raise self._error
            if slot not in self._live:
                raise RuntimeError("slot %d has left its group" % slot)
            self._pending[slot] = item
            self._cv.notify_all()
            while True:
                if self._error is not None:
                    raise self._error
                if slot in self._results:
                    return self._results.pop(slot)
                if not self._running and slot in self._pending and slot == min(self._live) and set(self._pending) >= self._live:
                    items = sorted(self._pending.items())
                    self._pending = {}
                    self._running = True
                    break
                self._cv.wait()
        try:                           # the leader, outside the lock: members that leave or fail meanwhile are not held up
            results = list(run([it for _, it in items]))
            if len(results) != len(items):
                raise RuntimeError("the group's run returned %d results for %d members" % (len(results), len(items)))
        except BaseException as e:     # noqa: BLE001 - published to the members, re-raised here
            self.fail(e)
            raise
        with self._cv:
            self._running = False
            for (s, _), r in zip(items, results):
                if s != slot:
                    self._results[s] = r
            self._cv.notify_all()
        return results[[s for s, _ in items].index(slot)]


def set_example(line):
    """the launcher's note for the calling thread: the parsed examples-file line its script is working on (None: none).  The
    entry scripts read a fixed set of keys from a line; optional per-example keys of this package (`motion_references`) are
    looked up here by the drop-in functions."""
    _LOCAL.example = line


def example():
    """the examples-file line of the calling thread's current example ({} outside a launcher run)"""
    return getattr(_LOCAL, "example", None) or {}


def begin(lane, n_lanes, device, slot=0, group=None):
    """mark the calling thread as slot `slot` of lane `lane` of `n_lanes`; its serial-RNG stream lives on `device`; `group` is the
    lane's `Group` when the lane carries several examples per launch sequence"""
    _LOCAL.lane, _LOCAL.n, _LOCAL.dev, _LOCAL.gen, _LOCAL.warm = lane, n_lanes, torch.device(device), None, False
    _LOCAL.slot, _LOCAL.group = slot, group


def warmed_up():
    """called by the launcher when the lane's first example is done: from here on the lanes run concurrently"""
    _LOCAL.warm = True


def may_capture():
    """hipGraph capture is only done while a lane runs ALONE (its first example: the launcher serialises those).  ROCm 7.2
    rejects synchronising calls of ANY host thread while a capture is open (hipErrorStreamCaptureUnsupported, also in
    thread-local capture mode), so a step whose graph is missing once the lanes run concurrently is issued eagerly."""
    return not active() or not getattr(_LOCAL, "warm", False)


def end():
    grp = group()
    if grp is not None:
        grp.leave(_LOCAL.slot)
    _LOCAL.lane = _LOCAL.group = None


def active():
    return getattr(_LOCAL, "lane", None) is not None


def lane_index():
    return getattr(_LOCAL, "lane", None)


def slot_index():
    """the thread's slot inside its lane (0 where a lane carries one example at a time); None outside a lane"""
    return getattr(_LOCAL, "slot", 0) if active() else None


def group():
    """the lane's `Group`, or None: outside a lane, and where a lane carries one example at a time"""
    return getattr(_LOCAL, "group", None) if active() else None


def seed(value):
    """set_all_seed inside a lane: (re)seed the lane's private stream the way torch.manual_seed seeds the global one"""
    if active():
        g = torch.Generator(device=_LOCAL.dev)
        g.manual_seed(int(value))
        _LOCAL.gen = g


def serial_generator():
    """None outside a lane (= torch's global generator, the reference's behaviour); the lane's stream inside one"""
    if not active():
        return None
    if _LOCAL.gen is None:   # a script that never seeds: same default the global generator would have had is unknowable
        seed(torch.initial_seed())
    return _LOCAL.gen
