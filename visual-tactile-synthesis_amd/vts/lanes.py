"""The concurrent lanes of a step schedule.

A lane is one stream plus everything a chain of launches on that stream must not share with a chain that runs beside it: the grow-only
scratch buffers, the counters of the fused finalize, and the arena and job list of its deferred weight-gradient partials.  Lane 0 is the
launch stream; lane n runs on side stream n - 1 of its device.  `enter` makes a lane current, `Fork` opens side lanes beside the
current stream and joins them back.  Nothing here launches: the wrappers of ops.py allocate from `current()`, engine.py schedules.
"""
import contextlib

import torch

_lanes = {}        # (device index, lane number) -> Lane
_streams = {}      # device index -> its side streams, in the order they were created
_retired = []      # outgrown buffers whose address a captured graph may still hold: kept alive, never reused
_reserved = set()  # lane numbers with a fixed owner (engine.SideQueue): no Fork hands them out
_discard_hooks = []
_current = 0       # number of the lane the wrappers allocate from
_base = 0          # number of side lanes taken by the forks that are open around the launch stream
_defer = 0         # nesting depth of ops.deferred_wgrad


class _Arena:
    """bump allocator over grow-only blocks; the allocation sequence of a training step is the same every step, so a reset
    at every flush hands out the same addresses again (captured HIP graphs stay valid; blocks are never freed)"""

    def __init__(self, device):
        self.device, self.blocks, self.cur, self.off = device, [], 0, 0

    def alloc(self, nfloats):
        nfloats = (int(nfloats) + 63) // 64 * 64
        while True:
            if self.cur < len(self.blocks):
                b = self.blocks[self.cur]
                if self.off + nfloats <= b.numel():
                    t = b[self.off:self.off + nfloats]
                    self.off += nfloats
                    return t
                if self.off == 0:      # an empty block that is too small: replace it by a larger one (the old one stays alive)
                    _retired.append(b)
                    self.blocks[self.cur] = torch.empty(max(nfloats, 2 * b.numel()), dtype=torch.float32, device=self.device)
                    continue
                self.cur, self.off = self.cur + 1, 0
            else:
                self.blocks.append(torch.empty(max(nfloats, 16 << 20), dtype=torch.float32, device=self.device))

    def reset(self):
        self.cur, self.off = 0, 0


class Lane:
    def __init__(self, device, index):
        self.device, self.index = device, index
        self.ws = self.stat_ws = self.counter_ws = None
        self.arena = _Arena(device)
        self.pending = []      # reduce jobs dict(dw, nel, accumulate, segs), in enqueue order
        self.by_dw = {}        # dw.data_ptr() -> its pending job

    @property
    def stream(self):
        """None for lane 0 (whatever stream the caller launches on), else side stream index - 1; the side streams of a device are
        created in order, up to the highest one asked for so far"""
        if self.index == 0:
            return None
        pool = _streams.setdefault(self.device.index, [])
        while len(pool) < self.index:
            pool.append(torch.cuda.Stream())
        return pool[self.index - 1]

    def _grow(self, name, nfloats, floor, frozen):
        t = getattr(self, name)
        if t is None or t.numel() < nfloats:
            if t is not None and frozen:
                _retired.append(t)   # captured HIP graphs hold the old pointer: keep that buffer alive, never reuse it
            t = torch.empty(max(int(nfloats), 2 * (t.numel() if t is not None else 0), floor), dtype=torch.float32, device=self.device)
            setattr(self, name, t)
        return t

    def workspace(self, nfloats, frozen):
        return self._grow("ws", nfloats, 1 << 20, frozen)

    def stat_workspace(self, nfloats, frozen):
        return self._grow("stat_ws", nfloats, 1 << 18, frozen)

    def counters(self):
        if self.counter_ws is None:
            self.counter_ws = torch.zeros(1 << 16, dtype=torch.int32, device=self.device)
        return self.counter_ws

    def enqueue(self, dw, nel, accumulate, seg):
        """seg = (partials, copies): one more contribution to dw, reduced at this lane's next flush"""
        q = self.by_dw.get(dw.data_ptr())
        if q is not None:
            assert accumulate, "a second deferred contribution to a weight gradient must accumulate"
            q["segs"].append(seg)
        else:
            q = self.by_dw[dw.data_ptr()] = dict(dw=dw, nel=nel, accumulate=accumulate, segs=[seg])
            self.pending.append(q)

    def pending_bytes(self):
        return sum(4.0 * pw * q["nel"] for q in self.pending for _, pw in q["segs"])

    def clear(self):
        """forget the pending jobs (reduced, or abandoned) and rewind the arena"""
        self.pending = []
        self.by_dw.clear()
        self.arena.reset()


def lane(n, device=None):
    d = torch.device(device) if device is not None else None
    if d is None or d.index is None:
        d = torch.device("cuda" if d is None else d.type, torch.cuda.current_device())
    ln = _lanes.get((d.index, n))
    if ln is None:
        ln = _lanes[(d.index, n)] = Lane(d, n)
    return ln


def current(device=None):
    return lane(_current, device)


@contextlib.contextmanager
def enter(n):
    """lane n is current and launches go to its stream; the previous lane is restored on every way out"""
    global _current
    prev, _current = _current, n
    try:
        st = current().stream
        with torch.cuda.stream(st) if st is not None else contextlib.nullcontext():
            yield
    finally:
        _current = prev


def base():
    return _base


def pending_lanes():
    """numbers of the lanes that hold unreduced weight-gradient partials"""
    return sorted({ln.index for ln in _lanes.values() if ln.pending})


def discard():
    """drop every lane's pending jobs and rewind the arenas (exceptional exit of a backward: nothing is reduced)"""
    for ln in _lanes.values():
        ln.clear()
    for hook in _discard_hooks:
        hook()


def on_discard(hook):
    """hook() runs with every discard: state of the caller's that an abandoned backward leaves invalid as well"""
    _discard_hooks.append(hook)


def defer(step=0):
    """the nesting depth of deferred_wgrad, after adding `step`"""
    global _defer
    _defer += step
    return _defer


class Fork:
    """Side lanes beside the current stream.  Fork(n) takes the n lanes behind those of every fork that is open around the launch stream
    (a fork is made from the launch stream only: hipStreamEndCapture does not survive one from a side stream); Fork(reserve=numbers)
    owns fixed lane numbers, which no Fork(n) may then reach.  `fork` lets side lanes start at the current point of the parent stream,
    `on(k)` enters side lane k, `join` makes the parent wait for all of them.  While `hold` is in force, forks made on the launch
    stream go behind this one.  As a context manager it leaves nothing behind: on an exception every pending partial is discarded, and
    in every case the hold is released and the side lanes are joined (a capture must not end with a dangling fork)."""

    def __init__(self, n=1, reserve=None):
        self.main = torch.cuda.current_stream()
        self.base, self.held = _base, False
        if reserve is not None:
            numbers = list(reserve)
            if min(numbers) <= _base:
                raise RuntimeError("the reserved lanes %s overlap the lanes 1..%d of the open forks" % (sorted(numbers), _base))
            _reserved.update(numbers)
        else:
            numbers = list(range(_base + 1, _base + n + 1))
            if _reserved.intersection(numbers):
                raise RuntimeError("lanes %d..%d overlap the reserved lanes %s" % (numbers[0], numbers[-1], sorted(_reserved)))
        self.lanes = [lane(k) for k in numbers]
        self.streams = [ln.stream for ln in self.lanes]      # (created here, in front of the first wait)

    def fork(self, *which):
        for k in which or range(len(self.streams)):
            self.streams[k].wait_stream(self.main)

    def on(self, k):
        return enter(self.lanes[k].index)

    def hold(self):
        global _base
        _base, self.held = self.base + len(self.lanes), True

    def release(self):
        global _base
        if self.held:
            _base, self.held = self.base, False

    def join(self, into=None):
        for st in self.streams:
            (into or self.main).wait_stream(st)

    def close(self, into=None):
        self.release()
        self.join(into)

    def __enter__(self):
        return self

    def __exit__(self, exc_type, exc, tb):
        if exc_type is not None:
            discard()
        self.close()
        return False
