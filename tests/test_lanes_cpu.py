"""Host logic of the lane schedule (vts/lanes.py and the primitives of vts/engine.py built on it), traced without a GPU: streams are
recording stubs, the weight-gradient reduce launch is a recorder.  A trace is a list of
    ("wait", waiting stream, awaited stream)   ("body:<tag>", lane number, stream)   ("flush", lane number, stream).
The expected traces were recorded from the schedule as it was before per-lane state moved into lanes.Lane (module globals of ops.py,
a hand-made fork / join in each primitive): the launches, their streams and the waits between streams are the same."""
import contextlib
import itertools
import os
import sys
import types

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "visual-tactile-synthesis_amd"))


class Boom(Exception):
    pass


class Rig:
    """the stubs and the trace they write"""

    def __init__(self, monkeypatch, parallel):
        from vts import engine, lanes, ops
        from vts import lib as L

        self.engine, self.lanes, self.ops = engine, lanes, ops
        self.trace, self.keep, self.owner = [], [], {}
        rig, names = self, itertools.count()

        class Stream:
            def __init__(self, name=None):
                self.name = name or "side%d" % next(names)

            def wait_stream(self, other):
                rig.trace.append(("wait", self.name, other.name))

        self.stack = [Stream("main")]

        @contextlib.contextmanager
        def on_stream(st):
            self.stack.append(st)
            try:
                yield
            finally:
                self.stack.pop()

        def reduce_launch(label, nbytes, flops, fn, jobs, n, stream):
            assert label == "wgrad_reduce_batch" and n == len(jobs)
            for ln in dict.fromkeys(self.owner[j.dw] for j in jobs):      # the lanes whose jobs this launch reduces
                self.trace.append(("flush", ln, stream))

        monkeypatch.setattr(torch.cuda, "Stream", Stream)
        monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: self.stack[-1])
        monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
        monkeypatch.setattr(torch.cuda, "stream", on_stream)
        monkeypatch.setattr(L, "load", lambda: types.SimpleNamespace(vts_wgrad_reduce_batch=None))
        monkeypatch.setattr(L, "stream", lambda: self.stack[-1].name)
        monkeypatch.setattr(ops, "_run", reduce_launch)
        monkeypatch.setattr(engine, "PARALLEL_SCALES", parallel)
        for name, fresh in (("_lanes", {}), ("_streams", {}), ("_reserved", set()), ("_current", 0), ("_base", 0), ("_defer", 0)):
            monkeypatch.setattr(lanes, name, fresh)

    def mark(self, tag):
        self.trace.append(("body:" + tag, self.lanes.current().index, self.stack[-1].name))

    def work(self, tag):
        """a lane body: one launch that leaves a deferred weight-gradient job on the current lane"""
        self.mark(tag)
        ln = self.lanes.current()
        dw, part = torch.zeros(16), torch.zeros(16)
        self.keep += [dw, part]
        self.owner[dw.data_ptr()] = ln.index
        ln.enqueue(dw, 16, False, (part, 1))

    def waits(self):
        return [e for e in self.trace if e[0] == "wait"]

    def settled(self):
        """what every primitive leaves behind, also when a body raised"""
        return self.lanes.current().index == 0 and self.lanes.base() == 0 and not self.lanes.pending_lanes() and len(self.stack) == 1


@pytest.fixture()
def rig(monkeypatch):
    return Rig(monkeypatch, True)


@pytest.fixture()
def serial_rig(monkeypatch):
    return Rig(monkeypatch, False)


# ---- the scenarios ------------------------------------------------------------------------------------------------------------------
def nested_lanes(r, fail=None):
    """_run_lanes(3) whose launch-stream lane calls _run_lanes(2), while a fork_lane is open; then join_lane"""
    e, ops = r.engine, r.ops

    def forked():
        with ops.deferred_wgrad():
            r.work("forked")

    def body(tag):
        r.work(tag)
        if tag == fail:
            raise Boom(tag)

    def outer(k):
        body("outer%d" % k)
        if k == 0:
            e._run_lanes(2, lambda j: body("inner%d" % j))

    h = e.fork_lane(forked)
    try:
        with ops.deferred_wgrad():
            e._run_lanes(3, outer)
    finally:
        e.join_lane(h)


def side_queue(r, fail=None):
    """three SideQueue.run and the join, inside a backward's deferred_wgrad"""
    def item(tag):
        r.work(tag)
        if tag == fail:
            raise Boom(tag)

    with r.ops.deferred_wgrad():
        sq = r.engine.SideQueue()
        r.work("chain0")
        for k in range(3):
            sq.run(lambda k=k: item("dw%d" % k))
        sq.join()


def _chain(r, fail=None):
    e = r.engine

    def scale_lane(D, s, passes, criterion, knocked_out=False):
        tag = "%s%d" % (passes, s)
        (r.work if passes == "update" else r.mark)(tag)      # the passes of the generator step write no weight gradient
        if tag == fail:
            raise Boom(tag)

    return dict(scale_lane=scale_lane, prepare=lambda jobs: r.mark("prepare:" + jobs[0][1]), finish=lambda jobs: r.mark("finish:" + jobs[0][1]),
                cost=lambda passes, s: (3.0, 2.0, 1.0)[s],
                chain=dict(D=types.SimpleNamespace(num_D=3), index0=0, update="update", mid=lambda: r.mark("mid"), gstep=lambda: "gstep"))


def _stub_chain(r, monkeypatch, fail=None):
    c = _chain(r, fail)
    for name, stub in (("_scale_lane", c["scale_lane"]), ("_prepare_passes", c["prepare"]), ("_finish_passes", c["finish"]), ("_lane_cost", c["cost"])):
        monkeypatch.setattr(r.engine, name, stub)
    return c["chain"]


def chain_two_streams(r, monkeypatch, fail=None):
    """msd_chain on the launch stream and one side stream, with a `side` callable"""
    r.engine.msd_chain(_stub_chain(r, monkeypatch, fail), None, side=lambda: r.work("side"), side_cost=0.5)


def chain_serial_in_lane(r, monkeypatch, fail=None):
    """msd_chain(serial=True) inside a lane of its own, as the D2 tail of the training step runs it"""
    chain = _stub_chain(r, monkeypatch, fail)
    h = r.engine.fork_lane(lambda: r.engine.msd_chain(chain, None, side=lambda: r.work("side"), serial=True))
    r.engine.join_lane(h)


# recorded from the schedule before the refactoring; stream names count the side streams in the order they were created
EXPECTED = {"chain_serial_in_lane": [("wait", "side0", "main"),
                          ("body:prepare:update", 1, "side0"),
                          ("body:update0", 1, "side0"),
                          ("body:update1", 1, "side0"),
                          ("body:update2", 1, "side0"),
                          ("body:side", 1, "side0"),
                          ("flush", 1, "side0"),
                          ("body:finish:update", 1, "side0"),
                          ("body:mid", 1, "side0"),
                          ("body:prepare:gstep", 1, "side0"),
                          ("body:gstep0", 1, "side0"),
                          ("body:gstep1", 1, "side0"),
                          ("body:gstep2", 1, "side0"),
                          ("body:finish:gstep", 1, "side0"),
                          ("wait", "main", "side0")],
 "chain_two_streams": [("body:prepare:update", 0, "main"),
                       ("wait", "side0", "main"),
                       ("body:update1", 1, "side0"),
                       ("body:update2", 1, "side0"),
                       ("flush", 1, "side0"),
                       ("body:update0", 0, "main"),
                       ("body:side", 0, "main"),
                       ("flush", 0, "main"),
                       ("wait", "main", "side0"),
                       ("body:finish:update", 0, "main"),
                       ("body:mid", 0, "main"),
                       ("body:prepare:gstep", 0, "main"),
                       ("wait", "side0", "main"),
                       ("body:gstep1", 1, "side0"),
                       ("body:gstep2", 1, "side0"),
                       ("body:gstep0", 0, "main"),
                       ("wait", "main", "side0"),
                       ("body:finish:gstep", 0, "main"),
                       ("wait", "main", "side0")],
 "nested_lanes": [("wait", "side0", "main"),
                  ("body:forked", 1, "side0"),
                  ("flush", 1, "side0"),
                  ("wait", "side1", "main"),
                  ("wait", "side2", "main"),
                  ("body:outer1", 2, "side1"),
                  ("flush", 2, "side1"),
                  ("body:outer2", 3, "side2"),
                  ("flush", 3, "side2"),
                  ("body:outer0", 0, "main"),
                  ("wait", "side3", "main"),
                  ("body:inner1", 4, "side3"),
                  ("flush", 4, "side3"),
                  ("body:inner0", 0, "main"),
                  ("flush", 0, "main"),
                  ("wait", "main", "side3"),
                  ("wait", "main", "side1"),
                  ("wait", "main", "side2"),
                  ("wait", "main", "side0")],
 "raise_chain_gstep1": [("body:prepare:update", 0, "main"),
                        ("wait", "side0", "main"),
                        ("body:update1", 1, "side0"),
                        ("body:update2", 1, "side0"),
                        ("flush", 1, "side0"),
                        ("body:update0", 0, "main"),
                        ("body:side", 0, "main"),
                        ("flush", 0, "main"),
                        ("wait", "main", "side0"),
                        ("body:finish:update", 0, "main"),
                        ("body:mid", 0, "main"),
                        ("body:prepare:gstep", 0, "main"),
                        ("wait", "side0", "main"),
                        ("body:gstep1", 1, "side0"),
                        ("wait", "main", "side0")],
 "raise_chain_update1": [("body:prepare:update", 0, "main"),
                         ("wait", "side0", "main"),
                         ("body:update1", 1, "side0"),
                         ("wait", "main", "side0")],
 "raise_fork_lane": [("wait", "side0", "main"), ("body:forked", 1, "side0"), ("wait", "main", "side0")],
 "raise_run_lanes_inner1": [("wait", "side0", "main"),
                            ("body:forked", 1, "side0"),
                            ("flush", 1, "side0"),
                            ("wait", "side1", "main"),
                            ("wait", "side2", "main"),
                            ("body:outer1", 2, "side1"),
                            ("flush", 2, "side1"),
                            ("body:outer2", 3, "side2"),
                            ("flush", 3, "side2"),
                            ("body:outer0", 0, "main"),
                            ("wait", "side3", "main"),
                            ("body:inner1", 4, "side3"),
                            ("wait", "main", "side3"),
                            ("wait", "main", "side1"),
                            ("wait", "main", "side2"),
                            ("wait", "main", "side0")],
 "raise_run_lanes_outer0": [("wait", "side0", "main"),
                            ("body:forked", 1, "side0"),
                            ("flush", 1, "side0"),
                            ("wait", "side1", "main"),
                            ("wait", "side2", "main"),
                            ("body:outer1", 2, "side1"),
                            ("flush", 2, "side1"),
                            ("body:outer2", 3, "side2"),
                            ("flush", 3, "side2"),
                            ("body:outer0", 0, "main"),
                            ("wait", "main", "side1"),
                            ("wait", "main", "side2"),
                            ("wait", "main", "side0")],
 "raise_run_lanes_outer1": [("wait", "side0", "main"),
                            ("body:forked", 1, "side0"),
                            ("flush", 1, "side0"),
                            ("wait", "side1", "main"),
                            ("wait", "side2", "main"),
                            ("body:outer1", 2, "side1"),
                            ("wait", "main", "side1"),
                            ("wait", "main", "side2"),
                            ("wait", "main", "side0")],
 "raise_side_queue": [("body:chain0", 0, "main"),
                      ("wait", "side6", "main"),
                      ("body:dw0", 7, "side6"),
                      ("wait", "side5", "main"),
                      ("body:dw1", 6, "side5"),
                      ("wait", "main", "side6"),
                      ("wait", "main", "side5")],
 "serial": [("body:forked", 0, "main"),
            ("flush", 0, "main"),
            ("body:outer0", 0, "main"),
            ("body:inner0", 0, "main"),
            ("body:inner1", 0, "main"),
            ("body:outer1", 0, "main"),
            ("body:outer2", 0, "main"),
            ("flush", 0, "main"),
            ("body:chain0", 0, "main"),
            ("body:dw0", 0, "main"),
            ("body:dw1", 0, "main"),
            ("body:dw2", 0, "main"),
            ("flush", 0, "main"),
            ("body:prepare:update", 0, "main"),
            ("body:update0", 0, "main"),
            ("body:update1", 0, "main"),
            ("body:update2", 0, "main"),
            ("body:side", 0, "main"),
            ("flush", 0, "main"),
            ("body:finish:update", 0, "main"),
            ("body:mid", 0, "main"),
            ("body:prepare:gstep", 0, "main"),
            ("body:gstep0", 0, "main"),
            ("body:gstep1", 0, "main"),
            ("body:gstep2", 0, "main"),
            ("body:finish:gstep", 0, "main")],
 "side_queue": [("body:chain0", 0, "main"),
                ("wait", "side6", "main"),
                ("body:dw0", 7, "side6"),
                ("wait", "side5", "main"),
                ("body:dw1", 6, "side5"),
                ("wait", "side6", "main"),
                ("body:dw2", 7, "side6"),
                ("flush", 7, "side6"),
                ("flush", 6, "side5"),
                ("wait", "main", "side6"),
                ("wait", "main", "side5"),
                ("flush", 0, "main")]}


def _check(r, name):
    assert r.trace == EXPECTED[name]
    assert r.settled()


def test_nested_run_lanes_beside_an_open_fork(rig):
    nested_lanes(rig)
    _check(rig, "nested_lanes")


def test_side_queue_alternates_its_two_lanes(rig):
    side_queue(rig)
    _check(rig, "side_queue")


def test_serial_schedule_runs_everything_inline(serial_rig, monkeypatch):
    nested_lanes(serial_rig)
    side_queue(serial_rig)
    chain_two_streams(serial_rig, monkeypatch)
    _check(serial_rig, "serial")
    assert not serial_rig.waits() and {e[1:] for e in serial_rig.trace} == {(0, "main")}


def test_chain_on_two_streams(rig, monkeypatch):
    chain_two_streams(rig, monkeypatch)
    _check(rig, "chain_two_streams")


def test_serial_chain_inside_a_forked_lane(rig, monkeypatch):
    chain_serial_in_lane(rig, monkeypatch)
    _check(rig, "chain_serial_in_lane")


# ---- a body that raises: every forked stream is joined, the lane and the base are what they were, no job survives ----------------------
def _joined(r, pairs):
    """every (parent, side) stream pair has a wait of parent for side behind the last launch on side"""
    last = {}
    for i, e in enumerate(r.trace):
        if e[0] != "wait":
            last[e[2]] = i
    return all(any(e == ("wait", parent, side) for e in r.trace[last.get(side, 0):]) for parent, side in pairs)


@pytest.mark.parametrize("fail", ["outer1", "outer0", "inner1"])
def test_run_lanes_body_raises(rig, fail):
    with pytest.raises(Boom):
        nested_lanes(rig, fail)
    _check(rig, "raise_run_lanes_" + fail)
    assert _joined(rig, [("main", s) for s in ("side0", "side1", "side2")] + ([("main", "side3")] if fail == "inner1" else []))


def test_fork_lane_body_raises(rig):
    def forked():
        with rig.ops.deferred_wgrad():
            rig.work("forked")
            raise Boom()

    with pytest.raises(Boom):
        rig.engine.fork_lane(forked)
    _check(rig, "raise_fork_lane")
    assert _joined(rig, [("main", "side0")])


def test_side_queue_item_raises(rig):
    with pytest.raises(Boom):
        side_queue(rig, "dw1")
    _check(rig, "raise_side_queue")
    assert _joined(rig, [("main", "side6"), ("main", "side5")])


@pytest.mark.parametrize("fail", ["update1", "gstep1"])
def test_chain_body_raises(rig, monkeypatch, fail):
    with pytest.raises(Boom):
        chain_two_streams(rig, monkeypatch, fail)
    _check(rig, "raise_chain_" + fail)
    assert _joined(rig, [("main", "side0")])


# ---- the scope of the outermost deferred_wgrad exit, and the lane allocator -----------------------------------------------------------
def test_outermost_deferred_exit_refuses_foreign_pending_jobs(rig):
    """the context ends on lane 0 while lane 2 still holds jobs: reducing them here would run on a stream that has no dependency on
    lane 2's launches.  Nothing is launched, nothing stays pending."""
    with pytest.raises(RuntimeError, match="lane 2"):
        with rig.ops.deferred_wgrad():
            rig.work("mine")
            with rig.lanes.enter(2):
                rig.work("foreign")
    assert not [e for e in rig.trace if e[0] == "flush"]
    assert rig.settled()


def test_outermost_deferred_exit_flushes_its_own_lane_only(rig):
    with rig.lanes.enter(2):
        with rig.ops.deferred_wgrad():
            with rig.ops.deferred_wgrad():
                rig.work("a")
            assert rig.lanes.pending_lanes() == [2]      # the inner exit reduces nothing
            rig.work("b")
    assert [e for e in rig.trace if e[0] == "flush"] == [("flush", 2, "side1")]
    assert rig.settled()


def test_lane_allocation_stops_at_the_side_queue_lanes(rig):
    sq = rig.engine.SideQueue()
    assert [ln.index for ln in sq.fork.lanes] == [7, 6] and [st.name for st in sq.fork.streams] == ["side6", "side5"]
    rig.engine._run_lanes(6, lambda k: rig.mark("ok%d" % k))          # lanes 1 .. 5
    with pytest.raises(RuntimeError, match="reserved"):
        rig.engine._run_lanes(7, lambda k: rig.mark("never%d" % k))   # would take lane 6
    h = rig.engine.fork_lane(lambda: None)
    with pytest.raises(RuntimeError, match="reserved"):
        rig.engine._run_lanes(6, lambda k: rig.mark("never%d" % k))   # behind the open fork: lanes 2 .. 6
    rig.engine.join_lane(h)
    assert not [e for e in rig.trace if e[0].startswith("body:never")]
    assert rig.settled()


def test_side_queue_lanes_cannot_be_reserved_under_an_open_fork_that_holds_them(rig):
    with pytest.raises(RuntimeError, match="open forks"):
        rig.engine._run_lanes(7, lambda k: rig.engine.SideQueue() if k == 0 else None)      # lanes 1 .. 6 are held while lane 0 runs
    assert _joined(rig, [("main", "side%d" % k) for k in range(6)]) and rig.settled()


def test_enter_restores_the_lane_when_the_body_raises(rig):
    with pytest.raises(Boom):
        with rig.lanes.enter(3):
            assert rig.lanes.current().index == 3 and rig.stack[-1].name == "side2"
            raise Boom()
    assert rig.settled()
