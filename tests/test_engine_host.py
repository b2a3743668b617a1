"""CPU checks of the host-side pieces the train steps share (explicit-tf2-recommendation_amd/engine.py): the
plan-buffer assignment of a many() call, the batch reader and the graph policy of every cached step."""
import pytest
import torch


def test_assign_plan_buffers_ring():
    from explicit_tf2_recommendation_amd.engine import _assign_plan_buffers as assign
    # nothing announced: every batch planned inline in the current half; the announced ones go to the other half
    assert assign(["a", "b", "c"], 2, {}, 0, 32) == ([0, 1, 2], [0, 1, 2], [32, 33], 1)
    # every batch announced: each reads its own buffer, nothing inline; nothing announced now: the half stays
    assert assign(["x", "y"], 0, {"x": 32, "y": 33}, 1, 32) == ([32, 33], [], [], 1)
    # announced batches reuse their buffers, the others take the free slots of the same half in order, a batch that
    # appears twice is planned again (inline, in a fresh buffer) at its second occurrence; the next call's batches go to
    # the other half from its start
    pre = {"a": 32, "b": 34}
    assert assign(["c", "a", "a", "b", "d"], 3, pre, 1, 32) == ([33, 32, 35, 34, 36], [0, 2, 4], [0, 1, 2], 0)
    # the buffer of an announced batch that does not come is free for the others
    assert assign(["c"], 1, {"a": 0}, 0, 4) == ([0], [0], [4], 1)
    # the whole half: every one of nhalf buffers
    keys = list(range(4))
    assert assign(keys, 4, {k: 4 + k for k in keys[::2]}, 1, 4) == ([4, 5, 6, 7], [1, 3], [0, 1, 2, 3], 0)


def test_assign_plan_buffers_chained_calls():
    """Calls chained as many() chains them: a call reads the half the previous one filled and never writes it."""
    from explicit_tf2_recommendation_amd.engine import _assign_plan_buffers as assign
    pre, half = {}, 0
    calls = [(["a", "b"], ["c", "d"]), (["c", "d"], ["a"]), (["a", "e"], []), (["b"], ["b", "c"]), (["b", "c"], [])]
    for keys, then in calls:
        bufs, inline, then_bufs, nxt = assign(keys, len(then), pre, half, 8)
        assert all(half * 8 <= b < half * 8 + 8 for b in bufs) and len(set(bufs)) == len(bufs)
        assert [i for i, k in enumerate(keys) if k not in pre] == inline
        assert set(then_bufs).isdisjoint(bufs) and all((1 - half) * 8 <= b < (1 - half) * 8 + 8 for b in then_bufs)
        assert nxt == (1 - half if then else half)
        pre, half = dict(zip(then, then_bufs)), nxt
    assert half == 1


def test_batch_reader():
    from explicit_tf2_recommendation_amd.engine import _BatchReader
    B = 8
    rd = _BatchReader(["u", "i"], B, cuda=False)
    batch = {"u": torch.arange(B), "i": torch.arange(B) + 100, "label": torch.ones(B, 1)}
    cols, key = rd.cols_key(batch)
    assert cols[0] is batch["u"] and cols[1] is batch["i"] and key == rd.key(cols)
    assert rd.cols_key(batch)[0] is cols                         # cached per dict
    batch["i"] = torch.arange(B) + 200                           # a replaced tensor is read again
    cols2, key2 = rd.cols_key(batch)
    assert cols2[1] is batch["i"] and key2 != key
    assert rd.label(batch, "label") is batch["label"]
    single = _BatchReader(["u"], B, cuda=False)
    cols1 = single.cols_key(batch)[0]
    assert len(cols1) == 1 and cols1[0] is batch["u"]
    for wrong in (torch.arange(B, dtype=torch.int32), torch.arange(B - 1), torch.arange(2 * B)[::2]):
        with pytest.raises(ValueError, match="feature 'i'"):
            rd.cols_key(dict(batch, i=wrong))
    y2 = torch.ones(B, 2)
    for wrong in (torch.ones(B, dtype=torch.float64), torch.ones(B // 2), y2[:, 0]):
        with pytest.raises(ValueError, match="label"):
            rd.label(dict(batch, label=wrong), "label")
    with pytest.raises(ValueError, match="CUDA"):
        _BatchReader(["u", "i"], B).cols_key(batch)
    with pytest.raises(ValueError, match="CUDA"):
        _BatchReader(["u", "i"], B).label(batch, "label")


class _Recorder:
    """Fakes of torch.cuda.CUDAGraph / graph / synchronize that log what the graph policy does.  Work enqueued inside a
    capture is recorded into the graph, not run; a replay runs what the graph recorded."""

    def __init__(self, monkeypatch):
        import contextlib
        from explicit_tf2_recommendation_amd import engine
        self.events, self.done, self.capturing = [], [], None
        rec = self

        class FakeGraph:
            def __init__(self):
                self.nodes = []

            def replay(self):
                rec.events.append("replay")
                rec.done.extend(self.nodes)

        @contextlib.contextmanager
        def graph(g, capture_error_mode=None):
            assert capture_error_mode == engine.CAPTURE_MODE
            rec.events.append("capture")
            rec.capturing = g
            try:
                yield
            finally:
                rec.capturing = None

        monkeypatch.setattr(torch.cuda, "CUDAGraph", FakeGraph)
        monkeypatch.setattr(torch.cuda, "graph", graph)
        monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **k: rec.events.append("sync"))

    def enqueue(self, work):
        if self.capturing is not None:
            self.capturing.nodes.append(work)
        else:
            self.events.append("eager")
            self.done.append(work)

    def take(self):
        ev, self.events = self.events, []
        return ev


def _stub(rec, graphable=True, use_graph=True):
    from explicit_tf2_recommendation_amd.engine import _GraphPolicy

    class Stub(_GraphPolicy):
        def _graphable(self):
            return graphable

        def __call__(self, key, *keep):
            self._run(key, lambda: rec.enqueue(key), *keep)

    s = Stub()
    s.use_graph = use_graph
    return s


def test_graph_policy_is_shared():
    from explicit_tf2_recommendation_amd import engine
    for cls in (engine.DeepFMTrainStep, engine.DeepFMFusedStep, engine.DSSMFusedStep, engine.ShardedDeepFMStep):
        assert issubclass(cls, engine._GraphPolicy) and cls._run is engine._GraphPolicy._run, cls
    assert not hasattr(engine.ShardedDeepFMStep, "release_graphs")


def test_graph_policy_sightings(monkeypatch):
    """First sighting: eager, nothing kept.  Second: eager, then captured without running.  Then: replay only.  Every
    call does its work exactly once."""
    rec = _Recorder(monkeypatch)
    s = _stub(rec)
    held = object()
    s("a", held)
    assert rec.take() == ["eager"] and len(s._graphs) == 0 and list(s._seen) == ["a"]
    s("a", held)
    assert rec.take() == ["eager", "sync", "capture"] and list(s._graphs) == ["a"] and len(s._seen) == 0
    g, kept = s._graphs["a"]
    assert g.nodes == ["a"] and kept is held                 # enqueued inside the capture; the inputs are held
    for _ in range(3):
        s("a", held)
        assert rec.take() == ["replay"]
    assert rec.done == ["a"] * 5                             # five calls, the work ran five times


def test_graph_policy_lru_and_bounded_seen(monkeypatch):
    rec = _Recorder(monkeypatch)
    s = _stub(rec)
    s.MAX_GRAPHS = 2
    for k in ("a", "a", "b", "b", "a", "c", "c"):            # "a" is used after "b": "b" is the least recently used
        s(k)
    assert list(s._graphs) == ["a", "c"]
    rec.take()
    s("b")                                                   # dropped with its graph: seen afresh, eager
    assert rec.take() == ["eager"] and "b" in s._seen
    keys = ["k%d" % i for i in range(40)]
    for k in keys:
        s(k)
    assert len(s._seen) == 8 * s.MAX_GRAPHS and list(s._seen) == keys[-8 * s.MAX_GRAPHS:]
    rec.take()
    s(keys[0])                                               # forgotten: a first sighting again, no capture
    assert rec.take() == ["eager"] and len(s._graphs) == 2
    assert len(rec.done) == 7 + 1 + 40 + 1


@pytest.mark.parametrize("graphable,use_graph", [(False, True), (True, False)])
def test_graph_policy_eager_when_not_graphable(monkeypatch, graphable, use_graph):
    rec = _Recorder(monkeypatch)
    s = _stub(rec, graphable=graphable, use_graph=use_graph)
    for _ in range(4):
        s("a", object())
    assert rec.take() == ["eager"] * 4 and len(s._graphs) == 0 and len(s._seen) == 0


def test_graph_policy_release(monkeypatch):
    rec = _Recorder(monkeypatch)
    s = _stub(rec)
    for k in ("a", "a", "b"):
        s(k)
    assert len(s._graphs) == 1 and len(s._seen) == 1
    s.release()
    assert len(s._graphs) == 0 and len(s._seen) == 0
    rec.take()
    s("a")                                                   # after release a key starts over
    assert rec.take() == ["eager"]


def test_captures_run_without_the_cyclic_collector(monkeypatch):
    """A dead reference cycle may hold a CUDAGraph, and destroying one waits for the device -- not allowed while a
    stream captures.  So every capture of this module first collects what is dead and keeps the cyclic collector off
    until the capture has ended, whatever thread the captured work runs in; afterwards the collector is as it was."""
    import gc
    import weakref
    from explicit_tf2_recommendation_amd import engine

    class Node:
        pass

    def dead_cycle():
        a, b = Node(), Node()
        a.other, b.other = b, a
        return weakref.ref(a)

    rec = _Recorder(monkeypatch)
    seen = []

    class Stub(engine._GraphPolicy):
        def __call__(self, key):
            self._run(key, lambda: seen.append((rec.capturing is not None, gc.isenabled(), ref() is None)))

    assert gc.isenabled()
    s = Stub()
    ref = dead_cycle()
    s("b")
    s("b")
    # first sighting and the second one's own run: eager, collector untouched; inside the capture: collector off, and
    # the cycle was collected before the capture began
    assert [x[:2] for x in seen] == [(False, True), (False, True), (True, False)] and seen[-1][2] and gc.isenabled()
    # a caller that keeps the collector off itself (a benchmark around its timed region) is left alone: no collection
    del seen[:]
    gc.disable()
    try:
        ref = dead_cycle()
        s("a")
        s("a")
        assert gc.isenabled() is False
    finally:
        gc.enable()
    assert seen == [(False, False, False)] * 2 + [(True, False, False)]
    with pytest.raises(RuntimeError):
        with engine._no_cyclic_gc():
            assert not gc.isenabled()
            raise RuntimeError("a failed capture")
    assert gc.isenabled()
