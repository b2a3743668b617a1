"""CPU checks of the host-side pieces the fused train steps share (explicit-tf2-recommendation_amd/engine.py): the
plan-buffer assignment of a many() call and the batch reader."""
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
