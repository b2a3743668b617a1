"""CPU checks of tests.helpers.plan_batch, the builder of the batches of tests/test_gpu_plan_edges.py: it must return
exactly the run spectrum it was asked for and honour the id contract -- a green GPU run would otherwise be testing
the wrong thing.  The GPU cases are also put through their regime guards on the host restatement of the plan."""
import numpy as np
import pytest

from tests import helpers as H
from tests import test_gpu_plan_edges as E


def runs_in_key_order(col, lo):
    keys, counts = np.unique(np.asarray(col).reshape(-1) - lo, return_counts=True)
    return keys, counts


@pytest.mark.parametrize("layout", H.PLAN_LAYOUTS)
def test_plan_batch_returns_the_prescribed_spectrum(layout):
    B = 1000
    dims = [1200, 1000, 3, 1, 5000]
    offsets = H.field_offsets(dims)
    spectra = [H.fill_spectrum(B, [129, 300, 17, 3, 18], pairs=40), [B - 1, 1], [400, 300, 300], [B], "uniform"]
    batch = H.plan_batch(B, dims, offsets, spectra, layout, seed=5)
    assert set(batch) == {"f0", "f1", "f2", "f3", "f4", "label"}
    assert batch["label"].shape == (B, 1) and batch["label"].dtype == np.float32
    assert set(np.unique(batch["label"]).tolist()) <= {0.0, 1.0} and 0 < batch["label"].sum() < B
    for f in range(len(dims)):
        col = batch["f%d" % f]
        assert col.shape == (B, 1) and col.dtype == np.int64
        assert col.min() >= offsets[f] and col.max() < offsets[f] + dims[f]          # id contract
        keys, counts = runs_in_key_order(col, offsets[f])
        assert keys[0] == 0 and keys[-1] == dims[f] - 1                              # ends forced
        if spectra[f] == "uniform":
            continue
        assert sorted(counts.tolist()) == sorted(spectra[f])                         # exactly the spectrum
        if layout == "hot":
            assert np.all(np.diff(counts) <= 0)                                      # longest runs on the smallest keys
        if layout == "ranked":
            assert counts.tolist() == list(spectra[f])
        if layout == "clustered":
            c = col.reshape(-1)
            for k in keys:
                where = np.nonzero(c == k + offsets[f])[0]
                assert where[-1] - where[0] + 1 == where.size                        # members adjacent
    # same seed, same batch; the layout and the seed change the placement
    again = H.plan_batch(B, dims, offsets, spectra, layout, seed=5)
    assert all(np.array_equal(batch[k], again[k]) for k in batch)
    other = H.plan_batch(B, dims, offsets, spectra, layout, seed=6)
    assert not np.array_equal(batch["f0"], other["f0"])


def test_plan_batch_refuses_impossible_spectra():
    with pytest.raises(ValueError):
        H.plan_batch(10, [100], [0], [[3, 3]])                                      # does not sum to B
    with pytest.raises(ValueError):
        H.plan_batch(10, [4], [0], [[2, 2, 2, 2, 1, 1]])                            # more runs than keys
    with pytest.raises(ValueError):
        H.plan_batch(10, [100], [0], [[10]], layout="sorted")


def test_host_plan_definition():
    col = np.array([7, 3, 7, 9, 3, 3], np.int64) + 100
    p = H.host_plan(col, 100)
    assert p["col_nu"] == 3
    assert p["perm"].tolist() == [1, 4, 5, 0, 2, 3]
    assert p["col_uid"].tolist() == [103, 107, 109]
    assert p["col_seg"].tolist() == [0, 3, 5, 6, 6, 6, 6]
    neg = -(1 << 31)
    assert p["dloc"].tolist() == [1, 0, 1 | neg, 2, 0 | neg, 0 | neg]


def test_width_cases_cover_the_word_widths():
    bits = E._bits
    widths = {bits(D) + bits(B) for B, D in E.WIDTHS}
    assert widths >= {8, 14, 15, 21, 22, 28, 29, 32}
    assert {bits(D) % 7 for B, D in E.WIDTHS} >= {0, 1}                             # both sides of a multiple of 7
    w32 = [(B, D) for B, D in E.WIDTHS if bits(D) + bits(B) == 32]
    assert any(B > 8192 for B, _ in w32) and any(B <= 8192 for B, _ in w32)         # kpt 16 and 8
    for B, D in w32:
        assert ((D - 1) << bits(B)) | (B - 1) == 0xFFFFFFFE                         # the widest legal word


def host_plans(batch, names, offsets):
    B = batch[names[0]].shape[0]
    plans = [H.host_plan(batch[nm], offsets[f]) for f, nm in enumerate(names)]
    out = {"col_nu": np.array([p["col_nu"] for p in plans], np.int32),
           "col_seg": np.stack([p["col_seg"] for p in plans]),
           "col_uid": np.stack([np.pad(p["col_uid"], (0, B - p["col_nu"])) for p in plans])}
    assert out["col_seg"].shape == (len(names), B + 1)
    return out


@pytest.mark.parametrize("name,fn", E.CASES, ids=[c[0] for c in E.CASES])
def test_gpu_cases_reach_their_regimes(name, fn):
    """the guard every GPU case applies to the plan the GPU built, here on the plan's definition"""
    seed = E.case_seed(name, fn)
    B, dims, offsets, host, guard = E.build_case(fn, seed)
    names = ["f%d" % i for i in range(len(dims))]
    for f, nm in enumerate(names):
        assert host[nm].min() >= offsets[f] and host[nm].max() < offsets[f] + dims[f]
    guard(host_plans(host, names, offsets))


def test_adversarial_and_many_batches_reach_their_regimes():
    for B in (4096, 4000):
        dims, offsets, host = E.adversarial_batches(B, 4, 100 + B)
        names = ["f%d" % i for i in range(len(dims))]
        plan = host_plans(host[1], names, offsets)
        E.expect(plan, B, 0, skew=True, wg0_huge=17)
        E.expect(plan, B, 1, skew=True)
        E.expect(plan, B, 2, skew=False)
    B, dims, offsets, pool = E.many_pool(26, 40, 526)
    assert len({tuple(p["f1"].reshape(-1)[:64]) for p in pool}) == 40                  # 40 distinct batches
