"""CPU checks behind tests/test_gpu_adam_classes.py: tests/adam_classes_ref.py restates the constants, the dispatch and the
update formulas that are in the text of csrc/dense_ops.hip and csrc/common.h today, every case is in the class it claims
and their union reaches every class and regime, the fp32 IEEE restatement of every case stays inside the share ROOM of
each bound (0.6; the whole bound for m, which adam_classes_ref.ROOM explains), and each mutant of that restatement breaks
a bound on the case named beside it.  A failure on the GPU can then not be blamed on the case table, and a pass cannot be
blamed on slack bounds."""
import os
import re

import numpy as np
import pytest

from tests import adam_classes_ref as AR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "csrc")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


@pytest.fixture(scope="module")
def dense_ops():
    return _read("dense_ops.hip")


@pytest.fixture(scope="module")
def common():
    return _read("common.h")


# ---- the restatements are the source's ------------------------------------------------------------------------------
def test_constants_are_the_ones_in_the_source(dense_ops):
    caps = re.findall(r"if \(blocks > (\d+) \* (\d+)\) blocks = (\d+) \* (\d+);", dense_ops)
    assert len(caps) == 3 and len(set(caps)) == 1, "dense_ops.hip: the grid cap of the three Adam sweeps reads %s" % caps
    a, b, c, d = (int(x) for x in caps[0])
    strides = re.findall(r"stride = \(int64_t\)gridDim\.x \* (\d+);", dense_ops)
    assert len(strides) == 3 and len(set(strides)) == 1, strides
    multi = re.findall(r"constexpr int ADAM_MULTI_MAX = (\d+);", dense_ops)
    assert len(multi) == 1
    src = AR.Consts(GRID_CAP=a * b, WG=int(strides[0]), VEC=4, ALIGN=16, ADAM_MULTI_MAX=int(multi[0]))
    assert (a * b, a * b) == (c * d, AR.K.GRID_CAP)
    for field in AR.Consts._fields:
        assert getattr(src, field) == getattr(AR.K, field), "the source has %s = %s, adam_classes_ref.K.%s = %s" % (
            field, getattr(src, field), field, getattr(AR.K, field))
    assert AR.PASS_ITEMS == 2097152 and AR.ADAM_MULTI_MAX == 16
    assert "return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }" in _read("common.h")          # ALIGN


def test_dispatch_text_is_what_the_restatements_read(dense_ops):
    for line in (
            "bool vec = E % 4 == 0 && ld % 4 == 0 && rec_is_aligned16(var) && rec_is_aligned16(m) && rec_is_aligned16(v);",
            "int64_t n4 = n / 4;\n    int64_t blocks = ceil_div64(n4, 256);",
            "int64_t blocks = ceil_div64(n, 256);\n    if (blocks > 256 * 32) blocks = 256 * 32;\n"
            "    hipLaunchKernelGGL(adam_sweep_scalar_kernel,",
            "V <= 0 || E <= 0 || (E & 3) != 0 || ld < E + 1 || (ld & 3) != 0 || cap < 0 || t < 1)\n    return REC_E_ARG;",
            "if (((reinterpret_cast<uintptr_t>(fused) | reinterpret_cast<uintptr_t>(m_e) | "
            "reinterpret_cast<uintptr_t>(v_e)) & 15) != 0)\n    return REC_E_ARG;",
            "int64_t blocks = ceil_div64(V * (E / 4 + 1), 256);",
            "const int lanes = lpr + 1;\n  const int64_t n = V * lanes;",
            "float mm = m_w[r], vv = v_w[r], xx = *xp;",
            "if (n_tensors > ADAM_MULTI_MAX) return REC_E_UNSUPPORTED;",
            "if (!var[i] || !m[i] || !v[i] || !g[i] || numel[i] < 0) return REC_E_ARG;",
            "if (!var || !m || !v || !g || n < 0 || t < 1) return REC_E_ARG;\n  if (n == 0) return REC_OK;",
            "if (u >= *n_uniq) return;\n  int64_t id = ids[u];\n  if ((uint64_t)id >= (uint64_t)V) return;",
            "float b1p = powf(b1, (float)t), b2p = powf(b2, (float)t);\n  return lr * sqrtf(1.f - b2p) / (1.f - b1p);"):
        assert line in dense_ops, "dense_ops.hip no longer holds: " + line
    assert dense_ops.count("if (u >= *n_uniq) return;\n  int64_t id = ids[u];\n"
                           "  if ((uint64_t)id >= (uint64_t)V) return;") == 3         # side, patch and lazy


def test_update_formulas_are_what_the_reference_restates(common):
    for line in (
            "const float num = lr_t * m;",
            "const float den = __builtin_amdgcn_sqrtf(v) + eps;\n  return __builtin_fmaf(-num, __builtin_amdgcn_rcpf(den), x);",
            "const float den = sqrtf(v) + eps;\n  return x - num / den;",
            "m = __builtin_fmaf(g, 1.f - b1, m * b1);\n  v = __builtin_fmaf(g * g, 1.f - b2, v * b2);\n"
            "  x = adam_step_x(x, m, v, lr_t, eps);",
            "m = __builtin_fmaf(g - m, 1.f - b1, m);\n  v = __builtin_fmaf(__builtin_fmaf(g, g, -v), 1.f - b2, v);\n"
            "  x = adam_step_x(x, m, v, lr_t, eps);",
            "m = m * b1;\n  v = v * b2;\n  x = adam_step_x(x, m, v, lr_t, eps);"):
        assert line in common, "common.h no longer holds: " + line


def test_class_functions():
    for E in range(1, 70):
        for ld in (E, E + 1, E + 4, 2 * E):
            for al in ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)):
                want = "vec" if E % 4 == 0 and ld % 4 == 0 and all(al) else "scalar"
                assert AR.sweep_class(E, ld, *al) == want
            assert AR.pair_args_ok(E, ld) == (E % 4 == 0 and ld % 4 == 0 and ld > E)
    assert not AR.pair_args_ok(16, 32, False) and not AR.pair_args_ok(16, 32, True, False)
    assert not AR.pair_args_ok(16, 32, True, True, False)
    assert [AR.passes(n) for n in (1, 2097152, 2097153, 4194304, 4194305)] == [1, 1, 2, 2, 3]
    with pytest.raises(ValueError):
        AR.sweep_class(4, 3)


# ---- the tables -----------------------------------------------------------------------------------------------------
def test_cases_are_in_the_class_they_claim_and_reach_every_class():
    reached = set()
    for c in AR.SPARSE_CASES:
        cls = AR.sweep_class(c.E, c.ld, *[o % 4 == 0 for o in c.off])
        npass = AR.passes(c.V * AR.items_per_row(cls, c.E))
        assert (cls, npass) == (c.cls, c.npass), c.name
        reached.add((cls, min(npass, 2)))
    assert reached == {(k, p) for k in ("vec", "scalar") for p in (1, 2)}
    shapes = {(c.V, c.E, c.ld, c.off) for c in AR.SPARSE_CASES}
    z = (0, 0, 0)
    assert shapes == {(257, 4, 4, z), (1000, 16, 16, z), (1000, 16, 32, z), (300, 64, 64, z), (140001, 64, 64, z),
                      (1000, 3, 3, z), (1000, 1, 32, z), (1000, 4, 5, z), (1000, 20, 21, z), (1000, 16, 16, (1, 0, 0)),
                      (1000, 16, 16, (0, 1, 0)), (1000, 16, 16, (0, 0, 1)), (700001, 3, 3, z)}
    assert 140001 * 16 == 2240016
    for c in AR.PAIR_CASES:
        assert AR.pair_args_ok(c.E, c.ld) and AR.passes(c.V * AR.items_per_row("pair", c.E)) == c.npass, c.name
    assert {(c.V, c.E, c.ld, c.npass) for c in AR.PAIR_CASES} == {(1000, 4, 8, 1), (1000, 16, 32, 1), (300, 64, 128, 1),
                                                                   (1048700, 4, 8, 2)}
    assert {(c.E, c.ld) for c in AR.LAZY_CASES} == {(1, 1), (1, 32), (3, 3), (3, 32), (16, 16), (16, 32)}
    assert [c.n for c in AR.DENSE_CASES] == [1, 255, 256, 257, 70001]
    assert [len(c.sizes) for c in AR.MULTI_CASES] == [1, 7, AR.ADAM_MULTI_MAX]
    for c in AR.MULTI_CASES[1:]:                       # a tensor ends inside a workgroup and one on its edge
        ends = np.cumsum(c.sizes)
        assert np.any(ends % 256 != 0) and np.any(ends % 256 == 0) and max(c.sizes) > 256 and min(c.sizes) == 1
    every = AR.SPARSE_CASES + AR.LAZY_CASES + AR.PAIR_CASES + AR.DENSE_CASES + AR.MULTI_CASES
    assert {c.t for c in every} == set(AR.STEPS) == {1, 2, 10, 1000, 100000}
    for table in (AR.SPARSE_CASES, AR.LAZY_CASES, AR.PAIR_CASES):
        assert {c.order for c in table} == {"asc", "first"}
        assert len({c.t for c in table}) >= 4 and 100000 in {c.t for c in table}
    assert {(c.cls, c.order) for c in AR.SPARSE_CASES} == {(k, o) for k in ("vec", "scalar") for o in ("asc", "first")}
    assert len({c.seed for c in every}) == len(every)
    assert max(c.V * c.ld for c in AR.SPARSE_CASES + AR.PAIR_CASES) <= 9_000_000


@pytest.mark.parametrize("name", [c.name for c in AR.SPARSE_CASES + AR.LAZY_CASES + AR.PAIR_CASES])
def test_inputs_hold_the_regimes_and_special_rows(name):
    c, S = AR.BY_NAME[name], AR.SPECIAL
    st = AR.case_state(name)
    x, m, v = st[:3]
    assert all(a.dtype == np.float32 for a in st) and x.shape == (c.V, c.E)
    assert not m[S["zero_u"]].any() and not v[S["zero_t"]].any() and np.all(v[S["den_u"]] == np.float32(1e-40))
    assert 0 < np.float32(1e-40) < np.finfo(np.float32).tiny and np.all(np.abs(x[S["tiny_t"]]) == np.float32(1e-6))
    assert np.abs(m).max() > 0.3 and 0.09 < v.max() <= 0.1 and np.abs(x).max() > 2     # no case starts from zero
    seen = set()
    for regime in AR.regimes_of(c):
        i = AR.case_input(name, regime)
        i = i[0] if isinstance(c, AR.PairCase) else i
        slots, rows = AR.valid_slots(i.ids, i.n_uniq, c.V)
        assert len(set(rows.tolist())) == len(rows) and len(i.ids) == max(i.cap, 1) == len(i.g)
        assert AR.ALIAS_ROW not in rows or regime == "full"
        seen.add("0" if i.cap == 0 else "n0" if i.n_uniq == 0 else "lt" if i.n_uniq < i.cap else "cap")
        if regime in ("partial", "oob"):
            assert {S["zero_t"], S["den_t"], S["tiny_t"], S["g0"], 0, c.V - 1} <= set(rows.tolist())
            assert not {S["zero_u"], S["den_u"], S["tiny_u"]} & set(rows.tolist())
            assert not i.g[i.ids == S["g0"]].any() and np.isfinite(i.g[:i.n_uniq]).all()
            asc = bool(np.all(np.diff(rows) > 0))
            assert asc == (c.order == "asc"), (name, regime)
        if regime in ("n0", "partial"):
            spare = i.ids[i.n_uniq:] if regime == "partial" else i.ids
            assert len(spare) >= 8 and np.isnan(i.g[i.n_uniq:]).all() and spare.min() >= 0 and spare.max() < c.V
            assert not set(spare.tolist()) & set(rows.tolist())
        if regime == "full":
            assert i.n_uniq == i.cap == c.V and sorted(rows.tolist()) == list(range(c.V))
        if regime == "oob":
            bad = i.ids[(i.ids < 0) | (i.ids >= c.V)]
            assert sorted(bad.tolist()) == [-1, c.V, 2 ** 32 + 3] and i.n_uniq == i.cap
            assert int(np.int64(2 ** 32 + 3).astype(np.int32)) == AR.ALIAS_ROW
        if regime == "partial" and c.V > AR.BIG_V:
            cls = "pair" if isinstance(c, AR.PairCase) else c.cls
            edges = AR.pass_edges(c.V, AR.items_per_row(cls, c.E))
            assert edges and rows.min() == 0 and rows.max() == c.V - 1
            for e in edges:                            # touched and untouched rows on both sides of every pass edge
                near = [r for r in rows.tolist() if abs(r - e) <= 50]
                assert min(near) < e <= max(near) and len(near) < 100
    if not isinstance(c, AR.PairCase):
        assert seen == {"0", "n0", "lt", "cap"}
        assert set(AR.regimes_of(c)) == set(AR.REGIMES)
    else:
        assert "lt" in seen


def test_pair_cases_together_reach_every_count():
    assert {r for c in AR.PAIR_CASES for r in c.regimes} == set(AR.REGIMES)


# ---- room and mutants -----------------------------------------------------------------------------------------------
def _case_ratios(name, regime, mut=None):
    """the ratios of the fp32 restatement (or a mutant of it), one dict per table of the case"""
    ref, got = AR.case_reference(name, regime), AR.case_f32(name, regime, mut)
    if isinstance(AR.BY_NAME[name], AR.PairCase):
        return [AR.ratios(*g, r) for g, r in zip(got, ref)]
    return [AR.ratios(*got, ref)]


@pytest.mark.parametrize("name", [c.name for c in AR.SPARSE_CASES + AR.LAZY_CASES + AR.PAIR_CASES])
def test_fp32_restatement_has_room_under_the_bounds(name):
    c = AR.BY_NAME[name]
    for regime in AR.regimes_of(c, gpu=False):
        ref, got = AR.case_reference(name, regime), AR.case_f32(name, regime)
        st = AR.case_state(name)
        trios = [(got[0], ref[0], st[:3]), (got[1], ref[1], st[3:])] if isinstance(c, AR.PairCase) else [(got, ref, st)]
        for g, r, start in trios:
            q = AR.ratios(*g, r)
            print("%s %s x %.3f m %.3f v %.3f" % (name, regime, q["x"], q["m"], q["v"]))
            assert AR.has_room(q), (name, regime, q)
            row = AR.SPECIAL["zero_u"]                  # an untouched m = v = 0 row stays bit-identical
            if not r.touched[row]:
                assert all(np.array_equal(a[row].view(np.uint32), b[row].view(np.uint32)) for a, b in zip(g, start))
            assert np.isfinite(r.x).all() and np.isfinite(r.bx).all()


@pytest.mark.parametrize("name", [c.name for c in AR.DENSE_CASES] + [c.name for c in AR.MULTI_CASES])
def test_dense_fp32_restatement_has_room(name):
    c = AR.BY_NAME[name]
    inputs = [AR.dense_input(c.n, c.seed)] if isinstance(c, AR.DenseCase) else AR.multi_input(c)
    for x, m, v, g in inputs:
        q = AR.ratios(*AR.f32_dense(x, m, v, g, AR.scalars(c.t, dt=np.float32)), AR.ref_dense(x, m, v, g, AR.scalars(c.t)))
        assert AR.has_room(q), (name, q)
        if x.size >= 16:
            got = AR.f32_dense(x, m, v, g, AR.scalars(c.t, dt=np.float32))
            assert got[0][6] == x[6] and got[1][6] == 0 and got[2][6] == 0 and m[5] == 0 and g[5] != 0 and g[11] == 0


# the case on which each mutant must break a bound, with the reason
MUTANT_BITES = {
    "decay_then_touch": ("vec_1000x16x16", "partial"),     # a touched row decayed twice: m is off by a factor b1
    "unpatched": ("scalar_1000x3x3", "partial"),           # a touched row with the plain decay
    "eps_in_sqrt": ("vec_257x4x4", "n0"),                  # v = 0 and v = 1e-40 rows divide by 3e-4 instead of 1e-7
    "t_plus_1": ("vec_257x4x4", "partial"),                # t = 1: lr_t of step 2
    "t_minus_1": ("vec_1000x16x16", "partial"),            # t = 2: lr_t of step 1
    "swap_b": ("scalar_1000x4x5", "partial"),
    "g_not_squared": ("vec_300x64x64", "partial"),
    "cap_slots": ("vec_1000x16x32", "partial"),            # the unused slots carry NaN gradients
    "narrow_ids": ("scalar_1000x1x32", "oob"),             # 2^32 + 3 becomes row 3
    "one_pass": ("vec_140001x64x64", "partial"),           # rows from 131072 on are never swept
    "pair_w_index": ("pair_1000x16x32", "partial"),
}


@pytest.mark.parametrize("mut", AR.MUTANTS)
def test_every_mutant_breaks_a_bound(mut):
    name, regime = MUTANT_BITES[mut]
    assert all(AR.has_room(r) for r in _case_ratios(name, regime))
    q = max(AR.worst(r) for r in _case_ratios(name, regime, mut))
    print("%s on %s/%s: %.3g of the bound" % (mut, name, regime, q))
    assert q > 1, "the mutant %s stays inside the bounds on %s/%s (%.3g)" % (mut, name, regime, q)


def test_one_pass_mutant_breaks_the_other_two_sweeps_too():
    for name in ("scalar_700001x3x3", "pair_1048700x4x8"):
        assert max(AR.worst(r) for r in _case_ratios(name, "partial", "one_pass")) > 1, name


def test_mutant_table_is_complete():
    assert set(MUTANT_BITES) == set(AR.MUTANTS) and len(AR.MUTANTS) == 11
    assert AR.BY_NAME["vec_257x4x4"].t == 1 and AR.BY_NAME["vec_1000x16x16"].t == 2


def test_lr_t_saturates_where_the_engine_says():
    """the oracle's own float32 lr_t equals float32(lr) from step 32769 on and not at 17000"""
    lr = np.float32(AR.LR)
    for t in AR.LR_T_FAR:
        assert AR.scalars(t, dt=np.float32).lr_t == lr
    assert AR.scalars(17000, dt=np.float32).lr_t != lr and AR.scalars(32768, dt=np.float32).lr_t == lr
