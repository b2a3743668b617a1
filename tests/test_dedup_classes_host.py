"""CPU checks behind tests/test_gpu_dedup_classes.py: tests/dedup_classes_ref.py restates the thresholds that are in the
text of csrc/dedup.hip today, every case of SUM_CASES and SORT_CASES is in the class and holds the regimes it claims,
their union reaches every class and regime, the integer-valued cases cannot round, the references agree with each other,
and ids_with_runs builds the runs it was asked for.  A failure on the GPU can then not be blamed on the case table."""
import os
import re

import numpy as np
import pytest

from oracle import layers_np as L
from tests import dedup_classes_ref as DR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "explicit-tf2-recommendation_amd", "csrc", "dedup.hip")
SUM_NAMES = [c.name for c in DR.SUM_CASES]


@pytest.fixture(scope="module")
def text():
    with open(SOURCE) as f:
        return f.read()


def test_constants_are_the_ones_in_the_source(text):
    found = {name: int(val) for name, val in re.findall(r"constexpr int (TILE|CH|LONG|RS_TILE) = (\d+)[;,]", text)}
    assert found == {"TILE": DR.TILE, "CH": DR.CH, "LONG": DR.LONG, "RS_TILE": DR.RS_TILE}
    assert DR.LONG >= DR.CH                    # at most two long runs touch a chunk
    assert "if (s1 - s0 > LONG)" in text and text.count("if (s1 - s0 <= LONG)") == 2
    assert "sizeof(float) * (size_t)ceil_div64(n, CH) * 2 * (size_t)E + 256" in text


def test_ladder_and_kernel_choice_are_the_ones_in_the_source(text):
    body = text[text.index('extern "C" int rec_segment_sum_f32('):]
    body = body[:body.index("\n}\n")]
    rungs = [(int(a), int(b)) for a, b in re.findall(r"if \(E <= (\d+)\) CHUNK\((\d+)\);", body)]
    last = re.findall(r"\n\s*else CHUNK\((\d+)\);", body)
    assert rungs == [(g, g) for g in DR.GE_LADDER[:-1]] and last == [str(DR.GE_LADDER[-1])]
    assert "if (E > 256) {" in body and body.index("if (E > 256) {") < body.index("CHUNK(1)")
    assert ("bool vec = E % 4 == 0 && rec_is_aligned16(vals) && rec_is_aligned16(out) && rec_is_aligned16(workspace);"
            in body)
    assert "int lpr = E / 4;" in body and "const int NG = 256 / lpr;" in text
    for E in range(1, 300):
        for aligned in (True, False):
            c = DR.sum_class(E, aligned)
            if E > 256:
                assert c.kernel == "wide"
                continue
            want = next(b for a, b in rungs + [(256, 256)] if E <= a)
            assert (c.GE, c.NS) == (want, 256 // want) and c.GE >= E and (c.GE == 1 or c.GE // 2 < E)
            assert c.kernel == ("vec" if E % 4 == 0 and aligned else "scalar")
            if c.kernel == "vec":
                assert (c.lpr, c.NG, c.lpr_divides_256) == (E // 4, 256 // (E // 4), 256 % (E // 4) == 0)


def test_sort_class_restates_the_source(text):
    for line in ("while (end_bit < 32 && (int64_t(1) << end_bit) < V) ++end_bit;",
                 "const int passes = (int)((bits + 7) / 8);", "const int w = (int)((bits + passes - 1) / passes);",
                 "const int dbits = ((int)bits - shift < w) ? (int)bits - shift : w;",
                 "const bool to_out = ((passes - 1 - p) & 1) == 0;"):
        assert line in text, line
    for V, (bits, widths) in DR.SORT_CLAIMS.items():
        c = DR.sort_class(V)
        assert (c.bits, c.passes, c.w, c.last_dbits) == (bits, len(widths), widths[0], widths[-1]), V
        assert sum(widths) == bits and all(x == c.w for x in widths[:-1]) and max(widths) <= 8
        assert c.first_pass_to_out == (len(widths) % 2 == 1)
    for V in list(range(1, 600)) + [(1 << k) + d for k in range(9, 33) for d in (-1, 0, 1) if (1 << k) + d <= 1 << 32]:
        c, end_bit = DR.sort_class(V), 1
        while end_bit < 32 and (1 << end_bit) < V:               # the loop of rec_dedup_plan_i64
            end_bit += 1
        assert c.bits == end_bit and (c.passes - 1) * c.w < c.bits <= c.passes * c.w and 1 <= c.last_dbits <= c.w <= 8
    for V in (0, -1, (1 << 32) + 1):
        with pytest.raises(ValueError):
            DR.sort_class(V)


def test_sort_cases_are_the_issue_s_and_hold_what_they_claim():
    assert set(DR.SORT_V) == {1, 2, 255, 256, 257, 511, 65536, 65537, 2 ** 17 + 1, 100003, 2 ** 24, 2 ** 24 + 1,
                              2 ** 31 + 5, 2 ** 32} == set(DR.SORT_CLAIMS)
    assert set(DR.SORT_N) == {1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4097}
    assert len(DR.SORT_CASES) == len(DR.SORT_V) * len(DR.SORT_N)
    for c in DR.SORT_CASES:
        ids = DR.sort_ids(c.name)
        assert ids.dtype == np.int64 and ids.shape == (c.n,) and ids.min() >= 0 and ids.max() < c.V
        assert c.V - 1 in ids and (0 in ids or c.n == 1)
        if c.n < 1000:
            continue
        pairs = DR.digit_pairs(c.V)
        sc = DR.sort_class(c.V)
        assert len(pairs) == (c.V >= 2) + (sc.passes >= 2)
        for k, (a, b) in enumerate(pairs):
            assert a in ids and b in ids and 0 <= a < b < c.V
            if k == 0:
                assert a ^ b == 1                                  # the lowest bit of the lowest digit
            else:
                assert a ^ b == 1 << (sc.bits - 1) and (sc.passes - 1) * sc.w <= sc.bits - 1      # of the top digit
            assert np.any((ids[:-1] == b) & (ids[1:] == a))        # side by side, the larger first
        uniq, counts = np.unique(ids, return_counts=True)
        assert ids[0] == ids[-1] and (c.V == 1 or counts.max() < c.n)      # a repeat as far apart as can be
        assert uniq.size < c.n                                     # and stability is observable in many runs


def test_sum_cases_are_in_the_class_they_claim():
    for c in DR.SUM_CASES:
        cls = DR.sum_class(c.E, c.aligned)
        assert (cls.kernel, cls.GE, cls.lpr_divides_256) == (c.kernel, c.GE, c.divides), c.name
        assert c.E in DR.E_VALUES and DR.E_CLAIMS[c.E][0] == c.GE


def test_sum_cases_hold_the_regimes_they_claim():
    for plan, lens in DR.PLANS.items():
        seg = DR.plan_seg(plan)
        got = DR.run_regimes(seg, seg[-1], 3) & set(DR.PLAN_REGIMES)
        assert got >= DR.PLAN_CLAIMS[plan], (plan, DR.PLAN_CLAIMS[plan] - got)
        assert (max(lens) > DR.LONG) == (plan not in DR.NO_LONG_RUN)
        padded = np.concatenate([seg, np.full(seg[-1] + 1 - seg.size, seg[-1])])       # as the plan pads seg_start
        assert DR.run_regimes(padded, seg[-1], 3) == DR.run_regimes(seg, seg[-1], 3)
    for c in DR.SUM_CASES:
        assert c.claims == DR.PLAN_CLAIMS[c.plan]


def test_sizes_stay_small():
    for c in DR.SUM_CASES:
        n = DR.plan_n(c.plan)
        assert n <= DR.MAX_N == 8192 and n * c.E <= DR.MAX_FLOATS == 1_200_000, c.name
        assert len(DR.PLANS[c.plan]) <= c.V and n % c.row_div == 0
    assert max(DR.SORT_N) <= DR.MAX_N


def test_union_of_sum_cases_reaches_every_class_and_regime():
    pairs = {(c.kernel, c.GE) for c in DR.SUM_CASES}
    assert pairs == {(k, g) for k in ("vec", "scalar") for g in DR.GE_LADDER if not (k == "vec" and g < 4)} | {
        ("wide", None)}
    assert {c.divides for c in DR.SUM_CASES if c.kernel == "vec"} == {True, False}
    assert {c.E for c in DR.SUM_CASES} == set(DR.E_VALUES) == {1, 2, 3, 4, 8, 12, 16, 20, 32, 40, 64, 100, 128, 130,
                                                               200, 256, 257, 300, 816}
    for E in DR.E_VALUES:                                          # E % 4 == 0: aligned and offset by 4 bytes
        assert {c.aligned for c in DR.SUM_CASES if c.E == E} == ({True, False} if E % 4 == 0 or E > 256 else {True})
    reached = {}
    for c in DR.SUM_CASES:
        seg = DR.plan_seg(c.plan)
        for reg in DR.run_regimes(seg, seg[-1], c.E, c.aligned):
            reached.setdefault(reg, set()).add((c.kernel, c.GE))
    assert set(reached) == set(DR.REGIMES), set(DR.REGIMES) - set(reached)
    narrow = {(k, g) for (k, g) in pairs if k != "wide"}
    for reg in DR.PLAN_REGIMES:                                    # every plan regime on every chunk / finish kernel
        assert reached[reg] >= narrow, (reg, narrow - reached[reg])
    for reg in ("long_run_straddles_two_workgroups",):             # every lpr that does not divide 256
        assert {c.E for c in DR.SUM_CASES if c.kernel == "vec" and not c.divides
                and reg in DR.run_regimes(DR.plan_seg(c.plan), DR.plan_n(c.plan), c.E)} == {12, 20, 40, 100, 200}
    # the unrolled loop of the vec kernel with every remainder, at NG = 5 (E = 200); NG = 4 (E = 256) reaches 0..2
    # inside the size cap
    at = {E: set().union(*(DR.run_regimes(DR.plan_seg(c.plan), DR.plan_n(c.plan), c.E) & set(DR.SPAN_REGIMES)
                           for c in DR.SUM_CASES if c.E == E and c.kernel == "vec")) for E in (200, 256)}
    assert at[200] == set(DR.SPAN_REGIMES) and at[256] == set(DR.SPAN_REGIMES[:3])
    # row_div > 1 at E = 1 and on a vec class, with and without long runs being all there is
    assert {(c.E, c.kernel) for c in DR.SUM_CASES if c.row_div > 1} >= {(1, "scalar"), (16, "vec"), (64, "vec")}
    assert {c.layout for c in DR.SUM_CASES} == {"scattered", "clustered"}


def test_union_of_cases_reaches_every_pass_count_even_and_narrow():
    for cases in (DR.SUM_CASES, DR.SORT_CASES):
        seen = {(s.passes, s.last_dbits == s.w) for s in (DR.sort_class(c.V) for c in cases)}
        assert seen == {(1, True), (2, True), (2, False), (3, True), (3, False), (4, True), (4, False)}, seen
        assert {DR.sort_class(c.V).first_pass_to_out for c in cases} == {True, False}
    assert {c.V for c in DR.SUM_CASES} >= {1, 1 << 32}


@pytest.mark.parametrize("plan,V,layout,seed", DR.distinct_plans())
def test_ids_with_runs_builds_the_prescribed_runs(plan, V, layout, seed):
    ids = DR.plan_ids(plan, V, layout, seed)
    lens = DR.PLANS[plan]
    uniq, counts = np.unique(ids, return_counts=True)
    assert ids.dtype == np.int64 and np.array_equal(counts, lens)          # run u of the u-th smallest key
    assert uniq[-1] == V - 1 and (uniq[0] == 0 or len(lens) == 1) and ids.min() >= 0
    uq, seg, perm = DR.host_plan(ids)
    assert np.array_equal(seg, DR.plan_seg(plan)) and np.array_equal(uq, uniq)
    for u in np.nonzero(np.asarray(lens) > 1)[0][:50]:
        pos = perm[seg[u]:seg[u + 1]]
        assert np.all(np.diff(pos) > 0)                            # stable: ascending positions inside a run
        if layout == "clustered":
            assert np.all(np.diff(pos) == 1)                       # the members of a run are adjacent


def test_ids_with_runs_refuses_what_it_cannot_build():
    with pytest.raises(ValueError):
        DR.ids_with_runs([1, 1, 1], 2)
    with pytest.raises(ValueError):
        DR.ids_with_runs([2, 0], 10)
    with pytest.raises(ValueError):
        DR.ids_with_runs([2], 10, layout="hot")
    assert DR.ids_with_runs([3], 10).tolist() == [9, 9, 9]
    assert sorted(DR.ids_with_runs([1, 2], 2, "clustered").tolist()) == [0, 1, 1]


@pytest.mark.parametrize("name", SUM_NAMES)
def test_integer_cases_cannot_round_and_the_references_agree(name):
    c = DR.SUM_BY_NAME[name]
    ids, vals = DR.case_ids(c), DR.int_vals(DR.case_rows(c), c.E, c.seed)
    assert vals.dtype == np.float32 and np.array_equal(vals, np.rint(vals)) and np.abs(vals).max() <= 8
    bound = DR.partial_sum_bound(ids, vals, c.row_div)
    assert 0 < bound < 2 ** 24, bound                              # every partial sum in every order is exact in fp32
    uniq, exact = DR.reference(name, "int")
    u64, s64 = L.dedup_indexed_slices(ids, np.repeat(vals.astype(np.float64), c.row_div, axis=0), "sorted")
    assert np.array_equal(uniq, u64) and exact.dtype == np.int64 and np.array_equal(exact, s64)
    assert exact.shape == (len(DR.PLANS[c.plan]), c.E) and np.any(exact != 0)


def test_normal_reference_and_tolerance():
    c = DR.SUM_BY_NAME["e8_al_edges"]
    uniq, ref = DR.reference(c.name, "normal")
    assert ref.dtype == np.float64 and ref.shape == (len(DR.PLANS["edges"]), 8)
    assert DR.tolerance(c, ref) == 1e-4 * np.abs(ref).max()
    c = DR.SUM_BY_NAME["e8_al_singles"]
    ref = DR.reference(c.name, "normal")[1]
    assert DR.tolerance(c, ref) == 1e-5 * max(1.0, np.abs(ref).max())
    small = np.full((2, 2), 0.25)
    assert DR.tolerance(c, small) == 1e-5
