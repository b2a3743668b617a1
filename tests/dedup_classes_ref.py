"""The kernel classes of the generic de-duplication path (csrc/dedup.hip: rec_dedup_plan_i64 and rec_segment_sum_f32)
restated for the tests, the tables of cases that reach every one of them, and the references the GPU tests compare with.
No GPU and no package import here: numpy alone.

sort_class() restates rec_dedup_plan_i64 / radix_sort_ids:
  bits   = ceil(log2 V), clamped to 1..32   (the significant key bits of the LSD radix sort)
  passes = ceil(bits / 8), w = ceil(bits / passes); pass p sorts bits [p w, min(bits, (p+1) w)): the last digit has
           last_dbits = bits - (passes-1) w <= w bits
  pass p writes keys_out / perm when (passes-1-p) is even, else the temporaries: first_pass_to_out = passes is odd
sum_class() restates rec_segment_sum_f32:
  E > 256                  segsum_wide_kernel alone (a workgroup per output row, no chunk partials)
  else                     segsum_chunk_kernel<GE>, GE = the smallest of 1, 2, 4, .., 256 that is >= E, NS = 256 / GE row
                           slots, then segsum_vec_kernel when E % 4 == 0 and vals, out, workspace are 16-byte aligned
                           (lpr = E / 4 lanes per row, NG = 256 // lpr lane groups finish a long run), else
                           segsum_scalar_kernel
run_regimes() names what a plan holds of the edges of the long-run logic (a run of more than LONG sorted positions is
summed chunk by chunk, CH positions per chunk, which = 0: the run covers the chunk's first position, 1: it starts inside).

Two kinds of values: int_vals() -- fp32 integers in [-8, 8], so small that every partial sum of every subset in every
order is an integer below 2^24 and the int64 segment sum is the answer bit for bit, whatever the order of the additions;
normal_vals() -- standard normal, compared with the fp64 oracle.layers_np.dedup_indexed_slices under the suite's bounds.
"""
import collections
import functools

import numpy as np

from tests import helpers as H_

TILE = 1024       # sorted keys per workgroup of count_heads_kernel / finalize_kernel
CH = 256          # sorted positions per chunk of the long-run path
LONG = 256        # runs longer than this take the chunked path
RS_TILE = 2048    # keys per workgroup of a radix-sort pass
GE_LADDER = (1, 2, 4, 8, 16, 32, 64, 128, 256)
MAX_N, MAX_FLOATS = 8192, 1_200_000          # no case above these (ids, n * E)

SortClass = collections.namedtuple("SortClass", "bits passes w last_dbits first_pass_to_out")
SumClass = collections.namedtuple("SumClass", "kernel GE NS lpr NG lpr_divides_256")


def sort_class(V):
    if not 1 <= V <= 1 << 32:
        raise ValueError("rec_dedup_plan_i64 takes 1 <= V <= 2^32, got %d" % V)
    bits = min(32, max(1, int(V - 1).bit_length()))          # smallest b >= 1 with 2^b >= V
    passes = (bits + 7) // 8
    w = -(-bits // passes)
    return SortClass(bits, passes, w, bits - (passes - 1) * w, (passes - 1) % 2 == 0)


def sum_class(E, aligned=True):
    if E < 1:
        raise ValueError("E >= 1")
    if E > 256:
        return SumClass("wide", None, None, None, None, None)
    GE = next(g for g in GE_LADDER if E <= g)
    if E % 4 == 0 and aligned:
        lpr = E // 4
        return SumClass("vec", GE, 256 // GE, lpr, 256 // lpr, 256 % lpr == 0)
    return SumClass("scalar", GE, 256 // GE, None, None, None)


# ---- regimes ------------------------------------------------------------------------------------------------------
SPAN_REGIMES = tuple("long_spans_ge_4NG_plus_%d_chunks" % r for r in range(4))
REMAINDER_REGIMES = tuple("group_left_with_%d_chunks" % j for j in range(4))
PLAN_REGIMES = ("short", "len_eq_LONG", "len_LONG_plus_1", "long_starts_on_chunk", "long_starts_inside_chunk",
                "long_ends_on_chunk", "two_long_in_one_chunk", "long_at_last_position_of_chunk_after_254_singletons",
                "long_is_first_run", "long_is_last_run", "n_eq_multiple_of_CH", "n_not_multiple_of_CH")
VEC_REGIMES = SPAN_REGIMES + REMAINDER_REGIMES + ("group_runs_unrolled_loop", "long_run_straddles_two_workgroups")
REGIMES = PLAN_REGIMES + VEC_REGIMES


def boundaries(seg_start, n):
    """the run boundaries [nu + 1] of a seg_start array that may carry the padded tail (entries equal to n)"""
    seg = np.asarray(seg_start, np.int64).reshape(-1)
    nu = int(np.searchsorted(seg, n, side="left"))
    if n == 0:
        return np.zeros(1, np.int64)
    assert seg[0] == 0 and seg[nu] == n and np.all(np.diff(seg[:nu + 1]) > 0)
    return seg[:nu + 1]


def group_shares(m, NG):
    """chunk partials each of the NG lane groups of segsum_vec_kernel adds for a run with m chunks after its first:
    group g takes chunks chb + 1 + g, + NG, ... <= che"""
    return [(m - 1 - g) // NG + 1 if m - 1 - g >= 0 else 0 for g in range(NG)]


def run_regimes(seg_start, n, E, aligned=True):
    """The set of REGIMES a plan holds at row width E.  The plan regimes read the run boundaries alone; the vec regimes
    exist for the vec class only:
      long_spans_ge_4NG_plus_r_chunks   a long run has m >= 4 NG chunks after its first and (m - 4 NG) % 4 == r: lane
                                        group 0 goes through the 4x-unrolled loop and r groups are left a chunk more
      group_runs_unrolled_loop          a lane group adds >= 4 partials of one run
      group_left_with_j_chunks          a lane group is left j partials (0..3) for the remainder loop
      long_run_straddles_two_workgroups the lpr lanes of a long run's output row lie in two workgroups"""
    b = boundaries(seg_start, n)
    nu = b.size - 1
    out = set()
    if n == 0:
        return out
    out.add("n_eq_multiple_of_CH" if n % CH == 0 else "n_not_multiple_of_CH")
    lens = np.diff(b)
    if np.any(lens <= LONG):
        out.add("short")
    if np.any(lens == LONG):
        out.add("len_eq_LONG")
    if np.any(lens == LONG + 1):
        out.add("len_LONG_plus_1")
    cls = sum_class(E, aligned)
    touched = collections.Counter()
    for u in np.nonzero(lens > LONG)[0]:
        u = int(u)
        s0, s1 = int(b[u]), int(b[u + 1])
        chb, che = s0 // CH, (s1 - 1) // CH
        touched.update(range(chb, che + 1))
        out.add("long_starts_on_chunk" if s0 % CH == 0 else "long_starts_inside_chunk")
        if s1 % CH == 0:
            out.add("long_ends_on_chunk")
        if u == 0:
            out.add("long_is_first_run")
        if u == nu - 1:
            out.add("long_is_last_run")
        # the chunk kernel tests runs lo .. lo + 255 (lo: the run that covers the chunk's first position), one per thread
        lo = int(np.searchsorted(b, chb * CH, side="right")) - 1
        if s0 % CH == CH - 1 and u - lo == 255 and np.all(lens[lo + 1:u] == 1):
            out.add("long_at_last_position_of_chunk_after_254_singletons")
        if cls.kernel == "vec":
            m = che - chb
            if m >= 4 * cls.NG:
                out.add(SPAN_REGIMES[(m - 4 * cls.NG) % 4])
            for share in group_shares(m, cls.NG):
                out.add(REMAINDER_REGIMES[share % 4])
                if share >= 4:
                    out.add("group_runs_unrolled_loop")
            if (u * cls.lpr) // 256 != (u * cls.lpr + cls.lpr - 1) // 256:
                out.add("long_run_straddles_two_workgroups")
    if touched and max(touched.values()) >= 2:
        out.add("two_long_in_one_chunk")
    return out


# ---- ids with prescribed runs -------------------------------------------------------------------------------------
def distinct_keys(r, k, V):
    """k distinct keys of [0, V), ascending, 0 and V-1 among them (k == 1: V-1 alone)"""
    if not 1 <= k <= V:
        raise ValueError("%d runs need as many distinct keys, V = %d" % (k, V))
    if k == 1:
        return np.array([V - 1], np.int64)
    need, inner = k - 2, np.zeros(0, np.int64)
    if need and V - 2 <= 4 * need:
        inner = r.choice(V - 2, need, replace=False).astype(np.int64) + 1
    while inner.size < need:                               # a huge id space: draw, drop the repeats, draw again
        draw = r.integers(1, V - 1, size=2 * (need - inner.size) + 8, dtype=np.int64)
        inner = np.unique(np.concatenate([inner, draw]))
        if inner.size > need:
            inner = r.permutation(inner)[:need]
    return np.sort(np.concatenate([[0, V - 1], inner]).astype(np.int64))


def ids_with_runs(lengths, V, layout="scattered", seed=0):
    """Flat int64 ids whose sorted runs have exactly lengths[u] members for the u-th smallest key (the ``ranked``
    placement of helpers.plan_batch: a run sits at a chosen plan slot).  Keys are distinct, 0 and V-1 among them.
    ``scattered``: the members of a run at random positions; ``clustered``: adjacent, the runs in random order."""
    if layout not in ("scattered", "clustered"):
        raise ValueError("layout is 'scattered' or 'clustered'")
    lens = np.asarray(lengths, np.int64).reshape(-1)
    if lens.size == 0 or lens.min() < 1:
        raise ValueError("run lengths must be >= 1")
    r = H_.rng(seed)
    keys = distinct_keys(r, lens.size, V)
    if layout == "clustered":
        order = r.permutation(lens.size)
        return np.repeat(keys[order], lens[order])
    return np.repeat(keys, lens)[r.permutation(int(lens.sum()))]


def int_vals(n_rows, E, seed=0):
    return H_.rng(seed).integers(-8, 9, size=(n_rows, E)).astype(np.float32)


def normal_vals(n_rows, E, seed=0):
    return H_.rng(seed).normal(size=(n_rows, E)).astype(np.float32)


def host_plan(ids):
    """(uniq ascending, seg_start [nu + 1], perm = stable order) as numpy defines them"""
    ids = np.asarray(ids, np.int64).reshape(-1)
    perm = np.argsort(ids, kind="stable")
    uniq, counts = np.unique(ids, return_counts=True)
    return uniq, np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), perm


def exact_sums(ids, vals, row_div=1):
    """int64 [nu, E]: the segment sums of integer-valued fp32 rows, lookup i reading row i // row_div"""
    _, seg, perm = host_plan(ids)
    rows = np.asarray(vals)[perm // row_div].astype(np.int64)
    assert np.array_equal(rows, np.asarray(vals)[perm // row_div])          # the values are integers
    return np.add.reduceat(rows, seg[:-1], axis=0)


def partial_sum_bound(ids, vals, row_div=1):
    """max over runs and columns of sum |v|: no partial sum of any subset in any order exceeds it"""
    return int(exact_sums(ids, np.abs(np.asarray(vals)), row_div).max())


# ---- plans: run lengths by ascending key ----------------------------------------------------------------------------
def _edges(pad_to=None):
    """runs of 1, 2, LONG, LONG+1, 2 CH and 2 CH + 1 at chosen sorted positions:
         0     [1] [2]
         3     [LONG]                 the longest short run
         259   [LONG+1]               long, starts and ends inside a chunk
         516   252 singletons
         768   [2 CH]                 long, starts and ends on a multiple of CH
         1280  [2 CH + 1]             long, starts on a multiple, ends one position into chunk 7
         1793  [300]                  a second long run that starts in chunk 7: two long runs in one chunk
         2093  211 singletons         up to 2304 = 9 CH
         2304  255 singletons         the run on the chunk's first position and 254 more ...
         2559  [400]                  ... then a long run on the chunk's last position: thread 255 of the chunk kernel
         2959  [1] [2] [1]            n = 2963; ``pad_to`` adds singletons"""
    lens = [1, 2, LONG, LONG + 1] + [1] * 252 + [2 * CH, 2 * CH + 1, 300] + [1] * 211 + [1] * 255 + [400, 1, 2, 1]
    assert sum(lens) == 2963
    if pad_to:
        lens += [1] * (pad_to - sum(lens))
    return lens


def _one_long(prefix, run, suffix):
    return [1] * prefix + [run] + [1] * suffix


PLANS = {
    "edges": _edges(),
    "edges_padded": _edges(3072),
    "short_mix": [LONG, LONG - 1, 200] + list(range(1, 41)) + [3, 2, 1] * 60 + [1] * 117,     # no long run
    "singles": [1] * 1300,
    "all_equal": [1300],
    "small_mix": [1, 2, 3, 4, 5, 7, 8, 9, LONG, LONG + 1, 300] + [1] * 150 + [2] * 20,       # the wide rows' plan
    # long runs at the plan slots u = 5, 10, 25, 51, 85: the lpr lanes of row u cross a multiple of 256 at lpr = 50, 25,
    # 10, 5, 3 (E = 200, 100, 40, 20, 12), so two workgroups of segsum_vec_kernel finish that run
    "straddle": [1] * 5 + [LONG + 1] + [1] * 4 + [LONG + 1] + [1] * 14 + [300] + [1] * 25 + [LONG + 1] + [1] * 33
                + [LONG + 1] + [1] * 20,
    # one long run of about 6000 with m = 23, 22, 21, 20 chunks after its first (NG = 5 at E = 200: 4 NG + 3 .. + 0)
    "long_m23": _one_long(255, 5634, 111),       # starts on the last position of chunk 0, n = 6000
    "long_m22": _one_long(0, 5888, 0),           # the whole plan, n = 23 CH
    "long_m21": _one_long(100, 5277, 10),
    "long_m20": _one_long(256, 5121, 0),         # starts on chunk 1, the last run
    # the same within 1.2 M floats at E = 256 (NG = 4: 4 NG + 2 .. + 0)
    "long_m18": _one_long(255, 4354, 70),
    "long_m17": _one_long(0, 4608, 0),
    "long_m16": _one_long(10, 4087, 3),
}
PLAN_CLAIMS = {
    "edges": {"short", "len_eq_LONG", "len_LONG_plus_1", "long_starts_on_chunk", "long_starts_inside_chunk",
              "long_ends_on_chunk", "two_long_in_one_chunk", "long_at_last_position_of_chunk_after_254_singletons",
              "n_not_multiple_of_CH"},
    "edges_padded": {"short", "len_eq_LONG", "len_LONG_plus_1", "long_starts_on_chunk", "long_starts_inside_chunk",
                     "long_ends_on_chunk", "two_long_in_one_chunk",
                     "long_at_last_position_of_chunk_after_254_singletons", "n_eq_multiple_of_CH"},
    "short_mix": {"short", "len_eq_LONG", "n_not_multiple_of_CH"},
    "singles": {"short", "n_not_multiple_of_CH"},
    "all_equal": {"long_starts_on_chunk", "long_is_first_run", "long_is_last_run", "n_not_multiple_of_CH"},
    "small_mix": {"short", "len_eq_LONG", "len_LONG_plus_1", "n_not_multiple_of_CH"},
    "straddle": {"short", "len_LONG_plus_1", "long_starts_inside_chunk", "two_long_in_one_chunk",
                 "n_not_multiple_of_CH"},
    "long_m23": {"short", "long_starts_inside_chunk", "n_not_multiple_of_CH"},
    "long_m22": {"long_starts_on_chunk", "long_ends_on_chunk", "long_is_first_run", "long_is_last_run",
                 "n_eq_multiple_of_CH"},
    "long_m21": {"short", "long_starts_inside_chunk", "n_not_multiple_of_CH"},
    "long_m20": {"short", "long_starts_on_chunk", "long_is_last_run", "n_not_multiple_of_CH"},
    "long_m18": {"short", "long_starts_inside_chunk", "n_not_multiple_of_CH"},
    "long_m17": {"long_starts_on_chunk", "long_ends_on_chunk", "long_is_first_run", "long_is_last_run",
                 "n_eq_multiple_of_CH"},
    "long_m16": {"short", "long_starts_inside_chunk", "n_not_multiple_of_CH"},
}
NO_LONG_RUN = ("short_mix", "singles")


def plan_seg(plan):
    return np.concatenate([[0], np.cumsum(PLANS[plan])]).astype(np.int64)


def plan_n(plan):
    return int(sum(PLANS[plan]))


# ---- the table of sums ----------------------------------------------------------------------------------------------
E_VALUES = (1, 2, 3, 4, 8, 12, 16, 20, 32, 40, 64, 100, 128, 130, 200, 256, 257, 300, 816)
# written out, not computed by sum_class: (GE, lpr divides 256) the issue's E values claim
E_CLAIMS = {1: (1, None), 2: (2, None), 3: (4, None), 4: (4, True), 8: (8, True), 12: (16, False), 16: (16, True),
            20: (32, False), 32: (32, True), 40: (64, False), 64: (64, True), 100: (128, False), 128: (128, True),
            130: (256, None), 200: (256, False), 256: (256, True), 257: (None, None), 300: (None, None),
            816: (None, None)}
# id spaces: the sort's pass counts 1..4, each with an even split and (2..4) a narrower last digit
V_CYCLE = (65536, 100003, (1 << 17) + 1, (1 << 24) + 1, 1 << 32, 5000, 1 << 24, (1 << 31) + 5)
V_ALL_EQUAL = (1, 200, 256, 257, (1 << 31) + 5)

SumCase = collections.namedtuple("SumCase", "name E aligned plan row_div V layout seed kernel GE divides claims")


def _sum_cases():
    out = []

    def add(E, aligned, plan, row_div=1):
        i = len(out)
        GE, divides = E_CLAIMS[E]
        kernel = "wide" if E > 256 else "vec" if (E % 4 == 0 and aligned) else "scalar"
        V = V_ALL_EQUAL[i % len(V_ALL_EQUAL)] if len(PLANS[plan]) == 1 else V_CYCLE[i % len(V_CYCLE)]
        name = "e%d_%s_%s%s" % (E, "al" if aligned else "mis", plan, "_div%d" % row_div if row_div > 1 else "")
        out.append(SumCase(name, E, aligned, plan, row_div, V, ("scattered", "clustered")[i % 2], i, kernel, GE,
                           divides if kernel == "vec" else None, frozenset(PLAN_CLAIMS[plan])))

    for E in E_VALUES:
        if E > 256:
            for plan in ("small_mix", "singles", "all_equal"):
                add(E, True, plan)
            add(E, False, "small_mix")
            continue
        for aligned in ((True, False) if E % 4 == 0 else (True,)):
            for plan in ("edges", "edges_padded", "short_mix", "singles", "all_equal"):
                add(E, aligned, plan)
    for E in (4, 16, 64, 200):
        for plan in ("long_m23", "long_m22", "long_m21", "long_m20"):
            add(E, True, plan)
            if plan in ("long_m23", "long_m22"):
                add(E, False, plan)
    for E in (256, 128, 100, 40):          # NG = 4, 8, 10, 25; at NG = 8 a lane group is left three partials
        for plan in ("long_m18", "long_m17", "long_m16"):
            add(E, True, plan)
    add(256, False, "long_m18")
    add(256, False, "long_m17")
    for E in (12, 20, 40, 100, 200):
        add(E, True, "straddle")
    for E, plan in ((3, "long_m23"), (130, "long_m22"), (1, "long_m20"), (2, "long_m21")):
        add(E, True, plan)
    # row_div > 1: lookup i reads row i // row_div (the w table's gradient: one value per example, F lookups)
    for E, aligned in ((1, True), (16, True), (16, False)):
        add(E, aligned, "edges_padded", row_div=3)
    add(1, True, "long_m22", row_div=4)
    add(64, True, "long_m22", row_div=4)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


SUM_CASES = _sum_cases()
SUM_BY_NAME = {c.name: c for c in SUM_CASES}


def case_ids(case):
    return plan_ids(case.plan, case.V, case.layout, case.seed)


@functools.lru_cache(maxsize=None)
def plan_ids(plan, V, layout, seed):
    ids = ids_with_runs(PLANS[plan], V, layout, seed)
    ids.setflags(write=False)
    return ids


def case_rows(case):
    n = plan_n(case.plan)
    assert n % case.row_div == 0
    return n // case.row_div


def distinct_plans(cases=None):
    """the (plan, V, layout, seed) of the id lists SUM_CASES sums over, one per distinct list of ids"""
    seen, out = set(), []
    for c in (SUM_CASES if cases is None else cases):
        key = (c.plan, c.V, c.layout)
        if key not in seen:
            seen.add(key)
            out.append((c.plan, c.V, c.layout, c.seed))
    return out


@functools.lru_cache(maxsize=8)
def reference(name, kind):
    """(uniq, sums) of a row of SUM_CASES: kind 'int' -> the exact int64 sums of int_vals, 'normal' -> the fp64 sums of
    normal_vals by oracle.layers_np.dedup_indexed_slices.  Shared: do not write to them."""
    from oracle import layers_np as L
    c = SUM_BY_NAME[name]
    ids = case_ids(c)
    if kind == "int":
        vals = int_vals(case_rows(c), c.E, c.seed)
        out = (np.unique(ids), exact_sums(ids, vals, c.row_div))
    else:
        vals = normal_vals(case_rows(c), c.E, c.seed)
        out = L.dedup_indexed_slices(ids, np.repeat(vals.astype(np.float64), c.row_div, axis=0), "sorted")
    for a in out:
        a.setflags(write=False)
    return out


def tolerance(case, ref):
    """The suite's own bounds: 1e-5 max(1, |ref|max) where no run exceeds LONG (tests/test_gpu_ops.py,
    test_fm_bwd_vals_and_dedup), 1e-4 |ref|max where one does (tests/test_gpu_din.py, test_dedup_long_runs)."""
    top = float(np.abs(ref).max())
    if max(PLANS[case.plan]) > LONG:
        return 1e-4 * top
    return 1e-5 * max(1.0, top)


# ---- the table of sorts ---------------------------------------------------------------------------------------------
SORT_V = (1, 2, 255, 256, 257, 511, 65536, 65537, (1 << 17) + 1, 100003, 1 << 24, (1 << 24) + 1, (1 << 31) + 5, 1 << 32)
SORT_N = (1, 2, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
# written out: V -> (bits, digit widths by pass)
SORT_CLAIMS = {1: (1, (1,)), 2: (1, (1,)), 255: (8, (8,)), 256: (8, (8,)), 257: (9, (5, 4)), 511: (9, (5, 4)),
               65536: (16, (8, 8)), 65537: (17, (6, 6, 5)), (1 << 17) + 1: (18, (6, 6, 6)), 100003: (17, (6, 6, 5)),
               1 << 24: (24, (8, 8, 8)), (1 << 24) + 1: (25, (7, 7, 7, 4)), (1 << 31) + 5: (32, (8, 8, 8, 8)),
               1 << 32: (32, (8, 8, 8, 8))}

SortCase = collections.namedtuple("SortCase", "name V n seed")
SORT_CASES = tuple(SortCase("v%d_n%d" % (V, n), V, n, 7 * i + j) for i, V in enumerate(SORT_V)
                   for j, n in enumerate(SORT_N))
SORT_BY_NAME = {c.name: c for c in SORT_CASES}


def digit_pairs(V):
    """[(a, b)] keys of [0, V) that differ in one bit of the lowest digit only, and in one bit of the top digit only"""
    sc = sort_class(V)
    out = []
    if V >= 2:
        a = min(V - 2, 0x5A5A5A5A & ((1 << sc.bits) - 1)) & ~1
        out.append((a, a | 1))
    top = 1 << (sc.bits - 1)
    if sc.passes >= 2:
        low = min(3, V - 1 - top)
        out.append((low, top + low))
    return out


@functools.lru_cache(maxsize=None)
def sort_ids(name):
    """n ids of [0, V): drawn from a pool of about n / 2 keys (so most repeat, far apart), 0 and V-1 among them, one key
    on the first and the last position, and the digit_pairs side by side"""
    c = SORT_BY_NAME[name]
    r = H_.rng(5000 + c.seed)
    V, n = c.V, c.n
    if n == 1:
        ids = np.array([V - 1], np.int64)
    elif n == 2:
        ids = np.array([V - 1, 0], np.int64)
    else:
        pool = distinct_keys(r, min(V, n // 2 + 1), V)
        ids = pool[r.integers(0, pool.size, size=n)]
        at = 8
        for a, b in digit_pairs(V):
            ids[at:at + 4] = (b, a, b, a)
            at += 4
        ids[1], ids[n // 2] = V - 1, 0
        ids[0] = ids[n - 1] = pool[pool.size // 2]
    ids.setflags(write=False)
    return ids
