"""The generic de-duplication path (csrc/dedup.hip: rec_dedup_plan_i64, rec_segment_sum_f32) on every kernel class its two
entry points can pick, against numpy.

tests/dedup_classes_ref.py holds the restatement of the dispatch (sort_class, sum_class), the regimes of the long-run
logic (run_regimes) and the tables SORT_CASES / SUM_CASES; tests/test_dedup_classes_host.py proves on the CPU that the
tables reach every (kernel, GE) pair, every regime, both kinds of lpr and every pass count of the sort, and that the
integer-valued cases cannot round.  Here:

  plans  n_uniq, uniq_ids, perm (= numpy's stable argsort) and seg_start bit for bit, the padded tail, two plans of the
         same ids identical, the status codes of the C ABI;
  sums   integer-valued rows: the exact int64 segment sums bit for bit, zeros beyond n_uniq; standard normal rows: the
         fp64 oracle.layers_np.dedup_indexed_slices under the suite's own bounds (1e-5 max(1, |ref|max) without a run of
         more than LONG rows, 1e-4 |ref|max with one); run-to-run bit identity; the 4-byte-misaligned (scalar) result
         bit-equal to the aligned (vec) one where no run is long; wide rows through the wide kernel and through 256-column
         slices;
  buffers  every call goes through ctypes with out, the workspace (sized exactly by the library's own query) and the
         plan's arrays carved out of poisoned buffers between two guard bands of tests/guarded.GUARD bytes: the guards
         hold afterwards, every float of out is finite under poison 0xFF (a chunk partial that is read but was never
         written would read NaN) and out is bit-equal under poison 0x7F.

Ids outside [0, V), as read from the code: the plan does not detect them.  Pass 0 of the sort takes (uint32)id, the
passes order the keys by their low ceil(log2 V) bits alone, run heads are found by comparing whole 32-bit keys and
uniq_ids holds the zero-extended 32-bit key.  Such an id therefore lands at the place of its low bits, can split the run
of an in-range id and comes back truncated to 32 bits; nothing faults, no flag is raised.  Detection is the lookup's job
(the ``oob`` flag of the gather kernels), which runs on the same ids before any plan is used.  No test here feeds such
ids.

Worst measured |got - ref| / bound of the normal-valued sums per class, MI355X (bound as above; the module prints the
table at the end of a run with -s):
  kernel  GE    ratio  case                    kernel  GE    ratio  case
  scalar  1     0.021  e1_al_all_equal         vec     4     0.033  e4_al_short_mix
  scalar  2     0.049  e2_al_short_mix         vec     8     0.031  e8_al_short_mix
  scalar  4     0.038  e4_mis_short_mix        vec     16    0.063  e12_al_short_mix
  scalar  8     0.029  e8_mis_short_mix        vec     32    0.049  e20_al_short_mix
  scalar  16    0.028  e12_mis_short_mix       vec     64    0.045  e64_al_short_mix
  scalar  32    0.035  e20_mis_short_mix       vec     128   0.041  e100_al_short_mix
  scalar  64    0.049  e64_mis_short_mix       vec     256   0.057  e256_al_short_mix
  scalar  128   0.045  e100_mis_short_mix      wide    -     0.016  e300_al_all_equal
  scalar  256   0.066  e256_mis_short_mix
The worst cases are the sequential sums of runs of up to LONG rows under the tighter bound; the chunked long runs stay
below 0.03 of theirs.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dedup_classes_ref as DR
from tests import guarded

pytestmark = pytest.mark.gpu
GUARD = guarded.GUARD
POISONS = (guarded.POISON_NAN, guarded.POISON_FINITE)


@pytest.fixture(scope="module")
def R():
    assert torch.cuda.is_available()
    import explicit_tf2_recommendation_amd as pkg
    return pkg


@pytest.fixture(scope="module")
def lib(R):
    from explicit_tf2_recommendation_amd._lib import lib
    return lib


@pytest.fixture(scope="module")
def limits(R):
    from explicit_tf2_recommendation_amd._lib import LIMITS
    return LIMITS


@pytest.fixture(scope="module")
def ratios():
    worst = {}
    yield worst
    print("\nworst |got - ref| / bound of the normal-valued sums per (kernel, GE):")
    for key in sorted(worst, key=lambda k: (k[0], k[1] or 0)):
        print("  %-6s GE=%-4s %.3f  (%s)" % (key[0], key[1], worst[key][0], worst[key][1]))


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the shared case arrays are read-only


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Carved:
    """``nbytes`` bytes as a ``dtype`` tensor in the middle of a buffer filled with ``poison``, GUARD bytes on both sides;
    ``offset`` moves the view off the allocator's alignment"""

    def __init__(self, nbytes, dtype, poison, offset=0):
        self.base = torch.full((GUARD + offset + nbytes + GUARD,), poison, dtype=torch.uint8, device="cuda")
        self.lo, self.hi, self.poison = GUARD + offset, GUARD + offset + nbytes, poison
        self.t = self.base[self.lo:self.hi].view(dtype)
        assert self.base.data_ptr() % 256 == 0 and self.t.data_ptr() % 16 == offset % 16

    @property
    def ptr(self):
        return C.c_void_p(self.t.data_ptr())

    def assert_guards(self, what):
        torch.cuda.synchronize()
        for side, band in (("before", self.base[:self.lo]), ("after", self.base[self.hi:])):
            bad = (band != self.poison).nonzero()
            assert bad.numel() == 0, "%s: guard %s the buffer damaged at byte %d" % (what, side, int(bad[0]))


def raw_plan(lib, ids_t, n, V, poison):
    """rec_dedup_plan_i64 into carved buffers -> (status, {uniq, seg, perm, nu} as numpy)"""
    wsb = lib.rec_dedup_workspace_bytes(n)
    bufs = {"uniq": Carved(8 * max(n, 1), torch.int64, poison), "seg": Carved(4 * (n + 1), torch.int32, poison),
            "perm": Carved(4 * max(n, 1), torch.int32, poison), "nu": Carved(8, torch.int64, poison),
            "ws": Carved(wsb, torch.uint8, poison)}
    rc = lib.rec_dedup_plan_i64(C.c_void_p(ids_t.data_ptr()), n, V, bufs["uniq"].ptr, bufs["seg"].ptr,
                                bufs["perm"].ptr, bufs["nu"].ptr, bufs["ws"].ptr, wsb, stream())
    for name, b in bufs.items():
        b.assert_guards("rec_dedup_plan_i64 %s" % name)
    return rc, {k: b.t.cpu().numpy() for k, b in bufs.items() if k != "ws"}


def check_plan(R, lib, ids, V):
    n = ids.size
    ids_t = dev(ids)
    uniq, seg, perm = DR.host_plan(ids)
    nu = uniq.size
    got = []
    for poison in POISONS:
        rc, p = raw_plan(lib, ids_t, n, V, poison)
        assert rc == 0
        got.append(p)
        assert int(p["nu"][0]) == nu
        assert np.array_equal(p["uniq"][:nu], uniq)
        assert np.array_equal(p["perm"], perm.astype(np.int32))                # stable: numpy's own stable order
        assert np.array_equal(p["seg"][:nu + 1], seg.astype(np.int32))
        assert np.all(p["uniq"][nu:] == uniq[0]) and np.all(p["seg"][nu:] == n)     # the padded tail
    plan = R.ops.DedupPlan(ids_t, V)
    for k, t in (("uniq", plan.uniq_ids), ("seg", plan.seg_start), ("perm", plan.perm), ("nu", plan.n_uniq)):
        assert np.array_equal(got[0][k], got[1][k]), k                          # two plans of the same ids
        assert np.array_equal(got[0][k], t.cpu().numpy()), k
    return plan


@pytest.mark.parametrize("name", [c.name for c in DR.SORT_CASES])
def test_plan_on_every_sort_class_and_tile_edge(R, lib, name):
    c = DR.SORT_BY_NAME[name]
    print(name, DR.sort_class(c.V))
    check_plan(R, lib, DR.sort_ids(name), c.V)


@pytest.mark.parametrize("plan,V,layout,seed", DR.distinct_plans())
def test_plan_of_every_list_of_ids_the_sums_use(R, lib, plan, V, layout, seed):
    p = check_plan(R, lib, DR.plan_ids(plan, V, layout, seed), V)
    assert DR.run_regimes(p.seg_start.cpu().numpy(), p.n, 4) >= DR.PLAN_CLAIMS[plan]    # read off the device's plan


def test_plan_status_codes(lib, limits):
    ids_t = dev(np.array([3, 1, 3], np.int64))
    for V, want in (((1 << 32) + 1, "REC_E_UNSUPPORTED"), (0, "REC_E_ARG"), (-5, "REC_E_ARG")):
        rc, p = raw_plan(lib, ids_t, 3, V, 0xFF)
        assert rc == limits[want], (V, rc)
        assert np.all(p["perm"] == -1) and np.all(p["seg"] == -1) and p["nu"][0] == -1       # nothing was written
    rc, p = raw_plan(lib, ids_t, 0, 10, 0xFF)
    assert rc == 0 and p["nu"][0] == 0 and p["seg"][0] == 0
    rc, p = raw_plan(lib, ids_t, 3, 1 << 32, 0xFF)
    assert rc == 0 and p["nu"][0] == 2 and p["perm"].tolist() == [1, 0, 2]


# ---- sums -------------------------------------------------------------------------------------------------------------
_plans = {}


def device_plan(R, case):
    """the DedupPlan of a case's ids (test_plan_of_every_list_of_ids_the_sums_use holds such plans to numpy)"""
    key = (case.plan, case.V, case.layout, case.seed)
    if key not in _plans:
        if len(_plans) > 16:
            _plans.clear()
        _plans[key] = R.ops.DedupPlan(dev(DR.case_ids(case)), case.V)
    return _plans[key]


def raw_sum(lib, vals, E, plan, row_div, aligned, poison, what):
    """rec_segment_sum_f32 with vals, out and the workspace carved out of poisoned buffers, all three 16-byte aligned or
    all three 4 bytes past it -> out [n, E] on the host"""
    off = 0 if aligned else 4
    n = plan.n
    v = Carved(vals.nbytes, torch.float32, poison, off)
    v.t.copy_(torch.from_numpy(vals.reshape(-1)))
    wsb = lib.rec_segment_sum_workspace_bytes(n, E)
    assert wsb % 4 == 0
    out, ws = Carved(4 * n * E, torch.float32, poison, off), Carved(wsb, torch.float32, poison, off)
    rc = lib.rec_segment_sum_f32(v.ptr, E, C.c_void_p(plan.perm.data_ptr()), C.c_void_p(plan.seg_start.data_ptr()), n,
                                 row_div, out.ptr, ws.ptr, stream())
    assert rc == 0
    for name, b in (("vals", v), ("out", out), ("workspace", ws)):
        b.assert_guards("%s: %s" % (what, name))
    assert torch.equal(v.t.cpu(), torch.from_numpy(vals.reshape(-1)))
    return out.t.cpu().numpy().reshape(n, E)


def both_poisons(lib, vals, E, plan, row_div, aligned, what):
    a, b = (raw_sum(lib, vals, E, plan, row_div, aligned, p, what) for p in POISONS)
    assert np.all(np.isfinite(a)), "%s: out holds a float no kernel wrote (or one made of such)" % what
    assert a.tobytes() == b.tobytes(), "%s: out depends on what the buffers held before the call" % what
    return a


@pytest.mark.parametrize("name", [c.name for c in DR.SUM_CASES])
def test_integer_sums_are_exact_on_every_class(R, lib, name):
    c = DR.SUM_BY_NAME[name]
    print(name, DR.sum_class(c.E, c.aligned), sorted(DR.run_regimes(DR.plan_seg(c.plan), DR.plan_n(c.plan), c.E, c.aligned)))
    plan = device_plan(R, c)
    uniq, exact = DR.reference(name, "int")
    nu = uniq.size
    assert int(plan.n_uniq.item()) == nu
    vals = DR.int_vals(DR.case_rows(c), c.E, c.seed)
    out = both_poisons(lib, vals, c.E, plan, c.row_div, c.aligned, name)
    wrong = np.nonzero(np.any(out[:nu] != exact, axis=1))[0]
    assert wrong.size == 0, "%s: %d rows differ from the exact sums, the first: slot %d of %d, run length %d" % (
        name, wrong.size, wrong[0], nu, DR.PLANS[c.plan][wrong[0]])
    assert np.all(out[nu:] == 0)
    if c.aligned:                                                   # the operator the layers call: the same kernels
        for wide in ((False, True) if c.E > 256 else (False,)):
            got = plan.segment_sum(dev(vals), c.E, c.row_div, wide=wide).cpu().numpy()
            assert got.shape == out.shape and np.array_equal(got[:nu], exact) and np.all(got[nu:] == 0), wide


@pytest.mark.parametrize("name", [c.name for c in DR.SUM_CASES])
def test_normal_sums_against_fp64_on_every_class(R, lib, ratios, name):
    c = DR.SUM_BY_NAME[name]
    plan = device_plan(R, c)
    uniq, ref = DR.reference(name, "normal")
    nu = uniq.size
    vals = DR.normal_vals(DR.case_rows(c), c.E, c.seed)
    out = both_poisons(lib, vals, c.E, plan, c.row_div, c.aligned, name)
    err, bound = float(np.abs(out[:nu] - ref).max()), DR.tolerance(c, ref)
    print("%s %s GE=%s err %.3e bound %.3e ratio %.3f" % (name, c.kernel, c.GE, err, bound, err / bound))
    key = (c.kernel, c.GE)
    if key not in ratios or err / bound > ratios[key][0]:
        ratios[key] = (err / bound, name)
    assert err <= bound, (err, bound)
    assert np.all(out[nu:] == 0)
    again = raw_sum(lib, vals, c.E, plan, c.row_div, c.aligned, 0xFF, name)
    assert out.tobytes() == again.tobytes()                         # run to run
    if c.aligned:
        got = plan.segment_sum(dev(vals), c.E, c.row_div, wide=c.E > 256).cpu().numpy()
        assert got.tobytes() == out.tobytes()


@pytest.mark.parametrize("E", [E for E in DR.E_VALUES if E % 4 == 0 and E <= 256])
@pytest.mark.parametrize("plan", DR.NO_LONG_RUN)
def test_scalar_path_equals_vec_path_bit_for_bit_without_long_runs(R, lib, E, plan):
    """both add the rows of a run one after the other in sorted order"""
    c = DR.SUM_BY_NAME["e%d_al_%s" % (E, plan)]
    assert DR.sum_class(E, True).kernel == "vec" and DR.sum_class(E, False).kernel == "scalar"
    p = device_plan(R, c)
    vals = DR.normal_vals(DR.case_rows(c), E, c.seed)
    vec = raw_sum(lib, vals, E, p, 1, True, 0xFF, c.name)
    scalar = raw_sum(lib, vals, E, p, 1, False, 0xFF, c.name)
    assert vec.tobytes() == scalar.tobytes()


def test_segment_sum_status_codes(lib, limits):
    one = torch.zeros(4, device="cuda")
    i32 = torch.zeros(4, dtype=torch.int32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    for E, n, row_div in ((0, 1, 1), (4, -1, 1), (4, 1, 0)):
        assert lib.rec_segment_sum_f32(p(one), E, p(i32), p(i32), n, row_div, p(one), p(one), stream()) == limits[
            "REC_E_ARG"]
    assert lib.rec_segment_sum_f32(None, 4, None, None, 0, 1, None, None, stream()) == 0        # n = 0: nothing to do
    assert lib.rec_segment_sum_workspace_bytes(0, 4) == 256
    for n, E in ((1, 1), (256, 4), (257, 4), (8192, 256)):
        assert lib.rec_segment_sum_workspace_bytes(n, E) == 4 * (-(-n // DR.CH)) * 2 * E + 256
