"""The embedding lookups (csrc/embedding.hip: rec_emb_gather_f32, rec_emb_gather_lists_f32, rec_emb_fm_fwd_f32,
rec_emb_fm_bwd_vals_f32) on every kernel class their four dispatchers can pick, against numpy.

tests/lookup_classes_ref.py holds the restatement of the dispatch (gather_class, lists_class, fm_fwd_class,
fm_bwd_class), the regimes inside a forward kernel (fm_fwd_regimes) and the tables FM_FWD_CASES / GATHER_CASES /
LISTS_CASES / FM_BWD_CASES; tests/test_lookup_classes_host.py proves on the CPU that the tables reach all 27
emb_fm_fwd_vec_kernel<LPR, SPLIT, FUSED> and all 9 emb_fm_fwd_gen_kernel<GW, NACC> instantiations, every regime, every
gather and list-gather width and both backward classes, and that the integer-valued cases cannot round.  Here:

  forward   rows bit-equal to embed[X]; integer values: z and sumvec bit-equal to the int64 evaluation; normal values:
            the fp64 oracle.layers_np.fm_forward under the suite's own bounds (1e-5 max(1, |z|max), 1e-5 on prob,
            1e-5 max(1, |S|max)); z alone (every other output null) bit-equal to z with every output; the fused and the
            separate class of the same data; per instantiation -1, V, 2^31 + 5 and 2^32 + 3 among the ids: flag 1 and the
            outputs of a zero row, the clean ids leave the flag at 0;
  gather    out bit-equal to table[idx] on rows<1..64>, vec4 and scalar, the same bad ids as zero rows with flag 1 in
            every class, the 4-byte-misaligned tables and outputs bit-equal to the aligned ones;
  lists     used slots bit-equal to the table rows, unused slots still poison bit for bit although each holds an id
            out of range, flag 0 until a used slot holds one, REC_E_UNSUPPORTED for E = 6 and a misaligned table;
  backward  integer values bit-equal to the int64 evaluation in both classes, normal values within the suite's
            2e-6 max(1, |ref|max) of fp64, table mode with ids out of range equal to rows mode with zero rows, the vec
            and the scalar class of the same integer data bit-equal;
  buffers   every call goes through ctypes with every output carved out of a poisoned buffer between two guard bands
            of tests/guarded.GUARD bytes, once under poison 0xFF and once under 0x7F: the guards hold, every float of an
            output is finite under the first and the outputs are bit-equal under both (which is also the run-to-run
            identity).  The padding columns of every strided table hold NaN.

Worst measured |got - ref| / bound of the normal values per class, MI355X (the larger of z, prob and sumvec; the module
prints the table at the end of a run with -s):
  forward, emb_fm_fwd_vec_kernel<LPR, SPLIT, FUSED>           separate tables            fused rows
    LPR   SPLIT = 1    SPLIT = 2    SPLIT = 4               LPR   SPLIT = 1    SPLIT = 2    SPLIT = 4
    1     0.018        0.016        0.037 (F = 240)
    2     0.017        0.016        0.008                   2     0.013        0.012        0.010
    4     0.019        0.015        0.051 (F = 70)          4     0.012        0.020        0.011
    8     0.019        0.013        0.009                   8     0.014        0.014        0.031 (F = 70)
    16    0.010        0.009        0.035 (F = 70)          16    0.011        0.011        0.014
  forward, emb_fm_fwd_gen_kernel<GW, NACC>
    <1,1> 0.010   <2,1> 0.010   <4,1> 0.118 (F = 241)   <8,1> 0.018   <16,1> 0.060   <32,1> 0.007   <64,1> 0.009
    <64,2> 0.014  <64,4> 0.009
  backward values     vec, rows 0.062    vec, table 0.059    scalar, rows 0.064    scalar, table 0.061
The worst forward figure is prob of gen_e4_b10_f241 (241 fields added one after the other); the backward values are
three roundings of numbers of size |ref|max under a bound of 2e-6.  No case failed on the way: embedding.hip is unchanged.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guarded
from tests import lookup_classes_ref as LR

pytestmark = pytest.mark.gpu
GUARD = guarded.GUARD
POISONS = (guarded.POISON_NAN, guarded.POISON_FINITE)


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    import explicit_tf2_recommendation_amd  # noqa: F401
    from explicit_tf2_recommendation_amd._lib import lib
    return lib


@pytest.fixture(scope="module")
def limits(lib):
    from explicit_tf2_recommendation_amd._lib import LIMITS
    return LIMITS


@pytest.fixture(scope="module")
def ratios():
    worst = {}
    yield worst
    print("\nworst |got - ref| / bound of the normal values per class:")
    for key in sorted(worst, key=str):
        print("  %-28s %.3f  (%s)" % (" ".join(str(k) for k in key), worst[key][0], worst[key][1]))


def note(ratios, key, ratio, name):
    if key not in ratios or ratio > ratios[key][0]:
        ratios[key] = (ratio, name)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the shared case arrays are read-only


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Carved:
    """``nbytes`` bytes as a ``dtype`` tensor in the middle of a buffer filled with ``poison``, GUARD bytes on both sides;
    ``offset`` moves the view off the allocator's alignment; ``data`` (numpy) is copied in"""

    def __init__(self, nbytes, dtype, poison, offset=0, data=None):
        self.base = torch.full((GUARD + offset + nbytes + GUARD,), poison, dtype=torch.uint8, device="cuda")
        self.lo, self.hi, self.poison = GUARD + offset, GUARD + offset + nbytes, poison
        self.t = self.base[self.lo:self.hi].view(dtype)
        assert self.base.data_ptr() % 256 == 0 and self.t.data_ptr() % 16 == offset % 16
        if data is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1)))

    @property
    def ptr(self):
        return self.t.data_ptr() if self.t.numel() else self.base.data_ptr() + self.lo

    def host(self):
        return self.t.cpu().numpy()

    def assert_guards(self, what):
        torch.cuda.synchronize()
        for side, band in (("before", self.base[:self.lo]), ("after", self.base[self.hi:])):
            bad = (band != self.poison).nonzero()
            assert bad.numel() == 0, "%s: guard %s the buffer damaged at byte %d" % (what, side, int(bad[0]))


def flag_of(poison):
    f = Carved(4, torch.int32, poison)
    f.t.zero_()
    return f


class Table:
    """vals [V, E] as the leading columns of a [V, ld] device table whose other columns hold NaN (``col`` [V]: column E
    instead), ``off`` floats past a 256-byte boundary"""

    def __init__(self, vals, ld, off=0, col=None):
        V, E = vals.shape
        self.flat = torch.full((off + V * ld + 4,), float("nan"), dtype=torch.float32, device="cuda")
        self.t = self.flat[off:off + V * ld].view(V, ld)
        self.t[:, :E] = dev(vals)
        if col is not None:
            self.t[:, E] = dev(col)
        assert self.flat.data_ptr() % 256 == 0
        self.ptr, self.ld = self.t.data_ptr(), ld


# ---- forward --------------------------------------------------------------------------------------------------------
class FwdTables:
    def __init__(self, c, p, separate=False):
        """the tables of a case in its own layout, or (``separate``) as two dense aligned tables"""
        self.bias = dev(p["bias"])
        if separate:
            self.e, self.w = Table(p["embed"], c.E), Table(p["w"], 1)
            self.w_ptr, self.ld_w = self.w.ptr, 1
        elif c.fused:
            self.e = Table(p["embed"], c.ld, 0, p["w"][:, 0])
            self.w_ptr, self.ld_w = self.e.ptr + 4 * c.E, c.ld
        else:
            self.e, self.w = Table(p["embed"], c.ld, 0 if c.aligned else 1), Table(p["w"], 1)
            self.w_ptr, self.ld_w = self.w.ptr, 1


def run_fwd(lib, c, tabs, X_t, poison, z_only=False):
    """rec_emb_fm_fwd_f32 into carved outputs -> {"z", "prob", "rows", "S", "flag"} on the host (z_only: z and flag)"""
    B, F, E = c.B, c.F, c.E
    bufs = {"z": Carved(4 * B, torch.float32, poison), "flag": flag_of(poison)}
    if not z_only:
        bufs.update(prob=Carved(4 * B, torch.float32, poison), rows=Carved(4 * B * F * E, torch.float32, poison),
                    S=Carved(4 * B * E, torch.float32, poison))
    ptr = lambda k: bufs[k].ptr if k in bufs else None
    rc = lib.rec_emb_fm_fwd_f32(tabs.e.ptr, tabs.e.ld, tabs.w_ptr, tabs.ld_w, tabs.bias.data_ptr(), c.V, E,
                                X_t.data_ptr(), B, F, ptr("z"), ptr("prob"), ptr("rows"), ptr("S"), ptr("flag"), stream())
    assert rc == 0, rc
    for k, b in bufs.items():
        b.assert_guards("%s: %s" % (c.name, k))
    out = {k: b.host() for k, b in bufs.items()}
    if not z_only:
        out["rows"], out["S"] = out["rows"].reshape(B, F, E), out["S"].reshape(B, E)
    return out


def fwd_both_poisons(lib, c, tabs, X_t):
    """every output under both poisons (two runs: bit-equal), then z alone"""
    a, b = (run_fwd(lib, c, tabs, X_t, p) for p in POISONS)
    for k in ("z", "prob", "rows", "S"):
        assert np.all(np.isfinite(a[k])), "%s: %s holds a float no kernel wrote (or one made of such)" % (c.name, k)
        assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs between two runs / two poisons" % (c.name, k)
    assert a["flag"][0] == b["flag"][0]
    alone = run_fwd(lib, c, tabs, X_t, guarded.POISON_NAN, z_only=True)
    assert alone["z"].tobytes() == a["z"].tobytes(), "%s: z alone differs from z with every output" % c.name
    assert alone["flag"][0] == a["flag"][0]
    return a


def check_exact(c, got, ref, what=""):
    assert np.array_equal(got["rows"], ref["rows"]), "%s%s: rows differ from embed[X]" % (c.name, what)
    wrong = np.nonzero(got["z"] != ref["z"])[0]
    assert wrong.size == 0, "%s%s: z of %d examples differs from the exact value, the first: example %d, %r != %r" % (
        c.name, what, wrong.size, wrong[0], got["z"][wrong[0]], ref["z"][wrong[0]])
    assert np.array_equal(got["S"], ref["S"]), "%s%s: sumvec differs from the exact sums" % (c.name, what)


def check_close(c, got, ref, ratios=None):
    assert np.array_equal(got["rows"], ref["rows"]), "%s: rows differ from embed[X]" % c.name
    bound = LR.fwd_bounds(ref)
    for k in ("z", "prob", "S"):
        err = float(np.abs(got[k] - ref[k]).max())
        print("%s %s %s err %.3e bound %.3e ratio %.3f" % (c.name, LR.class_key(c), k, err, bound[k], err / bound[k]))
        if ratios is not None:
            note(ratios, ("fwd",) + LR.class_key(c) + (k,), err / bound[k], c.name)
        assert err <= bound[k], (c.name, k, err, bound[k])


FWD_NAMES = [c.name for c in LR.FM_FWD_CASES]


@pytest.mark.parametrize("name", FWD_NAMES)
def test_forward_integer_values_are_exact_on_every_class(lib, name):
    c = LR.FWD_BY_NAME[name]
    print(name, LR.case_class(c), sorted(LR.case_regimes(c)))
    tabs = FwdTables(c, LR.fwd_params(name, "int"))
    got = fwd_both_poisons(lib, c, tabs, dev(LR.fwd_X(name)))
    check_exact(c, got, LR.fwd_reference(name, "int"))
    assert got["flag"][0] == 0


@pytest.mark.parametrize("name", FWD_NAMES)
def test_forward_normal_values_against_fp64_on_every_class(lib, ratios, name):
    c = LR.FWD_BY_NAME[name]
    tabs = FwdTables(c, LR.fwd_params(name, "normal"))
    got = fwd_both_poisons(lib, c, tabs, dev(LR.fwd_X(name)))
    check_close(c, got, LR.fwd_reference(name, "normal"), ratios)
    assert got["flag"][0] == 0


@pytest.mark.parametrize("name", [c.name for c in LR.FM_FWD_CASES if c.fused and c.B * c.F <= 1000])
def test_fused_class_and_separate_class_of_the_same_data(lib, name):
    c = LR.FWD_BY_NAME[name]
    sep = c._replace(ld=c.E, fused=False)
    assert LR.case_class(c).fused in (True, False) and not LR.case_class(sep).fused
    X_t = dev(LR.fwd_X(name))
    for kind, check in (("int", check_exact), ("normal", check_close)):
        p, ref = LR.fwd_params(name, kind), LR.fwd_reference(name, kind)
        a = run_fwd(lib, c, FwdTables(c, p), X_t, guarded.POISON_NAN)
        b = run_fwd(lib, sep, FwdTables(c, p, separate=True), X_t, guarded.POISON_NAN)
        assert a["rows"].tobytes() == b["rows"].tobytes()
        check(c, a, ref)
        check(c, b, ref)


@pytest.mark.parametrize("name", LR.oob_cases())
def test_forward_ids_out_of_range_raise_the_flag_and_read_a_zero_row(lib, name):
    c = LR.FWD_BY_NAME[name]
    tabs = FwdTables(c, LR.fwd_params(name, "int"))
    X = LR.fwd_X(name, True)
    got = fwd_both_poisons(lib, c, tabs, dev(X))
    assert got["flag"][0] == 1
    check_exact(c, got, LR.fwd_reference(name, "int", True), " (ids out of range)")
    clean = run_fwd(lib, c, tabs, dev(LR.fwd_X(name)), guarded.POISON_NAN, z_only=True)
    assert clean["flag"][0] == 0
    for bad in (X[0, 0], X[0, 1], X[-1, -2], X[-1, -1]):          # each of the four alone
        Xo = np.array(LR.fwd_X(name))
        Xo[-1, -1] = bad
        assert run_fwd(lib, c, tabs, dev(Xo), guarded.POISON_NAN, z_only=True)["flag"][0] == 1, bad


def test_forward_status_codes(lib, limits):
    t, i = torch.zeros(4096, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")
    z = Carved(16, torch.float32, 0xFF)
    p = t.data_ptr()

    def call(embed=p, ld_e=4, w=p, ld_w=1, bias=p, V=10, E=4, idx=i.data_ptr(), B=4, F=2):
        return lib.rec_emb_fm_fwd_f32(embed, ld_e, w, ld_w, bias, V, E, idx, B, F, z.ptr, None, None, None, None,
                                      stream())

    ARG, UNS = limits["REC_E_ARG"], limits["REC_E_UNSUPPORTED"]
    assert call(E=257, ld_e=260) == UNS and call(E=260, ld_e=260) == UNS
    assert call(ld_e=3) == ARG and call(ld_w=0) == ARG and call(V=0) == ARG and call(E=0) == ARG
    assert call(F=0) == ARG and call(B=-1) == ARG
    for null in ("embed", "w", "bias", "idx"):
        assert call(**{null: None}) == ARG, null
    assert call(V=1 << 31) == UNS
    assert call(B=0, embed=None, w=None, bias=None, idx=None) == 0
    z.assert_guards("status codes")
    assert np.all(z.t.view(torch.uint8).cpu().numpy() == 0xFF)          # none of them wrote anything
    assert call() == 0 and np.all(z.host() == 0)


# ---- gather ---------------------------------------------------------------------------------------------------------
def run_gather(lib, c, table, idx, poison):
    out, flag = Carved(4 * c.n * c.E, torch.float32, poison, c.out_off), flag_of(poison)
    idx_t = dev(idx)
    rc = lib.rec_emb_gather_f32(table.ptr, c.V, c.E, c.ld, idx_t.data_ptr(), c.n, out.ptr, flag.ptr, stream())
    assert rc == 0, rc
    out.assert_guards("%s: out" % c.name)
    flag.assert_guards("%s: flag" % c.name)
    return out.host().reshape(c.n, c.E), int(flag.host()[0])


def gather_both_poisons(lib, c, vals, idx):
    table = Table(vals, c.ld, c.table_off // 4)
    assert table.ptr % 16 == c.table_off
    (a, fa), (b, fb) = (run_gather(lib, c, table, idx, p) for p in POISONS)
    assert np.all(np.isfinite(a)), "%s: out holds a float no kernel wrote" % c.name
    assert a.tobytes() == b.tobytes() and fa == fb
    return a, fa


@pytest.mark.parametrize("name", [c.name for c in LR.GATHER_CASES])
def test_gather_is_bit_equal_on_every_class(lib, name):
    c = LR.GATHER_BY_NAME[name]
    print(name, LR.gather_class(c.E, c.ld, not c.table_off, not c.out_off), c.regime)
    vals, idx = LR.table_vals(c.V, c.E, c.seed), LR.gather_ids(c)
    out, flag = gather_both_poisons(lib, c, vals, idx)
    assert out.tobytes() == vals[idx].tobytes() and flag == 0
    if c.n >= 8:                                                   # the same bad ids in every class: zero rows, flag 1
        bad = LR.gather_ids(c, True)
        out, flag = gather_both_poisons(lib, c, vals, bad)
        assert out.tobytes() == LR.gather_reference(vals, bad).tobytes() and flag == 1
        assert np.all(out[[0, c.n // 3, c.n // 2, c.n - 1]] == 0)


@pytest.mark.parametrize("n", [1, 256, 259])
def test_gather_misaligned_results_equal_the_aligned_one(lib, n):
    al = LR.GATHER_BY_NAME["e16_n1"]._replace(n=n)
    vals, idx = LR.table_vals(al.V, 16, 99), LR.gather_ids(al, n >= 8)
    want, flag = gather_both_poisons(lib, al, vals, idx)
    assert LR.gather_class(16, 16).kernel == "rows"
    for other in ("e16_tmis_n%d" % n, "e16_omis_n%d" % n, "e16_ld17_n%d" % n):
        c = LR.GATHER_BY_NAME[other]
        assert c.kernel == "scalar"
        got, f = gather_both_poisons(lib, c, vals, idx)
        assert got.tobytes() == want.tobytes() and f == flag, other


def test_gather_status_codes(lib, limits):
    t, i = torch.zeros(1024, device="cuda"), torch.zeros(8, dtype=torch.int64, device="cuda")
    out = Carved(4 * 8 * 4, torch.float32, 0xFF)

    def call(table=t.data_ptr(), V=10, E=4, ld=4, idx=i.data_ptr(), n=8, o=out.ptr):
        return lib.rec_emb_gather_f32(table, V, E, ld, idx, n, o, None, stream())

    ARG = limits["REC_E_ARG"]
    assert call(ld=3) == ARG and call(E=0) == ARG and call(V=0) == ARG and call(n=-1) == ARG
    assert call(table=None) == ARG and call(idx=None) == ARG and call(o=None) == ARG
    assert call(n=0, table=None, idx=None, o=None) == 0
    out.assert_guards("status codes")
    assert np.all(out.t.view(torch.uint8).cpu().numpy() == 0xFF)
    assert call() == 0 and np.all(out.host() == 0)


# ---- list gather ----------------------------------------------------------------------------------------------------
def run_lists(lib, c, table, msg, poison):
    n = c.n_lists * c.cap
    out, flag = Carved(4 * n * c.E, torch.float32, poison), flag_of(poison)
    msg_t = dev(msg)
    rc = lib.rec_emb_gather_lists_f32(table.ptr, c.V, c.E, c.ld, msg_t.data_ptr(), c.n_lists, c.cap, out.ptr, flag.ptr,
                                      stream())
    assert rc == 0, rc
    out.assert_guards("%s: out" % c.name)
    flag.assert_guards("%s: flag" % c.name)
    return out.t.view(torch.uint8).cpu().numpy().reshape(n, 4 * c.E), int(flag.host()[0])


@pytest.mark.parametrize("name", [c.name for c in LR.LISTS_CASES])
def test_list_gather_writes_the_used_slots_alone(lib, name):
    c = LR.LISTS_BY_NAME[name]
    print(name, LR.lists_class(c.E, c.ld), c.counts)
    vals, used = LR.table_vals(c.V, c.E, c.seed), LR.lists_used(c)
    table = Table(vals, c.ld)
    for bad_slot in ((False, True) if used.any() else (False,)):
        msg = LR.lists_msg(c, bad_slot)
        ids = msg[:, LR.TH.HDR:].reshape(-1)
        want = LR.gather_reference(vals, ids[used]).view(np.uint8).reshape(-1, 4 * c.E)
        for poison in POISONS:
            out, flag = run_lists(lib, c, table, msg, poison)
            assert np.array_equal(out[used], want), "%s: a used slot differs from its table row" % name
            assert np.all(out[~used] == poison), "%s: an unused slot was written" % name
            assert flag == int(bad_slot)          # every unused slot holds an id out of range: that raises nothing


def test_list_gather_status_codes(lib, limits):
    t, m = torch.zeros(4096, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")
    out = Carved(4 * 4 * 256, torch.float32, 0xFF)

    def call(table=t.data_ptr(), V=10, E=8, ld=8, msg=m.data_ptr(), n_lists=2, cap=2, o=out.ptr):
        return lib.rec_emb_gather_lists_f32(table, V, E, ld, msg, n_lists, cap, o, None, stream())

    ARG, UNS = limits["REC_E_ARG"], limits["REC_E_UNSUPPORTED"]
    assert call(E=6) == UNS and call(E=6, ld=6) == UNS and call(table=t.data_ptr() + 4) == UNS
    assert call(o=out.ptr + 4) == UNS and call(ld=9, E=8) == UNS and call(E=260, ld=260) == UNS and call(E=2) == UNS
    assert call(ld=7) == ARG and call(E=0) == ARG and call(V=0) == ARG and call(n_lists=0) == ARG and call(cap=0) == ARG
    assert call(table=None) == ARG and call(msg=None) == ARG and call(o=None) == ARG
    out.assert_guards("status codes")
    assert np.all(out.t.view(torch.uint8).cpu().numpy() == 0xFF)
    assert call() == 0                                              # counts of 0: nothing is written
    assert np.all(out.t.view(torch.uint8).cpu().numpy() == 0xFF)


# ---- backward values ------------------------------------------------------------------------------------------------
def run_bwd(lib, c, inp, poison, rows=None, aligned=None):
    """rec_emb_fm_bwd_vals_f32 with sumvec, rows, extra and dvals carved, all aligned or all 4 bytes off (and the table
    with them); ``rows`` [B F, E] replaces embed[X] of rows mode"""
    aligned = c.aligned if aligned is None else aligned
    off = 0 if aligned else 4
    n = c.B * c.F
    table = Table(inp["embed"], c.ld, off // 4)
    S = Carved(4 * c.B * c.E, torch.float32, poison, off, inp["S"])
    bufs = {"S": S, "dvals": Carved(4 * n * c.E, torch.float32, poison, off)}
    if c.rows_given:
        ez, Xz = LR.with_zero_row(inp["embed"], inp["X"])
        bufs["rows"] = Carved(4 * n * c.E, torch.float32, poison, off, ez[Xz] if rows is None else rows)
    if c.extra:
        bufs["extra"] = Carved(4 * n * c.E, torch.float32, poison, off, inp["extra"])
    ptr = lambda k: bufs[k].ptr if k in bufs else None
    X_t, gz_t = dev(inp["X"]), dev(inp["gz"])                      # named: they live until the guards are read
    rc = lib.rec_emb_fm_bwd_vals_f32(table.ptr, c.ld, c.V, c.E, X_t.data_ptr(), c.B, c.F, gz_t.data_ptr(), S.ptr,
                                     ptr("rows"), ptr("extra"), ptr("dvals"), stream())
    assert rc == 0, rc
    for k, b in bufs.items():
        b.assert_guards("%s: %s" % (c.name, k))
    return bufs["dvals"].host().reshape(n, c.E)


def bwd_both_poisons(lib, c, inp, **kw):
    a, b = (run_bwd(lib, c, inp, p, **kw) for p in POISONS)
    assert np.all(np.isfinite(a)), "%s: dvals holds a float no kernel wrote" % c.name
    assert a.tobytes() == b.tobytes()
    return a


BWD_NAMES = [c.name for c in LR.FM_BWD_CASES]


@pytest.mark.parametrize("name", BWD_NAMES)
def test_backward_integer_values_are_exact_in_both_classes(lib, name):
    c = LR.BWD_BY_NAME[name]
    print(name, LR.fm_bwd_class(c.E, c.ld, c.rows_given, c.aligned), LR.bwd_units(c))
    inp = LR.bwd_inputs(c, "int")
    got = bwd_both_poisons(lib, c, inp)
    assert np.array_equal(got, inp["ref"]), "%s: %d values differ from the exact ones" % (
        name, int(np.sum(got != inp["ref"])))
    if c.E % 4 == 0:                                               # the other class of the same data: bit-equal
        other = run_bwd(lib, c, inp, guarded.POISON_NAN, aligned=not c.aligned)
        assert LR.fm_bwd_class(c.E, c.ld, c.rows_given, not c.aligned) != c.kernel
        assert other.tobytes() == got.tobytes()


@pytest.mark.parametrize("name", BWD_NAMES)
def test_backward_normal_values_against_fp64_in_both_classes(lib, ratios, name):
    c = LR.BWD_BY_NAME[name]
    inp = LR.bwd_inputs(c, "normal")
    got = bwd_both_poisons(lib, c, inp)
    err, bound = float(np.abs(got - inp["ref"]).max()), LR.bwd_bound(inp["ref"])
    print("%s %s err %.3e bound %.3e ratio %.3f" % (name, c.kernel, err, bound, err / bound))
    note(ratios, ("bwd", c.kernel, "rows" if c.rows_given else "table"), err / bound, name)
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("name", [n for n in BWD_NAMES if "_table_" in n and n.endswith("b37")])
def test_backward_table_mode_out_of_range_equals_rows_mode_with_a_zero_row(lib, name):
    c = LR.BWD_BY_NAME[name]
    for kind in ("int", "normal"):
        inp = LR.bwd_inputs(c, kind, oob=True)
        assert np.sum((inp["X"] < 0) | (inp["X"] >= c.V)) == 2
        from_table = bwd_both_poisons(lib, c, inp)
        from_rows = bwd_both_poisons(lib, c._replace(rows_given=True), inp)
        assert from_table.tobytes() == from_rows.tobytes()
        if kind == "int":
            assert np.array_equal(from_table, inp["ref"])
        else:
            assert np.abs(from_table - inp["ref"]).max() <= LR.bwd_bound(inp["ref"])


def test_backward_status_codes(lib, limits):
    t, i = torch.zeros(4096, device="cuda"), torch.zeros(64, dtype=torch.int64, device="cuda")
    out = Carved(4 * 8 * 4, torch.float32, 0xFF)
    p = t.data_ptr()

    def call(embed=p, ld_e=4, E=4, idx=i.data_ptr(), B=4, F=2, gz=p, S=p, rows=None, dvals=out.ptr):
        return lib.rec_emb_fm_bwd_vals_f32(embed, ld_e, 10, E, idx, B, F, gz, S, rows, None, dvals, stream())

    ARG = limits["REC_E_ARG"]
    assert call(ld_e=3) == ARG and call(E=0) == ARG and call(F=0) == ARG and call(B=-1) == ARG
    assert call(embed=None) == ARG and call(idx=None) == ARG and call(gz=None) == ARG and call(S=None) == ARG
    assert call(dvals=None) == ARG
    assert call(B=0, embed=None, idx=None, gz=None, S=None, dvals=None) == 0
    out.assert_guards("status codes")
    assert np.all(out.t.view(torch.uint8).cpu().numpy() == 0xFF)
    assert call(embed=None, ld_e=0, rows=p) == 0 and call() == 0 and np.all(out.host() == 0)
