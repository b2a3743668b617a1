"""The interaction kernels of csrc/interactions.hip (rec_emb_ipn_*, rec_emb_bi_*, rec_ip_attn_*, rec_ffm_*) on every kernel
class their dispatchers can pick, through the C ABI, against the fp64 references and the derived per-element bounds of
tests/interaction_classes_ref.py.

tests/test_interaction_classes_host.py proves on the CPU that the tables reach every (EX, vec4, partial last group) class of
the PNN forward and backward, every NPL of the attention in both directions, both VEC values of the four other kernels and
the listed regimes, that the bounds leave room for a correct fp32 evaluation and catch eleven wrong kernels.  Here:

  cases       every case of IPN_CASES, BI_CASES, ATTN_CASES and FFM_CASES, forward and backward, inside the bounds; each
              call runs twice from the same inputs and is bit-equal; the backward gets what the forward under test wrote
              (the forward output, sumvec, the scores -- those of padded steps replaced by NaN: they are never read);
  exact       the flatten part of the PNN output is a copy of the rows (zero rows for out-of-range ids); scores, gkeys and
              the pooled row of an all-padded example are exactly 0; g_rows at and beyond n_uniq is exactly 0;
  flags       the oob flag is 1 exactly on the cases that hold an out-of-range id;
  buffers     every input and output is a view inside a buffer of sentinels, nothing outside the view changes, inputs keep
              their bits, padding columns of strided outputs keep their poison (0xFF bytes, tests/guarded.py);
  twins       a vec case run again from the same values as its two fall-backs (ld % 4 != 0, table 4 bytes past a 16-byte
              boundary).  Bit-equal where the summation order is the same: the PNN flatten part and the whole PNN backward
              (it has no vec class), sumvec and vals of the bi-interaction (a lane owns a dim, the fields come in the same
              order, nothing to fuse), the FFM g_rows (a lane owns an element, the segment is walked in plan order).  Not
              the PNN pair products ((x0 y0 + x1 y1) + (x2 y2 + x3 y3) a float4 against a chain), the FFM z (4 products a
              lane item) nor the bi-interaction's out (fma contraction differs between the two instantiations);
  refusals    D = 257, T*C*4 + 16*D > 64 KB, FFM F = 256, a PNN shape beyond the common domain (F = 244), ld < E and
              ld_out < W return REC_E_ARG with every output untouched; ops.ip_attn_fwd / ip_attn_bwd raise ValueError for a
              q that is not [B, C E] and launch nothing; B = 0 is accepted;
  layer       PNNLayer forward + backward at F = 80, E = 64 (the backward needs 66880 bytes of LDS and was refused before)
              against oracle/torch_ref.py in fp64, with every allocation of ops guarded.

Worst measured |got - ref| / bound per class on the MI355X (the module prints the table at the end of a run with -s):
  ipn forward, pairs     EX=1    EX=2    EX=4    EX=8        ipn backward, vals   EX=1    EX=2    EX=4    EX=8
    vec4                 0.124   0.000   0.261   0.413         full groups        0.431   0.249   0.249   0.394
    vec4, partial        -       0.390   0.416   0.393         partial last       -       0.451   0.248   0.392
    scalar               0.332   0.331   0.436   0.539
    scalar, partial      -       0.467   0.413   0.540
  bi forward   vec: out 0.267, sumvec 0.303    scalar: out 0.223, sumvec 0.258      backward vals   vec 0.485   scalar 0.470
  attn         NPL=1   NPL=2   NPL=3   NPL=4                   ffm          vec     scalar
    scores     0.106   0.025   0.009   0.004                     z          0.102   0.038
    pooled     0.109   0.011   0.005   0.005                     prob       0.124   0.083
    gkeys      0.402   0.366   0.321   0.285                     g_rows     0.536   0.439
    gq         0.142   0.010   0.007   0.005
(EX=2 vec4 with full groups is the F = 1 case: it has no pair.)  The short sums sit near half of their bound, which is mostly
the final rounding; the long ones (D terms a score, P*E terms a z) use a few percent of a bound that charges every term the
whole chain.  The flatten part, the zeros of padded steps and of g_rows beyond n_uniq, and the oob flags were exact on every
case, and no case failed: interactions.hip computes what it did, the two argument-check defects aside.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import interaction_classes_ref as IR

pytestmark = pytest.mark.gpu
GUARD = 1024                  # sentinel floats on both sides of every buffer
SENT = -777.25
POISON = np.frombuffer(bytes([G.POISON_NAN] * 4), np.uint32)[0]


@pytest.fixture(scope="module")
def lib():
    assert torch.cuda.is_available()
    import explicit_tf2_recommendation_amd  # noqa: F401
    from explicit_tf2_recommendation_amd._lib import lib
    return lib


@pytest.fixture(scope="module")
def E_ARG(lib):
    from explicit_tf2_recommendation_amd._lib import LIMITS
    return LIMITS["REC_E_ARG"]


@pytest.fixture(scope="module")
def worst():
    table = {}
    yield table
    print("\nworst |got - ref| / bound per class:")
    for key in sorted(table):
        print("  %-34s %s" % (key, "  ".join("%s %.3f" % kv for kv in sorted(table[key].items()))))


def note(worst, key, **q):
    slot = worst.setdefault(key, {})
    for k, v in q.items():
        slot[k] = max(slot.get(k, 0.0), v)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


def poison(shape):
    return np.full(shape, POISON, np.uint32).view(np.float32)


def strided(x, ld):
    """x [R,E] as the leading columns of a [R,ld] array whose other columns hold the poison"""
    full = poison((x.shape[0], ld))
    full[:, :x.shape[1]] = x
    return full


def padding_kept(full, first):
    return bool(np.all(bits(full[:, first:]) == POISON))


class Buf:
    """``data`` (float32, any shape) as a view ``off`` floats past a 256-byte boundary inside a buffer of sentinels"""

    def __init__(self, data, off=0):
        data = np.array(data, np.float32)
        self.shape, n = data.shape, data.size
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.base = torch.full((self.hi + GUARD,), SENT, dtype=torch.float32, device="cuda")
        assert self.base.data_ptr() % 256 == 0
        self.ptr = self.base.data_ptr() + 4 * self.lo
        self.first = data.copy()
        if n:
            self.base[self.lo:self.hi].copy_(torch.from_numpy(data.reshape(-1)))

    def host(self):
        return self.base[self.lo:self.hi].cpu().numpy().reshape(self.shape)

    def settle(self):
        """what the buffer holds now is what a later call must leave alone"""
        self.first = self.host().copy()
        return self.first

    def guards_hold(self):
        return bool((self.base[:self.lo] == SENT).all()) and bool((self.base[self.hi:] == SENT).all())

    def unchanged(self):
        return self.guards_hold() and same_bits(self.host(), self.first)


class Ints:
    """an integer array on the device between two sentinel elements"""

    def __init__(self, data, dtype):
        data = np.asarray(data, dtype).reshape(-1)
        self.n, self.first = data.size, data.copy()
        self.t = torch.from_numpy(np.concatenate([[-99], data, [-99]]).astype(dtype)).cuda()
        self.ptr = self.t.data_ptr() + self.t.element_size()

    def host(self):
        return self.t[1:1 + self.n].cpu().numpy()

    def unchanged(self):
        h = self.t.cpu().numpy()
        return h[0] == -99 and h[-1] == -99 and np.array_equal(h[1:-1], self.first)


def finish(status, bufs, inputs):
    torch.cuda.synchronize()
    for b in bufs:
        assert b.guards_hold(), "written outside a buffer"
    for b in inputs:
        assert b.unchanged(), "an input was written"
    return status


# ---- PNN inner product --------------------------------------------------------------------------------------------------
def ipn_run(lib, table, X, g, ld, off, V=IR.V_IPN):
    """forward into a strided, poisoned output, then the backward on that very output -> (out [B, ld_out], flag, vals)"""
    B, F = X.shape
    E = table.shape[1]
    W = F * E + F * (F - 1) // 2
    ld_out, ld_g = W + 3, W + 5
    tb, Xd, out, flag = Buf(strided(table, ld), off), Ints(X, np.int64), Buf(poison((B, ld_out))), Ints([0], np.int32)
    assert (tb.ptr % 16 == 0) == (off % 4 == 0)
    st = lib.rec_emb_ipn_fwd_f32(tb.ptr, V, E, ld, Xd.ptr, B, F, out.ptr, ld_out, flag.ptr, stream())
    assert finish(st, [out], [tb, Xd]) == 0
    o = out.settle()
    gb, vals = Buf(strided(g, ld_g)), Buf(poison((B * F, E)))
    st = lib.rec_emb_ipn_bwd_vals_f32(out.ptr, ld_out, gb.ptr, ld_g, B, F, E, vals.ptr, stream())
    assert finish(st, [vals], [gb, out]) == 0
    return o, int(flag.host()[0]), vals.host()


@pytest.mark.parametrize("name", [c.name for c in IR.IPN_CASES])
def test_ipn_case(lib, worst, name):
    c, (table, X, g), (f, b) = IR.BY_NAME["ipn", name], IR.ipn_input(name), IR.ipn_reference(name)
    runs = [ipn_run(lib, table, X, g, c.ld, c.off) for _ in range(2)]
    (out, flag, vals), FE = runs[0], c.F * c.E
    assert same_bits(out, runs[1][0]) and same_bits(vals, runs[1][2]), "two runs from the same inputs differ"
    assert flag == runs[1][1] == int(c.oob)
    assert padding_kept(out, out.shape[1] - 3), "a column beyond W was written"
    assert same_bits(out[:, :FE], f.out[:, :FE].astype(np.float32)), "the flatten part is not a copy of the rows"
    qf = IR.ratio(out[:, FE:-3], f.out[:, FE:], f.bound[:, FE:])
    qb = IR.ratio(vals, b.vals, b.bound)
    print("%s: pairs %.3f vals %.3f of the bound" % (name, qf, qb))
    assert qf <= 1 and qb <= 1, (name, qf, qb)
    note(worst, "ipn fwd EX=%d %s%s" % (c.fwd.EX, "vec4" if c.fwd.vec4 else "scalar", " partial" * c.fwd.partial_last),
         pairs=qf)
    note(worst, "ipn bwd EX=%d%s" % (c.bwd.EX, " partial" * c.bwd.partial_last), vals=qb)


def test_ipn_fall_back_twins(lib):
    """ex8_vec_partial's values as the vec4 class and as both fall-backs"""
    table, X, g = IR.ipn_input("ex8_vec_partial")
    FE = X.shape[1] * table.shape[1]
    f, _ = IR.ipn_reference("ex8_vec_partial")
    vec = ipn_run(lib, table, X, g, 4, 0)
    for ld, off in ((5, 0), (4, 1), (8, 2)):
        assert IR.ipn_class(X.shape[0], X.shape[1], 4, ld, off % 4 == 0).vec4 is False
        twin = ipn_run(lib, table, X, g, ld, off)
        assert same_bits(twin[0][:, :FE], vec[0][:, :FE]) and twin[1] == vec[1] == 1
        assert IR.ratio(twin[0][:, FE:-3], f.out[:, FE:], f.bound[:, FE:]) <= 1
        # the backward reads the rows from `out` and has one class: the same bits wherever the rows came from
        assert same_bits(twin[2], vec[2])


# ---- NFM bi-interaction -------------------------------------------------------------------------------------------------
def bi_run(lib, table, X, g, ld, off, off_sum=0, off_vals=0, V=IR.V_BI):
    B, F = X.shape
    E = table.shape[1]
    tb, Xd, flag = Buf(strided(table, ld), off), Ints(X, np.int64), Ints([0], np.int32)
    out, S = Buf(poison((B, E + 3))), Buf(poison((B, E)), off_sum)
    st = lib.rec_emb_bi_fwd_f32(tb.ptr, V, E, ld, Xd.ptr, B, F, out.ptr, E + 3, S.ptr, flag.ptr, stream())
    assert finish(st, [out, S], [tb, Xd]) == 0
    o, s = out.host(), S.settle()
    gb, vals = Buf(strided(g, E + 2)), Buf(poison((B * F, E)), off_vals)
    st = lib.rec_emb_bi_bwd_vals_f32(tb.ptr, V, E, ld, Xd.ptr, B, F, gb.ptr, E + 2, S.ptr, vals.ptr, stream())
    assert finish(st, [vals], [tb, Xd, gb, S]) == 0
    return o, s, int(flag.host()[0]), vals.host()


@pytest.mark.parametrize("name", [c.name for c in IR.BI_CASES])
def test_bi_case(lib, worst, name):
    c, (table, X, g), f = IR.BY_NAME["bi", name], IR.bi_input(name), IR.bi_reference(name)
    runs = [bi_run(lib, table, X, g, c.ld, c.off, c.off_sum, c.off_vals) for _ in range(2)]
    out, S, flag, vals = runs[0]
    assert all(same_bits(a, b) for a, b in zip(runs[0][:2] + runs[0][3:], runs[1][:2] + runs[1][3:]))
    assert flag == runs[1][2] == int(c.oob)
    assert padding_kept(out, c.E), "a column beyond E was written"
    b = IR.ref_bi_bwd(table, X, g, S)
    q = dict(out=IR.ratio(out[:, :c.E], f.out, f.bout), S=IR.ratio(S, f.S, f.bS), vals=IR.ratio(vals, b.vals, b.bound))
    print("%s: %s of the bound" % (name, q))
    assert max(q.values()) <= 1, (name, q)
    note(worst, "bi fwd %s" % ("vec" if c.fwd.vec else "scalar"), out=q["out"], S=q["S"])
    note(worst, "bi bwd %s" % ("vec" if c.bwd.vec else "scalar"), vals=q["vals"])


def test_bi_fall_back_twins(lib):
    """a lane owns a dim and adds the fields in the same order in both classes: sumvec (additions alone) and vals (a
    difference, then a product: nothing to fuse) are bit-equal.  ``out`` is not asserted bit-equal: whether e*e fuses into
    the sum of squares and S*S - Q into one fma is the compiler's choice per instantiation (the two classes differed on the
    MI355X); both stay inside the bound, which holds for either form."""
    table, X, g = IR.bi_input("vec_f9")
    f, E = IR.bi_reference("vec_f9"), table.shape[1]
    vec = bi_run(lib, table, X, g, 8, 0)
    for ld, off, off_sum, off_vals in ((9, 0, 0, 0), (8, 1, 0, 0), (8, 0, 1, 0), (8, 0, 0, 1)):
        twin = bi_run(lib, table, X, g, ld, off, off_sum, off_vals)
        assert same_bits(twin[1], vec[1]), ("sumvec", ld, off, off_sum, off_vals)
        assert same_bits(twin[3], vec[3]), ("vals", ld, off, off_sum, off_vals)
        print("bi twin ld=%d off=%d/%d/%d: out bit-equal to the vec class: %s" % (ld, off, off_sum, off_vals,
                                                                                 same_bits(twin[0], vec[0])))
        assert IR.ratio(twin[0][:, :E], f.out, f.bout) <= 1


# ---- GSU attention ------------------------------------------------------------------------------------------------------
def attn_run(lib, c, table, series, q, gp, V=IR.V_ATTN):
    B, T, Cn = series.shape
    E, D = c.E, c.C * c.E
    tb, sd, qb, flag = Buf(strided(table, c.ld)), Ints(series, np.int64), Buf(strided(q, c.ld_q)), Ints([0], np.int32)
    scores, pooled = Buf(poison((B, T))), Buf(poison((B, c.ld_p)))
    st = lib.rec_ip_attn_fwd_f32(tb.ptr, c.ld, V, E, Cn, sd.ptr, B, T, qb.ptr, c.ld_q, IR.PAD, scores.ptr, pooled.ptr,
                                 c.ld_p, flag.ptr, stream())
    assert finish(st, [scores, pooled], [tb, sd, qb]) == 0
    s, p = scores.host(), pooled.host()
    given = s.copy()
    given[series[:, :, 0] == IR.PAD] = np.nan                # never read
    sb, gpb = Buf(given), Buf(strided(gp, c.ld_gp))
    gkeys, gq = Buf(poison((B, T, D))), Buf(poison((B, D)))
    st = lib.rec_ip_attn_bwd_f32(tb.ptr, c.ld, V, E, Cn, sd.ptr, B, T, qb.ptr, c.ld_q, IR.PAD, sb.ptr, gpb.ptr, c.ld_gp,
                                 gkeys.ptr, gq.ptr, stream())
    assert finish(st, [gkeys, gq], [tb, sd, qb, sb, gpb]) == 0
    return s, p, int(flag.host()[0]), given, gkeys.host(), gq.host()


@pytest.mark.parametrize("name", [c.name for c in IR.ATTN_CASES])
def test_attn_case(lib, worst, name):
    c, (table, series, q, gp), f = IR.BY_NAME["attn", name], IR.attn_input(name), IR.attn_reference(name)
    runs = [attn_run(lib, c, table, series, q, gp) for _ in range(2)]
    s, p, flag, given, gk, gq = runs[0]
    for i in (0, 1, 4, 5):
        assert same_bits(runs[0][i], runs[1][i]), "two runs from the same inputs differ"
    assert flag == runs[1][2] == int(c.oob)
    D, pad = c.C * c.E, ~f.valid
    assert padding_kept(p, D), "a column of pooled beyond D was written"
    assert not s[pad].any() and not gk[pad].any(), "a padded step has a score or a gradient"
    assert not p[pad.all(1), :D].any() and not gq[pad.all(1)].any(), "an all-padded example pools something"
    b = IR.ref_attn_bwd(table, q, series, IR.PAD, given, gp)
    qq = dict(scores=IR.ratio(s, f.scores, f.bs), pooled=IR.ratio(p[:, :D], f.pooled, f.bp),
              gkeys=IR.ratio(gk, b.gkeys, b.bgk), gq=IR.ratio(gq, b.gq, b.bgq))
    print("%s: %s of the bound" % (name, qq))
    assert max(qq.values()) <= 1, (name, qq)
    note(worst, "attn fwd NPL=%d" % c.cls.NPL, scores=qq["scores"], pooled=qq["pooled"])
    note(worst, "attn bwd NPL=%d" % c.cls.NPL, gkeys=qq["gkeys"], gq=qq["gq"])


# ---- FFM ----------------------------------------------------------------------------------------------------------------
def ffm_run(lib, v, w, bias, X, gz, plan, ld_v, off, ld_w, off_rows, V=IR.V_FFM):
    B, F = X.shape
    E = v.shape[2]
    vb, wb = Buf(strided(v.reshape(V, F * E), ld_v), off), Buf(strided(w.reshape(V, 1), ld_w))
    bb, Xd, flag = Buf(bias), Ints(X, np.int64), Ints([0], np.int32)
    z, prob = Buf(poison((B,))), Buf(poison((B,)))
    st = lib.rec_ffm_fwd_f32(vb.ptr, ld_v, wb.ptr, ld_w, bb.ptr, V, E, Xd.ptr, B, F, z.ptr, prob.ptr, flag.ptr, stream())
    assert finish(st, [z, prob], [vb, wb, bb, Xd]) == 0
    perm, seg, nu = plan
    gzb, pd, sd, nd = Buf(gz), Ints(perm, np.int32), Ints(seg, np.int32), Ints([nu], np.int64)
    rows = Buf(poison((B * F, F * E)), off_rows)
    st = lib.rec_ffm_bwd_rows_f32(vb.ptr, ld_v, V, E, Xd.ptr, B, F, gzb.ptr, pd.ptr, sd.ptr, nd.ptr, rows.ptr, stream())
    assert finish(st, [rows], [vb, Xd, gzb, pd, sd, nd]) == 0
    return z.host(), prob.host(), int(flag.host()[0]), rows.host().reshape(B * F, F, E)


@pytest.mark.parametrize("name", [c.name for c in IR.FFM_CASES])
def test_ffm_case(lib, worst, name):
    c, (v, w, bias, X, gz), (f, plan, b) = IR.BY_NAME["ffm", name], IR.ffm_input(name), IR.ffm_reference(name)
    runs = [ffm_run(lib, v, w, bias, X, gz, plan, c.ld_v, c.off, c.ld_w, c.off_rows) for _ in range(2)]
    z, prob, flag, rows = runs[0]
    assert all(same_bits(runs[0][i], runs[1][i]) for i in (0, 1, 3)), "two runs from the same inputs differ"
    assert flag == runs[1][2] == int(c.oob)
    assert not rows[plan[2]:].any(), "g_rows at or beyond n_uniq is not zero"
    q = dict(z=IR.ratio(z, f.z, f.bz), prob=IR.ratio(prob, f.prob, f.bprob), rows=IR.ratio(rows, b.vals, b.bound))
    print("%s: %s of the bound" % (name, q))
    assert max(q.values()) <= 1, (name, q)
    note(worst, "ffm fwd %s" % ("vec" if c.fwd.vec else "scalar"), z=q["z"], prob=q["prob"])
    note(worst, "ffm bwd %s" % ("vec" if c.bwd.vec else "scalar"), rows=q["rows"])


def test_ffm_fall_back_twins(lib):
    """a lane owns an element of g_rows and walks the segment in plan order in both classes: bit-equal; z is not (a vec
    lane adds four products before it adds to its sum) and stays inside its bound"""
    (v, w, bias, X, gz), (f, plan, _) = IR.ffm_input("f26_vec"), IR.ffm_reference("f26_vec")
    FE = v.shape[1] * v.shape[2]
    vec = ffm_run(lib, v, w, bias, X, gz, plan, FE, 0, 1, 0)
    for ld_v, off, off_rows in ((FE + 1, 0, 0), (FE, 1, 0), (FE, 0, 1)):
        twin = ffm_run(lib, v, w, bias, X, gz, plan, ld_v, off, 16, off_rows)
        assert same_bits(twin[3], vec[3]) and twin[2] == vec[2] == 1, (ld_v, off, off_rows)
        assert IR.ratio(twin[0], f.z, f.bz) <= 1


# ---- refusals -------------------------------------------------------------------------------------------------------------
def test_refusals_leave_every_output_alone(lib, E_ARG):
    """the buffers hold what the refused shape would need (or more): a launch that happened anyway would stay inside"""
    s = stream()
    ids, flag = Ints(np.ones(20000, np.int64), np.int64), Ints([0], np.int32)
    tab, outs = Buf(np.ones(40000, np.float32)), [Buf(poison((70000,))) for _ in range(3)]
    a, b, c = (o.ptr for o in outs)
    calls = {
        "attn D = 257": lambda: lib.rec_ip_attn_fwd_f32(tab.ptr, 257, 10, 257, 1, ids.ptr, 2, 4, tab.ptr, 257, 0, a, b, 257,
                                                        flag.ptr, s),
        "attn bwd D = 257": lambda: lib.rec_ip_attn_bwd_f32(tab.ptr, 257, 10, 257, 1, ids.ptr, 2, 4, tab.ptr, 257, 0, a,
                                                            tab.ptr, 257, b, c, s),
        "attn T*C*4 + 16 D > 64 KB": lambda: lib.rec_ip_attn_fwd_f32(tab.ptr, 64, 10, 64, 4, ids.ptr, 1, 3841, tab.ptr, 256,
                                                                     0, a, b, 256, flag.ptr, s),
        "ffm F = 256": lambda: lib.rec_ffm_fwd_f32(tab.ptr, 256, tab.ptr, 1, tab.ptr, 10, 1, ids.ptr, 2, 256, a, b,
                                                   flag.ptr, s),
        "ffm bwd F = 256": lambda: lib.rec_ffm_bwd_rows_f32(tab.ptr, 256, 10, 1, ids.ptr, 1, 256, tab.ptr, ids.ptr, ids.ptr,
                                                            ids.ptr, a, s),
        "ipn F = 244 (the backward would need 241072 bytes)": lambda: lib.rec_emb_ipn_fwd_f32(
            tab.ptr, 10, 1, 1, ids.ptr, 2, 244, a, 29890, flag.ptr, s),
        "ipn bwd F = 244": lambda: lib.rec_emb_ipn_bwd_vals_f32(tab.ptr, 29890, tab.ptr, 29890, 1, 244, 1, a, s),
        "ipn F = 256": lambda: lib.rec_emb_ipn_fwd_f32(tab.ptr, 10, 1, 1, ids.ptr, 1, 256, a, 32896, flag.ptr, s),
        "ipn ld < E": lambda: lib.rec_emb_ipn_fwd_f32(tab.ptr, 10, 8, 7, ids.ptr, 4, 3, a, 27, flag.ptr, s),
        "ipn ld_out < W": lambda: lib.rec_emb_ipn_fwd_f32(tab.ptr, 10, 8, 8, ids.ptr, 4, 3, a, 26, flag.ptr, s),
        "ipn bwd ld_g < W": lambda: lib.rec_emb_ipn_bwd_vals_f32(tab.ptr, 27, tab.ptr, 26, 4, 3, 8, a, s),
        "bi ld < E": lambda: lib.rec_emb_bi_fwd_f32(tab.ptr, 10, 8, 7, ids.ptr, 4, 3, a, 8, b, flag.ptr, s),
        "bi ld_out < E": lambda: lib.rec_emb_bi_fwd_f32(tab.ptr, 10, 8, 8, ids.ptr, 4, 3, a, 7, b, flag.ptr, s),
        "attn ld_q < D": lambda: lib.rec_ip_attn_fwd_f32(tab.ptr, 8, 10, 8, 2, ids.ptr, 2, 4, tab.ptr, 15, 0, a, b, 16,
                                                         flag.ptr, s),
        "attn ld_pooled < D": lambda: lib.rec_ip_attn_fwd_f32(tab.ptr, 8, 10, 8, 2, ids.ptr, 2, 4, tab.ptr, 16, 0, a, b, 15,
                                                              flag.ptr, s),
        "ffm ld_v < F*E": lambda: lib.rec_ffm_fwd_f32(tab.ptr, 23, tab.ptr, 1, tab.ptr, 10, 8, ids.ptr, 2, 3, a, b,
                                                      flag.ptr, s),
    }
    for what, call in calls.items():
        assert finish(call(), outs, [tab, ids, flag] + outs) == E_ARG, what
    # the ops wrappers of the attention refuse a q of the wrong shape themselves: the kernel would read past its end
    from explicit_tf2_recommendation_amd import ops
    B, T, Cn, E = 2, 4, 2, 8
    D = Cn * E
    embed, series = torch.ones((10, E), device="cuda"), torch.ones((B, T, Cn), dtype=torch.int64, device="cuda")
    scores, gpooled = torch.ones((B, T), device="cuda"), torch.ones((B, D), device="cuda")
    gkeys = torch.full((B, T, D), SENT, device="cuda")
    launched = []
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "_call", lambda fn, *args: launched.append(fn))
        for shape in ((B - 1, D), (B, D - 1)):
            q = torch.ones(shape, device="cuda")
            with pytest.raises(ValueError, match="q must be"):
                ops.ip_attn_fwd(embed, series, q, 0)
            with pytest.raises(ValueError, match="q must be"):
                ops.ip_attn_bwd(embed, series, q, 0, scores, gpooled, gkeys=gkeys)
    assert launched == [] and bool((gkeys == SENT).all())


def test_an_empty_batch_is_accepted(lib):
    s = stream()
    ids, flag = Ints(np.ones(64, np.int64), np.int64), Ints([0], np.int32)
    tab, outs = Buf(np.ones(4096, np.float32)), [Buf(poison((4096,))) for _ in range(3)]
    a, b, c = (o.ptr for o in outs)
    calls = [lib.rec_emb_ipn_fwd_f32(tab.ptr, 10, 8, 8, ids.ptr, 0, 3, a, 27, flag.ptr, s),
             lib.rec_emb_ipn_bwd_vals_f32(tab.ptr, 27, tab.ptr, 27, 0, 3, 8, a, s),
             lib.rec_emb_bi_fwd_f32(tab.ptr, 10, 8, 8, ids.ptr, 0, 3, a, 8, b, flag.ptr, s),
             lib.rec_emb_bi_bwd_vals_f32(tab.ptr, 10, 8, 8, ids.ptr, 0, 3, tab.ptr, 8, tab.ptr, a, s),
             lib.rec_ip_attn_fwd_f32(tab.ptr, 8, 10, 8, 2, ids.ptr, 0, 4, tab.ptr, 16, 0, a, b, 16, flag.ptr, s),
             lib.rec_ip_attn_bwd_f32(tab.ptr, 8, 10, 8, 2, ids.ptr, 0, 4, tab.ptr, 16, 0, tab.ptr, tab.ptr, 16, a, b, s),
             lib.rec_ffm_fwd_f32(tab.ptr, 24, tab.ptr, 1, tab.ptr, 10, 8, ids.ptr, 0, 3, a, b, flag.ptr, s),
             lib.rec_ffm_bwd_rows_f32(tab.ptr, 24, 10, 8, ids.ptr, 0, 3, tab.ptr, ids.ptr, ids.ptr, ids.ptr, a, s)]
    assert finish(0, outs, [tab, ids, flag] + outs) == 0 and calls == [0] * len(calls)


# ---- through ops and the layer ------------------------------------------------------------------------------------------------
def test_pnn_layer_trains_at_a_shape_the_old_backward_refused(lib):
    """F = 80, E = 64: the forward takes 28416 bytes of LDS, the backward 66880 (REC_E_ARG before the common domain)"""
    from explicit_tf2_recommendation_amd import functional, layers, ops
    from oracle import torch_ref as T
    from tests import helpers as H
    F, E, V, B = 80, 64, 300, 5
    assert IR.ipn_lds_bytes(1, F, E, True) > IR.K.LAUNCH_LDS and IR.ipn_accepts(F, E)
    names = ["f%d" % i for i in range(F)]
    pr = H.pnn_params(11, V, F, E)
    layer = layers.PNNLayer(feature_names=names, feature_dims=V, embedding_dims=E, mlp_dims=[32, 8]).cuda()
    sd = dict(layer.named_parameters())
    with torch.no_grad():
        for k, a in {"embed.embeddings": pr["embed"], "MLP_layer1.kernel_0": pr["k1"][0], "MLP_layer1.bias_0": pr["b1"][0],
                     "MLP_layer1.kernel_1": pr["k1"][1], "MLP_layer1.bias_1": pr["b1"][1],
                     "MLP_layer2.kernel_0": pr["k2"][0], "MLP_layer2.bias_0": pr["b2"][0]}.items():
            sd[k].copy_(torch.from_numpy(a))
    r = H.rng(12)
    ins = {n: r.integers(0, V, size=(B, 1)).astype(np.int64) for n in names}
    y = (r.uniform(size=(B, 1)) < 0.4).astype(np.float32)
    with G.guarded(ops):
        out = layer({k: torch.from_numpy(a).cuda() for k, a in ins.items()})["output"]
        loss = functional.KerasBCE.apply(out, torch.from_numpy(y).cuda())
        loss.backward()
        torch.cuda.synchronize()
    X = np.concatenate([ins[n] for n in names], 1)
    tp = H.to_torch(pr, torch.float64, True)
    o64 = T.pnn_forward(tp, torch.from_numpy(X))
    lt = T.keras_bce(torch.from_numpy(y).double(), o64)
    lt.backward()
    assert np.abs(out.detach().cpu().numpy() - o64.detach().numpy()).max() <= 1e-5
    assert abs(loss.item() - lt.item()) <= 1e-5
    got, want = layer.embed.embeddings.grad.to_dense().cpu().numpy(), tp["embed"].grad.numpy()
    assert np.abs(got - want).max() <= 2e-5 * max(1.0, np.abs(want).max())
    gk, wk = layer.MLP_layer1.kernel_0.grad.cpu().numpy(), tp["k1"][0].grad.numpy()
    assert np.abs(gk - wk).max() <= 2e-5 * max(1.0, np.abs(wk).max())
