"""The "K12 Adam" family (csrc/dense_ops.hip: rec_adam_sparse_keras_f32, rec_adam_sparse_keras_pair_f32, rec_adam_rows_f32,
rec_adam_dense_f32, rec_adam_dense_multi_f32, rec_adam_lr_t_f32) on every kernel class its entry points can pick,
against the fp64 reference and the bounds of tests/adam_classes_ref.py.

tests/test_adam_classes_host.py proves on the CPU that the tables reach the vec and the scalar sweep with one and with
several grid-stride passes, the pair sweep with one and two, every count regime (cap = 0, n_uniq = 0 < cap,
0 < n_uniq < cap, n_uniq = cap = V, ids outside [0, V)), that the bounds leave room for a correct fp32 evaluation and that
they catch eleven wrong ones.  Here:

  sparse      every case of SPARSE_CASES x every regime: var inside ulp32(x) + lr_t bound(m)/den + 6 u |step|, m and v of
              touched rows inside u (|b1 m| + |(1-b1) g|) and 2 u v, m and v of untouched rows the correctly rounded
              b1 m and b2 v bit for bit, the m = v = 0 rows bit-identical, the slots beyond n_uniq (valid ids, NaN
              gradients) and the row that 2^32 + 3 aliases with the plain decay, the padding columns of a strided table
              still NaN;
  lazy        rec_adam_rows_f32 the same, untouched rows bit-identical in var, m and v;
  pair        both tables of the fused rows against the reference, and the five refusals (REC_E_ARG, state untouched);
  dense       n in {1, 255, 256, 257, 70001}, n = 0 accepted, t = 0 refused; multi: 1, 7 and 16 tensors bit-equal to the
              single-tensor entry point and inside the bounds, 17 refused, a zero-element tensor;
  lr_t        within 4 ulp of the oracle's float32 value up to step 32768, float32(lr) beyond it;
  trajectory  20 steps of Zipf ids, each step against a reference restarted from the device's own state;
  buffers     every table is a view into a larger buffer of sentinels: none is written outside; every call runs twice
              from the same state and is bit-equal;
  ops         the wrappers refuse operands of the wrong dtype, shape or layout and leave the state alone.

Worst measured |got - ref| / bound per class on the MI355X (the module prints the table at the end of a run with -s):
  class             var     m       v            class                var     m       v
  vec, 1 pass       0.499   0.909   0.477        pair, 1 pass         0.500   0.838   0.481
  vec, 2 passes     0.500   0.958   0.494        pair, 2 passes       0.500   0.675   0.428
  scalar, 1 pass    0.500   0.899   0.479        dense                0.498   0.828   0.375
  scalar, 2 passes  0.500   0.939   0.493        dense multi          0.498   0.810   0.353
  lazy              0.500   0.864   0.481        trajectory, a step   0.500   0.944   0.490
m and v of every untouched row were the correctly rounded products bit for bit.  var never uses more than the half ulp of
its own rounding: the hardware square root and reciprocal of adam_step_x cost nothing that shows in x.  m sits where the
two roundings of fma(g, 1-b1, fl(m b1)) put it, close under its bound (adam_classes_ref.ROOM has the arithmetic).  After 20
steps the distance to the pure fp64 trajectory was 0.31 (var), 0.08 (m) and 0.15 (v) of 20 one-step bounds.  lr_t differed
from the oracle by 0 ulp at every step listed.  No case failed on the way: dense_ops.hip and common.h compute what they
did.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import adam_classes_ref as AR

pytestmark = pytest.mark.gpu
GUARD = 1024                  # sentinel floats on both sides of every buffer
SENT = -777.25
NAN_BITS = np.float32(np.nan).view(np.uint32)
HYPER = (AR.LR, AR.B1, AR.B2, AR.EPS)


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
def ops(lib):
    from explicit_tf2_recommendation_amd import ops
    return ops


@pytest.fixture(scope="module")
def worst():
    table = {}
    yield table
    print("\nworst |got - ref| / bound per class (x, m, v):")
    for key in sorted(table):
        print("  %-22s x %.3f (%s)  m %.3f  v %.3f" % (key, table[key]["x"][0], table[key]["x"][1], table[key]["m"][0],
                                                      table[key]["v"][0]))


def note(worst, key, q, name):
    slot = worst.setdefault(key, {k: (0.0, "-") for k in "xmv"})
    for k in "xmv":
        if q[k] > slot[k][0]:
            slot[k] = (q[k], name)


def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


class Buf:
    """``data`` (float32, any shape) as a view ``off`` floats past a 256-byte boundary inside a buffer of sentinels"""

    def __init__(self, data, off=0):
        data = np.array(data, np.float32)                # a copy: the shared case arrays are read-only
        self.shape, n = data.shape, data.size
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.base = torch.full((self.hi + GUARD,), SENT, dtype=torch.float32, device="cuda")
        assert self.base.data_ptr() % 256 == 0
        self.ptr = self.base.data_ptr() + 4 * self.lo
        self.t = self.base[self.lo:self.hi]
        if n:
            self.t.copy_(torch.from_numpy(data.reshape(-1)))

    def host(self):
        return self.t.cpu().numpy().reshape(self.shape)

    def check(self, what):
        for side, band in (("before", self.base[:self.lo]), ("after", self.base[self.hi:])):
            assert bool((band == SENT).all()), "%s: written %s the buffer" % (what, side)


def strided(x, ld, col=None):
    """x [V,E] as the leading columns of a [V,ld] table whose other columns hold NaN (``col`` [V,1]: column E)"""
    V, E = x.shape
    full = np.full((V, ld), np.nan, np.float32)
    full[:, :E] = x
    if col is not None:
        full[:, E] = col[:, 0]
    return full


def padding_is_nan(full, first):
    return bool(np.all(bits(full[:, first:]) == NAN_BITS))


class Tables:
    """var [V,ld], m and v [V,E] of one table on the device, each in its own guarded buffer"""

    def __init__(self, x, m, v, ld, off=(0, 0, 0)):
        self.V, self.E, self.ld = x.shape[0], x.shape[1], ld
        self.x, self.m, self.v = Buf(strided(x, ld), off[0]), Buf(m, off[1]), Buf(v, off[2])

    def host(self):
        full = self.x.host()
        return full, full[:, :self.E], self.m.host(), self.v.host()

    def check(self, what):
        for b in (self.x, self.m, self.v):
            b.check(what)


def sparse_call(lib, tab, inp, t, lazy=False):
    ids, g = dev(inp.ids), Buf(inp.g)
    nu = torch.tensor([inp.n_uniq], dtype=torch.int64, device="cuda")
    head = (tab.x.ptr, tab.ld, tab.m.ptr, tab.v.ptr, tab.V, tab.E, ids.data_ptr(), g.ptr, nu.data_ptr(), inp.cap)
    if lazy:
        status = lib.rec_adam_rows_f32(*head, t, *HYPER, stream())
        side = None
    else:
        side = Buf(np.full((max(inp.cap, 1), 3, tab.E), np.nan, np.float32))
        status = lib.rec_adam_sparse_keras_f32(*head, side.ptr, t, *HYPER, stream())
    torch.cuda.synchronize()
    tab.check("tables")
    g.check("g_rows")
    assert same_bits(g.host(), inp.g)
    if side is not None:
        side.check("side")
    return status


def check_sparse(got, ref, start, name, lazy=False):
    """got = (var, m, v) [V,E] against a SparseRef; ``start`` the state before the step"""
    q = AR.ratios(*got, ref)
    print("%s: x %.3f m %.3f v %.3f of the bound, untouched m and v exact: %s" % (name, q["x"], q["m"], q["v"], q["bits"]))
    assert q["bits"], "%s: m or v of an untouched row is not the correctly rounded product" % name
    assert AR.inside(q), (name, q)
    u = ~ref.touched
    rows = np.nonzero(u)[0] if lazy else np.array([r for r in (AR.SPECIAL["zero_u"],) if u[r]], np.int64)
    for a, b in zip(got, start):                       # bit-identical: every untouched row (lazy), the m = v = 0 row
        assert same_bits(a[rows], b[rows]), "%s: an untouched row moved" % name
    return q


# ---- rec_adam_sparse_keras_f32 and rec_adam_rows_f32 ------------------------------------------------------------------
SPARSE_RUNS = [(c.name, r) for c in AR.SPARSE_CASES + AR.LAZY_CASES for r in AR.REGIMES]


@pytest.mark.parametrize("name,regime", SPARSE_RUNS)
def test_sparse_step_against_the_reference(lib, worst, name, regime):
    c = AR.BY_NAME[name]
    lazy = isinstance(c, AR.LazyCase)
    start, inp, ref = AR.case_state(name), AR.case_input(name, regime), AR.case_reference(name, regime)
    runs = []
    for _ in range(2):
        tab = Tables(*start, c.ld, getattr(c, "off", (0, 0, 0)))
        if not lazy:
            aligned = [b.ptr % 16 == 0 for b in (tab.x, tab.m, tab.v)]
            assert AR.sweep_class(c.E, c.ld, *aligned) == c.cls
        assert sparse_call(lib, tab, inp, c.t, lazy) == 0
        runs.append(tab.host())
    full, x, m, v = runs[0]
    assert all(same_bits(a, b) for a, b in zip(runs[0], runs[1])), "two runs from the same state differ"
    assert padding_is_nan(full, c.E), "a column beyond E was written"
    q = check_sparse((x, m, v), ref, start, "%s/%s" % (name, regime), lazy)
    if regime == "oob":
        assert not ref.touched[AR.ALIAS_ROW]
    note(worst, "lazy" if lazy else "%s, %d pass" % (c.cls, min(c.npass, 2)), q, "%s/%s" % (name, regime))


# ---- rec_adam_sparse_keras_pair_f32 -----------------------------------------------------------------------------------
class PairTables:
    def __init__(self, st, E, ld, off_fused=0, off_me=0):
        xe, me, ve, xw, mw, vw = st
        self.E, self.ld, self.V = E, ld, xe.shape[0]
        self.fused = Buf(strided(xe, ld, xw), off_fused)
        self.me, self.ve, self.mw, self.vw = Buf(me, off_me), Buf(ve), Buf(mw), Buf(vw)

    def bufs(self):
        return self.fused, self.me, self.ve, self.mw, self.vw

    def host(self):
        return [b.host() for b in self.bufs()]


def pair_call(lib, p, e, gw, t, V=None, E=None, ld=None):
    ids, ge, gwb = dev(e.ids), Buf(e.g), Buf(gw)
    nu = torch.tensor([e.n_uniq], dtype=torch.int64, device="cuda")
    E_ = p.E if E is None else E
    side_e = Buf(np.full((max(e.cap, 1), 3, p.E), np.nan, np.float32))
    side_w = Buf(np.full((max(e.cap, 1), 3, 1), np.nan, np.float32))
    status = lib.rec_adam_sparse_keras_pair_f32(
        p.fused.ptr, p.ld if ld is None else ld, p.me.ptr, p.ve.ptr, p.mw.ptr, p.vw.ptr, p.V if V is None else V, E_,
        ids.data_ptr(), ge.ptr, gwb.ptr, nu.data_ptr(), e.cap, side_e.ptr, side_w.ptr, t, *HYPER, stream())
    torch.cuda.synchronize()
    for b in p.bufs() + (ge, gwb, side_e, side_w):
        b.check("pair")
    return status


@pytest.mark.parametrize("name,regime", [(c.name, r) for c in AR.PAIR_CASES for r in c.regimes])
def test_pair_step_against_the_reference(lib, worst, name, regime):
    c = AR.BY_NAME[name]
    start, (e, gw), (ref_e, ref_w) = AR.case_state(name), AR.case_input(name, regime), AR.case_reference(name, regime)
    runs = []
    for _ in range(2):
        p = PairTables(start, c.E, c.ld)
        assert pair_call(lib, p, e, gw, c.t) == 0
        runs.append(p.host())
    assert all(same_bits(a, b) for a, b in zip(*runs)), "two runs from the same state differ"
    fused, me, ve, mw, vw = runs[0]
    assert padding_is_nan(fused, c.E + 1), "a padding column of the fused rows was written"
    qe = check_sparse((fused[:, :c.E], me, ve), ref_e, start[:3], "%s/%s embed" % (name, regime))
    qw = check_sparse((fused[:, c.E:c.E + 1], mw, vw), ref_w, start[3:], "%s/%s w" % (name, regime))
    for q in (qe, qw):
        note(worst, "pair, %d pass" % min(c.npass, 2), q, "%s/%s" % (name, regime))


@pytest.mark.parametrize("what,E,ld,off_fused,off_me", [
    ("ld = E", 16, 16, 0, 0), ("ld % 4 != 0", 16, 18, 0, 0), ("E % 4 != 0", 6, 8, 0, 0),
    ("misaligned fused table", 16, 32, 1, 0), ("misaligned m_e", 16, 32, 0, 1)])
def test_pair_refusals_leave_the_state_alone(lib, limits, what, E, ld, off_fused, off_me):
    """the buffers are those of E = 16, ld = 32 whatever is passed: a launch that happened anyway would stay inside"""
    assert not AR.pair_args_ok(E, ld, off_fused == 0, off_me == 0)
    V = 300
    st = AR.state(V, 16, 600) + AR.state(V, 1, 601)
    e = AR.sparse_input(V, 16, 5, "asc", 602, "partial")
    gw = np.random.default_rng(603).standard_normal((len(e.ids), 1), dtype=np.float32)
    p = PairTables(st, 16, 32, off_fused, off_me)
    before = p.host()
    assert pair_call(lib, p, e, gw, 3, E=E, ld=ld) == limits["REC_E_ARG"], what
    assert all(same_bits(a, b) for a, b in zip(before, p.host())), what


# ---- rec_adam_dense_f32 and rec_adam_dense_multi_f32 ------------------------------------------------------------------
def dense_call(lib, bufs, n, t):
    status = lib.rec_adam_dense_f32(*[b.ptr for b in bufs], n, t, *HYPER, stream())
    torch.cuda.synchronize()
    for b in bufs:
        b.check("dense")
    return status


@pytest.mark.parametrize("name", [c.name for c in AR.DENSE_CASES])
def test_dense_step_against_the_reference(lib, worst, name):
    c = AR.BY_NAME[name]
    inp = AR.dense_input(c.n, c.seed)
    runs = []
    for _ in range(2):
        bufs = [Buf(a) for a in inp]
        assert dense_call(lib, bufs, c.n, c.t) == 0
        runs.append([b.host() for b in bufs])
    assert all(same_bits(a, b) for a, b in zip(*runs))
    x, m, v, g = runs[0]
    assert same_bits(g, inp[3])
    q = AR.ratios(x, m, v, AR.ref_dense(*inp, AR.scalars(c.t)))
    print("%s: x %.3f m %.3f v %.3f of the bound" % (name, q["x"], q["m"], q["v"]))
    assert AR.inside(q), (name, q)
    if c.n >= 16:                                       # m = v = 0 and g = 0: bit-identical
        assert all(same_bits(a[6:7], b[6:7]) for a, b in zip((x, m, v), inp))
    note(worst, "dense", q, name)


def test_dense_accepts_no_elements_and_refuses_step_zero(lib, limits):
    inp = AR.dense_input(300, 700)
    for n, t, want in ((0, 3, limits["REC_OK"]), (300, 0, limits["REC_E_ARG"]), (-1, 3, limits["REC_E_ARG"])):
        bufs = [Buf(a) for a in inp]
        assert dense_call(lib, bufs, n, t) == want, (n, t)
        assert all(same_bits(b.host(), a) for b, a in zip(bufs, inp)), (n, t)


def multi_call(lib, tensors, sizes, lr_t_dev, ptrs=None):
    """tensors: [(var, m, v, g) Bufs]; ``ptrs`` replaces the addresses of chosen tensors: {index: address}"""
    n = len(tensors)
    arrays = []
    for k in range(4):
        addr = [t[k].ptr for t in tensors]
        for i, p in (ptrs or {}).items():
            addr[i] = p
        arrays.append((C.c_void_p * n)(*addr))
    numel = (C.c_int64 * n)(*sizes)
    status = lib.rec_adam_dense_multi_f32(n, *arrays, numel, lr_t_dev.data_ptr(), AR.B1, AR.B2, AR.EPS, stream())
    torch.cuda.synchronize()
    for t in tensors:
        for b in t:
            b.check("multi")
    return status


def lr_t_on_device(lib, t):
    return torch.tensor([lib.rec_adam_lr_t_f32(AR.LR, AR.B1, AR.B2, t)], dtype=torch.float32, device="cuda")


@pytest.mark.parametrize("name", [c.name for c in AR.MULTI_CASES])
def test_multi_equals_the_single_tensor_entry_point(lib, worst, name):
    c = AR.BY_NAME[name]
    inputs = AR.multi_input(c)
    single = []
    for inp, n in zip(inputs, c.sizes):
        bufs = [Buf(a) for a in inp]
        assert dense_call(lib, bufs, n, c.t) == 0
        single.append([b.host() for b in bufs])
    runs = []
    for _ in range(2):
        tensors = [[Buf(a) for a in inp] for inp in inputs]
        assert multi_call(lib, tensors, c.sizes, lr_t_on_device(lib, c.t)) == 0
        runs.append([[b.host() for b in t] for t in tensors])
    for i, (one, a, b, inp) in enumerate(zip(single, runs[0], runs[1], inputs)):
        assert all(same_bits(p, q) for p, q in zip(a, b)), "tensor %d: two runs differ" % i
        assert all(same_bits(p, q) for p, q in zip(one, a)), "tensor %d differs from rec_adam_dense_f32" % i
        q = AR.ratios(*a[:3], AR.ref_dense(*inp, AR.scalars(c.t)))
        assert AR.inside(q), (name, i, q)
        note(worst, "dense multi", q, "%s[%d]" % (name, i))


def test_multi_refuses_17_tensors(lib, limits):
    inputs = [AR.dense_input(20, 800 + i) for i in range(AR.ADAM_MULTI_MAX + 1)]
    tensors = [[Buf(a) for a in inp] for inp in inputs]
    sizes = [20] * len(inputs)
    assert multi_call(lib, tensors, sizes, lr_t_on_device(lib, 3)) == limits["REC_E_UNSUPPORTED"]
    assert multi_call(lib, tensors[:0] + tensors[:1], [-1], lr_t_on_device(lib, 3)) == limits["REC_E_ARG"]
    for t, inp in zip(tensors, inputs):
        assert all(same_bits(b.host(), a) for b, a in zip(t, inp))


def test_multi_with_a_zero_element_tensor(lib, limits):
    """What a zero-element tensor in the list does today.  With a valid address and numel = 0 it is skipped: the call
    succeeds and its neighbours get the update of rec_adam_dense_f32.  An empty torch tensor has the address 0, and the
    null check of the entry point then refuses the whole list (REC_E_ARG) before anything is launched, although no
    element of that tensor would be read: a caller has to leave empty parameters out of the list."""
    sizes = (257, 0, 300)
    inputs = [AR.dense_input(max(n, 1), 810 + i) for i, n in enumerate(sizes)]
    want = []
    for inp, n in zip(inputs, sizes):
        bufs = [Buf(a) for a in inp]
        assert dense_call(lib, bufs, n, 5) == 0
        want.append([b.host() for b in bufs])
    tensors = [[Buf(a) for a in inp] for inp in inputs]
    assert multi_call(lib, tensors, sizes, lr_t_on_device(lib, 5)) == limits["REC_OK"]
    for t, w, inp in zip(tensors, want, inputs):
        assert all(same_bits(b.host(), a) for b, a in zip(t, w))
    assert all(same_bits(b.host(), a) for b, a in zip(tensors[1], inputs[1]))
    empty = torch.empty(0, dtype=torch.float32, device="cuda")
    assert empty.data_ptr() == 0
    tensors = [[Buf(a) for a in inp] for inp in inputs]
    assert multi_call(lib, tensors, sizes, lr_t_on_device(lib, 5), ptrs={1: empty.data_ptr()}) == limits["REC_E_ARG"]
    for t, inp in zip(tensors, inputs):
        assert all(same_bits(b.host(), a) for b, a in zip(t, inp))


# ---- rec_adam_lr_t_f32 ------------------------------------------------------------------------------------------------
def test_lr_t_is_the_oracle_s_and_saturates_at_the_end_of_the_engine_s_table(lib):
    """Up to step 32768 (the table of engine._init_device_adam) within 4 ulp of the oracle's float32 value; measured
    difference: 0 ulp at every step listed.  Beyond the table the value is float32(lr), which is what the engine relies
    on when it says that the corrections are 1.0f there."""
    for t in AR.LR_T_NEAR:
        got, want = np.float32(lib.rec_adam_lr_t_f32(*HYPER[:3], t)), AR.scalars(t, dt=np.float32).lr_t
        ulps = abs(int(got.view(np.int32)) - int(want.view(np.int32)))
        print("lr_t(%d) = %r, oracle %r: %d ulp" % (t, got, want, ulps))
        assert ulps <= 4, (t, got, want)
    for t in AR.LR_T_FAR:
        assert np.float32(lib.rec_adam_lr_t_f32(*HYPER[:3], t)) == np.float32(AR.LR), t
    assert np.float32(lib.rec_adam_lr_t_f32(*HYPER[:3], 17000)) != np.float32(AR.LR)


# ---- 20 steps -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["keras", "lazy"])
def test_trajectory_of_20_steps(lib, worst, entry):
    """Each step against a reference restarted from the device's own state, under the one-step bounds.  After step 20 the
    distance to a pure fp64 trajectory is reported and asserted against 20 times the one-step bound, taken per element as
    the largest over the steps: the bounds of 20 steps add up to at most that, and what an error of m or v carries into
    later steps is of second order beside it."""
    V, E, lazy = 5000, 16, entry == "lazy"
    r = np.random.default_rng(900)
    tab = Tables(*AR.state(V, E, 901), E)
    pure = [a.astype(np.float64) for a in AR.state(V, E, 901)]
    most = [np.zeros((V, E)) for _ in range(3)]
    for t in range(1, 21):
        raw = (r.zipf(1.05, size=2000) - 1) % V
        first = np.unique(raw, return_index=True)[1]
        ids = (np.unique(raw) if t % 2 else raw[np.sort(first)]).astype(np.int64)
        g = r.standard_normal((len(ids), E), dtype=np.float32)
        inp = AR.SparseInput(ids, g, len(ids), len(ids))
        start = tab.host()[1:]
        ref = AR.ref_sparse(*start, ids, g, len(ids), AR.scalars(t), lazy)
        far = AR.ref_sparse(*pure, ids, g, len(ids), AR.scalars(t), lazy)
        assert sparse_call(lib, tab, inp, t, lazy) == 0
        q = check_sparse(tab.host()[1:], ref, start, "%s step %d" % (entry, t), lazy)
        note(worst, "trajectory " + entry, q, "step %d" % t)
        pure = [far.x, far.m, far.v]
        most = [np.maximum(a, b) for a, b in zip(most, (far.bx, far.bm, far.bv))]
    got = tab.host()[1:]
    dist = [float((np.abs(a.astype(np.float64) - b) / (20 * c)).max()) for a, b, c in zip(got, pure, most)]
    print("%s: after 20 steps x %.3f m %.3f v %.3f of 20 one-step bounds from the fp64 trajectory" % (entry, *dist))
    assert max(dist) <= 1, dist


# ---- the wrappers of ops ------------------------------------------------------------------------------------------------
def _ops_state(V=50, E=4, cap=9):
    x, m, v = (dev(a) for a in AR.state(V, E, 950))
    ids = torch.arange(20, 20 + cap, dtype=torch.int64, device="cuda")
    g = dev(np.random.default_rng(951).standard_normal((cap, E), dtype=np.float32))
    nu = torch.tensor([cap - 2], dtype=torch.int64, device="cuda")
    return dict(var=x, m=m, v=v, uniq_ids=ids, g_rows=g, n_uniq=nu)


def _held(a, violate):
    """applies ``violate`` to the operands ``a``; -> [(tensor, copy)] of every tensor before and after it"""
    tensors = [t for t in a.values() if isinstance(t, torch.Tensor)]
    violate(a)
    tensors += [t for t in a.values() if isinstance(t, torch.Tensor) and not any(t is u for u in tensors)]
    return [(t, t.clone()) for t in tensors]


def _assert_untouched(held):
    torch.cuda.synchronize()
    for t, copy in held:
        assert torch.equal(t.reshape(-1).view(torch.uint8), copy.reshape(-1).view(torch.uint8))


SPARSE_VIOLATIONS = {
    "m transposed": lambda a: a.update(m=a["m"].t().contiguous().t()),
    "m float64": lambda a: a.update(m=a["m"].double()),
    "m of another height": lambda a: a.update(m=a["m"][:-1].contiguous()),
    "v one column wider": lambda a: a.update(v=torch.zeros((50, 5), device="cuda")),
    "v strided": lambda a: a.update(v=torch.zeros((50, 8), device="cuda")[:, :4]),
    "g_rows one column wider": lambda a: a.update(g_rows=torch.zeros((9, 5), device="cuda")),
    "g_rows flat": lambda a: a.update(g_rows=a["g_rows"].reshape(-1)),
    "g_rows float64": lambda a: a.update(g_rows=a["g_rows"].double()),
    "g_rows transposed": lambda a: a.update(g_rows=torch.zeros((4, 9), device="cuda").t()),
    "uniq_ids int32": lambda a: a.update(uniq_ids=a["uniq_ids"].int()),
    "uniq_ids shorter than g_rows": lambda a: a.update(uniq_ids=a["uniq_ids"][:5].contiguous()),
    "uniq_ids two-dimensional": lambda a: a.update(uniq_ids=a["uniq_ids"].reshape(3, 3)),
    "n_uniq int32": lambda a: a.update(n_uniq=a["n_uniq"].int()),
    "n_uniq a host number": lambda a: a.update(n_uniq=7),
    "n_uniq on the host": lambda a: a.update(n_uniq=a["n_uniq"].cpu()),
    "n_uniq of two": lambda a: a.update(n_uniq=torch.zeros(2, dtype=torch.int64, device="cuda")),
    "var of three axes": lambda a: a.update(var=a["var"].reshape(50, 2, 2)),
}


@pytest.mark.parametrize("fn", ["adam_sparse_keras", "adam_rows"])
@pytest.mark.parametrize("what", sorted(SPARSE_VIOLATIONS))
def test_sparse_wrappers_refuse_and_leave_the_state_alone(ops, fn, what):
    a = _ops_state()
    held = _held(a, SPARSE_VIOLATIONS[what])
    with pytest.raises((TypeError, ValueError, RuntimeError)):
        getattr(ops, fn)(a["var"], a["m"], a["v"], a["uniq_ids"], a["g_rows"], a["n_uniq"], 3, AR.LR)
    _assert_untouched(held)


@pytest.mark.parametrize("fn", ["adam_sparse_keras", "adam_rows"])
def test_sparse_wrappers_accept_what_the_callers_pass(ops, fn):
    """a strided table of the fused layout, ids longer than g_rows, n_uniq of shape [1] or []: all the same step"""
    lazy = fn == "adam_rows"
    base = _ops_state()
    host = [base[k].cpu().numpy() for k in ("var", "m", "v")]
    ref = AR.ref_sparse(*host, base["uniq_ids"].cpu().numpy(), base["g_rows"].cpu().numpy(), 7, AR.scalars(3), lazy)
    outs = []
    for form in ("plain", "strided", "long ids", "scalar n_uniq"):
        a = _ops_state()
        if form == "strided":
            wide = torch.full((50, 8), float("nan"), device="cuda")
            wide[:, :4] = a["var"]
            a["var"] = wide[:, :4]
        if form == "long ids":
            a["uniq_ids"] = torch.cat([a["uniq_ids"], torch.full((3,), 1, dtype=torch.int64, device="cuda")])
        if form == "scalar n_uniq":
            a["n_uniq"] = a["n_uniq"].reshape(())
        getattr(ops, fn)(a["var"], a["m"], a["v"], a["uniq_ids"], a["g_rows"], a["n_uniq"], 3, AR.LR)
        outs.append([a[k].cpu().numpy() for k in ("var", "m", "v")])
        check_sparse(outs[-1], ref, host, "%s %s" % (fn, form), lazy)
        assert all(same_bits(p, q) for p, q in zip(outs[0], outs[-1])), form


DENSE_VIOLATIONS = {
    "m float64": lambda a: a.update(m=a["m"].double()),
    "m transposed": lambda a: a.update(m=a["m"].t().contiguous().t()),
    "v of another shape": lambda a: a.update(v=a["v"].reshape(-1)),
    "g of another shape": lambda a: a.update(g=a["g"][:-1].contiguous()),
    "g transposed": lambda a: a.update(g=a["g"].t().contiguous().t()),
    "g on the host": lambda a: a.update(g=a["g"].cpu()),
    "v missing": lambda a: a.update(v=None),
}


@pytest.mark.parametrize("what", sorted(DENSE_VIOLATIONS))
def test_dense_wrapper_refuses_and_leaves_the_state_alone(ops, what):
    def fresh():
        x, m, v = (dev(a) for a in AR.state(50, 4, 960))
        return dict(var=x, m=m, v=v, g=dev(np.random.default_rng(961).standard_normal((50, 4), dtype=np.float32)))
    a = fresh()
    held = _held(a, DENSE_VIOLATIONS[what])
    with pytest.raises((TypeError, ValueError, RuntimeError)):
        ops.adam_dense(a["var"], a["m"], a["v"], a["g"], 3, AR.LR)
    _assert_untouched(held)


def test_dense_wrapper_takes_any_shape(ops):
    for shape in ((200,), (50, 4), (5, 10, 4)):
        inp = AR.dense_input(200, 970)
        x, m, v, g = (dev(a.reshape(shape)) for a in inp)
        ops.adam_dense(x, m, v, g, 4, AR.LR)
        q = AR.ratios(*[a.cpu().numpy().reshape(-1) for a in (x, m, v)], AR.ref_dense(*inp, AR.scalars(4)))
        assert AR.inside(q), (shape, q)
