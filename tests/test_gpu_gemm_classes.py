"""rec_gemm_f32 (csrc/gemm.hip) on every kernel instance its dispatcher can launch -- tile64<TA,TB>, skinny<1|2>,
big<TA,TB>, panel<0,TB,1..7> with one and with several column panels, and the split-K reduce -- through ops.gemm (and the
C ABI where ops.gemm cannot express the call), on the inputs of tests/gemm_classes_ref.py.

tests/test_gemm_classes_host.py proves on the CPU that every case is in the class it claims, that the tables reach all 25
instances and every regime, that the exact inputs have one fp32 answer in any summation order, that the real-valued bound
leaves room for a correct fp32 evaluation and that eleven wrong kernels are caught.  Here:

  cases       every case with all seven epilogues: none, bias, relu, cross (with aux) and add are asserted with BIT
              equality against the float64 result cast to fp32; sigmoid within 6 * 2^-24 and tanh within 2e-5 absolute of
              the float64 activation of the exact argument.  The operands are column slices, three floats into a wider
              buffer of odd row stride (4-byte but not 16-byte aligned rows; lda, ldb, ldc, lde0, lde1 all differ and none
              is minimal), `out` and `aux` column slices of two wider buffers of one row stride.  Everything around the
              operands, two guard rows after the last included, is NaN: a read the kernel should have guarded shows in
              the result, a clamped read stays invisible.  Everything outside the M x N window of `out` and `aux` keeps
              its bits.  Every exact call runs twice and is bit-equal.
  footprint   a NaN at A[i,k] makes exactly row i of C NaN, a NaN at B[k,j] exactly column j, and every other element
              keeps its exact bits: i in the last (partial) row block, j in the last column block, k in the tail slab of
              the last slice, and all three at 0; one case a kernel and a column-panel regime.
  degenerate  M = 0 or N = 0: REC_OK, nothing written; K = 0: epi(0) on a tile64, a skinny and a panel shape; split_k > 1
              without a workspace: REC_E_WORKSPACE; every REC_E_ARG line of the entry point, nothing written; a request that
              collapses to one slice leaves the workspace it was given alone.
  real        one case a kernel, standard normal inputs, against the per-element bound.

No tolerance here comes from a measurement of the kernels: the exact cases have none, the two activation bounds and the
real-valued bound are derived in tests/gemm_classes_ref.py.

Measured on the MI355X (the module prints every figure with -s): all 205 cases bit-exact in the five exact epilogues, no
canary touched, every footprint one row or one column; worst sigmoid error 8.1e-8 of the 3.6e-7 allowed, worst tanh error
7.2e-8 of 2e-5; real-valued inputs at most 0.60 of the bound (K = 5, where the bound is mostly the final rounding), 0.001
at K = 641 in 41 slices.  No case failed: gemm.hip computes what its header says.  237 tests in 14 s.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import gemm_classes_ref as GR

pytestmark = pytest.mark.gpu
NAN = float("nan")
GUARD_ROWS = 2
OFF = 3                       # the column at which an operand starts inside its buffer
PADS = dict(A=5, B=7, e0=9, e1=11)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from explicit_tf2_recommendation_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def abi():
    assert torch.cuda.is_available()
    from explicit_tf2_recommendation_amd._lib import lib, LIMITS
    return lib, LIMITS


def code_of(ops, epi):
    return {"none": ops.EPI_NONE, "bias": ops.EPI_BIAS, "relu": ops.EPI_BIAS_RELU, "sigmoid": ops.EPI_BIAS_SIGMOID,
            "tanh": ops.EPI_BIAS_TANH, "cross": ops.EPI_CROSS, "add": ops.EPI_ADD}[epi]


def operand(m, pad):
    """the matrix ``m`` as a column slice, OFF floats into a NaN buffer of odd row stride with guard rows behind it"""
    m = np.ascontiguousarray(m, np.float32)
    R, W = m.shape
    ld = (W + pad) | 1
    buf = torch.full((R + GUARD_ROWS, ld), NAN, dtype=torch.float32, device="cuda")
    view = buf[:R, OFF:OFF + W]
    view.copy_(torch.from_numpy(m))
    assert view.stride(0) % 2 == 1 and view.data_ptr() % 16 != 0
    return view


def vector(v):
    buf = torch.full((v.size + 8,), NAN, dtype=torch.float32, device="cuda")
    buf[OFF:OFF + v.size].copy_(torch.from_numpy(np.ascontiguousarray(v, np.float32)))
    return buf[OFF:OFF + v.size]


class Operands:
    """the device side of one case's inputs"""

    def __init__(self, c, x):
        self.c = c
        self.A = operand(x.A.T if c.tA else x.A, PADS["A"])
        self.B = operand(x.B.T if c.tB else x.B, PADS["B"])
        self.bias, self.e0, self.e1 = vector(x.bias), operand(x.e0, PADS["e0"]), operand(x.e1, PADS["e1"])
        assert len({t.stride(0) for t in (self.e0, self.e1)} | {c.N + 6}) == 3


class Out:
    """``out`` and ``aux`` of one call: column slices (at columns 1 and 2) of two sentinel buffers of one row stride"""

    def __init__(self, M, N):
        self.M, self.N, ld = M, N, N + 6
        self.cbuf = torch.full((M + GUARD_ROWS, ld), GR.SENT, dtype=torch.float32, device="cuda")
        self.abuf = torch.full((M + GUARD_ROWS, ld), GR.SENT, dtype=torch.float32, device="cuda")
        self.out, self.aux = self.cbuf[:M, 1:1 + N], self.abuf[:M, 2:2 + N]

    def expected(self, ref, u):
        """the two buffers as a right kernel leaves them"""
        ec, ea = torch.full_like(self.cbuf, GR.SENT), torch.full_like(self.abuf, GR.SENT)
        ec[:self.M, 1:1 + self.N].copy_(torch.from_numpy(ref))
        if u is not None:
            ea[:self.M, 2:2 + self.N].copy_(torch.from_numpy(u))
        return ec, ea

    def canaries_hold(self, aux_too=True):
        c = self.cbuf.clone()
        c[:self.M, 1:1 + self.N] = GR.SENT
        a = self.abuf.clone()
        if not aux_too:
            a[:self.M, 2:2 + self.N] = GR.SENT
        return bool((c == GR.SENT).all()) and bool((a == GR.SENT).all())


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def run(ops, d, epi, A=None, B=None):
    """one ops.gemm call of case d.c with epilogue ``epi`` into fresh buffers; only the side operands the epilogue reads are
    passed"""
    c, o = d.c, Out(d.c.M, d.c.N)
    kw = {}
    if epi in ("bias", "relu", "sigmoid", "tanh", "cross"):
        kw["bias"] = d.bias
    if epi == "cross":
        kw.update(e0=d.e0, e1=d.e1, aux=o.aux)
    if epi == "add":
        kw["e1"] = d.e1
    got = ops.gemm(d.A if A is None else A, d.B if B is None else B, bool(c.tA), bool(c.tB), epi=code_of(ops, epi),
                   split_k=c.split, out=o.out, **kw)
    assert got.data_ptr() == o.out.data_ptr()
    return o


# ---- every case, every epilogue ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c.name for c in GR.ALL_CASES])
def test_case(ops, name):
    c, x = GR.BY_NAME[name], GR.exact_input(name)
    assert GR.instance(GR.path_of(c)) == c.cls
    d, acc = Operands(c, x), GR.product64(x)
    for epi in GR.EXACT_EPIS:
        ref, u = GR.exact_reference(x, epi, acc)
        first, second = run(ops, d, epi), run(ops, d, epi)
        ec, ea = first.expected(ref, u)
        ok_c, ok_a = same_bits(first.cbuf, ec), same_bits(first.abuf, ea)
        if not (ok_c and ok_a):                                  # say where before failing
            got = first.out.cpu().numpy()
            bad = np.argwhere(got.view(np.uint32) != ref.view(np.uint32))
            print("%s %s: %d of %d elements of C differ, the first at %s: got %r, want %r; canaries hold: %s" % (
                name, epi, len(bad), ref.size, bad[:1].tolist(), got[tuple(bad[0])] if len(bad) else None,
                ref[tuple(bad[0])] if len(bad) else None, first.canaries_hold(aux_too=epi != "cross")))
        assert ok_c, (name, epi, "C, or a canary around it")
        assert ok_a, (name, epi, "aux, or a canary around it")
        assert same_bits(first.cbuf, second.cbuf) and same_bits(first.abuf, second.abuf), (name, epi, "two runs differ")
    sa, sb = GR.activation_scale(c.K)
    xs = x._replace(A=x.A * np.float32(sa), B=x.B * np.float32(sb))
    As = d.A if sa == 1.0 else operand(xs.A.T if c.tA else xs.A, PADS["A"])
    Bs = d.B if sb == 1.0 else operand(xs.B.T if c.tB else xs.B, PADS["B"])
    for epi, bound in (("sigmoid", GR.SIGMOID_BOUND), ("tanh", GR.TANH_BOUND)):
        ref = torch.from_numpy(GR.reference(xs, epi, acc * (sa * sb))[0]).cuda()
        o = run(ops, d, epi, As, Bs)
        err = float((o.out.double() - ref).abs().max())
        print("%s %s: worst error %.3g of %.3g" % (name, epi, err, bound))
        assert err <= bound, (name, epi, err)                    # (a NaN fails the comparison)
        assert o.canaries_hold(), (name, epi)


# ---- poison footprint ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GR.REAL_CASES)
def test_poison_footprint(ops, name):
    c, x = GR.BY_NAME[name], GR.exact_input(name)
    ref = torch.from_numpy(GR.exact_reference(x, "none")[0]).cuda()
    d = Operands(c, x)
    M, N, K = c.M, c.N, c.K
    for which, (r, col) in (("A", (M - 1, K - 1)), ("A", (0, 0)), ("B", (K - 1, N - 1)), ("B", (0, 0)),
                            ("A", (M // 2, K // 2)), ("B", (K // 2, N // 2))):
        m = (x.A if which == "A" else x.B).copy()
        m[r, col] = np.nan
        trans = c.tA if which == "A" else c.tB
        dirty = operand(m.T if trans else m, PADS[which])
        o = run(ops, d, "none", A=dirty if which == "A" else None, B=dirty if which == "B" else None)
        want = torch.zeros((M, N), dtype=torch.bool, device="cuda")
        if which == "A":
            want[r, :] = True
        else:
            want[:, col] = True
        got = torch.isnan(o.out)
        assert torch.equal(got, want), "%s: a NaN at %s[%d,%d] reached %d elements of C, %d were expected" % (
            name, which, r, col, int(got.sum()), int(want.sum()))
        zero = torch.zeros_like(ref)
        assert same_bits(torch.where(want, zero, o.out), torch.where(want, zero, ref)), (name, which, r, col)
        assert o.canaries_hold(), (name, which)


# ---- real-valued inputs against the per-element bound ---------------------------------------------------------------------
@pytest.mark.parametrize("name", GR.REAL_CASES)
def test_real_valued_bound(ops, name):
    c, x, p = GR.BY_NAME[name], GR.real_input(name), GR.path_of(GR.BY_NAME[name])
    d = Operands(c, x)
    for epi in GR.REAL_EPIS:
        (ref, u), (bC, bu) = GR.reference(x, epi), GR.real_bounds(x, p, epi)
        o, again = run(ops, d, epi), run(ops, d, epi)
        q = float(((o.out.double() - torch.from_numpy(ref).cuda()).abs() / torch.from_numpy(bC).cuda()).max())
        qa = 0.0 if u is None else float(((o.aux.double() - torch.from_numpy(u).cuda()).abs() / torch.from_numpy(bu).cuda()).max())
        print("%s %s: C at %.3f, aux at %.3f of the bound" % (name, epi, q, qa))
        assert q <= 1 and qa <= 1, (name, epi, q, qa)
        assert o.canaries_hold(aux_too=u is None), (name, epi)
        assert same_bits(o.cbuf, again.cbuf) and same_bits(o.abuf, again.abuf), (name, epi, "two runs differ")


# ---- degenerate calls through the C ABI ---------------------------------------------------------------------------------
def stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class Abi:
    """one well-formed rec_gemm_f32 call on exact inputs, whose arguments a test replaces one at a time"""

    def __init__(self, abi, tA, tB, M, N, K, epi="cross", split=1, ws_floats=0):
        self.lib, self.lim = abi
        r = np.random.Generator(np.random.PCG64(M * 131 + N * 17 + K))
        self.shape = (M, N, K)
        self.x = GR.Inputs(GR.dyadic(r, (M, K), 8), GR.dyadic(r, (K, N), 8), GR.dyadic(r, (max(N, 1),), 16)[:N],
                           GR.dyadic(r, (M, N), 16), GR.dyadic(r, (M, N), 16))
        pad = lambda m: np.pad(m, ((0, 4 - min(m.shape[0], 3)), (0, 4 - min(m.shape[1], 3))), constant_values=np.nan)
        a, b = (self.x.A.T if tA else self.x.A), (self.x.B.T if tB else self.x.B)
        self.A, self.B = operand(pad(a), PADS["A"]), operand(pad(b), PADS["B"])       # never empty, NaN where no operand is
        self.bias = vector(np.concatenate([self.x.bias, [np.nan]]))
        self.e0, self.e1 = operand(pad(self.x.e0), PADS["e0"]), operand(pad(self.x.e1), PADS["e1"])
        self.o = Out(max(M, 1), max(N, 1))
        self.ws = torch.full((max(ws_floats, 1),), GR.SENT, dtype=torch.float32, device="cuda")
        self.args = dict(tA=tA, tB=tB, M=M, N=N, K=K, A=self.A.data_ptr(), lda=self.A.stride(0), B=self.B.data_ptr(),
                         ldb=self.B.stride(0), C=self.o.out.data_ptr(), ldc=self.o.out.stride(0), epi=GR.EPIS.index(epi),
                         bias=self.bias.data_ptr(), e0=self.e0.data_ptr(), lde0=self.e0.stride(0), e1=self.e1.data_ptr(),
                         lde1=self.e1.stride(0), split=split, ws=self.ws.data_ptr() if ws_floats else None,
                         aux=self.o.aux.data_ptr())

    def call(self, **change):
        a = dict(self.args, **change)
        st = self.lib.rec_gemm_f32(a["tA"], a["tB"], a["M"], a["N"], a["K"], a["A"], a["lda"], a["B"], a["ldb"], a["C"],
                                   a["ldc"], a["epi"], a["bias"], a["e0"], a["lde0"], a["e1"], a["lde1"], a["split"], a["ws"],
                                   a["aux"], stream())
        torch.cuda.synchronize()
        return st

    def untouched(self):
        return (bool((self.o.cbuf == GR.SENT).all()) and bool((self.o.abuf == GR.SENT).all())
                and bool((self.ws == GR.SENT).all()))


def test_argument_errors_write_nothing(abi):
    g = Abi(abi, 0, 0, 5, 3, 2, ws_floats=4 * 5 * 3)
    E_ARG, E_WS = g.lim["REC_E_ARG"], g.lim["REC_E_WORKSPACE"]
    lda, ldb, ldc = g.args["lda"], g.args["ldb"], g.args["ldc"]
    bad = [dict(A=None), dict(B=None), dict(C=None), dict(M=-1), dict(N=-1), dict(K=-1), dict(epi=-1), dict(epi=7),
           dict(epi=5, e0=None), dict(epi=5, e1=None), dict(epi=6, e1=None), dict(lda=1), dict(ldb=2), dict(ldc=2),
           dict(tA=1, lda=4), dict(tB=1, ldb=1)]
    bad += [dict(epi=e, bias=None) for e in (1, 2, 3, 4, 5)]
    assert lda >= 5 and ldb >= 3 and ldc >= 3                    # what the last two change is only the layout flag
    for change in bad:
        assert g.call(**change) == E_ARG, change
        assert g.untouched(), change
    assert g.call(split=4, ws=None) == E_WS and g.untouched()
    assert g.call(split=2, ws=None, epi=0) == E_WS and g.untouched()
    # the smallest leading dimensions are accepted: A [5,2] and B [2,3] contiguous inside the same buffers
    assert g.call(epi=0, lda=2, ldb=3, ldc=3, split=0) == g.lim["REC_OK"]


@pytest.mark.parametrize("M,N", [(0, 3), (5, 0), (0, 0)])
def test_empty_output_is_accepted_and_writes_nothing(abi, M, N):
    g = Abi(abi, 0, 0, M, N, 2, ws_floats=64)
    for change in (dict(), dict(epi=0), dict(split=4), dict(tA=1, lda=max(M, 1)), dict(tB=1)):
        assert g.call(**change) == g.lim["REC_OK"], change
        assert g.untouched(), change


@pytest.mark.parametrize("tA,tB,M,N,kernel", [(0, 0, 5, 3, "tile64"), (1, 0, 70, 65, "tile64"), (0, 1, 5, 3, "tile64"),
                                              (0, 0, 257, 8, "skinny"), (0, 0, 256, 33, "skinny"),
                                              (0, 0, 8193, 65, "panel"), (0, 1, 8192, 129, "panel")])
def test_an_empty_sum_is_zero(abi, tA, tB, M, N, kernel):
    """K = 0 with valid pointers: C = epi(0)"""
    assert GR.gemm_path(tA, tB, M, N, 0, 1).kernel == kernel
    for epi in GR.EXACT_EPIS:
        g = Abi(abi, tA, tB, M, N, 0, epi=epi)
        assert g.call() == g.lim["REC_OK"]
        ref, u = GR.exact_reference(g.x, epi)                    # (aux is written by the cross epilogue alone)
        assert epi != "none" or not ref.any()
        ec, ea = g.o.expected(ref, u)
        assert same_bits(g.o.cbuf, ec) and same_bits(g.o.abuf, ea), (kernel, epi)


def test_a_collapsed_request_leaves_its_workspace_alone(abi):
    M, N, K = 48, 32, 16
    assert GR.gemm_path(1, 0, M, N, K, 4).split_k == 1 and GR.gemm_path(1, 0, M, N, 2 * K, 4).split_k == 2
    for k, used in ((K, False), (2 * K, True)):
        g = Abi(abi, 1, 0, M, N, k, epi="cross", split=4, ws_floats=4 * M * N)
        assert g.call() == g.lim["REC_OK"]
        ref, u = GR.exact_reference(g.x, "cross")
        ec, ea = g.o.expected(ref, u)
        assert same_bits(g.o.cbuf, ec) and same_bits(g.o.abuf, ea)
        assert bool((g.ws == GR.SENT).all()) == (not used)
        if used:                                                 # two slices of M x N floats and nothing behind them
            assert bool((g.ws[2 * M * N:] == GR.SENT).all()) and not bool((g.ws[:2 * M * N] == GR.SENT).any())
