"""The dispatcher of rec_gemm_f32 (csrc/gemm.hip) and of ops.gemm / ops.split_k_for restated for the tests, inputs whose
product has ONE fp32 answer in any summation order, a derived per-element bound for real-valued inputs, numpy restatements
of eleven wrong kernels, and the case tables.  No GPU and no package import here: numpy alone.

C holds every constant the dispatcher reads, so that tests/test_gemm_classes_host.py can compare it with the source.

gemm_path()   split-K normalisation (kchunk rounded up to BK, split_k = ceil(K / kchunk): a request can shrink, down to 1
              with a workspace that is then unused), then in the order of the source: skinny (row-major operands, N <= 64,
              M >= 256, one slice; NT = 1 up to 32 columns), panel (row-major A, one slice, N > 64; one column panel at
              M >= 64 * 128, or 2..64 of them of ncp columns at K <= 256 with >= 192 workgroups), big (M, N > 64 and
              >= 160 tiles x slices of 128 x 128), else tile64.  split_k=None is what ops.gemm does: 1 on a skinny shape,
              split_k_for() elsewhere.

Exact inputs.  A and B hold multiples of 1/8 in [-1, 1], bias, e0 and e1 multiples of 1/8 in [-2, 2].  A product is a
multiple of 1/64 of magnitude <= 1, so every partial sum of any subset of the K products is a multiple of 1/64 of magnitude
<= K: exactly representable in fp32 while 64 K < 2^24, K < 2^18.  Every fp32 evaluation of the dot product -- any order,
fused or not, in slices or not -- therefore commits no rounding at all and ends on the float64 result.  u = acc + bias is a
multiple of 1/64 with |u| <= K + 2; max(u, 0) and acc + e1 likewise.  The cross epilogue e0 * u + e1 is a multiple of 1/512
of magnitude <= 2 (K + 2) + 2, exact (product, sum, or one fused multiply-add) while 512 (2 K + 6) < 2^24, K < 16381: the
deepest case here has K = 4096.  For NONE, BIAS, BIAS_RELU, CROSS (with aux = u) and ADD the expected output is the float64
result cast to fp32 and the assertion is bit equality.

Sigmoid and tanh.  On the same inputs u is exact, so the only error is the activation's: sigmoid within 6 u32 absolute
(U = 2^-24; expf within 2 ulp moves p by p (1 - p) 4 U <= U, 1 + e rounds: p U, the quotient within 2 ulp: 4 U p -- the
derivation of "ffm prob" in tests/interaction_classes_ref.py with an exact argument), tanh within the 2e-5 absolute that
tests/test_gpu_ops.py::test_gemm_epilogues uses.  To keep |u| of order 1 the activation runs divide A by 8 when K > 4
and B by 8 as well when K > 256 (multiples of 1/4096 of magnitude <= K / 64: still exact): |u| <= 6 up to K = 4,
<= K / 8 + 2 with a standard deviation below 0.75 up to K = 256, below 0.4 beyond; the host test holds max |u| <= 8.

Real-valued inputs (standard normal).  U = 2^-24, gamma(k) = k U / (1 - k U).  A sum of K products evaluated in fp32 in ANY
order is within gamma(K) (|A| |B|)_ij of the exact one: a product passes its own rounding and at most K - 1 additions.
  acc   |C_ij - ref_ij| <= gamma(K + c) (|A| |B|)_ij + ulp32(ref_ij), c the extra additions the path's text shows:
          tile64, big, panel   c = 0   one chain a slice
          skinny               c = 2   (part[0] + part[1]) + (part[2] + part[3]): two additions on top of a wave's chain
          split-K              c = ceil(split / 4) + 2   a slice's partial enters one of four chains (a0 += ws[z]: at most
                               ceil(split / 4) additions) and then the tree (a0 + a1) + (a2 + a3): two more
  bias  c + 1: u = acc + bias[gn] is one more addition (the bound of u = aux, with ulp32(u))
  cross C = e0 u^ + e1 with |u^ - u| <= b_u: the two further roundings of the issue's "+2" (the product, the sum; one if
        fused) act on e0 u and on C, not on the dot product, so they are carried where they act:
        |C - ref| <= |e0| b_u + gamma(2) |e0| (|u| + b_u) + ulp32(ref)
ulp32(x) >= U |x| covers the final rounding of each.
"""
import collections
import functools
import zlib

import numpy as np

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
SENT = -777.25                       # what every canary holds
PADC = 3                             # canary columns the restated kernels write into a buffer of N + PADC columns

Consts = collections.namedtuple(
    "Consts", "BM BN BK LM LN LK PNB PMt PKt EDGE BIG_MIN SKINNY_N SKINNY_M SKINNY_NT1 SKINNY_ROWS PANEL_ROWS PANEL_MAX_COLS "
              "PANEL_MAX_K PANEL_MIN_WG SK_MIN_K SK_MAX_TILES SK_FEW SK_SLOTS_FEW SK_SLOTS SK_MAX SK_MIN_DEPTH SK_WS_BYTES "
              "SK_CAP_MIN")
C = Consts(BM=64, BN=64, BK=16,              # tile64; BK is also the unit of kchunk
           LM=128, LN=128, LK=16,            # big
           PNB=28, PMt=64, PKt=16,           # panel: column blocks of 32 a panel, rows a workgroup, slab depth
           EDGE=64,                          # big and panel want N > EDGE (big: M too); split_k_for picks its tile by it
           BIG_MIN=160,                      # fewest 128 x 128 tiles x slices of the big kernel
           SKINNY_N=64, SKINNY_M=256, SKINNY_NT1=32, SKINNY_ROWS=32,
           PANEL_ROWS=64 * 128,              # fewest rows of a one-column-panel launch
           PANEL_MAX_COLS=64, PANEL_MAX_K=256, PANEL_MIN_WG=192,
           SK_MIN_K=1024, SK_MAX_TILES=512, SK_FEW=16, SK_SLOTS_FEW=512, SK_SLOTS=768, SK_MAX=256, SK_MIN_DEPTH=64,
           SK_WS_BYTES=64 << 20, SK_CAP_MIN=8)

EPIS = ("none", "bias", "relu", "sigmoid", "tanh", "cross", "add")      # in the order of the REC_EPI_* codes, 0..6
EXACT_EPIS = ("none", "bias", "relu", "cross", "add")
SIGMOID_BOUND = 6 * U
TANH_BOUND = 2e-5


def cdiv(a, b):
    return -(-a // b)


# ---- dispatch -------------------------------------------------------------------------------------------------------
Path = collections.namedtuple(
    "Path", "kernel TA TB NT MAXB ncol_panels ncp split_k kchunk partial_rows ktail kfull0 kfull1 narrow_last straddle "
            "empty_waves last_depth")


def split_k_for(K, M, N, k=C):
    """ops.split_k_for"""
    t = k.LM if (M > k.EDGE and N > k.EDGE) else k.BM
    tiles = cdiv(M, t) * cdiv(N, t)
    if tiles >= k.SK_MAX_TILES or K < k.SK_MIN_K:
        return 1
    slots = k.SK_SLOTS_FEW if tiles < k.SK_FEW else k.SK_SLOTS
    split = max(1, min(k.SK_MAX, slots // max(tiles, 1), K // k.SK_MIN_DEPTH))
    cap = max(k.SK_CAP_MIN, k.SK_WS_BYTES // max(1, 4 * M * N))
    return int(min(split, cap))


def skinny_ranges(K, k=C):
    """[k_begin, k_end) of the four waves of the skinny kernel"""
    kper = cdiv(cdiv(K, 16), 4) * 16
    return [(w * kper, max(w * kper, min(w * kper + kper, K))) for w in range(4)]


def gemm_path(transA, transB, M, N, K, split_k=None, k=C):
    """what rec_gemm_f32 launches for a call that passes its argument checks with M, N >= 1; ``split_k`` None: as ops.gemm
    chooses it"""
    tA, tB = int(bool(transA)), int(bool(transB))
    if split_k is None:
        skinny = (not tA) and (not tB) and N <= k.SKINNY_N and M >= k.SKINNY_M
        split_k = 1 if skinny else split_k_for(K, M, N, k)
    split, kchunk = max(1, int(split_k)), K
    if split > 1:
        kchunk = max(k.BK, cdiv(cdiv(K, split), k.BK) * k.BK)
        split = max(1, cdiv(K, kchunk))
    last_depth = K - (split - 1) * kchunk
    big = M > k.EDGE and N > k.EDGE and cdiv(M, k.LM) * cdiv(N, k.LN) * split >= k.BIG_MIN
    ncol = 1 if N <= k.PNB * 32 else cdiv(N, k.PNB * 32)
    ncp = 0 if ncol == 1 else cdiv(cdiv(N, ncol), 32) * 32
    panel = (not tA) and split == 1 and N > k.EDGE and (
        (ncol == 1 and M >= k.PANEL_ROWS) or
        (1 < ncol <= k.PANEL_MAX_COLS and K <= k.PANEL_MAX_K and cdiv(M, k.PMt) * ncol >= k.PANEL_MIN_WG))
    none = dict(NT=0, MAXB=0, ncol_panels=0, ncp=0, kfull0=False, kfull1=False, narrow_last=False, straddle=False,
                empty_waves=0)
    if (not tA) and (not tB) and N <= k.SKINNY_N and M >= k.SKINNY_M and split == 1:
        ranges = skinny_ranges(K, k)
        none.update(NT=1 if N <= k.SKINNY_NT1 else 2, empty_waves=sum(b >= K for b, _ in ranges))
        return Path(kernel="skinny", TA=0, TB=0, split_k=1, kchunk=K, partial_rows=M % k.SKINNY_ROWS != 0,
                    ktail=K % 16, last_depth=K, **none)
    if panel:
        none.update(MAXB=cdiv(cdiv(ncp if ncp else N, 32), 4), ncol_panels=ncol, ncp=ncp, kfull0=K < k.PKt,
                    kfull1=K // k.PKt == 1, narrow_last=ncol > 1 and N - (ncol - 1) * ncp < ncp)
        return Path(kernel="panel", TA=0, TB=tB, split_k=1, kchunk=K, partial_rows=M % k.PMt != 0, ktail=K % k.PKt,
                    last_depth=K, **none)
    if big:
        none.update(straddle=bool((tA and M % 4) or ((not tB) and N % 4)))
        return Path(kernel="big", TA=tA, TB=tB, split_k=split, kchunk=kchunk, partial_rows=M % k.LM != 0,
                    ktail=last_depth % k.LK, last_depth=last_depth, **none)
    return Path(kernel="tile64", TA=tA, TB=tB, split_k=split, kchunk=kchunk, partial_rows=M % k.BM != 0,
                ktail=last_depth % k.BK, last_depth=last_depth, **none)


def instance(p):
    """the template instance(s) a Path launches, as the case tables name them"""
    if p.kernel == "skinny":
        return "skinny<%d>" % p.NT
    if p.kernel == "panel":
        return "panel<0,%d,%d>" % (p.TB, p.MAXB) + ("x%d" % p.ncol_panels if p.ncol_panels > 1 else "")
    return "%s<%d,%d>" % (p.kernel, p.TA, p.TB) + ("+reduce%d" % p.split_k if p.split_k > 1 else "")


ALL_INSTANCES = (["tile64<%d,%d>" % (a, b) for a in (0, 1) for b in (0, 1)] + ["skinny<1>", "skinny<2>"] +
                 ["big<%d,%d>" % (a, b) for a in (0, 1) for b in (0, 1)] +
                 ["panel<0,%d,%d>" % (b, m) for b in (0, 1) for m in range(1, 8)] + ["reduce"])


def instances_of(p):
    """members of ALL_INSTANCES a Path runs"""
    name = instance(p).split("+")[0].split("x")[0]
    return [name] + (["reduce"] if p.split_k > 1 else [])


def k_ranges(p, K):
    """the k ranges whose partial sums the path adds: the slices of split-K, the four waves of the skinny kernel"""
    if p.kernel == "skinny":
        return skinny_ranges(K)
    return [(z * p.kchunk, min(K, (z + 1) * p.kchunk)) for z in range(p.split_k)]


def extra_additions(p):
    """c of the real-valued bound, see the module docstring"""
    if p.kernel == "skinny":
        return 2
    return cdiv(p.split_k, 4) + 2 if p.split_k > 1 else 0


# ---- case tables ----------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name cls tA tB M N K split")
LAYOUTS = ((0, 0), (0, 1), (1, 0), (1, 1))
LAYOUT_NAME = {(0, 0): "nn", (0, 1): "nt", (1, 0): "tn", (1, 1): "tt"}


def _case(prefix, cls, tA, tB, M, N, K, split=None):
    name = "%s_%s_%dx%dx%d" % (prefix, LAYOUT_NAME[tA, tB], M, N, K) + ("_s%d" % split if split else "")
    return Case(name, cls, tA, tB, M, N, K, split)


TILE_CASES = [_case("tile", "tile64<%d,%d>" % (a, b), a, b, M, N, K)
              for a, b in LAYOUTS
              for M, N, K in [(5, 3, 2), (64, 64, 16), (65, 65, 17), (130, 70, 1), (1, 1, 1), (77, 1, 8), (70, 70, 15),
                              (70, 70, 16), (70, 70, 17), (70, 70, 31), (70, 70, 33)]]

SKINNY_K = (1, 15, 16, 17, 47, 48, 49, 63, 64, 65, 129)
SKINNY_CASES = (
    # every K at one ragged shape of each instance, every (M, N) at a K whose four waves all work and at one where three idle
    [_case("skinny", "skinny<1>", 0, 0, 257, 31, K) for K in SKINNY_K] +
    [_case("skinny", "skinny<2>", 0, 0, 287, 63, K) for K in SKINNY_K] +
    [_case("skinny", "skinny<1>", 0, 0, M, N, K) for M in (256, 257, 287) for N in (1, 31, 32) for K in (49, 15)
     if (M, N) != (257, 31)] +
    [_case("skinny", "skinny<2>", 0, 0, M, N, K) for M in (256, 257, 287) for N in (33, 63, 64) for K in (49, 15)
     if (M, N) != (287, 63)])

BIG_CASES = (
    [_case("big", "big<0,0>", 0, 0, 1665, 1665, 19),            # 196 tiles
     _case("big", "big<0,0>", 0, 0, 1663, 1665, 1),
     _case("big", "big<0,0>", 0, 0, 1664, 1665, 16),            # one slice, no K tail, full row blocks
     _case("big", "big<0,1>", 0, 1, 1663, 1665, 15),
     _case("big", "big<0,1>", 0, 1, 1665, 1663, 35),
     _case("big", "big<1,0>", 1, 0, 1665, 1663, 17),
     _case("big", "big<1,0>", 1, 0, 1664, 1664, 16),            # full row blocks, no piece straddles an edge
     _case("big", "big<1,1>", 1, 1, 1663, 1663, 35),
     _case("big", "big<1,1>", 1, 1, 1665, 1665, 16),
     # the neighbours of the column-panel cases that must not take the panel path
     _case("near_panel", "big<0,1>", 0, 1, 6080, 897, 5),       # 95 x 2 = 190 workgroups
     _case("near_panel", "big<0,0>", 0, 0, 4096, 1793, 257)] +  # K above 256
    [_case("big", "big<%d,%d>+reduce%d" % (a, b, s), a, b, 129, 129, K, s)
     for a, b in LAYOUTS for K, s in ((640, 40), (641, 41))] +  # kchunk 16, 160 / 164 tiles x slices; a last slice of one k
    [_case("big", "big<1,0>+reduce43", 1, 0, 129, 129, 688, 43)])   # 43 = 4 * 10 + 3: the reduce's third remainder line

_PANEL_N = ((65, 1), (128, 1), (129, 2), (257, 3), (385, 4), (513, 5), (641, 6), (769, 7), (896, 7))
_PANEL_M = (8192, 8193, 8255)
PANEL_CASES = (
    # every MAXB with both TB at a tail-only, an exact and a ragged K; M takes its three values in turn
    [_case("panel", "panel<0,%d,%d>" % (tb, mb), 0, tb, _PANEL_M[(i + j + tb) % 3], N, K)
     for i, (N, mb) in enumerate(_PANEL_N) for tb in (0, 1)
     for j, K in enumerate((7, (16, 32)[(i + tb) % 2], (33, 53, 17)[(i + tb) % 3]))] +
    # every K at two values of N
    [_case("panel", "panel<0,%d,%d>" % (tb, mb), 0, tb, 8193, N, K)
     for N, mb, tb in ((65, 1, 1), (129, 2, 0)) for K in (1, 7, 15, 16, 17, 32, 33, 53)] +
    # several column panels
    [_case("panels", "panel<0,1,4>x2", 0, 1, 6081, 897, 5),     # ncp 480, the last one 417 wide
     _case("panels", "panel<0,0,5>x3", 0, 0, 4096, 1793, 37),   # ncp 608, the last one 577 wide
     _case("panels", "panel<0,0,7>x64", 0, 0, 129, 56449, 5),   # the upper limit; the last panel is one column
     _case("panels", "panel<0,1,7>x64", 0, 1, 129, 56449, 5),
     _case("panels", "panel<0,0,4>x2", 0, 0, 6100, 960, 16)])   # two full panels of 480
PANEL_CASES = list(collections.OrderedDict((c.name, c) for c in PANEL_CASES).values())

SPLIT_CASES = (
    # (48,32,K) TN: effective slice counts 1 (the request collapses), 2, 3, 4, 5, 7, 8: every remainder of the reduce's
    # four-chain loop; then a last slice of one k, a request that shrinks to 3 slices, a ragged last slice
    [_case("split", "tile64<1,0>" + ("+reduce%d" % eff if eff > 1 else ""), 1, 0, 48, 32, K, s)
     for K, s, eff in ((16, 4, 1), (32, 2, 2), (48, 3, 3), (64, 4, 4), (80, 5, 5), (112, 7, 7), (128, 8, 8), (65, 5, 5),
                       (40, 8, 3), (100, 7, 7))] +
    [_case("split", "tile64<0,0>+reduce7", 0, 0, 48, 32, 100, 7),
     _case("split", "tile64<0,1>+reduce5", 0, 1, 70, 33, 65, 5),
     _case("split", "tile64<1,1>+reduce3", 1, 1, 65, 70, 40, 8),
     _case("split", "tile64<1,0>+reduce64", 1, 0, 70, 70, 4096, 64)])   # the deepest exact case

ALL_CASES = TILE_CASES + SKINNY_CASES + BIG_CASES + PANEL_CASES + SPLIT_CASES
BY_NAME = {c.name: c for c in ALL_CASES}
assert len(BY_NAME) == len(ALL_CASES)

# one case a kernel for the real-valued bound and for the poison footprint; the panel kernel once per ncp regime
REAL_CASES = ("tile_tn_65x65x17", "skinny_nn_287x63x129", "skinny_nn_257x31x65", "big_nt_1665x1663x35",
              "big_tn_129x129x641_s41", "panel_nt_8193x65x33", "panel_nn_8193x129x53", "panels_nt_6081x897x5",
              "panels_nn_4096x1793x37", "split_tn_48x32x100_s7")
REAL_EPIS = ("none", "bias", "cross")


def path_of(c):
    return gemm_path(c.tA, c.tB, c.M, c.N, c.K, c.split)


# ---- inputs ---------------------------------------------------------------------------------------------------------
Inputs = collections.namedtuple("Inputs", "A B bias e0 e1")        # A [M,K], B [K,N] (the logical operands), e* [M,N]


def _rng(name, salt):
    return np.random.Generator(np.random.PCG64(zlib.crc32(("%s/%s" % (name, salt)).encode())))


def dyadic(r, shape, span):
    return r.integers(-span, span + 1, size=shape, dtype=np.int8) * F32(0.125)


@functools.lru_cache(maxsize=4)
def exact_input(name):
    c, r = BY_NAME[name], _rng(name, "exact")
    return Inputs(dyadic(r, (c.M, c.K), 8), dyadic(r, (c.K, c.N), 8), dyadic(r, (c.N,), 16), dyadic(r, (c.M, c.N), 16),
                  dyadic(r, (c.M, c.N), 16))


def activation_scale(K):
    """(scale of A, scale of B) of the sigmoid and tanh runs"""
    return (0.125 if K > 4 else 1.0), (0.125 if K > 256 else 1.0)


@functools.lru_cache(maxsize=2)
def real_input(name):
    c, r = BY_NAME[name], _rng(name, "real")
    n = lambda *s: r.normal(size=s).astype(F32)
    return Inputs(n(c.M, c.K), n(c.K, c.N), n(c.N), n(c.M, c.N), n(c.M, c.N))


# ---- references ------------------------------------------------------------------------------------------------------
def product64(x):
    return x.A.astype(F64) @ x.B.astype(F64)


def reference(x, epi, acc=None):
    """float64 (C, aux): aux is u = acc + bias for the cross epilogue, else None; ``acc``: product64(x), if at hand"""
    acc = product64(x) if acc is None else acc
    u = acc + x.bias.astype(F64)[None, :]
    if epi == "none":
        return acc, None
    if epi == "bias":
        return u, None
    if epi == "relu":
        return np.maximum(u, 0.0), None
    if epi == "sigmoid":
        return 1.0 / (1.0 + np.exp(-u)), None
    if epi == "tanh":
        return np.tanh(u), None
    if epi == "cross":
        return x.e0.astype(F64) * u + x.e1, u
    if epi == "add":
        return acc + x.e1, None
    raise ValueError(epi)


def exact_reference(x, epi, acc=None):
    """reference() as the one fp32 answer of the exact inputs; asserts that the cast loses nothing"""
    out = []
    for v in reference(x, epi, acc):
        if v is not None:
            assert np.array_equal(v.astype(F32).astype(F64), v), "the exact inputs left fp32"
            v = v.astype(F32)
        out.append(v)
    return tuple(out)


def gamma(n):
    return n * U / (1 - n * U)


def ulp32(x):
    return np.spacing(np.abs(x).astype(F32)).astype(F64)


def real_bounds(x, p, epi):
    """(bound of C, bound of aux or None) for real-valued inputs on Path ``p``; the module docstring derives them"""
    K = x.A.shape[1]
    c = extra_additions(p)
    sabs = np.abs(x.A).astype(F64) @ np.abs(x.B).astype(F64)
    ref, u = reference(x, epi)
    if epi == "none":
        return gamma(K + c) * sabs + ulp32(ref), None
    if epi == "bias":
        return gamma(K + c + 1) * sabs + ulp32(ref), None
    if epi == "cross":
        bu = gamma(K + c + 1) * sabs + ulp32(u)
        e0 = np.abs(x.e0).astype(F64)
        return e0 * bu + gamma(2) * e0 * (np.abs(u) + bu) + ulp32(ref), bu
    raise ValueError(epi)


def ratio(got, ref, bound):
    """the worst |got - ref| / bound; inf where got is not finite"""
    got = np.asarray(got, F64)
    if not np.isfinite(got).all():
        return np.inf
    return float((np.abs(got - ref) / bound).max()) if got.size else 0.0


# ---- fp32 evaluations of the product in three orders ------------------------------------------------------------------
ORDERS = ("blas", "chain", "slabs")


def f32_product(A, B, order):
    """A @ B in fp32: numpy's own product, a k-ascending chain of separately rounded multiply-adds, and 16-deep slabs
    summed from the last one down"""
    A, B = np.ascontiguousarray(A, F32), np.ascontiguousarray(B, F32)
    M, K = A.shape
    if order == "blas":
        return A @ B
    acc = np.zeros((M, B.shape[1]), F32)
    if order == "chain":
        for k in range(K):
            acc += A[:, k:k + 1] * B[k:k + 1, :]
        return acc
    for k0 in reversed(range(0, K, 16)):
        acc += A[:, k0:k0 + 16] @ B[k0:k0 + 16]
    return acc


def f32_epilogue(acc, x, epi):
    """(C, aux) of an exact or real-valued epilogue, every operation rounded to fp32"""
    acc = np.asarray(acc, F32)
    if epi == "none":
        return acc, None
    if epi == "add":
        return acc + x.e1, None
    u = acc + x.bias[None, :]
    if epi == "bias":
        return u, None
    if epi == "relu":
        return np.maximum(u, F32(0)), None
    return x.e0 * u + x.e1, u


# ---- wrong kernels ----------------------------------------------------------------------------------------------------
# families a mutant can occur on: every kernel writes C and has an epilogue; a tail slab needs a k range that is no
# multiple of 16; slices need the reduce; column offsets need several column panels
FAMILIES = ("tile64", "skinny", "big", "panel", "panels", "reduce")
MUTANTS = collections.OrderedDict([
    ("drop_tail_k", ("tile64", "skinny", "big", "panel", "panels")),     # the last k of a tail slab
    ("skip_last_slice", ("reduce",)),
    ("skip_z2", ("reduce",)),                                            # `if (z + 2 < split) a2 += ...` missing
    ("c_transposed_32", ("tile64", "skinny", "big", "panel", "panels", "reduce")),
    ("bias_gm", ("tile64", "skinny", "big", "panel", "panels", "reduce")),
    ("e_swapped", ("tile64", "skinny", "big", "panel", "panels", "reduce")),
    ("aux_ld_n", ("tile64", "skinny", "big", "panel", "panels", "reduce")),
    ("row_guard_le", ("tile64", "skinny", "big", "panel", "panels", "reduce")),
    ("last_panel_ncp", ("panels",)),                                     # the last column panel computed with N = ncp
    ("no_noff", ("panels",)),                                            # bias / e1 not moved by n_off
    ("relu_before_bias", ("tile64", "skinny", "big", "panel", "panels", "reduce")),
])
MUTANT_EPI = {"drop_tail_k": "none", "skip_last_slice": "none", "skip_z2": "none", "c_transposed_32": "none",
              "bias_gm": "bias", "e_swapped": "cross", "aux_ld_n": "cross", "row_guard_le": "none",
              "last_panel_ncp": "none", "no_noff": "cross", "relu_before_bias": "relu"}


def family(p):
    if p.kernel == "panel":
        return "panels" if p.ncol_panels > 1 else "panel"
    return p.kernel


def families_of(p):
    return [family(p)] + (["reduce"] if p.split_k > 1 else [])


def restated(c, x, epi, mut=None):
    """(C buffer, aux buffer), float32 [M + 1, N + PADC] each, as the kernels of case ``c`` leave them on inputs ``x``:
    canaries SENT in the row after the last and in the PADC columns after N, the leading dimension of both N + PADC.  The
    arithmetic is float64 (exact on the exact inputs; on real-valued ones a mutant is not a matter of rounding).  ``mut``
    names a wrong kernel."""
    p, (M, N, K) = path_of(c), (c.M, c.N, c.K)
    A, B = x.A.astype(F64), x.B.astype(F64)
    parts = []
    for k0, k1 in k_ranges(p, K):
        if mut == "drop_tail_k" and k1 > k0 and (k1 - k0) % 16:
            k1 -= 1
        parts.append(A[:, k0:k1] @ B[k0:k1])
    if p.split_k > 1:
        if mut == "skip_last_slice":
            parts = parts[:-1]
        if mut == "skip_z2" and p.split_k % 4 == 3:
            del parts[p.split_k // 4 * 4 + 2]
    acc = np.sum(parts, axis=0)
    gm, gn = np.arange(M)[:, None], np.arange(N)[None, :]
    bias, e0, e1 = x.bias.astype(F64), x.e0.astype(F64), x.e1.astype(F64)
    brow = np.broadcast_to(bias[None, :], (M, N))
    if mut == "bias_gm":
        brow = np.broadcast_to(bias[gm % N], (M, N))
    if mut == "no_noff" and p.ncp:
        brow, e1 = brow[:, (gn % p.ncp)[0]], e1[:, (gn % p.ncp)[0]]
    if mut == "e_swapped":
        e0, e1 = e1, e0
    u = acc + brow
    out = {"none": acc, "bias": u, "relu": np.maximum(u, 0.0), "cross": e0 * u + e1, "add": acc + e1}[epi]
    if mut == "relu_before_bias" and epi == "relu":
        out = np.maximum(acc, 0.0) + brow
    if mut == "c_transposed_32":
        out = out.copy()
        for m0 in range(0, M - 31, 32):
            for n0 in range(0, N - 31, 32):
                out[m0:m0 + 32, n0:n0 + 32] = out[m0:m0 + 32, n0:n0 + 32].T.copy()
    ld = N + PADC
    Cb, auxb = np.full((M + 1, ld), SENT, F64), np.full((M + 1, ld), SENT, F64)
    Cb[:M, :N] = out
    zero = {"none": 0.0, "add": 0.0}.get(epi)                    # epi(0) of a row or column past the matrix
    if mut == "row_guard_le":
        Cb[M, :N] = 0.0 if zero is not None else bias
    if mut == "last_panel_ncp" and p.ncp:
        Cb[:M, N:min(ld, p.ncol_panels * p.ncp)] = 0.0
    if epi == "cross":
        if mut == "aux_ld_n":
            auxb.reshape(-1)[:M * N] = u.reshape(-1)
        else:
            auxb[:M, :N] = u
    return Cb.astype(F32), auxb.astype(F32)


def caught_exact(c, mut):
    """a wrong kernel writes other bits than the right one, on the exact inputs of the case"""
    x, epi = exact_input(c.name), MUTANT_EPI[mut]
    good, bad = restated(c, x, epi), restated(c, x, epi, mut)
    return any(not np.array_equal(g.view(np.uint32), b.view(np.uint32)) for g, b in zip(good, bad))


def caught_by_bound(c, mut):
    """a wrong kernel leaves the real-valued bound, or writes a canary"""
    x, epi, p = real_input(c.name), MUTANT_EPI[mut], path_of(c)
    if epi not in REAL_EPIS:
        return None
    Cb, auxb = restated(c, x, epi, mut)
    (ref, u), (bC, bu) = reference(x, epi), real_bounds(x, p, epi)
    M, N = c.M, c.N
    window = lambda b: b[:M, :N]
    canary = lambda b: np.concatenate([b[M], b[:M, N:].reshape(-1)])
    bad = ratio(window(Cb), ref, bC) > 1 or (canary(Cb) != F32(SENT)).any()
    if epi == "cross":
        bad = bad or ratio(window(auxb), u, bu) > 1 or (canary(auxb) != F32(SENT)).any()
    return bool(bad)
