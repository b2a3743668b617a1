"""The kernel classes of the "K12 Adam" family (csrc/dense_ops.hip: rec_adam_dense_f32, rec_adam_dense_multi_f32,
rec_adam_sparse_keras_f32, rec_adam_sparse_keras_pair_f32, rec_adam_rows_f32, rec_adam_lr_t_f32; the element forms
adam_touch / adam_decay / adam_dense_elem / adam_step_x of csrc/common.h) restated for the tests, an fp64 reference of one
step with its error bounds, a plain fp32 IEEE restatement with the mutants the bounds must catch, and the tables of cases.
No GPU and no package import here: numpy and the oracle alone.

K holds every constant the dispatch reads, so that tests/test_adam_classes_host.py can compare it with the source text.

sweep_class()   the dense sweep of rec_adam_sparse_keras_f32 is adam_sweep_vec_kernel (one float4 of a row per item) when
                E % 4 == 0, ld % 4 == 0 and var, m and v are 16-byte aligned, else adam_sweep_scalar_kernel (one float).
passes()        the three sweeps launch at most K.GRID_CAP workgroups of K.WG threads and loop: PASS_ITEMS items a pass.
pair_args_ok()  what rec_adam_sparse_keras_pair_f32 accepts; its sweep has E/4 + 1 items a row (the last one is w).

The reference is fp64 on the fp32 inputs.  Keras' own float32 scalars stay float32, they are semantics and not rounding
error: lr_t = oracle.layers_np.adam_lr_t(.., dt=float32), 1 - b1 and 1 - b2 formed in float32, eps as float32.

Bounds, u = 2^-23, den = sqrt(v_new) + eps, everything from the reference:
  m (touched, dense)   u (|b1 m| + |(1-b1) g|)               dense: u (|m| + |(1-b1)(g - m)|)
  v                    2 u v_new
  m, v (untouched)     one fp32 multiply each: float32(float64(m) b1) and float32(float64(v) b2) bit for bit
  var                  ulp32(x_ref) + lr_t bound(m) / den + 6 u |step_ref|
The last term is the contract of common.h (hardware square root and reciprocal: the step is off by about 3 ulp of itself,
plus the product and the fma).  The relative bounds of m and v presume normal numbers: the spacing of fp32 below 2^-126 is
2^-149 whatever the value, so both carry that one quantum (TINY) as a floor -- without it the correctly rounded
float32(1e-40 * b2) of a touched row with g = 0 would already be outside 2 u v_new.

Every case starts from m ~ 0.1 N(0,1), v ~ U(0, 0.1), var ~ N(0,1) and carries the special rows of SPECIAL: m = v = 0
(bit-identical when untouched), v = 1e-40 (a denormal), |var| = 1e-6, and a touched row with g = 0.  Row 3 is never touched
on purpose: the id 2^32 + 3 of the out-of-range regime aliases it once narrowed to 32 bits.
"""
import collections
import functools

import numpy as np

from oracle import layers_np as L

Consts = collections.namedtuple("Consts", "GRID_CAP WG VEC ALIGN ADAM_MULTI_MAX")
K = Consts(GRID_CAP=256 * 32,        # most workgroups a sweep launches
           WG=256,                   # threads of a workgroup, one item each a pass
           VEC=4,                    # floats of a vec item
           ALIGN=16,                 # bytes var, m and v are aligned to in the vec class and the pair entry point
           ADAM_MULTI_MAX=16)        # most tensors of one rec_adam_dense_multi_f32 call
ADAM_MULTI_MAX = K.ADAM_MULTI_MAX
PASS_ITEMS = K.GRID_CAP * K.WG       # 2,097,152
U = 2.0 ** -23
TINY = 2.0 ** -149
LR, B1, B2, EPS = 0.01, 0.9, 0.999, 1e-7
STEPS = (1, 2, 10, 1000, 100000)
REGIMES = ("cap0", "n0", "partial", "full", "oob")
SPECIAL = collections.OrderedDict(zero_u=5, zero_t=6, den_u=7, den_t=8, tiny_u=9, tiny_t=10, g0=11)
FIRST_FREE = 12                      # rows below hold the specials, row 3 and the always-touched row 0
ALIAS_ROW = 3
F32 = np.float32


# ---- dispatch -------------------------------------------------------------------------------------------------------
def sweep_class(E, ld, var_aligned=True, m_aligned=True, v_aligned=True):
    if E < 1 or ld < E:
        raise ValueError("rec_adam_sparse_keras_f32 takes E >= 1 and ld >= E")
    vec = E % K.VEC == 0 and ld % K.VEC == 0 and var_aligned and m_aligned and v_aligned
    return "vec" if vec else "scalar"


def items_per_row(cls, E):
    return {"vec": E // K.VEC, "scalar": E, "pair": E // K.VEC + 1}[cls]


def passes(items, k=K):
    """grid-stride passes of a sweep over ``items`` items"""
    return -(-items // (k.GRID_CAP * k.WG))


def pair_args_ok(E, ld, fused_aligned=True, m_aligned=True, v_aligned=True):
    return E > 0 and E % 4 == 0 and ld >= E + 1 and ld % 4 == 0 and bool(fused_aligned and m_aligned and v_aligned)


# ---- one step -------------------------------------------------------------------------------------------------------
Scal = collections.namedtuple("Scal", "lr_t b1 b2 omb1 omb2 eps")
Ref = collections.namedtuple("Ref", "x m v bx bm bv")
SparseRef = collections.namedtuple("SparseRef", "x m v bx bm bv touched")


def scalars(t, lr=LR, b1=B1, b2=B2, eps=EPS, dt=np.float64):
    """Keras' float32 scalars of step ``t``, held in ``dt``"""
    vals = (L.adam_lr_t(lr, b1, b2, t, dt=F32), F32(b1), F32(b2), F32(1) - F32(b1), F32(1) - F32(b2), F32(eps))
    assert all(type(x) is F32 for x in vals)
    return Scal(*[dt(x) for x in vals])


def ulp32(x):
    return np.spacing(np.abs(x).astype(F32)).astype(np.float64)


def _f64(*arrays):
    return [np.asarray(a, np.float64) for a in arrays]


def _finish(x, mn, vn, bm, bv, s):
    den = np.sqrt(vn) + s.eps
    step = s.lr_t * mn / den
    xn = x - step
    return Ref(xn, mn, vn, ulp32(xn) + s.lr_t * bm / den + 6 * U * np.abs(step), bm, bv)


def ref_touch(x, m, v, g, s):
    """adam_touch: m <- b1 m + (1-b1) g ; v <- b2 v + (1-b2) g^2 ; x <- x - lr_t m / (sqrt(v) + eps)"""
    x, m, v, g = _f64(x, m, v, g)
    mn, vn = s.b1 * m + s.omb1 * g, s.b2 * v + s.omb2 * g * g
    return _finish(x, mn, vn, U * (np.abs(s.b1 * m) + np.abs(s.omb1 * g)) + TINY, 2 * U * vn + TINY, s)


def ref_decay(x, m, v, s):
    """adam_decay: m <- b1 m ; v <- b2 v ; the same x.  m and v are exact products here: their float32 is what a
    kernel must give bit for bit (the sign of a zero included: -0.0 stays -0.0, which adding (1-b1) 0 would lose), bm and
    bv only feed the bound of x"""
    x, m, v = _f64(x, m, v)
    mn, vn = s.b1 * m, s.b2 * v
    return _finish(x, mn, vn, U * np.abs(mn) + TINY, 2 * U * vn + TINY, s)


def ref_dense(x, m, v, g, s):
    """adam_dense_elem: m <- m + (g - m)(1-b1) ; v <- v + (g^2 - v)(1-b2)"""
    x, m, v, g = _f64(x, m, v, g)
    mn, vn = m + (g - m) * s.omb1, v + (g * g - v) * s.omb2
    return _finish(x, mn, vn, U * (np.abs(m) + np.abs((g - m) * s.omb1)) + TINY, 2 * U * vn + TINY, s)


def valid_slots(ids, n_uniq, V):
    """(slots, rows) of the ids a kernel applies: below n_uniq and inside [0, V)"""
    head = np.asarray(ids[:n_uniq], np.int64)
    slots = np.nonzero((head >= 0) & (head < V))[0]
    return slots, head[slots]


def ref_sparse(x, m, v, ids, g, n_uniq, s, lazy=False):
    """One sparse step on [V,E] tables with the unique ids and their gradient rows as given.  ``lazy``: untouched rows
    stay (rec_adam_rows_f32), else they get the plain decay (Keras' dense sweep)."""
    V = x.shape[0]
    slots, rows = valid_slots(ids, n_uniq, V)
    touched = np.zeros(V, bool)
    touched[rows] = True
    if lazy:
        x64, m64, v64 = _f64(x, m, v)
        tiny = np.full(x64.shape, TINY)
        out = [x64.copy(), m64.copy(), v64.copy(), tiny, tiny.copy(), tiny.copy()]
    else:
        out = list(ref_decay(x, m, v, s))
    new = ref_touch(x[rows], m[rows], v[rows], g[slots], s)
    for a, b in zip(out, new):
        a[rows] = b
    return SparseRef(*out, touched)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _ratio(got, want, bound):
    if got.size == 0:
        return 0.0
    with np.errstate(invalid="ignore", over="ignore"):
        q = np.abs(got.astype(np.float64) - want) / bound
    q[~np.isfinite(got)] = np.inf
    return float(q.max())


def ratios(got_x, got_m, got_v, ref):
    """worst |got - ref| / bound of x (all rows) and of m and v (touched rows; every row of a Ref), and whether m and v
    of the untouched rows are the correctly rounded products bit for bit"""
    if isinstance(ref, SparseRef):
        t, u = ref.touched, ~ref.touched
        bits = bool(np.array_equal(_bits(got_m[u]), _bits(ref.m[u])) and np.array_equal(_bits(got_v[u]), _bits(ref.v[u])))
        return {"x": _ratio(got_x, ref.x, ref.bx), "m": _ratio(got_m[t], ref.m[t], ref.bm[t]),
                "v": _ratio(got_v[t], ref.v[t], ref.bv[t]), "bits": bits}
    return {"x": _ratio(got_x, ref.x, ref.bx), "m": _ratio(got_m, ref.m, ref.bm), "v": _ratio(got_v, ref.v, ref.bv),
            "bits": True}


# The share of each bound the fp32 restatement may use (tests/test_adam_classes_host.py).  x and v: 0.6.  m cannot have
# that room under the bound above, whatever evaluates it in fp32: fma(g, 1-b1, fl(m b1)) rounds twice, by up to
# 2^-24 |b1 m| and 2^-24 |m_new|, and |m_new| <= |b1 m| + |(1-b1) g| makes the sum reach
# u (|b1 m| + |(1-b1) g| / 2): the whole bound where (1-b1) g is small beside b1 m (0.91 of it on the cases here).  The
# same two roundings prove that the pinned sequence never leaves the bound, so a kernel outside it is still wrong.
ROOM = {"x": 0.6, "m": 1.0, "v": 0.6}


def has_room(r):
    return r["bits"] and all(r[k] <= ROOM[k] for k in ROOM)


def worst(r):
    return max(r["x"], r["m"], r["v"]) if r["bits"] else np.inf


def inside(r, share=1.0):
    return worst(r) <= share


# ---- the plain fp32 IEEE restatement and its mutants ------------------------------------------------------------------
MUTANTS = ("decay_then_touch", "unpatched", "eps_in_sqrt", "t_plus_1", "t_minus_1", "swap_b", "g_not_squared",
           "cap_slots", "narrow_ids", "one_pass", "pair_w_index")


def _fma(a, b, c):
    """float32 fma: the product of two float32 is exact in float64 (the sum is then rounded twice, to 53 and to 24 bits,
    which moves a result by one ulp in about one element of 2^29: nothing to the bounds)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F32)


def f32_touch(x, m, v, g, s, eps_in_sqrt=False, g_plain=False):
    """adam_touch as common.h pins it, with the correctly rounded square root and quotient of -DREC_ADAM_IEEE"""
    g = np.asarray(g, F32)
    mn = _fma(g, s.omb1, m * s.b1)
    vn = _fma(g if g_plain else g * g, s.omb2, v * s.b2)
    den = np.sqrt(vn + s.eps) if eps_in_sqrt else np.sqrt(vn) + s.eps
    return x - s.lr_t * mn / den, mn, vn


def f32_decay(x, m, v, s, eps_in_sqrt=False):
    mn, vn = m * s.b1, v * s.b2
    den = np.sqrt(vn + s.eps) if eps_in_sqrt else np.sqrt(vn) + s.eps
    return x - s.lr_t * mn / den, mn, vn


def f32_dense(x, m, v, g, s):
    mn = _fma(g - m, s.omb1, m)
    vn = _fma(_fma(g, g, -v), s.omb2, v)
    return x - s.lr_t * mn / (np.sqrt(vn) + s.eps), mn, vn


def f32_sparse(x, m, v, ids, g, n_uniq, t, mut=None, lazy=False, per_row=None, sweep_m=None):
    """One sparse step in float32, operation by operation as common.h pins them.  ``mut`` names one of MUTANTS;
    ``per_row`` (sweep items a row) places the end of the first pass for 'one_pass'; ``sweep_m`` replaces the m the sweep
    reads ('pair_w_index')."""
    with np.errstate(all="ignore"):
        s = scalars({"t_plus_1": t + 1, "t_minus_1": t - 1}.get(mut, t), dt=F32)
        if mut == "swap_b":
            s = s._replace(b1=s.b2, b2=s.b1, omb1=s.omb2, omb2=s.omb1)
        V = x.shape[0]
        head = np.asarray(ids[:len(ids) if mut == "cap_slots" else n_uniq], np.int64)
        if mut == "narrow_ids":
            head = head.astype(np.int32).astype(np.int64)
        slots = np.nonzero((head >= 0) & (head < V))[0]
        rows = head[slots]
        eps_in = mut == "eps_in_sqrt"
        if lazy:
            out = [x.copy(), m.copy(), v.copy()]
        else:
            out = list(f32_decay(x, m if sweep_m is None else sweep_m, v, s, eps_in))
            if mut == "one_pass":
                stop = -(-PASS_ITEMS // per_row)
                for a, b in zip(out, (x, m, v)):
                    a[stop:] = b[stop:]
        if mut != "unpatched":
            src = [a.copy() for a in out] if mut == "decay_then_touch" else (x, m, v)
            new = f32_touch(src[0][rows], src[1][rows], src[2][rows], g[slots], s, eps_in, mut == "g_not_squared")
            for a, b in zip(out, new):
                a[rows] = b
    assert all(a.dtype == F32 for a in out)
    return out


# ---- case tables ----------------------------------------------------------------------------------------------------
SparseCase = collections.namedtuple("SparseCase", "name V E ld off t order seed cls npass")
LazyCase = collections.namedtuple("LazyCase", "name V E ld t order seed")
PairCase = collections.namedtuple("PairCase", "name V E ld t order seed npass regimes")
DenseCase = collections.namedtuple("DenseCase", "name n t seed")
MultiCase = collections.namedtuple("MultiCase", "name sizes t seed")
SparseInput = collections.namedtuple("SparseInput", "ids g n_uniq cap")


def _sparse_cases():
    rows = [  # V, E, ld, float offsets of (var, m, v), class, passes
        (257, 4, 4, (0, 0, 0), "vec", 1), (1000, 16, 16, (0, 0, 0), "vec", 1), (1000, 16, 32, (0, 0, 0), "vec", 1),
        (300, 64, 64, (0, 0, 0), "vec", 1), (140001, 64, 64, (0, 0, 0), "vec", 2),
        (1000, 3, 3, (0, 0, 0), "scalar", 1), (1000, 1, 32, (0, 0, 0), "scalar", 1), (1000, 4, 5, (0, 0, 0), "scalar", 1),
        (1000, 20, 21, (0, 0, 0), "scalar", 1),
        (1000, 16, 16, (1, 0, 0), "scalar", 1), (1000, 16, 16, (0, 1, 0), "scalar", 1), (1000, 16, 16, (0, 0, 1), "scalar", 1),
        (700001, 3, 3, (0, 0, 0), "scalar", 2)]
    out = []
    for i, (V, E, ld, off, cls, npass) in enumerate(rows):
        name = "%s_%dx%dx%d" % (cls, V, E, ld) + ("_off" + "".join(str(o) for o in off) if any(off) else "")
        out.append(SparseCase(name, V, E, ld, off, STEPS[i % 5], ("asc", "first")[i % 2], 100 + i, cls, npass))
    return tuple(out)


SPARSE_CASES = _sparse_cases()
LAZY_CASES = tuple(LazyCase("lazy_%dx%d" % (E, ld), 1000, E, ld, STEPS[i % 5], ("first", "asc")[i % 2], 200 + i)
                   for i, (E, ld) in enumerate((E, ld) for E in (1, 3, 16) for ld in (E, 32)))
PAIR_CASES = tuple(PairCase("pair_%dx%dx%d" % (V, E, ld), V, E, ld, STEPS[(i + 1) % 5], ("asc", "first")[i % 2], 300 + i,
                            npass, regimes)
                   for i, (V, E, ld, npass, regimes) in enumerate((
                       (1000, 4, 8, 1, ("partial", "oob", "full")), (1000, 16, 32, 1, ("partial", "oob", "n0")),
                       (300, 64, 128, 1, ("partial", "oob", "cap0")), (1048700, 4, 8, 2, ("partial",)))))
DENSE_CASES = tuple(DenseCase("dense_%d" % n, n, STEPS[i % 5], 400 + i) for i, n in enumerate((1, 255, 256, 257, 70001)))
MULTI_CASES = (MultiCase("multi_1", (257,), 2, 500), MultiCase("multi_7", (1, 255, 256, 257, 1000, 3, 70), 10, 501),
               MultiCase("multi_16", (1, 255, 256, 257, 1000, 3, 2, 511, 512, 513, 64, 7, 300, 5, 129, 1), 1000, 502))
BY_NAME = {c.name: c for c in SPARSE_CASES + LAZY_CASES + PAIR_CASES + DENSE_CASES + MULTI_CASES}
assert len(BY_NAME) == len(SPARSE_CASES + LAZY_CASES + PAIR_CASES + DENSE_CASES + MULTI_CASES)
LR_T_NEAR, LR_T_FAR = (1, 2, 3, 10, 1000, 17000, 32768), (32769, 10 ** 6, 10 ** 7)
BIG_V = 2000                          # above it only the 'partial' regime runs on the CPU and ids sit at the edges


def state(V, E, seed):
    """(var, m, v) [V,E] float32 with the special rows of SPECIAL (tables of at least 16 rows)"""
    r = np.random.default_rng(seed)
    x = r.standard_normal((V, E), dtype=F32)
    m = r.standard_normal((V, E), dtype=F32) * F32(0.1)
    v = r.random((V, E), dtype=F32) * F32(0.1)
    if V >= 16:
        S = SPECIAL
        for row in (S["zero_u"], S["zero_t"]):
            m[row] = 0
            v[row] = 0
        for row in (S["den_u"], S["den_t"]):
            v[row] = F32(1e-40)
        for row in (S["tiny_u"], S["tiny_t"]):
            x[row] = F32(1e-6) * np.where(np.arange(E) % 2, -1, 1).astype(F32)
    return x, m, v


def pass_edges(V, per_row):
    """the first row of every grid-stride pass after the first"""
    return [b * PASS_ITEMS // per_row for b in range(1, passes(V * per_row))]


def touched_rows(V, per_row, order, seed):
    """The ids of a case: small tables a random third, large ones rows at both ends and around every pass edge (two of
    three rows, so that touched and untouched rows alternate there); always rows 0 and V-1 and the touched specials,
    never row 3 or the untouched specials."""
    r = np.random.default_rng(seed + 1)
    S = SPECIAL
    rows = {0, V - 1, S["zero_t"], S["den_t"], S["tiny_t"], S["g0"]}
    if V <= BIG_V:
        rows |= set(r.choice(np.arange(FIRST_FREE, V), size=min(V // 3, 150), replace=False).tolist())
    else:
        spans = [(FIRST_FREE, 100), (V - 100, V)] + [(e - 50, e + 50) for e in pass_edges(V, per_row)]
        rows |= {i for a, b in spans for i in range(max(a, FIRST_FREE), min(b, V)) if i % 3}
    rows = np.array(sorted(rows), np.int64)
    return rows if order == "asc" else r.permutation(rows)


def spare_rows(V, taken, n=8):
    """``n`` valid rows that no slot below n_uniq names (the ids of the unused slots)"""
    taken = set(np.asarray(taken).tolist()) | set(SPECIAL.values()) | {ALIAS_ROW}
    out = [i for i in range(V - 2, 0, -1) if i not in taken][:n]
    return np.array(out, np.int64)


def sparse_input(V, E, per_row, order, seed, regime):
    """ids [max(cap,1)], gradient rows [max(cap,1), E], n_uniq and cap of one regime of REGIMES.  Slots at or beyond
    n_uniq hold valid ids of untouched rows with NaN gradients."""
    r = np.random.default_rng(seed + 2)
    T = touched_rows(V, per_row, order, seed)
    if regime == "cap0":
        return SparseInput(np.zeros(1, np.int64), np.full((1, E), np.nan, F32), 0, 0)
    if regime == "full":
        ids = np.arange(V, dtype=np.int64) if order == "asc" else r.permutation(V).astype(np.int64)
    elif regime == "oob":
        ids = np.insert(T, [0, len(T) // 2, len(T)], [-1, V, 2 ** 32 + 3])
    else:
        ids = np.concatenate([T, spare_rows(V, T)])
    g = r.standard_normal((len(ids), E), dtype=F32)
    g[ids == SPECIAL["g0"]] = 0
    n_uniq = {"n0": 0, "partial": len(T)}.get(regime, len(ids))
    g[n_uniq:] = np.nan
    return SparseInput(ids, g, n_uniq, len(ids))


def regimes_of(case, gpu=True):
    if isinstance(case, PairCase):
        return case.regimes
    return REGIMES if gpu or case.V <= BIG_V else ("partial",)


@functools.lru_cache(maxsize=2)
def case_state(name):
    """the read-only starting state of a sparse, lazy or pair case: (var, m, v), for a pair case (embed.., w..)"""
    c = BY_NAME[name]
    out = state(c.V, c.E, c.seed)
    if isinstance(c, PairCase):
        out = out + state(c.V, 1, c.seed + 7)
    for a in out:
        a.setflags(write=False)
    return out


def case_input(name, regime):
    c = BY_NAME[name]
    if isinstance(c, PairCase):
        e = sparse_input(c.V, c.E, items_per_row("pair", c.E), c.order, c.seed, regime)
        gw = np.random.default_rng(c.seed + 3).standard_normal((len(e.ids), 1), dtype=F32)
        gw[e.ids == SPECIAL["g0"]] = 0
        gw[e.n_uniq:] = np.nan
        return e, gw
    cls = c.cls if isinstance(c, SparseCase) else "scalar"
    return sparse_input(c.V, c.E, items_per_row(cls, c.E), c.order, c.seed, regime)


def case_reference(name, regime):
    """SparseRef of a sparse or lazy case, (SparseRef of embed, SparseRef of w) of a pair case"""
    c, st, s = BY_NAME[name], case_state(name), scalars(BY_NAME[name].t)
    if isinstance(c, PairCase):
        e, gw = case_input(name, regime)
        return ref_sparse(*st[:3], e.ids, e.g, e.n_uniq, s), ref_sparse(*st[3:], e.ids, gw, e.n_uniq, s)
    i = case_input(name, regime)
    return ref_sparse(*st, i.ids, i.g, i.n_uniq, s, lazy=isinstance(c, LazyCase))


def case_f32(name, regime, mut=None):
    """the fp32 restatement of a case, in the layout of case_reference"""
    c, st = BY_NAME[name], case_state(name)
    if isinstance(c, PairCase):
        e, gw = case_input(name, regime)
        per_row = items_per_row("pair", c.E)
        sweep_m = None
        if mut == "pair_w_index":        # the w lane reads m_w at the index of the lane, not of the row
            sweep_m = st[4][(np.arange(c.V) * (per_row - 1) + per_row - 1) % c.V]
            mut = None
        return (f32_sparse(*st[:3], e.ids, e.g, e.n_uniq, c.t, mut, per_row=per_row),
                f32_sparse(*st[3:], e.ids, gw, e.n_uniq, c.t, mut, per_row=per_row, sweep_m=sweep_m))
    i = case_input(name, regime)
    lazy = isinstance(c, LazyCase)
    return f32_sparse(*st, i.ids, i.g, i.n_uniq, c.t, mut, lazy=lazy,
                      per_row=None if lazy else items_per_row(c.cls, c.E))


def dense_input(n, seed):
    """(var, m, v, g) [n] float32; from 16 elements on: 5 m = v = 0, 6 the same with g = 0 (comes back bit-identical),
    7 v = 1e-40, 9 |var| = 1e-6, 11 g = 0"""
    x, m, v = (a[:, 0].copy() for a in state(n, 1, seed))
    g = np.random.default_rng(seed + 2).standard_normal(n, dtype=F32)
    if n >= 16:
        g[[6, 11]] = 0
    return x, m, v, g


def multi_input(case):
    return [dense_input(n, case.seed + 10 * i) for i, n in enumerate(case.sizes)]
