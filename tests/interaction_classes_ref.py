"""The kernel classes of csrc/interactions.hip (PNN inner product rec_emb_ipn_*, NFM bi-interaction rec_emb_bi_*, GSU
attention rec_ip_attn_*, FFM rec_ffm_*) restated for the tests, fp64 references of all eight entry points with derived
per-element error bounds, plain fp32 restatements (the kernel's own summation order and two others) with the mutants the
bounds must catch, and the case tables.  No GPU and no package import here: numpy alone.

K holds every constant the dispatchers read, so that tests/test_interaction_classes_host.py can compare it with the source.

ipn_class()      EX examples a workgroup: the largest power of two <= 8 with B // EX >= 1024 groups, halved until the LDS of
                 a group is <= 16 KB; a single example may take more (forward 64 KB, backward K.CU_LDS through the LDS
                 opt-in).  Both directions accept a shape only if both can run it.  vec4 (forward only): E % 4 == 0,
                 ld % 4 == 0 and a 16-byte aligned table.
bi_class()       vec under the same three conditions (the backward also wants sumvec and vals aligned); fields are loaded
                 in blocks of 8, the last one ragged when F % 8 != 0.
ip_attn_class()  NPL = ceil(C*E / 64) dims a lane, a lane tail when C*E % 64 != 0, chunks of TB = 8 steps dealt round-robin
                 to 4 waves.
ffm_class()      vec when E % 4 == 0, ld_v % 4 == 0 and v (backward: and g_rows) aligned; the forward's pair loop strides
                 256 lanes, the backward's item loop 128.

Kernel-defined behaviour the references follow: an out-of-range id contributes a zero row (FFM: a zero pair and a zero w);
a step is padded when channel 0 equals padding_index, whatever the other channels hold; a padded step has score 0 and gkeys
0 and is never read; rows of g_rows at and beyond n_uniq are 0.

Bounds.  u = 2^-24, gamma(k) = k u / (1 - k u).  A sum of n terms (products or plain addends) evaluated in fp32 in ANY order,
fused or not, is within gamma(n) * sum|terms| of the exact sum: a term passes one product rounding and at most n - 1
additions.  sum_bound(n, c, sabs, res) = gamma(n + c) * sabs + ulp32(res), c the extra roundings the kernel text shows:
  ipn pair        n = E, c = 0            v += x*y over d, the vec4 form only regroups them
  ipn vals        n = F, c = 0            acc = g[k], then F multiply-adds (the diagonal one adds an exact zero)
  bi S, Q         n = F, c = 0            S has no product rounding: gamma(F) is one more than it needs
  bi out          0.5 (S*S - Q) from S^ = S + dS, Q^ = Q + dQ:  A = 2|S| bS + bS^2 + bQ is what the inputs carry, the square
                  rounds (u (S^2 + A)), the difference rounds (u (|S^2 - Q| + A + u (S^2 + A))), the half is exact
  bi vals         g (S - e) on the sumvec the kernel is GIVEN: gamma(2) |g| (|S| + |e|)
  attn scores     n = D, c = 0            NPL products a lane, then the 6-step butterfly: any order
  attn pooled     sum_t s^_t k_td with |s^_t - s_t| <= bs_t:  sum_t bs_t |k_td| + gamma(T + 2) sum_t (|s_t| + bs_t) |k_td|;
                  c = 2 are the two additions of the 4-partial tree on top of a wave's chain of at most T terms
  attn gq         the same with gs_t = <gpooled, k_t>
  attn gkeys      s gp + gs^ q, s the score the kernel is GIVEN:  bgs |q| + gamma(2) (|s gp| + (|gs| + bgs) |q|)
  ffm z           n = P*E + F + 1 (pair products, the w's, the bias), c = 0: lane chain, butterfly, 4-partial tree, bias
  ffm prob        sigmoid'(z) <= 1/4: bz / 4 + 6 u (expf within 2 ulp moves p by p (1-p) 4u <= u, 1 + e rounds: p u, the
                  quotient within 2 ulp: 4 u p)
  ffm g_rows      n = lookups of the segment, c = 0
"""
import collections
import functools

import numpy as np

Consts = collections.namedtuple(
    "Consts", "GROUPS GROUP_LDS FWD_LDS_MAX CU_LDS IPN_MAX_F EX_MAX WG ROW_UNROLL F_BLOCK TB WAVES LANES ATTN_MAX_D "
              "ATTN_LDS_MAX FFM_MAX_F FFM_FWD_STRIDE FFM_BWD_STRIDE LAUNCH_LDS")
K = Consts(GROUPS=1024,              # fewest workgroups the IPN grid rule keeps
           GROUP_LDS=16 * 1024,      # LDS of an IPN group of more than one example
           FWD_LDS_MAX=64 * 1024,    # LDS of a single IPN example, forward
           CU_LDS=160 * 1024,        # LDS of one CU: what the backward of a single example may take
           IPN_MAX_F=255,            # pair endpoints are bytes
           EX_MAX=8, WG=256, ROW_UNROLL=4,
           F_BLOCK=8,                # fields a bi-interaction lane loads at a time
           TB=8, WAVES=4, LANES=64,  # ip_attn: steps a chunk, waves a workgroup, lanes a wave
           ATTN_MAX_D=256, ATTN_LDS_MAX=64 * 1024,
           FFM_MAX_F=254,            # the largest F whose forward LDS request fits LAUNCH_LDS
           FFM_FWD_STRIDE=256, FFM_BWD_STRIDE=128,
           LAUNCH_LDS=64 * 1024)     # dynamic LDS a kernel may ask for without the opt-in
F32, F64 = np.float32, np.float64
U = 2.0 ** -24
OOB_IDS = (-1, None, 2 ** 32 + 3)    # None stands for V; the last one aliases row 3 once narrowed to 32 bits


# ---- dispatch -------------------------------------------------------------------------------------------------------
IpnClass = collections.namedtuple("IpnClass", "EX vec4 groups partial_last")
BiClass = collections.namedtuple("BiClass", "vec f_blocks ragged_f groups grid_tail")
AttnClass = collections.namedtuple("AttnClass", "NPL lane_tail chunks_per_wave")
FfmClass = collections.namedtuple("FfmClass", "vec pair_passes item_passes")


def ipn_lds_bytes(EX, F, E, bwd):
    P = F * (F - 1) // 2
    if bwd:
        return EX * (F * (E + 1) + F * E + F * F) * 4
    return EX * F * (E + 4) * 4 + EX * F * 4 + 2 * P + 16


def ipn_bwd_lds_max(k=K):
    """what the backward of one example needs at the widest row the forward's 64 KB admits, over every F; the CU if that is
    more than a CU has"""
    need = 0
    for F in range(1, k.IPN_MAX_F + 1):
        fixed = ipn_lds_bytes(1, F, 0, False)
        if fixed + 4 * F > k.FWD_LDS_MAX:
            break
        need = max(need, ipn_lds_bytes(1, F, (k.FWD_LDS_MAX - fixed) // (4 * F), True))
    return min(need, k.CU_LDS)


def ipn_accepts(F, E, k=K):
    """the one domain of rec_emb_ipn_fwd_f32 and rec_emb_ipn_bwd_vals_f32"""
    return (1 <= F <= k.IPN_MAX_F and E >= 1 and ipn_lds_bytes(1, F, E, False) <= k.FWD_LDS_MAX
            and ipn_lds_bytes(1, F, E, True) <= ipn_bwd_lds_max(k))


def ipn_class(B, F, E, ld, aligned=True, bwd=False, k=K):
    """IpnClass of a launch, None when the entry point refuses (or B = 0: nothing is launched)"""
    if ld < E or B <= 0 or not ipn_accepts(F, E, k):
        return None
    EX = k.EX_MAX
    while EX > 1 and B // EX < k.GROUPS:
        EX //= 2
    while EX > 1 and ipn_lds_bytes(EX, F, E, bwd) > k.GROUP_LDS:
        EX //= 2
    vec4 = (not bwd) and E % 4 == 0 and ld % 4 == 0 and aligned
    return IpnClass(EX, bool(vec4), -(-B // EX), B % EX != 0)


def ipn_row_passes(cls, F, E, bwd, k=K):
    """passes of the row-load loop of a FULL group (4 loads a lane a pass)"""
    per = k.WG * k.ROW_UNROLL
    items = cls.EX * (F * E + F * F) if bwd else cls.EX * F * (E // 4 if cls.vec4 else E)
    return -(-items // per)


def bi_class(B, F, E, ld, aligned=True, bwd=False, sumvec_aligned=True, vals_aligned=True, k=K):
    vec = E % 4 == 0 and ld % 4 == 0 and aligned and (not bwd or (sumvec_aligned and vals_aligned))
    lanes = B * (F if bwd else 1) * (E // 4 if vec else E)
    return BiClass(bool(vec), -(-F // k.F_BLOCK), F % k.F_BLOCK != 0, -(-lanes // k.WG), lanes % k.WG != 0)


def ip_attn_accepts(C, E, T, k=K):
    D = C * E
    return C >= 1 and E >= 1 and T >= 1 and D <= k.ATTN_MAX_D and T * C * 4 + k.WAVES * D * 4 <= k.ATTN_LDS_MAX


def ip_attn_class(C, E, T, k=K):
    if not ip_attn_accepts(C, E, T, k):
        return None
    D = C * E
    chunks = -(-T // k.TB)
    return AttnClass(min(-(-D // k.LANES), 4), D % k.LANES != 0, -(-chunks // k.WAVES))


def ffm_fwd_lds_bytes(F):
    return F * 4 + 16 + F * (F - 1)


def ffm_class(F, E, ld_v, aligned=True, bwd=False, rows_aligned=True, k=K):
    if not (1 <= F <= k.FFM_MAX_F and E >= 1 and ld_v >= F * E):
        return None
    vec = E % 4 == 0 and ld_v % 4 == 0 and aligned and (not bwd or rows_aligned)
    EL = E // 4 if vec else E
    P = F * (F - 1) // 2
    return FfmClass(bool(vec), -(-(P * EL) // k.FFM_FWD_STRIDE), -(-(F * EL) // k.FFM_BWD_STRIDE))


# ---- arithmetic ------------------------------------------------------------------------------------------------------
def gamma(n):
    n = np.asarray(n, F64)
    return n * U / (1 - n * U)


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, F64)).astype(F32)).astype(F64)


def sum_bound(n, c, sabs, res):
    return gamma(np.asarray(n) + c) * sabs + ulp32(res)


def pairs(F):
    """(i, j) of pair p in the row-major order of the upper triangle"""
    i, j = np.triu_indices(F, 1)
    return i.astype(np.int64), j.astype(np.int64)


def rows_of(table, ids, dt=F64, oob_row0=False):
    """table[ids] in ``dt`` with a zero row for every id outside [0, V) -> (rows, in-range mask)"""
    V = table.shape[0]
    ok = (ids >= 0) & (ids < V)
    e = table.astype(dt)[np.where(ok, ids, 0)]
    if not oob_row0:
        e[~ok] = 0
    return e, ok


def ratio(got, ref, bound):
    """worst |got - ref| / bound; an element that is not finite, or off where the bound is 0, counts as infinite"""
    got = np.asarray(got, F64)
    if got.size == 0:
        return 0.0
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    q[~np.isfinite(got)] = np.inf
    return float(np.nanmax(np.where(np.isnan(q), np.inf, q)))


# ---- fp64 references: every one returns values and their bounds -------------------------------------------------------
IpnFwd = collections.namedtuple("IpnFwd", "out bound")
BiFwd = collections.namedtuple("BiFwd", "out bout S bS")
AttnFwd = collections.namedtuple("AttnFwd", "scores bs pooled bp valid")
AttnBwd = collections.namedtuple("AttnBwd", "gkeys bgk gq bgq")
FfmFwd = collections.namedtuple("FfmFwd", "z bz prob bprob")
Vals = collections.namedtuple("Vals", "vals bound")


def ref_ipn_fwd(table, X):
    e, _ = rows_of(table, X)
    B, F, E = e.shape
    pi, pj = pairs(F)
    dot, sabs = np.zeros((B, len(pi))), np.zeros((B, len(pi)))
    for d in range(E):
        t = e[:, pi, d] * e[:, pj, d]
        dot += t
        sabs += np.abs(t)
    return IpnFwd(np.concatenate([e.reshape(B, F * E), dot], 1),
                  np.concatenate([np.zeros((B, F * E)), sum_bound(E, 0, sabs, dot)], 1))


def _sym(g, F):
    """the pair part of a gradient row as the symmetric F x F matrix with a zero diagonal"""
    pi, pj = pairs(F)
    G = np.zeros((g.shape[0], F, F), g.dtype)
    G[:, pi, pj] = g[:, :len(pi)]
    G[:, pj, pi] = G[:, pi, pj]
    return G


def ref_ipn_bwd(table, X, g):
    """g [B, F*E + P] (the leading columns of the gradient rows)"""
    e, _ = rows_of(table, X)
    B, F, E = e.shape
    g = np.asarray(g, F64)
    flat, G = g[:, :F * E].reshape(B, F, E), _sym(g[:, F * E:], F)
    vals = flat + np.einsum("bij,bjd->bid", G, e)
    sabs = np.abs(flat) + np.einsum("bij,bjd->bid", np.abs(G), np.abs(e))
    return Vals(vals.reshape(B * F, E), sum_bound(F, 0, sabs, vals).reshape(B * F, E))


def ref_bi_fwd(table, X):
    e, _ = rows_of(table, X)
    F = e.shape[1]
    S, Q = e.sum(1), (e * e).sum(1)
    bS, bQ = sum_bound(F, 0, np.abs(e).sum(1), S), sum_bound(F, 0, Q, Q)
    out = 0.5 * (S * S - Q)
    A = 2 * np.abs(S) * bS + bS * bS + bQ
    sq = U * (S * S + A)
    return BiFwd(out, 0.5 * (A + sq + U * (np.abs(S * S - Q) + A + sq)) + ulp32(out), S, bS)


def ref_bi_bwd(table, X, g, sumvec=None):
    """``sumvec``: the float32 sums the kernel is given (the forward's own); None: the exact ones"""
    e, _ = rows_of(table, X)
    B, F, E = e.shape
    S = (e.sum(1) if sumvec is None else np.asarray(sumvec, F64))[:, None, :]
    g = np.asarray(g, F64)[:, None, :E]
    vals = g * (S - e)
    return Vals(vals.reshape(B * F, E), sum_bound(2, 0, np.abs(g) * (np.abs(S) + np.abs(e)), vals).reshape(B * F, E))


def _keys(table, series, padding_index, dt=F64, oob_row0=False, any_channel=False):
    B, T, C = series.shape
    k, _ = rows_of(table, series, dt, oob_row0)
    valid = (series != padding_index).any(2) if any_channel else series[:, :, 0] != padding_index
    return k.reshape(B, T, -1) * valid[:, :, None].astype(dt), valid


def ref_attn_fwd(table, q, series, padding_index):
    k, valid = _keys(table, series, padding_index)
    T, D = k.shape[1], k.shape[2]
    q = np.asarray(q, F64)[:, None, :D]
    s = (q * k).sum(2)
    bs = np.where(valid, sum_bound(D, 0, (np.abs(q) * np.abs(k)).sum(2), s), 0.0)
    pooled = np.einsum("bt,btd->bd", s, k)
    carried = np.einsum("bt,btd->bd", bs, np.abs(k))
    sabs = np.einsum("bt,btd->bd", np.abs(s) + bs, np.abs(k))
    return AttnFwd(s, bs, pooled, carried + sum_bound(T, 2, sabs, pooled), valid)


def ref_attn_bwd(table, q, series, padding_index, scores, gpooled):
    """``scores``: the float32 scores the kernel is given; those of padded steps are not read"""
    k, valid = _keys(table, series, padding_index)
    T, D = k.shape[1], k.shape[2]
    q, gp = np.asarray(q, F64)[:, None, :D], np.asarray(gpooled, F64)[:, None, :D]
    s = np.where(valid, np.asarray(scores, F64), 0.0)[:, :, None]
    gs = (gp * k).sum(2)
    bgs = np.where(valid, sum_bound(D, 0, (np.abs(gp) * np.abs(k)).sum(2), gs), 0.0)
    gq = np.einsum("bt,btd->bd", gs, k)
    bgq = np.einsum("bt,btd->bd", bgs, np.abs(k)) + sum_bound(
        T, 2, np.einsum("bt,btd->bd", np.abs(gs) + bgs, np.abs(k)), gq)
    gkeys = s * gp + gs[:, :, None] * q
    bgk = bgs[:, :, None] * np.abs(q) + sum_bound(
        2, 0, np.abs(s * gp) + (np.abs(gs) + bgs)[:, :, None] * np.abs(q), gkeys)
    return AttnBwd(gkeys, np.where(valid[:, :, None], bgk, 0.0), gq, bgq)


def _ffm_rows(v, X, dt=F64, oob_row0=False):
    """A[b, a, c, :] = v[X[b,a], c, :], zero where X[b,a] is out of range"""
    return rows_of(v, X, dt, oob_row0)


def ref_ffm_fwd(v, w, bias, X):
    """v [V,F,E], w [V], bias [1]"""
    A, ok = _ffm_rows(v, X)
    B, F = X.shape
    E = v.shape[2]
    M = np.einsum("bace,bcae->bac", A, A)
    Mabs = np.einsum("bace,bcae->bac", np.abs(A), np.abs(A))
    up = np.triu(np.ones((F, F), bool), 1)
    wx, _ = rows_of(np.asarray(w).reshape(-1, 1), X)
    b0 = float(np.asarray(bias, F64).reshape(-1)[0])
    z = b0 + wx[:, :, 0].sum(1) + (M * up).sum((1, 2))
    sabs = abs(b0) + np.abs(wx[:, :, 0]).sum(1) + (Mabs * up).sum((1, 2))
    bz = sum_bound(F * (F - 1) // 2 * E + F + 1, 0, sabs, z)
    prob = 1.0 / (1.0 + np.exp(-z))
    return FfmFwd(z, bz, prob, 0.25 * bz + 6 * U)


def host_plan(X):
    """the de-duplication plan of X.reshape(-1) as rec_dedup_plan_i64 lays it out: unique ids ascending, the lookups of
    one id in ascending position -> (perm int32 [n], seg_start int32 [n+1], n_uniq)"""
    flat = np.asarray(X, np.int64).reshape(-1)
    n = flat.size
    perm = np.argsort(flat, kind="stable").astype(np.int32)
    srt = flat[perm]
    starts = np.nonzero(np.concatenate([[True], srt[1:] != srt[:-1]]))[0] if n else np.zeros(0, np.int64)
    seg = np.full(n + 1, n, np.int32)
    seg[:len(starts)] = starts
    return perm, seg, len(starts)


def _ffm_contrib(v, X, gz, dt=F64, keep_diag=False, oob_row0=False):
    """contrib[b*F + a, c, :] = gz[b] * v[X[b,c], a, :] for c != a"""
    A, _ = _ffm_rows(v, X, dt, oob_row0)
    B, F = X.shape
    c = np.asarray(gz, dt).reshape(B, 1, 1, 1) * A.transpose(0, 2, 1, 3)
    if not keep_diag:
        c[:, np.arange(F), np.arange(F)] = 0
    return c.reshape(B * F, F, -1)


def ref_ffm_bwd(v, X, gz, plan):
    perm, seg, nu = plan
    n, F = X.size, X.shape[1]
    c = _ffm_contrib(v, X, gz)
    rows, sabs = np.zeros((max(n, 1),) + c.shape[1:]), np.zeros((max(n, 1),) + c.shape[1:])
    lens = np.diff(seg[:nu + 1].astype(np.int64))
    owner = np.repeat(np.arange(nu), lens)
    np.add.at(rows, owner, c[perm[:len(owner)]])
    np.add.at(sabs, owner, np.abs(c[perm[:len(owner)]]))
    count = np.zeros(max(n, 1))
    count[:nu] = lens
    return Vals(rows, sum_bound(np.maximum(count, 1)[:, None, None], 0, sabs, rows) * (count > 0)[:, None, None])


# ---- plain fp32 restatements: order in ("kernel", "reverse", "pairwise"); ``mut`` one of MUTANTS ---------------------------
ORDERS = ("kernel", "reverse", "pairwise")
MUTANTS = ("pair_off_by_one", "pair_transposed", "partial_example_dropped", "ragged_field_dropped", "diag_not_zero",
           "valid_any_channel", "wave_partial_dropped", "oob_row0", "ffm_own_field", "ffm_diag_kept", "segment_last_dropped")


def fsum(t, order, axis=-1):
    """float32 sum of ``t`` along ``axis``: left to right, right to left, or numpy's pairwise tree"""
    t = np.moveaxis(np.asarray(t, F32), axis, 0)
    if order == "pairwise":
        return np.add.reduce(np.ascontiguousarray(np.moveaxis(t, 0, -1)), axis=-1, dtype=F32)
    acc = np.zeros(t.shape[1:], F32)
    for x in (t[::-1] if order == "reverse" else t):
        acc = acc + x
    return acc


def _butterfly(part):
    """group_sum<64> over the last axis (64 lanes): every lane ends with the same sum; lane 0's is returned"""
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        part = part + part[..., lane ^ o]
    return part[..., 0]


CHUNK = 1024                                               # examples a restatement holds in memory at a time


def f32_ipn_fwd(table, X, order="kernel", vec4=False, EX=1, mut=None):
    if X.shape[0] > CHUNK:
        out = np.concatenate([f32_ipn_fwd(table, X[i:i + CHUNK], order, vec4, 1, mut) for i in range(0, len(X), CHUNK)])
        if mut == "partial_example_dropped" and len(X) % EX:
            out[-1] = 0
        return out
    e, _ = rows_of(table, X, F32, mut == "oob_row0")
    B, F, E = e.shape
    pi, pj = pairs(F)
    t = e[:, pi, :] * e[:, pj, :]
    if order == "kernel" and vec4:
        q = t.reshape(B, len(pi), E // 4, 4)
        dot = fsum((q[..., 0] + q[..., 1]) + (q[..., 2] + q[..., 3]), "kernel")
    else:
        dot = fsum(t, order)
    P = len(pi)
    if mut == "pair_off_by_one" and P:
        dot = dot[:, (np.arange(P) + 1) % P]
    if mut == "pair_transposed" and P:                     # pair (i, j) lands where the column-major walk puts it
        where = np.argsort(np.lexsort((pi, pj)))
        moved = np.empty_like(dot)
        moved[:, where] = dot
        dot = moved
    out = np.concatenate([e.reshape(B, F * E), dot], 1)
    if mut == "partial_example_dropped" and B % EX:
        out[B - 1] = 0
    return out


def f32_ipn_bwd(table, X, g, order="kernel", EX=1, mut=None):
    if X.shape[0] > CHUNK:
        vals = np.concatenate([f32_ipn_bwd(table, X[i:i + CHUNK], g[i:i + CHUNK], order, 1, mut)
                               for i in range(0, len(X), CHUNK)])
        if mut == "partial_example_dropped" and len(X) % EX:
            vals[-X.shape[1]:] = 0
        return vals
    e, _ = rows_of(table, X, F32)
    B, F, E = e.shape
    g = np.asarray(g, F32)
    flat, G = g[:, :F * E].reshape(B, F, E), _sym(g[:, F * E:], F)
    if mut == "diag_not_zero" and F > 1:
        G[:, np.arange(F), np.arange(F)] = g[:, F * E + np.minimum(np.arange(F), F * (F - 1) // 2 - 1)]
    t = np.concatenate([flat[:, :, None, :], G[:, :, :, None] * e[:, None, :, :]], 2)       # [B, i, 1 + j, d]
    vals = fsum(t, order, axis=2)
    if mut == "partial_example_dropped" and B % EX:
        vals[B - 1] = 0
    return vals.reshape(B * F, E)


def f32_bi_fwd(table, X, order="kernel", mut=None):
    e, _ = rows_of(table, X, F32, mut == "oob_row0")
    F = e.shape[1]
    if mut == "ragged_field_dropped" and F % K.F_BLOCK:
        e = e[:, :F - 1]
    S, Q = fsum(e, order, 1), fsum(e * e, order, 1)
    return F32(0.5) * (S * S - Q), S


def f32_bi_bwd(table, X, g, sumvec, mut=None):
    e, _ = rows_of(table, X, F32, mut == "oob_row0")
    B, F, E = e.shape
    return (np.asarray(g, F32)[:, None, :E] * (np.asarray(sumvec, F32)[:, None, :] - e)).reshape(B * F, E)


def _dot_d(a, k, order):
    """<a, k_t> over D as the kernel sums it (NPL products a lane, then the butterfly) or in another order"""
    t = a * k
    if order != "kernel":
        return fsum(t, order)
    D = t.shape[-1]
    pad = np.zeros(t.shape[:-1] + (-D % 64,), F32)
    lanes = np.concatenate([t, pad], -1).reshape(t.shape[:-1] + (-1, 64))      # [.., a, lane]
    return _butterfly(fsum(lanes, "kernel", axis=-2))


def _over_t(s, k, order, mut=None):
    """sum_t s_t k_td: a chain per wave over its chunks of TB steps and the 4-partial tree, or another order"""
    t = s[:, :, None] * k
    if order != "kernel":
        return fsum(t, order, 1)
    T = t.shape[1]
    wave = (np.arange(T) // K.TB) % K.WAVES
    p = [fsum(t[:, wave == w], "kernel", 1) for w in range(K.WAVES)]
    if mut == "wave_partial_dropped":
        p[3] = np.zeros_like(p[3])
    return (p[0] + p[1]) + (p[2] + p[3])


def f32_attn_fwd(table, q, series, padding_index, order="kernel", mut=None):
    k, valid = _keys(table, series, padding_index, F32, mut == "oob_row0", mut == "valid_any_channel")
    D = k.shape[2]
    s = _dot_d(np.asarray(q, F32)[:, None, :D], k, order) * valid
    return s, _over_t(s, k, order, mut)


def f32_attn_bwd(table, q, series, padding_index, scores, gpooled, order="kernel", mut=None):
    k, valid = _keys(table, series, padding_index, F32, mut == "oob_row0", mut == "valid_any_channel")
    D = k.shape[2]
    q, gp = np.asarray(q, F32)[:, None, :D], np.asarray(gpooled, F32)[:, None, :D]
    gs = _dot_d(gp, k, order) * valid
    s = np.where(valid, np.asarray(scores, F32), F32(0))
    return s[:, :, None] * gp + gs[:, :, None] * q, _over_t(gs, k, order, mut)


def f32_ffm_fwd(v, w, bias, X, order="kernel", vec=False, mut=None):
    A, _ = _ffm_rows(v, X, F32, mut == "oob_row0")
    B, F = X.shape
    E = v.shape[2]
    pi, pj = pairs(F)
    left = A[:, pi, pi if mut == "ffm_own_field" else pj, :]
    t = (left * A[:, pj, pi, :]).reshape(B, -1)                      # [B, P*E], item-major as the kernel walks it
    wx, _ = rows_of(np.asarray(w, F32).reshape(-1, 1), X, F32, mut == "oob_row0")
    b0 = np.asarray(bias, F32).reshape(-1)[0]
    if order != "kernel":
        return fsum(np.concatenate([t, wx[:, :, 0], np.full((B, 1), b0, F32)], 1), order)
    if vec:
        q = t.reshape(B, -1, 4)
        t = ((q[..., 0] + q[..., 1]) + q[..., 2]) + q[..., 3]
    lanes = np.concatenate([t, np.zeros((B, -t.shape[1] % 256), F32)], 1).reshape(B, -1, 256)
    acc = fsum(lanes, "kernel", 1) if lanes.shape[1] else np.zeros((B, 256), F32)
    acc[:, :F] = acc[:, :F] + wx[:, :, 0]                            # lane i < F then adds w[X[b,i]]
    red = _butterfly(acc.reshape(B, 4, 64))
    return b0 + ((red[:, 0] + red[:, 1]) + (red[:, 2] + red[:, 3]))


def f32_ffm_bwd(v, X, gz, plan, order="kernel", mut=None):
    perm, seg, nu = plan
    n = X.size
    c = _ffm_contrib(v, X, gz, F32, mut == "ffm_diag_kept", mut == "oob_row0")
    rows = np.zeros((max(n, 1),) + c.shape[1:], F32)
    s, e = seg[:nu].astype(np.int64), seg[1:nu + 1].astype(np.int64)
    if mut == "segment_last_dropped":
        e = e - 1
    if order == "pairwise":
        for u in range(nu):
            rows[u] = np.add.reduce(c[perm[s[u]:e[u]]], axis=0, dtype=F32)
        return rows
    for step in range(int((e - s).max()) if nu else 0):
        at = (e - 1 - step) if order == "reverse" else (s + step)
        live = np.nonzero(step < e - s)[0]
        rows[live] = rows[live] + c[perm[at[live]]]
    return rows


# ---- case tables ----------------------------------------------------------------------------------------------------
IpnCase = collections.namedtuple("IpnCase", "name B F E ld off oob seed fwd bwd")
BiCase = collections.namedtuple("BiCase", "name B F E ld off off_sum off_vals oob seed fwd bwd")
AttnCase = collections.namedtuple("AttnCase", "name T C E ld ld_q ld_p ld_gp oob seed cls")
FfmCase = collections.namedtuple("FfmCase", "name B F E ld_v off ld_w off_rows zipf oob seed fwd bwd")
V_IPN, V_BI, V_ATTN, V_FFM = 1000, 700, 900, 300
PAD = 0                                                     # padding_index of every attention case


def _ipn_cases():
    rows = [  # name, B, F, E, ld, float offset of the table, out-of-range ids
        ("ex8_vec_partial", 8195, 3, 4, 4, 0, True), ("ex8_scalar_partial", 8195, 3, 3, 3, 0, False),
        ("ex8_vec_exact", 8192, 3, 4, 8, 0, False), ("ex8_scalar_exact", 8192, 3, 3, 3, 0, True),
        ("ex8_fallback_ld", 8195, 3, 4, 5, 0, False), ("ex8_fallback_align", 8195, 3, 4, 4, 1, True),
        ("ex4_grid_vec_partial", 4097, 2, 4, 4, 0, True), ("ex4_grid_scalar_partial", 4097, 2, 5, 5, 0, False),
        ("ex4_vec_exact", 4100, 2, 8, 8, 0, False), ("ex4_scalar_exact", 4100, 2, 3, 4, 0, False),
        ("ex4_lds_bwd_ex2", 8195, 26, 16, 16, 0, True),
        ("ex2_vec_partial", 2049, 2, 4, 4, 0, False), ("ex2_scalar_partial", 2049, 5, 6, 6, 0, True),
        ("ex2_vec_exact_f1", 2050, 1, 4, 4, 0, False), ("ex2_scalar_exact_e1", 2050, 2, 1, 1, 0, False),
        ("ex1_f1", 7, 1, 4, 4, 0, True), ("ex1_scalar", 9, 7, 6, 6, 0, True), ("ex1_vec_strided", 65, 5, 16, 32, 0, False),
        ("ex1_over16k_vec", 5, 64, 64, 64, 0, True), ("ex1_over16k_scalar", 3, 64, 64, 65, 0, False),
        ("ex1_bwd_optin_f80", 3, 80, 64, 64, 0, False), ("ex1_bwd_optin_f100", 2, 100, 32, 32, 0, True),
        ("ex1_bwd_near_cu", 2, 200, 1, 1, 0, False)]
    return tuple(IpnCase(n, B, F, E, ld, off, oob, 1000 + i, ipn_class(B, F, E, ld, off == 0),
                         ipn_class(B, F, E, ld, off == 0, bwd=True))
                 for i, (n, B, F, E, ld, off, oob) in enumerate(rows))


def _bi_cases():
    rows = []  # name, B, F, E, ld, offsets of table, sumvec and vals, out-of-range ids
    for i, F in enumerate((1, 7, 8, 9, 16, 17)):
        rows.append(("vec_f%d" % F, 33, F, 8, (8, 12)[i % 2], 0, 0, 0, i % 2 == 0))
        rows.append(("scalar_f%d" % F, 33, F, 5, (5, 8)[i % 2], 0, 0, 0, i % 2 == 1))
    rows += [("vec_grid_tail", 300, 9, 16, 20, 0, 0, 0, True), ("scalar_grid_tail", 77, 17, 5, 7, 0, 0, 0, False),
             ("vec_grid_exact", 64, 8, 16, 16, 0, 0, 0, False),
             ("fallback_align", 33, 8, 4, 4, 1, 0, 0, True), ("fallback_ld", 33, 9, 8, 9, 0, 0, 0, False),
             ("bwd_fallback_sumvec", 33, 16, 8, 8, 0, 1, 0, True), ("bwd_fallback_vals", 33, 17, 8, 8, 0, 0, 1, False)]
    return tuple(BiCase(n, B, F, E, ld, off, os, ov, oob, 2000 + i, bi_class(B, F, E, ld, off == 0),
                        bi_class(B, F, E, ld, off == 0, True, os == 0, ov == 0))
                 for i, (n, B, F, E, ld, off, os, ov, oob) in enumerate(rows))


def _attn_cases():
    rows = [  # name, T, C, E, ld, ld_q - D, ld_pooled - D, ld_gpooled - D, out-of-range ids
        ("d4_t1", 1, 1, 4, 4, 0, 0, 0, False), ("d63_t8", 8, 3, 21, 21, 0, 0, 0, False), ("d63_t8_oob", 8, 3, 21, 24, 5, 1, 7, True),
        ("d64_t9", 9, 2, 32, 32, 0, 0, 0, False), ("d65_t32", 32, 5, 13, 16, 3, 2, 1, True),
        ("d128_t33", 33, 4, 32, 32, 0, 0, 0, False), ("d128_t33_oob", 33, 4, 32, 36, 4, 4, 4, True),
        ("d130_t65", 65, 2, 65, 65, 0, 0, 0, True), ("d192_t8", 8, 3, 64, 64, 0, 0, 0, False),
        ("d192_t33_oob", 33, 3, 64, 68, 1, 3, 5, True), ("d250_t9", 9, 5, 50, 50, 6, 0, 2, False),
        ("d256_t33", 33, 4, 64, 64, 0, 0, 0, True), ("d256_t65", 65, 1, 256, 256, 0, 8, 0, False)]
    out = []
    for i, (n, T, C, E, ld, a, b, c, oob) in enumerate(rows):
        D = C * E
        out.append(AttnCase(n, T, C, E, ld, D + a, D + b, D + c, oob, 3000 + i, ip_attn_class(C, E, T)))
    return tuple(out)


def _ffm_cases():
    rows = [  # name, B, F, E, ld_v - F*E, offset of v, ld_w, offset of g_rows, zipf, out-of-range ids
        ("f1", 4, 1, 4, 0, 0, 1, 0, False, True), ("f2_vec", 5, 2, 4, 0, 0, 1, 0, False, False),
        ("f26_vec", 33, 26, 16, 0, 0, 1, 0, False, True), ("f40_vec", 9, 40, 16, 4, 0, 1, 0, False, False),
        ("f26_scalar", 9, 26, 6, 0, 0, 1, 0, False, True), ("f7_scalar", 65, 7, 6, 2, 0, 1, 0, False, False),
        ("fallback_align", 5, 3, 4, 0, 1, 1, 0, False, True), ("fallback_ld", 5, 3, 4, 1, 0, 1, 0, False, False),
        ("fused_ld_w16", 7, 5, 8, 8, 0, 16, 0, False, True), ("bwd_fallback_rows", 6, 4, 8, 0, 0, 1, 1, False, False),
        ("zipf_long", 500, 10, 8, 0, 0, 1, 0, True, False)]
    return tuple(FfmCase(n, B, F, E, F * E + x, off, ld_w, orow, zipf, oob, 4000 + i, ffm_class(F, E, F * E + x, off == 0),
                         ffm_class(F, E, F * E + x, off == 0, True, orow == 0))
                 for i, (n, B, F, E, x, off, ld_w, orow, zipf, oob) in enumerate(rows))


IPN_CASES, BI_CASES, ATTN_CASES, FFM_CASES = _ipn_cases(), _bi_cases(), _attn_cases(), _ffm_cases()
BY_NAME = {(t, c.name): c for t, cases in (("ipn", IPN_CASES), ("bi", BI_CASES), ("attn", ATTN_CASES), ("ffm", FFM_CASES))
           for c in cases}
assert len(BY_NAME) == len(IPN_CASES) + len(BI_CASES) + len(ATTN_CASES) + len(FFM_CASES)
ATTN_PATTERNS = ("none", "tail", "middle", "all", "pad_live_channels", "oob_valid_step", "pad_oob_channels")


# ---- inputs ---------------------------------------------------------------------------------------------------------
def values(r, shape, scale=1.0):
    """Not Gaussian: magnitudes log-uniform over 2^-8 .. 2^1 times ``scale``, random signs, one element in sixteen an exact
    zero -- sums with cancellation and terms of very different size, which one global tolerance cannot judge"""
    mag = np.exp2(r.uniform(-8, 1, size=shape)) * scale
    x = (mag * r.choice([-1.0, 1.0], size=shape)).astype(F32)
    x[r.random(size=shape) < 1 / 16] = 0
    return x


def _oob(V, i):
    x = OOB_IDS[i % 3]
    return V if x is None else x


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def ipn_input(name):
    """(table [V,E], X [B,F], g [B, F*E + P]); duplicates across and inside examples; the out-of-range ids of an ``oob``
    case sit in the first and the last example of the first group and in the last example of all"""
    c = BY_NAME["ipn", name]
    r = np.random.default_rng(c.seed)
    table = values(r, (V_IPN, c.E))
    X = r.integers(0, V_IPN, size=(c.B, c.F)).astype(np.int64)
    if c.B > 4:
        X[3] = X[2]
        X[4, :] = X[4, 0]
    if c.oob:
        EX = c.fwd.EX
        X[0, 0] = _oob(V_IPN, 0)
        X[min(EX, c.B) - 1, c.F - 1] = _oob(V_IPN, 1)
        X[c.B - 1, c.F // 2] = _oob(V_IPN, 2)
    g = values(r, (c.B, c.F * c.E + c.F * (c.F - 1) // 2))
    return _frozen(table, X, g)


@functools.lru_cache(maxsize=None)
def bi_input(name):
    """(table, X, g [B,E])"""
    c = BY_NAME["bi", name]
    r = np.random.default_rng(c.seed)
    table = values(r, (V_BI, c.E))
    X = r.integers(0, V_BI, size=(c.B, c.F)).astype(np.int64)
    X[1, :] = X[1, 0]
    if c.oob:
        X[0, 0] = _oob(V_BI, 0)
        X[2, c.F - 1] = _oob(V_BI, 1)
        X[c.B - 1, c.F // 2] = _oob(V_BI, 2)
    return _frozen(table, X, values(r, (c.B, c.E)))


def attn_patterns(c):
    return tuple(p for p in ATTN_PATTERNS
                 if (c.oob or p not in ("oob_valid_step", "pad_oob_channels"))
                 and (c.C > 1 or p not in ("pad_live_channels", "pad_oob_channels")))


@functools.lru_cache(maxsize=None)
def attn_input(name):
    """(table, series [B,T,C], q [B,D], gpooled [B,D]): one example per pattern of attn_patterns(case), then two plain
    ones.  Valid steps hold ids in 1..V-1 (channel 0 never equals PAD by accident)."""
    c = BY_NAME["attn", name]
    r = np.random.default_rng(c.seed)
    pats = attn_patterns(c) + ("none", "tail")
    B, T, C, D = len(pats), c.T, c.C, c.C * c.E
    table = values(r, (V_ATTN, c.E))
    s = r.integers(1, V_ATTN, size=(B, T, C)).astype(np.int64)
    for b, p in enumerate(pats):
        mid = T // 2
        if p == "tail":
            s[b, max(T - 1 - b % 3, 0):, :] = PAD
        elif p == "middle":
            s[b, mid, :] = PAD
            s[b, 0, :] = PAD if T > 2 else s[b, 0, :]
        elif p == "all":
            s[b] = PAD
        elif p == "pad_live_channels":
            s[b, mid, 0] = PAD                            # the other channels keep their live ids
            s[b, T - 1, 1:] = PAD                         # and a VALID step whose other channels hold the padding id
        elif p == "oob_valid_step":
            s[b, mid, C - 1] = _oob(V_ATTN, 1)
            s[b, 0, C - 1] = _oob(V_ATTN, 2 if C > 1 else 1)
            if C > 1:
                s[b, T - 1, 1] = _oob(V_ATTN, 0)
        elif p == "pad_oob_channels":
            s[b, mid, 0] = PAD
            s[b, mid, 1:] = _oob(V_ATTN, 1)
    return _frozen(table, s, values(r, (B, D)), values(r, (B, D)))


@functools.lru_cache(maxsize=None)
def ffm_input(name):
    """(v [V,F,E], w [V], bias [1], X [B,F], gz [B]); from F = 2 on, one id sits in two fields of example 1 (and in all
    fields of example 2)"""
    c = BY_NAME["ffm", name]
    r = np.random.default_rng(c.seed)
    v, w = values(r, (V_FFM, c.F, c.E)), values(r, (V_FFM,))
    if c.zipf:
        X = np.minimum(r.zipf(1.3, size=(c.B, c.F)) - 1, V_FFM - 1).astype(np.int64)
    else:
        X = r.integers(0, V_FFM, size=(c.B, c.F)).astype(np.int64)
    X[1, c.F - 1] = X[1, 0]
    X[2, :] = X[2, 0]
    if c.oob:
        X[0, 0] = _oob(V_FFM, 0)
        X[3, c.F - 1] = _oob(V_FFM, 1)
        X[c.B - 1, c.F // 2] = _oob(V_FFM, 2)
    return _frozen(v, w, np.array([0.3], F32), X, values(r, (c.B,)))


def has_oob(ids, V):
    return bool(((np.asarray(ids) < 0) | (np.asarray(ids) >= V)).any())


# ---- the references of a case, computed once and shared -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ipn_reference(name):
    table, X, g = ipn_input(name)
    return ref_ipn_fwd(table, X), ref_ipn_bwd(table, X, g)


@functools.lru_cache(maxsize=None)
def bi_reference(name):
    table, X, _ = bi_input(name)
    return ref_bi_fwd(table, X)


@functools.lru_cache(maxsize=None)
def attn_reference(name):
    table, s, q, _ = attn_input(name)
    return ref_attn_fwd(table, q, s, PAD)


@functools.lru_cache(maxsize=None)
def ffm_reference(name):
    v, w, bias, X, gz = ffm_input(name)
    plan = host_plan(X)
    return ref_ffm_fwd(v, w, bias, X), plan, ref_ffm_bwd(v, X, gz, plan)
