"""Reference readings of the SINE kernels and layer (csrc/sine.hip, layers.SINELayer), written from the formulas (a)-(g)
of include/mi355rec.h: an fp64 numpy forward with a hand-derived backward of the sparse-interest extractor and of the
auxiliary loss, a torch-CPU transcription of both and of the whole layer whose gradients come from autograd (fp32: the
error floor of the tolerance; fp64: the check of the hand-derived backward), the generators of the test cases and the
near-tie rule of the top-K.

Generators: table and pool ~ N(0, 0.5), W1, W3, Wk1 ~ N(0, 1 / sqrt(D)), W2, W4, Wk2 ~ N(0, 1 / sqrt(D)), every value
fp32-exact.  The first four examples of a case have 0, 1, 2 and T padded positions (comirec_ref.comirec_series); only
the FIRST series feature carries the padding id.

The mask of (a) is the additive -1e9f in fp32: the fp64 readings round the masked score to fp32 the way the addition
does (its value; the gradient is the addition's, 1), so that a row padded throughout attends uniformly in fp64 too.

The top-K is a kink: an example is NEAR A TIE when, in fp64, sim_(K) - sim_(K+1) < GAP_EPS (never when K == L).  Near-tie
examples of a body case are left out of out and chosen, their rows of gout are zero on both sides, and they may be at
most 10 % of a case; the seed of a layer case is the first of 1, 2, 3, ... with none at all."""
import functools

import numpy as np
import torch

from tests import mind_ref as MR
from tests.comirec_ref import comirec_series
from tests.mind_ref import V_CASE, f32_exact, gather, rel_err  # noqa: F401
from tests.masknet_ref import clean_seed

# (B, T, C, E, L, K)
CASES = [(1, 1, 1, 1, 1, 1), (3, 5, 1, 8, 4, 4), (33, 6, 3, 16, 100, 5), (33, 50, 3, 16, 100, 5), (33, 65, 3, 8, 33, 16),
         (17, 33, 3, 16, 7, 1), (5, 9, 4, 64, 100, 5), (2049, 10, 3, 16, 100, 5)]
SKEW_CASE = (40, 7, 3, 16, 100, 5)             # every example shares one series row
GAP_EPS = 1e-4
TAU, LN_EPS = 0.1, 1e-3
WEIGHTS = ("pool", "W1", "W2", "Wk1", "Wk2", "W3", "W4")
MASK = np.float32(-1e9)

# the slab plan of the backward, as csrc/sine.hip and the header state it
SLAB_BYTES, SLAB_MAX = 64 << 20, 2048


def slab_examples(B, D, K):
    return min(B, min(SLAB_MAX, max(1, SLAB_BYTES // 4 // (K * (D * D + 2 * D)))))


def scratch_bytes(B, D, K):
    n = slab_examples(B, D, K)
    grid = min(n, 1024 if ((D + 31) // 32) ** 2 <= 4 else 256)
    return 4 * (n * K * (D * D + 2 * D) + grid * (2 * D * D + 2 * D) + 4)


def _softmax(z, axis):
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def _ln(r, eps):
    mu = r.mean(-1, keepdims=True)
    rs = 1.0 / np.sqrt(((r - mu) ** 2).mean(-1, keepdims=True) + eps)
    return (r - mu) * rs, rs


def _ln_bwd(y, rs, dy):
    return rs * (dy - dy.mean(-1, keepdims=True) - y * (dy * y).mean(-1, keepdims=True))


def top_k(sim, K):
    """tf.math.top_k: descending, the lower index first on equal values"""
    return np.argsort(-sim, axis=1, kind="stable")[:, :K]


def boundary_gap(sim, K):
    """sim_(K) - sim_(K+1) per example; inf when K == L"""
    if K == sim.shape[1]:
        return np.full(len(sim), np.inf)
    top = -np.sort(-sim, axis=1)
    return top[:, K - 1] - top[:, K]


def sine_numpy(table, series, w, K, tau=TAU, eps=LN_EPS, pad=0, gout=None, chosen=None):
    """fp64.  w: dict of WEIGHTS.  -> out [B,D], chosen [B,K], sim [B,L], a [B,T] and, with gout, gkeys [B,T,D] and the
    gradient of every weight under its name prefixed with d"""
    pool, W1, W2, Wk1, Wk2, W3, W4 = (np.asarray(w[k], np.float64) for k in WEIGHTS)
    x = gather(table, series)
    B, T, D = x.shape
    padm = series[:, :, 0] == pad
    H1 = np.tanh(x @ W1)
    s = H1 @ W2
    sm = np.where(padm, (s.astype(np.float32) + MASK).astype(np.float64), s)
    a = _softmax(sm, 1)
    z = np.einsum("bt,btd->bd", a, x)
    sim = z @ pool.T
    idx = top_k(sim, K) if chosen is None else np.asarray(chosen, np.int64)
    g = 1.0 / (1.0 + np.exp(-np.take_along_axis(sim, idx, 1)))
    pk = pool[idx]
    Cu = g[..., None] * pk
    Cn, rsC = _ln(Cu, eps)
    Yn, rsY = _ln(x @ W3, eps)
    P = _softmax(np.einsum("btd,bkd->btk", Yn, Cn), -1)
    Hk = np.stack([np.tanh(np.einsum("btd,bde->bte", x, Wk1[idx[:, k]])) for k in range(K)], 1)      # [B,K,T,D]
    wk2 = Wk2[idx]
    A = _softmax(np.einsum("bkte,bke->bkt", Hk, wk2), -1)
    Pt = P.transpose(0, 2, 1)
    Z, rsZ = _ln(np.einsum("bkt,btd->bkd", Pt * A, x), eps)
    Xh = np.einsum("btk,bkd->btd", P, Cu)
    H3 = np.tanh(Xh @ W3)
    bb = _softmax(H3 @ W4, 1)
    cap, rscap = _ln(np.einsum("bt,btd->bd", bb, Xh), eps)
    e = _softmax(np.einsum("bd,bkd->bk", cap, Z) / tau, 1)
    res = dict(out=np.einsum("bk,bkd->bd", e, Z), chosen=idx.astype(np.int32), sim=sim, a=a)
    if gout is None:
        return res
    # (g)
    de = np.einsum("bd,bkd->bk", gout, Z)
    dl = e * (de - (e * de).sum(1, keepdims=True)) / tau
    dcap = np.einsum("bk,bkd->bd", dl, Z)
    dZ = e[..., None] * gout[:, None, :] + dl[..., None] * cap[:, None, :]
    # (f)
    dcapu = _ln_bwd(cap, rscap, dcap)
    dZu = _ln_bwd(Z, rsZ, dZ)
    db = np.einsum("bd,btd->bt", dcapu, Xh)
    dr = bb * (db - (bb * db).sum(1, keepdims=True))
    dW4 = np.einsum("bt,btd->d", dr, H3)
    dpre3 = dr[..., None] * W4 * (1 - H3 * H3)
    dW3 = np.einsum("btd,bte->de", Xh, dpre3)
    dXh = bb[..., None] * dcapu[:, None, :] + dpre3 @ W3.T
    dP = np.einsum("btd,bkd->btk", dXh, Cu)
    dCu = np.einsum("btk,btd->bkd", P, dXh)
    # (e)
    dw = np.einsum("bkd,btd->bkt", dZu, x)
    dX = np.einsum("bkt,bkd->btd", Pt * A, dZu)
    dP = dP + (A * dw).transpose(0, 2, 1)
    dA = Pt * dw
    # (d)
    dq = A * (dA - (A * dA).sum(-1, keepdims=True))
    dWk1, dWk2, dpool = np.zeros_like(Wk1), np.zeros_like(Wk2), np.zeros_like(pool)
    np.add.at(dWk2, idx, np.einsum("bkt,bktd->bkd", dq, Hk))
    dprek = dq[..., None] * wk2[:, :, None, :] * (1 - Hk * Hk)
    for k in range(K):
        np.add.at(dWk1, idx[:, k], np.einsum("btd,bte->bde", x, dprek[:, k]))
        dX += np.einsum("bte,bde->btd", dprek[:, k], Wk1[idx[:, k]])
    # (c)
    dS = P * (dP - (P * dP).sum(-1, keepdims=True))
    dCu = dCu + _ln_bwd(Cn, rsC, np.einsum("btk,btd->bkd", dS, Yn))
    dY = _ln_bwd(Yn, rsY, np.einsum("btk,bkd->btd", dS, Cn))
    dW3 = dW3 + np.einsum("btd,bte->de", x, dY)
    dX += dY @ W3.T
    # (b)
    dsim = (dCu * pk).sum(-1) * g * (1 - g)
    np.add.at(dpool, idx, g[..., None] * dCu + dsim[..., None] * z[:, None, :])
    dz = np.einsum("bk,bkd->bd", dsim, pk)
    # (a)
    dX += a[..., None] * dz[:, None, :]
    da = np.einsum("bd,btd->bt", dz, x)
    ds = a * (da - (a * da).sum(1, keepdims=True))
    dW2 = np.einsum("bt,btd->d", ds, H1)
    dpre1 = ds[..., None] * W2 * (1 - H1 * H1)
    dX += dpre1 @ W1.T
    res.update(gkeys=dX, dpool=dpool, dW1=np.einsum("btd,bte->de", x, dpre1), dW2=dW2, dWk1=dWk1, dWk2=dWk2, dW3=dW3,
               dW4=dW4)
    return res


def _ln_t(r, eps):
    mu = r.mean(-1, keepdim=True)
    return (r - mu) * torch.rsqrt(((r - mu) ** 2).mean(-1, keepdim=True) + eps)


def sine_torch(x, padm, w, idx, tau=TAU, eps=LN_EPS):
    """SINELayer.generate_user_interest on looked-up rows x [B,T,D] with the concepts idx [B,K] (int64) given, or with
    idx = K selected by torch.topk (whose order on equal values is its own: for timing, not for parity): the reference's
    five methods in its order, its LayerNormalization layers written out"""
    pool, W1, W2, Wk1, Wk2, W3, W4 = (w[k] for k in WEIGHTS)
    s = torch.einsum("bne,e->bn", torch.tanh(torch.einsum("bnd,de->bne", x, W1)), W2)
    masked = (s.detach().float() - 1e9).to(s.dtype) + (s - s.detach())                     # the fp32 value, gradient 1
    a = torch.softmax(torch.where(padm, masked, s), dim=1)
    z = torch.einsum("bn,bnd->bd", a, x)
    sim = z @ pool.T
    if isinstance(idx, int):
        idx = torch.topk(sim.detach(), idx, dim=1).indices
    g = torch.sigmoid(torch.gather(sim, 1, idx))
    Cu = pool[idx] * g[..., None]
    P = torch.softmax(torch.einsum("bnd,bkd->bnk", _ln_t(torch.einsum("bnd,de->bne", x, W3), eps), _ln_t(Cu, eps)), -1)
    Hk = torch.tanh(torch.einsum("bnd,bkde->bnke", x, Wk1[idx]))
    A = torch.softmax(torch.einsum("bnkd,bkd->bkn", Hk, Wk2[idx]), -1)
    Z = _ln_t(torch.einsum("bnk,bnd->bkd", P * A.transpose(1, 2), x), eps)
    Xh = torch.einsum("bnk,bkd->bnd", P, Cu)
    bb = torch.softmax(torch.einsum("bnd,d->bn", torch.tanh(torch.einsum("bnd,dm->bnm", Xh, W3)), W4), -1)
    cap = _ln_t(torch.einsum("bn,bnd->bd", bb, Xh), eps)
    e = torch.softmax(torch.einsum("bd,bkd->bk", cap, Z) / tau, 1)
    return torch.einsum("bk,bkd->bd", e, Z), sim


def sine_torch_grads(table, series, w, idx, gout, dtype, pad=0):
    t = lambda v: torch.tensor(np.asarray(v), dtype=dtype)
    x = t(gather(table, series)).requires_grad_()
    wt = {k: t(w[k]).requires_grad_() for k in WEIGHTS}
    out, _ = sine_torch(x, torch.from_numpy(series[:, :, 0] == pad), wt, torch.from_numpy(np.asarray(idx, np.int64)))
    (out * t(gout)).sum().backward()
    res = {"d" + k: v.grad.numpy() for k, v in wt.items()}
    res.update(out=out.detach().numpy(), gkeys=x.grad.numpy())
    return res


def make_weights(r, D, L):
    sd = 1 / np.sqrt(D)
    return dict(pool=f32_exact(r.normal(0, 0.5, (L, D))), W1=f32_exact(r.normal(0, sd, (D, D))),
                W2=f32_exact(r.normal(0, sd, D)), Wk1=f32_exact(r.normal(0, sd, (L, D, D))),
                Wk2=f32_exact(r.normal(0, sd, (L, D))), W3=f32_exact(r.normal(0, sd, (D, D))),
                W4=f32_exact(r.normal(0, sd, D)))


@functools.lru_cache(maxsize=None)
def inputs(*case):
    """-> table, series, w, gout and near [B] bool (the near-tie examples on the fp64 reading, whose rows of gout are
    zero already)"""
    B, T, C, E, L, K = case
    r = np.random.default_rng(7)
    D = C * E
    c = dict(table=f32_exact(r.normal(0, 0.5, (V_CASE, E))), w=make_weights(r, D, L),
             series=comirec_series(r, B, T, C, V_CASE), gout=f32_exact(r.uniform(-1, 1, (B, D))), K=K)
    if case == SKEW_CASE:
        c["series"][:] = c["series"][4]
    c["near"] = boundary_gap(sine_numpy(c["table"], c["series"], c["w"], K)["sim"], K) < GAP_EPS
    c["gout"][c["near"]] = 0.0
    return c


@functools.lru_cache(maxsize=None)
def ref(case):
    c = inputs(*case)
    return sine_numpy(c["table"], c["series"], c["w"], c["K"], gout=c["gout"])


@functools.lru_cache(maxsize=None)
def case_t(case, dtype):
    c = inputs(*case)
    return sine_torch_grads(c["table"], c["series"], c["w"], ref(case)["chosen"], c["gout"], dtype)


# ---- aux -------------------------------------------------------------------------------------------------------------
def aux_numpy(pool, gloss=None):
    """fp64.  -> loss and, with gloss, dpool.  The one deliberate deviation from the reference: it writes the loss as
    0.5 square(norm), whose gradient is NaN at a zero off-diagonal; here that gradient is zero."""
    Cc = pool - pool.mean(0, keepdims=True)
    M = Cc @ Cc.T
    off = M - np.diag(np.diag(M))
    res = dict(loss=0.5 * (off * off).sum())
    if gloss is not None:
        dCc = gloss * 2.0 * off @ Cc
        res["dpool"] = dCc - dCc.mean(0, keepdims=True)
    return res


def aux_torch(pool):
    Cc = pool - pool.mean(0, keepdim=True)
    M = Cc @ Cc.T
    off = M - torch.diag(torch.diagonal(M))
    return 0.5 * (off * off).sum()


def aux_torch_grads(pool, gloss, dtype):
    p = torch.tensor(np.asarray(pool), dtype=dtype).requires_grad_()
    loss = aux_torch(p)
    (loss * gloss).backward()
    return dict(loss=loss.detach().numpy(), dpool=p.grad.numpy())


# (L, D)
AUX_CASES = [(1, 1), (2, 3), (7, 48), (100, 48), (33, 256), (1024, 5)]


@functools.lru_cache(maxsize=None)
def aux_pool(L, D):
    return f32_exact(np.random.default_rng(11).normal(0, 0.5, (L, D)))


# ---- the layer ---------------------------------------------------------------------------------------------------------
ITEM, SERIES = MR.ITEM, MR.SERIES
LAYER_V, LAYER_E, LAYER_NS, LAYER_B, LAYER_TS = MR.LAYER_V, MR.LAYER_E, MR.LAYER_NS, MR.LAYER_B, MR.LAYER_TS
LAYER_D = LAYER_E * len(SERIES)
LAYER_L, LAYER_K = 100, 5
STATE_SHAPES = {"embed.embeddings": (LAYER_V, LAYER_E), "interest_pool": (LAYER_L, LAYER_D), "W1": (LAYER_D, LAYER_D),
                "W2": (LAYER_D,), "Wk1": (LAYER_L, LAYER_D, LAYER_D), "Wk2": (LAYER_L, LAYER_D),
                "W3": (LAYER_D, LAYER_D), "W4": (LAYER_D,)}
REFERENCE_SIGNATURE = [("item_categorical_features", ["label_goods_ids", "label_shop_ids", "label_cate_ids"]),
                       ("behavior_series_features", ["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"]),
                       ("feature_dims", 160000), ("embedding_dims", 16), ("padding_index", 0), ("L", 100), ("K", 5),
                       ("tau", 0.1)]


def layer_state(seed):
    r = np.random.default_rng(seed)
    w = make_weights(r, LAYER_D, LAYER_L)
    sd = {"embed.embeddings": f32_exact(r.normal(0, 0.5, (LAYER_V, LAYER_E))), "interest_pool": w["pool"]}
    sd.update({k: w[k] for k in WEIGHTS[1:]})
    assert {k: v.shape for k, v in sd.items()} == STATE_SHAPES
    return sd


def layer_inputs(seed, B, T):
    """mind_ref's batch with the series' first feature re-drawn: the first four rows get 0, 1, 2 and T padded positions"""
    ins = {k: v for k, v in MR.layer_inputs(seed, B, T).items() if k in ITEM + SERIES}
    r = np.random.default_rng(3000 + seed)
    for b, n in enumerate(np.minimum([0, 1, 2, T], T)[:B]):
        ins[SERIES[0]][b] = r.integers(1, LAYER_V, T)
        ins[SERIES[0]][b, r.permutation(T)[:n]] = 0
    return ins


def layer_torch(sd, ins, dtype, gui=None, gmain=None, gaux=None):
    """SINELayer.call on the CPU.  -> dict(user_interest, main_loss, aux_loss, chosen, gap [B]) and, with the three
    upstream gradients, grads of every parameter"""
    P = {k: torch.tensor(v, dtype=dtype).requires_grad_() for k, v in sd.items()}
    series = torch.from_numpy(np.stack([ins[n] for n in SERIES], axis=2))
    items = torch.from_numpy(np.stack([ins[n] for n in ITEM], axis=2))
    B, T, C = series.shape
    tab = P["embed.embeddings"]
    x = tab[series].reshape(B, T, -1)
    w = dict(P, pool=P["interest_pool"])
    padm = series[:, :, 0] == 0
    with torch.no_grad():
        sim = sine_torch(x, padm, w, torch.zeros(B, LAYER_K, dtype=torch.int64))[1].numpy()
    idx = top_k(sim, LAYER_K)
    ui, _ = sine_torch(x, padm, w, torch.from_numpy(idx))
    inner = torch.einsum("bne,be->bn", tab[items].reshape(B, items.shape[1], -1), ui)
    main = torch.logsumexp(inner, dim=1) - inner[:, 0]
    aux = aux_torch(P["interest_pool"])
    res = dict(user_interest=ui.detach().numpy(), main_loss=main.detach().numpy(), aux_loss=aux.detach().numpy(),
               chosen=idx.astype(np.int32), gap=boundary_gap(sim, LAYER_K))
    if gui is not None:
        t = lambda v: torch.tensor(v, dtype=dtype)
        ((ui * t(gui)).sum() + (main * t(gmain)).sum() + aux * gaux).backward()
        res["grads"] = {k: p.grad.numpy() for k, p in P.items()}
    return res


@functools.lru_cache(maxsize=None)
def layer_seed(T, B=LAYER_B):
    """the first seed 1, 2, 3, ... whose fp64 reading has no near-tie example at all"""
    def near(seed):
        res = layer_torch(layer_state(seed), layer_inputs(seed, B, T), torch.float64)
        return bool((res["gap"] < GAP_EPS).any())
    return clean_seed(near)


def layer_upstream(seed, B=LAYER_B):
    r = np.random.default_rng(2000 + seed)
    return f32_exact(r.uniform(-1, 1, (B, LAYER_D))), f32_exact(r.uniform(-1, 1, B)), 0.25
