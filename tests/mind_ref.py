"""Reference readings of the MIND kernels and layers (csrc/mind.hip, layers.MINDLayer), written from the formulas of
include/mi355rec.h: an fp64 numpy forward with a hand-derived backward of the capsule routing and of the label-aware
attention + sampled-softmax loss, a torch-CPU transcription of both and of the whole layer whose gradients come from
autograd (fp32: the error floor of the tolerance; fp64: the check of the hand-derived backward), the generators of the
test cases, and rel_err.

Generators: table ~ N(0, 0.5), S ~ N(0, 1 / sqrt(D)), B0 ~ N(0, 0.05), every value fp32-exact.  The first four examples
of a routing case have 0, 1, 2 and T valid positions (at most T), the others draw the number uniformly from 0..T and
scatter the padding over the row; only the FIRST series feature carries the padding id, the others hold any id.  The
valid capsule count of an attention case cycles through 0..K."""
import functools

import numpy as np
import torch

from tests.masknet_ref import PRE_EPS, clean_seed, glorot, rel_err  # noqa: F401

FMIN = float(np.finfo(np.float32).min)         # tf.float32.min: the lowest finite float
LN_EPS = BN_EPS = 1e-3
V_CASE = 211

# (B, T, C, E, Dc, K, R)
ROUTING_CASES = [(1, 1, 1, 1, 1, 1, 1), (3, 5, 1, 8, 8, 4, 3), (33, 6, 3, 16, 48, 4, 3), (33, 50, 3, 16, 48, 4, 3),
                 (33, 65, 3, 8, 40, 16, 3), (17, 6, 3, 16, 48, 4, 1), (17, 6, 3, 16, 48, 4, 5), (17, 33, 3, 16, 48, 1, 3),
                 (5, 33, 4, 64, 256, 16, 3), (2049, 50, 3, 16, 48, 4, 3)]
# (B, Ns, C, E, K)
LAA_CASES = [(1, 1, 1, 1, 1), (3, 2, 1, 8, 4), (33, 11, 3, 16, 4), (33, 65, 3, 16, 16), (5, 33, 4, 64, 16),
             (2049, 11, 3, 16, 4)]
# the capsule count of an example with n valid behaviours at K = 4: the values the layer's host table must reproduce
COUNT_K4 = {0: 0, 1: 0, 2: 1, 3: 1, 4: 2, 7: 2, 8: 3, 15: 3, 16: 4, 100: 4}


def f32_exact(a):
    return np.asarray(a, np.float32).astype(np.float64)


def _softmax(z, axis):
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def gather(table, ids):
    """rows of the ids, concatenated over the last id axis; an id outside the table is a zero row"""
    V = table.shape[0]
    ok = (ids >= 0) & (ids < V)
    rows = np.where(ok[..., None], table[np.clip(ids, 0, V - 1)], 0.0)
    return rows.reshape(ids.shape[:-1] + (-1,))


def series_ids(r, B, T, C, V, pad=0):
    n_valid = r.integers(0, T + 1, B)
    n_valid[:4] = np.minimum([0, 1, 2, T], T)[:B]
    ids = r.integers(1, V, (B, T, C))
    for b in range(B):
        ids[b, r.permutation(T)[n_valid[b]:], 0] = pad
    return ids.astype(np.int64)


# ---- capsule routing ----------------------------------------------------------------------------------------------------
def routing_numpy(table, series, S, B0, R, pad=0, gout=None):
    """fp64.  -> out [B,K,Dc], W (the weights of the last round) and, with gout, gkeys [B,T,D] and dS [D,Dc]"""
    x = gather(table, series)
    valid = (series[:, :, 0] != pad)[:, None, :]
    u = x @ S
    L = np.broadcast_to(B0, (len(x),) + B0.shape).copy()
    Ws, ss = [], []
    for r in range(R):
        W = _softmax(np.where(valid, L, FMIN), axis=2)
        s = W @ u
        n2 = (s * s).sum(-1, keepdims=True)
        c = s * np.sqrt(n2) / (1 + n2)
        Ws.append(W)
        ss.append(s)
        if r < R - 1:
            L = L + c @ u.transpose(0, 2, 1)
    res = dict(out=c, W=Ws[-1], valid=valid[:, 0, :])
    if gout is None:
        return res
    du, dL = np.zeros_like(u), np.zeros_like(L)
    for r in range(R - 1, -1, -1):
        W, s = Ws[r], ss[r]
        n2 = (s * s).sum(-1, keepdims=True)
        n = np.sqrt(n2)
        f = n / (1 + n2)
        dc = gout if r == R - 1 else dL @ u
        if r < R - 1:
            du += dL.transpose(0, 2, 1) @ (s * f)
        g = np.where(n > 0, (1 - n2) / ((1 + n2) ** 2 * np.where(n > 0, n, 1.0)), 0.0)
        ds = f * dc + s * g * (s * dc).sum(-1, keepdims=True)
        dW = ds @ u.transpose(0, 2, 1)
        du += W.transpose(0, 2, 1) @ ds
        dL = dL + np.where(valid, W * (dW - (dW * W).sum(-1, keepdims=True)), 0.0)
    res["gkeys"] = du @ S.T
    res["dS"] = np.einsum("btd,btc->dc", x, du)
    return res


def routing_torch(x, valid, S, B0, R):
    """x [B,T,D] looked-up rows, valid [B,T] bool -> the capsules [B,K,Dc]; MultiInterestExtractorLayer.call with the
    squash written as c n / (1 + n^2)"""
    u = x @ S
    L = B0[None].expand(x.shape[0], -1, -1)
    drop = torch.full_like(L, FMIN)
    for i in range(R):
        W = torch.softmax(torch.where(valid[:, None, :], L, drop), dim=2)
        s = W @ u
        n = torch.linalg.vector_norm(s, dim=2, keepdim=True)
        c = s * n / (1 + n * n)
        if i < R - 1:
            L = L + c @ u.transpose(1, 2)
    return c


def routing_torch_grads(table, series, S, B0, R, gout, dtype, pad=0):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x = t(gather(table, series)).requires_grad_()
    St = t(S).requires_grad_()
    out = routing_torch(x, torch.from_numpy(series[:, :, 0] != pad), St, t(B0), R)
    (out * t(gout)).sum().backward()
    return dict(out=out.detach().numpy(), gkeys=x.grad.numpy(), dS=St.grad.numpy())


@functools.lru_cache(maxsize=None)
def routing_case(*case):
    B, T, C, E, Dc, K, R = case
    r = np.random.default_rng(1)
    D = C * E
    c = dict(table=f32_exact(r.normal(0, 0.5, (V_CASE, E))), S=f32_exact(r.normal(0, 1 / np.sqrt(D), (D, Dc))),
             B0=f32_exact(r.normal(0, 0.05, (K, T))), series=series_ids(r, B, T, C, V_CASE),
             gout=f32_exact(r.uniform(-1, 1, (B, K, Dc))), R=R)
    c["ref"] = routing_numpy(c["table"], c["series"], c["S"], c["B0"], R, 0, c["gout"])
    return c


@functools.lru_cache(maxsize=None)
def routing_case_t(case, dtype):
    c = routing_case(*case)
    return routing_torch_grads(c["table"], c["series"], c["S"], c["B0"], c["R"], c["gout"], dtype)


def routed_share(ref):
    """share of the (b, k) rows with two or more valid positions whose last-round weights have max / min >= 2 over the
    valid positions (None: no such row)"""
    W, valid = ref["W"], ref["valid"]
    hit = tot = 0
    for b in np.nonzero(valid.sum(1) >= 2)[0]:
        w = W[b][:, valid[b]]
        hit += int((w.max(1) / w.min(1) >= 2).sum())
        tot += len(w)
    return hit / tot if tot else None


# ---- label-aware attention + sampled-softmax loss ------------------------------------------------------------------
def laa_numpy(table, items, m, kv, gout=None, gloss=None):
    """fp64.  -> out [B,Ns], loss [B] and, with gout and / or gloss, gm [B,K,Dc] and gitems [B,Ns,Dc]"""
    x = gather(table, items)
    K = m.shape[1]
    sc = np.einsum("bkd,bsd->bks", m, x)
    mask = np.arange(K)[None, :, None] < kv[:, None, None]
    w = _softmax(np.where(mask, sc, FMIN), axis=1)
    out = (w * sc).sum(1)
    mx = out.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(out - mx).sum(1))
    res = dict(out=out, loss=lse - out[:, 0])
    if gout is None and gloss is None:
        return res
    g = np.zeros_like(out) if gout is None else gout.copy()
    if gloss is not None:
        p = np.exp(out - lse[:, None])
        p[:, 0] -= 1.0
        g = g + gloss[:, None] * p
    dsc = g[:, None, :] * (w + np.where(mask, w * (sc - out[:, None, :]), 0.0))
    res["gm"] = np.einsum("bks,bsd->bkd", dsc, x)
    res["gitems"] = np.einsum("bks,bkd->bsd", dsc, m)
    return res


def laa_torch(x, m, kv):
    """x [B,Ns,Dc] looked-up items, m [B,K,Dc], kv [B] -> (out [B,Ns], loss [B]): LabelAwareAttention.call, the inner
    products and compute_loss of MINDLayer"""
    K = m.shape[1]
    sc = torch.einsum("bck,bsk->bcs", m, x)
    mask = torch.arange(K)[None, :, None] < kv[:, None, None]
    w = torch.softmax(torch.where(mask, sc, torch.full_like(sc, FMIN)), dim=1)
    att = torch.einsum("bck,bcs->bsk", m, w)
    out = (att * x).sum(-1)
    return out, torch.logsumexp(out, dim=1) - out[:, 0]


def laa_torch_grads(table, items, m, kv, gout, gloss, dtype):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x, mt = t(gather(table, items)).requires_grad_(), t(m).requires_grad_()
    out, loss = laa_torch(x, mt, torch.from_numpy(kv))
    tot = 0
    if gout is not None:
        tot = tot + (out * t(gout)).sum()
    if gloss is not None:
        tot = tot + (loss * t(gloss)).sum()
    tot.backward()
    return dict(out=out.detach().numpy(), loss=loss.detach().numpy(), gm=mt.grad.numpy(), gitems=x.grad.numpy())


@functools.lru_cache(maxsize=None)
def laa_case(*case):
    B, Ns, C, E, K = case
    r = np.random.default_rng(2)
    return dict(table=f32_exact(r.normal(0, 0.5, (V_CASE, E))), items=r.integers(0, V_CASE, (B, Ns, C)).astype(np.int64),
                m=f32_exact(r.normal(0, 0.5, (B, K, C * E))), kv=(np.arange(B) % (K + 1)).astype(np.int32),
                gout=f32_exact(r.uniform(-1, 1, (B, Ns))), gloss=f32_exact(r.uniform(-1, 1, B)))


LAA_WAYS = {"gout": (True, False), "gloss": (False, True), "both": (True, True)}


def laa_way(c, way):
    use_out, use_loss = LAA_WAYS[way]
    return (c["gout"] if use_out else None), (c["gloss"] if use_loss else None)


# ---- the layer -----------------------------------------------------------------------------------------------------
USER = ["uid", "utag1", "utag2", "utag3", "utag4"]
ITEM = ["label_goods_ids", "label_shop_ids", "label_cate_ids"]
SERIES = ["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"]
LAYER_V, LAYER_E, LAYER_K, LAYER_R, LAYER_NS = 1000, 16, 4, 3, 11
STATE_KEYS = ["MIE_layer.B", "MIE_layer.S", "context_bn.beta", "context_bn.gamma", "context_bn.moving_mean",
              "context_bn.moving_variance", "context_mlp.bias", "context_mlp.kernel", "embed.embeddings",
              "final_mlp.layers.0.bias", "final_mlp.layers.0.kernel", "final_mlp.layers.1.beta",
              "final_mlp.layers.1.gamma", "final_mlp.layers.3.bias", "final_mlp.layers.3.kernel",
              "final_mlp.layers.4.beta", "final_mlp.layers.4.gamma"]
BUFFERS = ("MIE_layer.B", "context_bn.moving_mean", "context_bn.moving_variance")


def capsule_count(n_valid, K):
    """the numpy-float32 reading of 6.MIND/CustomLayers.py:214-218: capsule k is masked where k + 1 > min(log(n) / log(2.), K)"""
    with np.errstate(divide="ignore"):
        v = np.minimum(np.log(np.asarray(n_valid, np.float32)) / np.log(np.float32(2.)), np.float32(K))
    return (~((np.arange(K, dtype=np.float32) + np.float32(1))[None, :] > v.reshape(-1, 1))).sum(1).astype(np.int32)


def layer_state(seed, T):
    r = np.random.default_rng(seed)
    D = LAYER_E * len(SERIES)
    half, n_user = D // 2, LAYER_E * len(USER)
    sd = {"embed.embeddings": r.normal(0, 0.5, (LAYER_V, LAYER_E)), "MIE_layer.S": r.normal(0, 1 / np.sqrt(D), (D, D)),
          "MIE_layer.B": r.normal(0, 0.05, (LAYER_K, T)), "context_mlp.kernel": glorot(r, n_user, half),
          "context_mlp.bias": r.normal(0, 0.1, half), "context_bn.gamma": r.uniform(0.5, 1.5, half),
          "context_bn.beta": r.normal(0, 0.1, half), "context_bn.moving_mean": r.normal(0.5, 0.1, half),
          "context_bn.moving_variance": r.uniform(0.5, 1.5, half)}
    d = half + D
    for i, units in ((0, 4 * D), (3, D)):
        sd["final_mlp.layers.%d.kernel" % i] = glorot(r, d, units)
        sd["final_mlp.layers.%d.bias" % i] = r.normal(0, 0.1, units)
        sd["final_mlp.layers.%d.gamma" % (i + 1)] = r.uniform(0.5, 1.5, units)
        sd["final_mlp.layers.%d.beta" % (i + 1)] = r.normal(0, 0.1, units)
        d = units
    assert sorted(sd) == STATE_KEYS
    return {k: f32_exact(v) for k, v in sd.items()}


def layer_inputs(seed, B, T):
    r = np.random.default_rng(1000 + seed)
    ins = {n: r.integers(0, LAYER_V, B).astype(np.int64) for n in USER}
    series = series_ids(r, B, T, len(SERIES), LAYER_V)
    for i, n in enumerate(SERIES):
        ins[n] = np.ascontiguousarray(series[:, :, i])
    items = r.integers(0, LAYER_V, (B, LAYER_NS, len(ITEM)))
    for i, n in enumerate(ITEM):
        ins[n] = np.ascontiguousarray(items[:, :, i]).astype(np.int64)
    return ins


def layer_torch(sd, ins, dtype, training, gout=None, gloss=None):
    """MINDLayer.call / generate_interest_capsules on the CPU.  -> dict(output, loss, mlped, mask, kv, pre [B]: the
    smallest |relu pre-activation| of each example) and, with gout / gloss, grads of every trainable parameter"""
    P = {k: torch.tensor(v, dtype=dtype) for k, v in sd.items()}
    for k in P:
        if k not in BUFFERS:
            P[k].requires_grad_()
    series = torch.from_numpy(np.stack([ins[n] for n in SERIES], axis=2))
    items = torch.from_numpy(np.stack([ins[n] for n in ITEM], axis=2))
    Xc = torch.from_numpy(np.stack([ins[n] for n in USER], axis=1))
    B, T, C = series.shape
    tab = P["embed.embeddings"]
    valid = series[:, :, 0] != 0
    caps = routing_torch(tab[series].reshape(B, T, -1), valid, P["MIE_layer.S"], P["MIE_layer.B"], LAYER_R)
    kv = torch.from_numpy(capsule_count(valid.sum(1).numpy(), LAYER_K))
    h = torch.sigmoid(tab[Xc].reshape(B, -1) @ P["context_mlp.kernel"] + P["context_mlp.bias"])
    if training:
        mean = h.mean(0)
        var = torch.square(h - mean).mean(0)
    else:
        mean, var = P["context_bn.moving_mean"], P["context_bn.moving_variance"]
    h = (h - mean) * torch.rsqrt(var + BN_EPS) * P["context_bn.gamma"] + P["context_bn.beta"]
    a = torch.cat([h[:, None, :].expand(-1, LAYER_K, -1), caps], dim=2).reshape(B * LAYER_K, -1)
    pre = []
    for i in (0, 3):
        z = a @ P["final_mlp.layers.%d.kernel" % i] + P["final_mlp.layers.%d.bias" % i]
        mu = z.mean(1, keepdim=True)
        zc = z - mu
        z = zc * torch.rsqrt(torch.square(zc).mean(1, keepdim=True) + LN_EPS)
        z = z * P["final_mlp.layers.%d.gamma" % (i + 1)] + P["final_mlp.layers.%d.beta" % (i + 1)]
        pre.append(z.detach().abs().reshape(B, -1).min(1).values)
        a = torch.relu(z)
    mlped = a.reshape(B, LAYER_K, -1)
    out, loss = laa_torch(tab[items].reshape(B, items.shape[1], -1), mlped, kv)
    res = dict(output=out.detach().numpy(), loss=loss.detach().numpy(), mlped=mlped.detach().numpy(),
               mask=(torch.arange(LAYER_K)[None, :] >= kv[:, None]).numpy(), kv=kv.numpy(),
               pre=torch.minimum(pre[0], pre[1]).numpy())
    if gout is not None:
        ((out * torch.tensor(gout, dtype=dtype)).sum() + (loss * torch.tensor(gloss, dtype=dtype)).sum()).backward()
        res["grads"] = {k: p.grad.numpy() for k, p in P.items() if k not in BUFFERS}
    return res


LAYER_B = 32
LAYER_TS = (6, 50)


@functools.lru_cache(maxsize=None)
def layer_seed(T, training):
    """the first seed 1, 2, 3, ... whose fp64 reading has no example with a relu pre-activation nearer to 0 than PRE_EPS"""
    def near(seed):
        res = layer_torch(layer_state(seed, T), layer_inputs(seed, LAYER_B, T), torch.float64, training)
        return bool((res["pre"] < PRE_EPS).any())
    return clean_seed(near)


def layer_upstream(seed):
    r = np.random.default_rng(2000 + seed)
    return f32_exact(r.uniform(-1, 1, (LAYER_B, LAYER_NS))), f32_exact(r.uniform(-1, 1, LAYER_B))
