"""What the SIM tests share (not a test file): the fp64 numpy reading of SIM's soft search fused with the GSU pooling
(7.SIM/CustomLayers.py:88-96, 236-260) and of Keras' MultiHeadAttention with one query (:159, 191-196), each with its
hand-derived backward; a torch transcription in the reference's operation order parametrised by dtype (autograd, the
einsum form of Keras' attention); the layer-level transcription; the inputs of a case from a fixed seed; the case list.

TensorFlow and Keras are not available: the definition is the one include/mi355rec.h states.  Both readings apply the
mask as float32(l + (1 - m) * (-1e9)), so a row whose positions are all masked attends uniformly, and both order the
search by a stable descending sort (tf.argsort(direction='DESCENDING'): the lower index first among equals).

Two conditions are asserted here, on the CPU, for every case (none is skipped or filtered; the seeds in CASES were chosen
so that the reference alone satisfies both), so that the selection is never a rounding accident:
  1. in every row, any two valid steps whose keys are not bit-identical differ in fp64 score by more than 1e-3 max|score|
     of the row (steps with identical keys tie exactly and are ordered by index);
  2. every attention logit satisfies |l| <= 16."""
import numpy as np
import torch

from tests import dien_ref as DR

V_CASE = 200
POOL = 5                       # distinct items a row draws its behaviours from: repeats are the normal case
# (B, T, C, E, k, H) -> seed.  D = C E, K = min(k, T), dk = D
CASES = {(1, 1, 1, 4, 3, 1): 0, (33, 2, 1, 4, 3, 2): 0, (33, 7, 3, 16, 3, 8): 0, (65, 9, 1, 64, 4, 2): 1,
         (5, 300, 3, 16, 3, 8): 0, (3, 5, 1, 64, 1, 8): 0}
SMALLEST, DEFAULTS, RAGGED, LONG = (1, 1, 1, 4, 3, 1), (33, 7, 3, 16, 3, 8), (65, 9, 1, 64, 4, 2), (5, 300, 3, 16, 3, 8)
SEARCH_OUT, SEARCH_GRADS = ("scores", "pooled", "sel"), ("gkeys", "gq")
ATTN_OUT = ("out", "probs")
ATTN_GRADS = ("gq", "gx", "dWq", "dbq", "dWk", "dbk", "dWv", "dbv", "dWo", "dbo")
WEIGHTS = ("Wq", "bq", "Wk", "bk", "Wv", "bv", "Wo", "bo")
MASKS = ("zeros", "ones", "mixed", "search")
rel_err = DR.rel_err
lookup = DR.lookup


def dims(case):
    B, T, Cn, E, k, H = case
    return B, T, Cn, E, min(k, T), H, Cn * E


# ---- the search ---------------------------------------------------------------------------------------------------------
def search_numpy(c, gpooled=None, gsel=None):
    """fp64: scores, pooled, chosen, sel, sel_valid (and gkeys, gq from gpooled [B,D] and gsel [B,K,D] or None)"""
    x, q, valid, K = c["x"], c["q"], c["valid"], c["K"]
    raw = np.einsum("be,ble->bl", q, x)
    scores = raw * valid
    pooled = np.einsum("bl,ble->be", scores, x)
    rank = np.where(valid, raw, -np.inf)
    chosen = np.argsort(-rank, axis=-1, kind="stable")[:, :K]
    rows = np.arange(x.shape[0])[:, None]
    out = {"scores": scores, "pooled": pooled, "chosen": chosen, "sel": x[rows, chosen], "sel_valid": valid[rows, chosen],
           "raw": raw}
    if gpooled is not None:
        gs = np.einsum("be,ble->bl", gpooled, x) * valid
        gkeys = scores[..., None] * gpooled[:, None, :] + gs[..., None] * q[:, None, :]
        if gsel is not None:
            gkeys[rows, chosen] += gsel              # positions in a row are distinct
        out.update(gkeys=gkeys, gq=np.einsum("bl,ble->be", gs, x))
    return out


def _f64(t):
    return t.detach().to(torch.float64).numpy()


def search_torch(c, dtype, gpooled=None, gsel=None):
    """GSULayer.inner_product_attention and SIMLayer.soft_index_search, op for op, at ``dtype`` through autograd.  One
    op is spelled differently: the scores einsum('be,ble->bl') are a product and a row sum, which rounds a step's score
    from its key and q alone.  A blocked matrix product may round two steps with the SAME key differently by position,
    and the order among equal items would then be a rounding accident of the transcription itself."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x, q = t(c["x"]).requires_grad_(True), t(c["q"]).requires_grad_(True)
    valid, K = torch.from_numpy(c["valid"]), c["K"]
    inner = (q.unsqueeze(1) * x).sum(-1)                         # einsum('be,ble->bl'), see the docstring
    masked = inner * valid.to(dtype)
    pooled = torch.einsum("bl,ble->be", masked, x)
    ranked = torch.where(valid, inner, torch.full_like(inner, -np.inf))
    chosen = torch.sort(ranked, dim=-1, descending=True, stable=True).indices[:, :K]
    sel = torch.gather(x, 1, chosen.unsqueeze(-1).expand(-1, -1, x.shape[2]))
    out = {"scores": _f64(masked), "pooled": _f64(pooled), "chosen": chosen.numpy(), "sel": _f64(sel),
           "sel_valid": torch.gather(valid, 1, chosen).numpy()}
    if gpooled is not None:
        loss = (pooled * t(gpooled)).sum()
        if gsel is not None:
            loss = loss + (sel * t(gsel)).sum()
        gx, gq = torch.autograd.grad(loss, [x, q])
        out.update(gkeys=_f64(gx), gq=_f64(gq))
    return out


# ---- the attention ------------------------------------------------------------------------------------------------------
def masked_logits(l, m):
    """Keras' additive mask, applied in fp32 whatever the precision of l"""
    return (np.asarray(l, np.float32) + (np.float32(1) - np.asarray(m, np.float32)[:, None, :]) * np.float32(-1e9)) \
        .astype(np.float64)


def softmax(a):
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def attention_numpy(q, x, mask, w, gout=None, collapsed=False):
    """fp64 Keras MultiHeadAttention with one query q [B,D] over x [B,K,D], mask [B,K] (1 = attend); ``w`` maps WEIGHTS
    to arrays.  ``collapsed``: the one-query form the kernels use (no key or value projection) -- the same function."""
    Wq, bq, Wk, bk, Wv, bv, Wo, bo = (np.asarray(w[n], np.float64) for n in WEIGHTS)
    dk = Wq.shape[2]
    scale = 1.0 / np.sqrt(float(dk))
    Q = (np.einsum("bd,dhk->bhk", q, Wq) + bq) * scale
    if collapsed:
        u = np.einsum("dhk,bhk->bhd", Wk, Q)
        l = np.einsum("bjd,bhd->bhj", x, u) + np.einsum("hk,bhk->bh", bk, Q)[..., None]
    else:
        Kp = np.einsum("bjd,dhk->bjhk", x, Wk) + bk
        Vp = np.einsum("bjd,dhk->bjhk", x, Wv) + bv
        l = np.einsum("bhk,bjhk->bhj", Q, Kp)
    p = softmax(masked_logits(l, mask))
    if collapsed:
        s = np.einsum("bhj,bjd->bhd", p, x)
        o = np.einsum("bhd,dhk->bhk", s, Wv) + bv
    else:
        o = np.einsum("bhj,bjhk->bhk", p, Vp)
    out = {"out": np.einsum("bhk,hkd->bd", o, Wo) + bo, "probs": p, "logits": l}
    if gout is None or collapsed:
        return out
    go = np.einsum("bd,hkd->bhk", gout, Wo)
    gp = np.einsum("bhk,bjhk->bhj", go, Vp)
    dVp = np.einsum("bhj,bhk->bjhk", p, go)
    dl = p * (gp - (p * gp).sum(-1, keepdims=True))           # the Jacobian at p, for every j, masked or not
    dKp = np.einsum("bhj,bhk->bjhk", dl, Q)
    dQr = np.einsum("bhj,bjhk->bhk", dl, Kp) * scale
    out.update(dl=dl, gq=np.einsum("bhk,dhk->bd", dQr, Wq),
               gx=np.einsum("bjhk,dhk->bjd", dKp, Wk) + np.einsum("bjhk,dhk->bjd", dVp, Wv),
               dWq=np.einsum("bd,bhk->dhk", q, dQr), dbq=dQr.sum(0), dWk=np.einsum("bjd,bjhk->dhk", x, dKp),
               dbk=dKp.sum((0, 1)), dWv=np.einsum("bjd,bjhk->dhk", x, dVp), dbv=dVp.sum((0, 1)),
               dWo=np.einsum("bhk,bd->hkd", o, gout), dbo=gout.sum(0))
    return out


class _MaskInF32(torch.autograd.Function):
    """float32(l + adder) at a wider dtype; the gradient of the add is the identity, unrounded"""

    @staticmethod
    def forward(ctx, logits, adder):
        return (logits.to(torch.float32) + adder).to(logits.dtype)

    @staticmethod
    def backward(ctx, g):
        return g, None


def mha_torch(query, value, mask, Wq, bq, Wk, bk, Wv, bv, Wo, bo):
    """Keras 2.x MultiHeadAttention._compute_attention in its einsum form: query [B,1,D], value = key [B,K,D], mask
    [B,1,K] (1 = attend) -> [B,1,D], probabilities [B,H,1,K]"""
    dk = Wq.shape[2]
    q = torch.einsum("bqd,dhk->bqhk", query, Wq) + bq
    k = torch.einsum("bjd,dhk->bjhk", value, Wk) + bk
    v = torch.einsum("bjd,dhk->bjhk", value, Wv) + bv
    q = q * (1.0 / float(np.sqrt(float(dk))))
    logits = torch.einsum("bjhk,bqhk->bhqj", k, q)
    adder = (1.0 - mask[:, None].to(torch.float32)) * -1e9
    logits = logits + adder if logits.dtype == torch.float32 else _MaskInF32.apply(logits, adder)
    p = torch.softmax(logits, -1)
    o = torch.einsum("bhqj,bjhk->bqhk", p, v)
    return torch.einsum("bqhk,hkd->bqd", o, Wo) + bo, p


def attention_torch(q, x, mask, w, dtype, gout=None):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype).requires_grad_(True)
    qt, xt = t(q), t(x)
    wt = [t(w[n]) for n in WEIGHTS]
    out, p = mha_torch(qt.unsqueeze(1), xt, torch.from_numpy(np.asarray(mask))[:, None, :], *wt)
    res = {"out": _f64(out[:, 0]), "probs": _f64(p[:, :, 0])}
    if gout is not None:
        grads = torch.autograd.grad((out[:, 0] * torch.tensor(np.asarray(gout), dtype=dtype)).sum(), [qt, xt] + wt)
        res.update({n: _f64(g) for n, g in zip(ATTN_GRADS, grads)})
    return res


# ---- the inputs of a case -----------------------------------------------------------------------------------------------
_INPUTS = {}


def _keys_differ(x, a, b):
    return x[a].tobytes() != x[b].tobytes()


def check_conditions(c):
    """the two conditions of the module docstring, asserted"""
    ref = search_numpy(c)
    raw, valid, x = ref["raw"], c["valid"], c["x"]
    for b in range(raw.shape[0]):
        ts = np.flatnonzero(valid[b])
        if len(ts) < 2:
            continue
        top = np.abs(raw[b, ts]).max()
        order = ts[np.argsort(raw[b, ts], kind="stable")]
        for a, d in zip(order[:-1], order[1:]):                  # neighbours in score order bound every pair
            if _keys_differ(x[b], a, d):
                assert raw[b, d] - raw[b, a] > 1e-3 * top, ("condition 1", c["case"], b, a, d, raw[b, a], raw[b, d])
            else:
                assert raw[b, d] == raw[b, a]
    for m in MASKS:
        l = attention_numpy(c["q"], ref["sel"], c["masks"][m], c["w"])["logits"]
        assert np.abs(l).max() <= 16.0, ("condition 2", c["case"], float(np.abs(l).max()))


def inputs(case, seed=None):
    """table [200,E], series ids [B,T,C] drawn per row from POOL items (duplicates are the rule), the candidate's rows q,
    the attention's weights, masks and every upstream gradient; cached, never changed.  Rows are shaped on purpose:
    pattern b % 5 of tests/dien_ref.py (holes, left-padded, ALL padded, right-padded, none padded); row 4 repeats its
    best item, so the same item occurs twice among the top K; row 9 repeats its K-th item further down, a tie across the
    K-th boundary; row 6 (padded on the left) gets a q that scores every valid step negative."""
    if seed is None and case in _INPUTS:
        return _INPUTS[case]
    B, T, Cn, E, K, H, D = dims(case)
    rng = np.random.default_rng(7000 + 1000 * (CASES[case] if seed is None else seed) +
                                sum(p * v for p, v in zip((1, 3, 5, 7, 11, 13), case)))
    table = rng.standard_normal((V_CASE, E)) * 0.5
    pool = rng.integers(1, V_CASE, (B, POOL, Cn))
    series = pool[np.arange(B)[:, None], rng.integers(0, POOL, (B, T))]
    series = DR.mask_series(rng, np.ascontiguousarray(series))
    q = rng.standard_normal((B, D)) * (2.0 / np.sqrt(D))
    valid = series[:, :, 0] != 0
    if B > 6 and D >= min(POOL, T):                                      # row 6: every valid score negative, 0.5 apart at least
        ts = np.flatnonzero(valid[6])
        if len(ts):
            _, first = np.unique(series[6, ts], axis=0, return_index=True)
            keys = lookup(table, series[6, ts[np.sort(first)]])
            q[6] = np.linalg.pinv(keys) @ -(0.5 + 0.5 * np.arange(len(keys)))
    raw = np.einsum("be,ble->bl", q, lookup(table, series))
    rank = np.argsort(-np.where(valid, raw, -np.inf), axis=-1, kind="stable")
    if B > 4 and T >= 3:
        series[4, rank[4, T - 1]] = series[4, rank[4, 0]]        # the best item twice
    if B > 9 and T >= K + 2:
        series[9, rank[9, T - 1]] = series[9, rank[9, K - 1]]    # the K-th item again, below the boundary
    s = 1.0 / np.sqrt(D)
    w = {"Wq": rng.standard_normal((D, H, D)) * s, "bq": rng.standard_normal((H, D)) * 0.2,
         "Wk": rng.standard_normal((D, H, D)) * s, "bk": rng.standard_normal((H, D)) * 0.2,
         "Wv": rng.standard_normal((D, H, D)) * s, "bv": rng.standard_normal((H, D)) * 0.2,
         "Wo": rng.standard_normal((H, D, D)) * (s / np.sqrt(H)), "bo": rng.standard_normal(D) * 0.2}
    c = {"case": case, "K": K, "table": table, "series": series, "q": q, "valid": series[:, :, 0] != 0, "w": w,
         "x": lookup(table, series), "gpooled": rng.standard_normal((B, D)), "gsel": rng.standard_normal((B, K, D)),
         "gout": rng.standard_normal((B, D))}
    ref = search_numpy(c)
    mixed = rng.integers(0, 2, (B, K))
    c["masks"] = {"zeros": np.zeros((B, K), np.int32), "ones": np.ones((B, K), np.int32),
                  "mixed": mixed.astype(np.int32), "search": (~ref["sel_valid"]).astype(np.int32)}
    c["sel"] = ref["sel"]
    check_conditions(c)
    if seed is None:
        _INPUTS[case] = c
    return c


_CACHE = {}


def cached(fn, case, *key):
    """the fp64 reading or the fp32 transcription of a case with its standard upstream gradients, computed once"""
    k = (fn.__name__, case) + key
    if k not in _CACHE:
        c = inputs(case)
        if fn is search_numpy:
            _CACHE[k] = fn(c, c["gpooled"], c["gsel"] if key[0] else None)
        elif fn is search_torch:
            _CACHE[k] = fn(c, torch.float32, c["gpooled"], c["gsel"] if key[0] else None)
        elif fn is attention_numpy:
            _CACHE[k] = fn(c["q"], c["sel"], c["masks"][key[0]], c["w"], c["gout"])
        else:
            _CACHE[k] = fn(c["q"], c["sel"], c["masks"][key[0]], c["w"], torch.float32, c["gout"])
    return _CACHE[k]


# ---- the loss -----------------------------------------------------------------------------------------------------------
def sim_loss_numpy(gsu, esu, label, alpha=0.2, beta=0.8):
    """7.SIM/ModelManager.py:173-180: softmax cross entropy ON the heads' softmax outputs, weighted, summed"""
    label = np.asarray(label, np.float64)
    if label.ndim == 1:
        label = np.stack([1 - label, label], 1)
    ce = lambda z: -(label * np.log(softmax(np.asarray(z, np.float64)))).sum(-1)
    return float((alpha * ce(gsu) + beta * ce(esu)).sum())


# ---- the layer ----------------------------------------------------------------------------------------------------------
LAYER_V, LAYER_B, LAYER_E, LAYER_H = DR.LAYER_V, DR.LAYER_B, DR.LAYER_E, DR.LAYER_H
LAYER_HEADS = 8
DIEN_KIND = "AUGRU"
DIEN_WIDTH = (len(DR.USER) + len(DR.ITEM)) * LAYER_E + LAYER_H


def _mlp_shapes(prefix, d):
    s = {}
    for i, unit in zip((0, 3), (200, 80)):
        s.update({prefix + "layers.%d.kernel" % i: (d, unit), prefix + "layers.%d.bias" % i: (unit,),
                  prefix + "layers.%d.gamma" % (i + 1): (unit,), prefix + "layers.%d.beta" % (i + 1): (unit,),
                  prefix + "layers.%d.alpha" % (i + 2): (unit,)})
        d = unit
    s.update({prefix + "layers.6.dense.kernel": (d, 2), prefix + "layers.6.dense.bias": (2,)})
    return s


def esu_state_shapes(prefix=""):
    D, H = LAYER_H, LAYER_HEADS
    s = {prefix + "embed.embeddings": (LAYER_V, LAYER_E)}
    s.update({prefix + "dien_layer." + k: v for k, v in DR.state_shapes(DIEN_KIND).items()})
    s.update(_mlp_shapes(prefix + "mlp.", DIEN_WIDTH + D))
    for n in ("_query_dense", "_key_dense", "_value_dense"):
        s.update({prefix + "mha.%s.kernel" % n: (D, H, D), prefix + "mha.%s.bias" % n: (H, D)})
    s.update({prefix + "mha._output_dense.kernel": (H, D, D), prefix + "mha._output_dense.bias": (D,)})
    return s


def sim_state_shapes():
    s = {"embed.embeddings": (LAYER_V, LAYER_E), "gsu_layer.embed.embeddings": (LAYER_V, LAYER_E)}
    s.update(_mlp_shapes("gsu_layer.mlp.", 2 * LAYER_H))
    s.update(esu_state_shapes("esu_layer."))
    return s


def layer_state(seed, shapes):
    """values for a state dict; every 'embed.embeddings' outside the DIEN sub-layer is ONE table"""
    rng = np.random.default_rng(500 + seed)
    sd, shared = {}, None
    for k, shape in shapes.items():
        if k.endswith("embeddings") and "dien_layer" not in k:
            shared = rng.standard_normal(shape) * 0.3 if shared is None else shared
            v = shared
        elif k.endswith("embeddings") or k.endswith(".W"):
            v = rng.standard_normal(shape) * 0.3
        elif k.endswith("gamma"):
            v = 1 + 0.1 * rng.standard_normal(shape)
        elif len(shape) == 3:
            v = rng.standard_normal(shape) / np.sqrt(LAYER_H)
        elif len(shape) == 2 and not k.endswith("bias"):
            v = rng.uniform(-1, 1, shape) * np.sqrt(6.0 / sum(shape))
        else:
            v = rng.standard_normal(shape) * 0.2
        sd[k] = v
    return sd


def layer_inputs(seed, B, T):
    """DIEN's layer inputs (the negatives are never read in stage 'inference') with the series drawn from a small pool
    per row, and a [B,4] upstream for [gsu_logits | esu_logits]"""
    ins = DR.layer_inputs(seed, B, T)
    rng = np.random.default_rng(900 + seed)
    pool = rng.integers(1, LAYER_V, (B, POOL, len(DR.SERIES)))
    series = DR.mask_series(rng, np.ascontiguousarray(pool[np.arange(B)[:, None], rng.integers(0, POOL, (B, T))]))
    for i, k in enumerate(DR.SERIES):
        ins[k] = np.ascontiguousarray(series[:, :, i])
    ins["weight"] = rng.standard_normal((B, 4)).astype(np.float32)
    return ins


def _mlp_torch(p, prefix, h):
    for i in (0, 3):
        h = h @ p[prefix + "layers.%d.kernel" % i] + p[prefix + "layers.%d.bias" % i]
        mean, var = h.mean(-1, keepdim=True), h.var(-1, unbiased=False, keepdim=True)
        h = (h - mean) / torch.sqrt(var + 1e-3) * p[prefix + "layers.%d.gamma" % (i + 1)] \
            + p[prefix + "layers.%d.beta" % (i + 1)]
        h = torch.clamp(h, min=0) + p[prefix + "layers.%d.alpha" % (i + 2)] * torch.clamp(h, max=0)
    return torch.softmax(h @ p[prefix + "layers.6.dense.kernel"] + p[prefix + "layers.6.dense.bias"], -1)


def _ids(ins, names):
    return torch.stack([torch.as_tensor(np.asarray(ins[k])).long() for k in names], -1)


def esu_torch(p, prefix, ins, X_item, extracted, series_mask, mask_mode, dien_mask_valid):
    """ESULayer.call after the item lookup: the frozen DIEN's X_combined (no gradient), the attention, the MLP"""
    d = {k[len(prefix + "dien_layer."):]: v.detach() for k, v in p.items() if k.startswith(prefix + "dien_layer.")}
    table = d["embed.embeddings"]
    B = X_item.shape[0]
    series = _ids(ins, DR.SERIES)
    x = table[series].reshape(B, series.shape[1], -1)
    evolved, _ = DR.body_torch(d, x, None, table[_ids(ins, DR.ITEM)].reshape(B, -1), series[:, :, 0] != 0, DIEN_KIND,
                               dien_mask_valid, "inference")
    dien_output = torch.cat([table[_ids(ins, DR.USER + DR.ITEM)].reshape(B, -1), evolved], 1)
    attend = series_mask if mask_mode == "reference" else ~series_mask
    w = [p[prefix + "mha.%s.%s" % (m, n)] for m in ("_query_dense", "_key_dense", "_value_dense", "_output_dense")
         for n in ("kernel", "bias")]
    interest, _ = mha_torch(X_item.unsqueeze(1), extracted, attend[:, None, :], *w)
    return _mlp_torch(p, prefix + "mlp.", torch.cat([dien_output, interest[:, 0]], 1))


def _grads(p, loss, skip):
    names = [k for k in p if not skip(k)]
    grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    return {k: (np.zeros(tuple(p[k].shape)) if g is None else _f64(g)) for k, g in zip(names, grads)}


def sim_layer_torch(sd, ins, dtype, mask_mode, k=3, dien_mask_valid=1):
    """SIMLayer.call (:263-282) with PReLU on the CPU at ``dtype`` under sum([gsu_logits | esu_logits] (.) weight) ->
    both outputs and the dense gradient of every trainable entry, the shared table once as 'embed.embeddings'"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    table = p["embed.embeddings"]
    B = len(ins[DR.USER[0]])
    X_item = table[_ids(ins, DR.ITEM)].reshape(B, -1)
    series = _ids(ins, DR.SERIES)
    X_series = table[series].reshape(B, series.shape[1], -1)
    valid = series[:, :, 0] != 0
    inner = (X_item.unsqueeze(1) * X_series).sum(-1)             # einsum('be,ble->bl'), see search_torch
    pooled = torch.einsum("bl,ble->be", inner * valid.to(dtype), X_series)
    gsu = _mlp_torch(p, "gsu_layer.mlp.", torch.cat([X_item, pooled], 1))
    ranked = torch.where(valid, inner, torch.full_like(inner, -np.inf))
    chosen = torch.sort(ranked, dim=-1, descending=True, stable=True).indices[:, :k]
    top = torch.gather(X_series, 1, chosen.unsqueeze(-1).expand(-1, -1, X_series.shape[2]))
    esu = esu_torch(p, "esu_layer.", ins, X_item, top, ~torch.gather(valid, 1, chosen), mask_mode, dien_mask_valid)
    loss = (torch.cat([gsu, esu], 1) * torch.tensor(np.asarray(ins["weight"]), dtype=dtype)).sum()
    skip = lambda n: "dien_layer" in n or n in ("gsu_layer.embed.embeddings", "esu_layer.embed.embeddings")
    return {"gsu_logits": _f64(gsu), "esu_logits": _f64(esu), "chosen": chosen.numpy(), "loss": float(loss.detach()),
            "grads": _grads(p, loss, skip)}


def esu_layer_torch(sd, ins, extracted, series_mask, dtype, mask_mode, dien_mask_valid=1):
    """ESULayer.call (:164-201) alone, with given extracted_series [B,K,D] and series_mask [B,K]"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    B = len(ins[DR.USER[0]])
    X_item = p["embed.embeddings"][_ids(ins, DR.ITEM)].reshape(B, -1)
    out = esu_torch(p, "", ins, X_item, torch.tensor(np.asarray(extracted), dtype=dtype),
                    torch.from_numpy(np.asarray(series_mask, bool)), mask_mode, dien_mask_valid)
    loss = (out * torch.tensor(np.asarray(ins["weight"])[:, :2], dtype=dtype)).sum()
    return {"output": _f64(out), "grads": _grads(p, loss, lambda n: "dien_layer" in n)}
