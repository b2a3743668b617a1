"""What the DMR tests share (not a test file): the fp64 numpy reading of DMRI2INetworkLayer, DMRU2INetworkLayer and
compute_auxiliary_loss (8.DMR/CustomLayers.py:203-316) with the hand-derived backward, a torch transcription in the
reference's operation order parametrised by dtype, the inputs of a case from a fixed seed, the layer-level transcription
and the case list.

The reference fails on an example without a valid position (gather_nd at index -1, softmax of all -inf); both readings
here are GIVEN the project's definition for it explicitly: zero attention, score sum 0, inner product 0, loss 0.
tf.keras.losses.CosineSimilarity returns MINUS the cosine: ``cos_sign`` is that sign, -1 in the reference."""
import numpy as np
import torch

V_CASE = 200
EPS = 1e-12
# (B, T, C, E, H, Nn)
CASES = [(1, 1, 1, 1, 1, 1), (3, 5, 1, 8, 4, 1), (33, 10, 3, 16, 48, 6), (33, 7, 3, 5, 15, 33), (5, 100, 3, 32, 96, 6),
         (2, 9, 4, 64, 256, 3), (2049, 10, 3, 16, 48, 6)]
LARGEST = CASES[-1]
OUTPUTS = ("i2i", "u2i", "aux")
GRADS = ("gkeys", "gneg", "gitem", "gq", "dP", "dWe", "dz")
UPSTREAM = ("g_i2i", "g_u2i", "g_aux")


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    diff = np.abs(got - want).max() if want.size else 0.0
    return diff / scale if scale > 0 else diff


def mask_series(rng, series):
    """the mask pattern of a batch with B >= 5: example 0 no padding, 1 one valid position, 2 none, 3 padding in the
    middle (the first feature alone: it decides), the rest tail padding of random length >= 1"""
    B, T, _ = series.shape
    if B < 5:
        return series
    series[1, 1:] = 0
    series[2] = 0
    series[3, T // 2, 0] = 0
    for b in range(4, B):
        series[b, T - int(rng.integers(1, T)):] = 0
    return series


_INPUTS = {}


def inputs(case):
    """table N(0,1) [200,E] (duplicate ids occur), ids, weights and upstream gradients of a case; cached, never changed"""
    if case in _INPUTS:
        return _INPUTS[case]
    B, T, Cn, E, H, Nn = case
    D = Cn * E
    rng = np.random.default_rng(1000 + sum(p * v for p, v in zip((1, 3, 5, 7, 11, 13), case)))
    c = {"table": rng.standard_normal((V_CASE, E)),
         "series": mask_series(rng, rng.integers(1, V_CASE, (B, T, Cn))),
         "negatives": rng.integers(1, V_CASE, (B, Nn, Cn)),
         "items": rng.integers(1, V_CASE, (B, Cn))}
    s = 1.0 / np.sqrt(D)
    c["w"] = {"pos": rng.standard_normal((T, D)), "Wc": rng.standard_normal((D, H)) * s,
              "Wp_i": rng.standard_normal((D, H)) * s, "We_i": rng.standard_normal((D, H)) * s,
              "z_i": rng.standard_normal(H), "Wp_u": rng.standard_normal((D, H)) * s,
              "We_u": rng.standard_normal((D, H)) * s, "z_u": rng.standard_normal(H)}
    c["g_i2i"], c["g_u2i"], c["g_aux"] = (rng.standard_normal((B, D + 1)), rng.standard_normal((B, D + 1)),
                                          rng.standard_normal(B))
    _INPUTS[case] = c
    return c


def lookup(table, ids):
    """rows of ``ids`` [..., C] side by side -> [..., C E]; an id outside the table reads as a zero row"""
    ok = (ids >= 0) & (ids < table.shape[0])
    rows = table[np.where(ok, ids, 0)] * ok[..., None]
    return rows.reshape(ids.shape[:-1] + (-1,))


def operands(c, series=None, negatives=None):
    """what the kernels are given, in fp64: x [B,T,D], xn [B,Nn,D], xi [B,D], valid [B,T], q, P, We [D,2H], z [2,H]"""
    w = c["w"]
    series = c["series"] if series is None else series
    negatives = c["negatives"] if negatives is None else negatives
    xi = lookup(c["table"], c["items"])
    return {"x": lookup(c["table"], series), "xn": lookup(c["table"], negatives), "xi": xi, "valid": series[:, :, 0] != 0,
            "q": xi @ w["Wc"], "P": w["pos"] @ np.concatenate([w["Wp_i"], w["Wp_u"]], 1),
            "We": np.concatenate([w["We_i"], w["We_u"]], 1), "z": np.stack([w["z_i"], w["z_u"]])}


def softplus(x):
    return np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def _softmax_valid(s, valid):
    m = np.where(valid, s, -np.inf).max(1, keepdims=True)
    e = np.where(valid, np.exp(s - np.where(np.isfinite(m), m, 0.0)), 0.0)
    tot = e.sum(1, keepdims=True)
    return e / np.where(tot > 0, tot, 1.0)


def _dcos(p, sp, rp, q, rq, c):
    """d cos(p, q) / dp with TF's gradient of the clamp: rp (nrm(q) - c nrm(p)), or rp nrm(q) where sum p^2 < 1e-12"""
    return rp * np.where(sp >= EPS, q * rq - c * (p * rp), q * rq)


def dmr_numpy(o, g_i2i=None, g_u2i=None, g_aux=None, cos_sign=-1.0, backward=True):
    """fp64 forward over ``operands`` and the hand-derived backward -> dict of OUTPUTS (+ GRADS)"""
    x, xn, xi, valid, q, P, We, z = (o[k] for k in ("x", "xn", "xi", "valid", "q", "P", "We", "z"))
    B, T, D = x.shape
    H = z.shape[1]
    n = valid.sum(1)
    last = n - 1
    tt = np.arange(T)[None, :]
    xw = x @ We
    h0 = np.tanh((q[:, None, :] + xw[:, :, :H]) + P[None, :, :H])
    h1 = np.tanh(xw[:, :, H:] + P[None, :, H:])
    s0, s1 = h0 @ z[0], h1 @ z[1]
    A0, A1 = _softmax_valid(s0, valid), _softmax_valid(s1, valid)
    ssum = np.where(valid, s0, 0.0).sum(1)
    u = np.einsum("bt,btd->bd", A1, x)
    inner = (u * xi).sum(1)
    av = A1[:, :, None] * x
    is_last, before = (tt == last[:, None]), (tt < last[:, None])
    lv = (av * is_last[:, :, None]).sum(1)
    ov = (av * before[:, :, None]).sum(1)
    sl, so, sn = (lv * lv).sum(-1), (ov * ov).sum(-1), (xn * xn).sum(-1)
    rl, ro, rn = (1.0 / np.sqrt(np.maximum(v, EPS)) for v in (sl, so, sn))
    cp = ((lv * rl[:, None]) * (ov * ro[:, None])).sum(-1)
    cn = ((xn * rn[:, :, None]) * (ov * ro[:, None])[:, None, :]).sum(-1)
    pl, nl = (cos_sign * cp + 1) / 2, (cos_sign * cn + 1) / 2
    aux = np.where(n > 0, softplus(-pl) + softplus(nl).sum(-1), 0.0)
    out = {"i2i": np.concatenate([np.einsum("bt,btd->bd", A0, x), ssum[:, None]], 1),
           "u2i": np.concatenate([u, inner[:, None]], 1), "aux": aux}
    if not backward:
        return out
    given = lambda g, shape: np.zeros(shape) if g is None else np.asarray(g, np.float64)
    g_i2i, g_u2i = given(g_i2i, (B, D + 1)), given(g_u2i, (B, D + 1))
    ga = given(g_aux, (B,)) * (n > 0)
    gi, gss, gu, gin = g_i2i[:, :D], g_i2i[:, D], g_u2i[:, :D], g_u2i[:, D]
    dcp = -sigmoid(-pl) * ga * cos_sign / 2
    dcn = sigmoid(nl) * ga[:, None] * cos_sign / 2
    dlv = dcp[:, None] * _dcos(lv, sl[:, None], rl[:, None], ov, ro[:, None], cp[:, None])
    dov = dcp[:, None] * _dcos(ov, so[:, None], ro[:, None], lv, rl[:, None], cp[:, None]) + \
        (dcn[:, :, None] * _dcos(ov[:, None, :], so[:, None, None], ro[:, None, None], xn, rn[:, :, None],
                                 cn[:, :, None])).sum(1)
    gneg = dcn[:, :, None] * _dcos(xn, sn[:, :, None], rn[:, :, None], ov[:, None, :], ro[:, None, None], cn[:, :, None])
    gav = (gu + gin[:, None] * xi)[:, None, :] + is_last[:, :, None] * dlv[:, None, :] + before[:, :, None] * dov[:, None, :]
    dA1, dA0 = (gav * x).sum(-1), x @ gi[:, :, None]
    dA0 = dA0[:, :, 0]
    gx = A1[:, :, None] * gav + A0[:, :, None] * gi[:, None, :]
    ds0 = A0 * (dA0 - (A0 * dA0).sum(1, keepdims=True)) + gss[:, None] * valid
    ds1 = A1 * (dA1 - (A1 * dA1).sum(1, keepdims=True))
    dpre0 = ds0[:, :, None] * z[0] * (1 - h0 * h0)
    dpre1 = ds1[:, :, None] * z[1] * (1 - h1 * h1)
    dpre = np.concatenate([dpre0, dpre1], 2)
    out.update({"gkeys": gx + dpre @ We.T, "gneg": gneg, "gitem": gin[:, None] * u, "gq": dpre0.sum(1),
                "dP": dpre.sum(0), "dWe": np.einsum("btd,bth->dh", x, dpre),
                "dz": np.stack([np.einsum("bt,bth->h", ds0, h0), np.einsum("bt,bth->h", ds1, h1)])})
    return out


def ref(case, **kw):
    c = inputs(case)
    return dmr_numpy(operands(c), c["g_i2i"], c["g_u2i"], c["g_aux"], **kw)


# ---- the torch transcription, in the reference's operation order -----------------------------------------------------
def attention_torch(scores, valid):
    """tf.where(valid, scores, -inf) then tf.nn.softmax; the example without a valid position is given zeros"""
    has = valid.any(1, keepdim=True)
    masked = torch.where(valid, scores, torch.ones_like(scores) * (-np.inf))
    masked = torch.where(has, masked, torch.zeros_like(scores))
    return torch.softmax(masked, dim=-1) * (valid & has).to(scores.dtype)


def l2_normalize(v):
    """tf.math.l2_normalize(axis=-1): v rsqrt(max(sum v^2, 1e-12))"""
    eps = torch.tensor(EPS, dtype=v.dtype)
    return v * torch.rsqrt(torch.maximum((v * v).sum(-1, keepdim=True), eps))


def sigmoid_ce(logits, labels):
    """tf.nn.sigmoid_cross_entropy_with_logits, its stable form: max(x, 0) - x z + log(1 + exp(-|x|))"""
    return torch.clamp(logits, min=0) - logits * labels + torch.log1p(torch.exp(-torch.abs(logits)))


def units_torch(x, xn, xi, valid, q, P, We, z, cos_sign=-1.0):
    """both units and the loss from their operands (torch tensors of one dtype) -> (i2i, u2i, aux)"""
    B, T, D = x.shape
    H = z.shape[1]
    # I2I (:232-248)
    s = z[0][None, None, :].repeat(B, T, 1) * torch.tanh(q[:, None, :].repeat(1, T, 1) + x @ We[:, :H] +
                                                          P[None, :, :H].repeat(B, 1, 1))
    s = s.sum(-1)
    score_sum = torch.where(valid, s, torch.zeros_like(s)).sum(-1, keepdim=True)
    a = attention_torch(s, valid)
    i2i = torch.cat([(a[:, :, None].repeat(1, 1, D) * x).sum(1), score_sum], 1)
    # U2I (:298-311)
    s = z[1][None, None, :].repeat(B, T, 1) * torch.tanh(x @ We[:, H:] + P[None, :, H:].repeat(B, 1, 1))
    a = attention_torch(s.sum(-1), valid)
    av = a[:, :, None].repeat(1, 1, D) * x
    out = av.sum(1)
    u2i = torch.cat([out, (out * xi).sum(-1, keepdim=True)], 1)
    # compute_auxiliary_loss (:273-289)
    n = valid.to(torch.int64).sum(1)
    last = n - 1
    lv = av[torch.arange(B), last.clamp(min=0)]
    new_mask = torch.arange(T)[None, :] < last[:, None]
    ov = (av * new_mask.to(x.dtype)[:, :, None].repeat(1, 1, D)).sum(1)
    pos_logits = (cos_sign * (l2_normalize(lv) * l2_normalize(ov)).sum(-1) + 1) / 2
    neg_logits = (cos_sign * (l2_normalize(xn) * l2_normalize(ov[:, None, :].repeat(1, xn.shape[1], 1))).sum(-1) + 1) / 2
    aux = sigmoid_ce(pos_logits, torch.ones_like(pos_logits)) + sigmoid_ce(neg_logits, torch.zeros_like(neg_logits)).sum(-1)
    return i2i, u2i, torch.where(n > 0, aux, torch.zeros_like(aux))


LEAVES = ("x", "xn", "xi", "q", "P", "We", "z")
GRAD_OF = dict(zip(GRADS, LEAVES))


def dmr_torch(o, dtype, g_i2i=None, g_u2i=None, g_aux=None, cos_sign=-1.0):
    """the transcription at ``dtype`` with torch autograd -> dict of OUTPUTS and GRADS as float64 numpy"""
    t = {k: torch.tensor(np.asarray(o[k]), dtype=dtype, requires_grad=True) for k in LEAVES}
    valid = torch.tensor(o["valid"])
    res = units_torch(t["x"], t["xn"], t["xi"], valid, t["q"], t["P"], t["We"], t["z"], cos_sign)
    out = {k: v.detach().numpy().astype(np.float64) for k, v in zip(OUTPUTS, res)}
    total = sum((r * torch.tensor(np.asarray(g), dtype=dtype)).sum() for r, g in zip(res, (g_i2i, g_u2i, g_aux))
                if g is not None)
    grads = torch.autograd.grad(total, [t[k] for k in LEAVES], allow_unused=True)
    for name, leaf, g in zip(GRADS, LEAVES, grads):
        out[name] = (torch.zeros_like(t[leaf]) if g is None else g).numpy().astype(np.float64)
    return out


_T32 = {}


def case_t32(case):
    if case not in _T32:
        c = inputs(case)
        _T32[case] = dmr_torch(operands(c), torch.float32, c["g_i2i"], c["g_u2i"], c["g_aux"])
    return _T32[case]


_REF = {}


def case_ref(case):
    if case not in _REF:
        _REF[case] = ref(case)
    return _REF[case]


# ---- the layer ----------------------------------------------------------------------------------------------------------
LAYER_V, LAYER_B, LAYER_E, LAYER_NN = 500, 37, 16, 6
LAYER_TS = (10, 50)
USER = ["uid", "utag1", "utag2", "utag3", "utag4"]
ITEM = ["i_goods_id", "i_shop_id", "i_cate_id"]
SERIES = ["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"]
NEGATIVE = ["negative_goods_ids", "negative_shop_ids", "negative_cate_ids"]
LAYER_D = len(ITEM) * LAYER_E


def state_shapes(T):
    D, Din = LAYER_D, (len(USER) + len(ITEM)) * LAYER_E + 2 * (LAYER_D + 1)
    s = {"id_embed.embeddings": (LAYER_V, LAYER_E), "pos_embed.embeddings": (T, D)}
    for k in ("Wc", "Wp", "We"):
        s["i2i_network." + k] = (D, D)
    s.update({"i2i_network.b": (D,), "i2i_network.z": (D,), "u2i_network.Wp": (D, D), "u2i_network.We": (D, D),
              "u2i_network.b": (D,), "u2i_network.z": (D,)})
    d = Din
    for i, unit in zip((0, 3), (200, 80)):
        s.update({"mlp.layers.%d.kernel" % i: (d, unit), "mlp.layers.%d.bias" % i: (unit,),
                  "mlp.layers.%d.gamma" % (i + 1): (unit,), "mlp.layers.%d.beta" % (i + 1): (unit,),
                  "mlp.layers.%d.alpha" % (i + 2): (unit,)})
        d = unit
    s.update({"mlp.layers.6.kernel": (d, 1), "mlp.layers.6.bias": (1,)})
    return s


def layer_state(seed, T):
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in state_shapes(T).items():
        if k.endswith("embeddings"):
            v = rng.standard_normal(shape) * 0.3
        elif k.endswith("gamma"):
            v = 1 + 0.1 * rng.standard_normal(shape)
        elif len(shape) == 2:
            v = rng.uniform(-1, 1, shape) * np.sqrt(6.0 / sum(shape))
        else:
            v = rng.standard_normal(shape) * 0.2
        sd[k] = v
    return sd


def layer_inputs(seed, B, T):
    rng = np.random.default_rng(100 + seed)
    ins = {k: rng.integers(1, LAYER_V, B) for k in USER + ITEM}
    series = mask_series(rng, rng.integers(1, LAYER_V, (B, T, len(SERIES))))
    for i, k in enumerate(SERIES):
        ins[k] = np.ascontiguousarray(series[:, :, i])
    for k in NEGATIVE:
        ins[k] = rng.integers(1, LAYER_V, (B, LAYER_NN))
    ins["label"] = rng.integers(0, 2, (B, 1)).astype(np.float32)
    return ins


def keras_bce(y, p):
    p = torch.clamp(p, 1e-7, 1 - 1e-7)
    return -(y * torch.log(p + 1e-7) + (1 - y) * torch.log(1 - p + 1e-7)).mean()


def layer_torch(sd, ins, dtype):
    """DMRLayer.call (:154-200) on the CPU at ``dtype`` under BCE(output) + auxiliary_loss.mean() -> output,
    auxiliary_loss and the dense gradient of every state entry but the unused ``b``"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    ids = lambda names: torch.stack([torch.as_tensor(np.asarray(ins[k])).long() for k in names], -1)
    table = p["id_embed.embeddings"]
    B = len(ins[USER[0]])
    profile = table[ids(USER + ITEM)].reshape(B, -1)
    xi = table[ids(ITEM)].reshape(B, -1)
    series, negatives = ids(SERIES), ids(NEGATIVE)
    x = table[series].reshape(B, series.shape[1], -1)
    xn = table[negatives].reshape(B, negatives.shape[1], -1)
    pos = p["pos_embed.embeddings"]
    valid = series[:, :, 0] != 0
    i2n, u2n = "i2i_network.", "u2i_network."
    q = xi @ p[i2n + "Wc"]
    P = torch.cat([pos @ p[i2n + "Wp"], pos @ p[u2n + "Wp"]], 1)
    We = torch.cat([p[i2n + "We"], p[u2n + "We"]], 1)
    z = torch.stack([p[i2n + "z"], p[u2n + "z"]])
    i2i, u2i, aux = units_torch(x, xn, xi, valid, q, P, We, z)
    h = torch.cat([profile, i2i, u2i], 1)
    for i in (0, 3):
        h = h @ p["mlp.layers.%d.kernel" % i] + p["mlp.layers.%d.bias" % i]
        mean, var = h.mean(-1, keepdim=True), h.var(-1, unbiased=False, keepdim=True)
        h = (h - mean) / torch.sqrt(var + 1e-3) * p["mlp.layers.%d.gamma" % (i + 1)] + p["mlp.layers.%d.beta" % (i + 1)]
        h = torch.clamp(h, min=0) + p["mlp.layers.%d.alpha" % (i + 2)] * torch.clamp(h, max=0)
    output = torch.sigmoid(h @ p["mlp.layers.6.kernel"] + p["mlp.layers.6.bias"])
    loss = keras_bce(torch.tensor(np.asarray(ins["label"]), dtype=dtype), output) + aux.mean()
    names = [k for k in p if not k.endswith(".b")]
    grads = torch.autograd.grad(loss, [p[k] for k in names])
    f64 = lambda t: t.detach().numpy().astype(np.float64)
    return {"output": f64(output), "auxiliary_loss": f64(aux), "loss": float(loss.detach()),
            "grads": {k: f64(g) for k, g in zip(names, grads)}}
