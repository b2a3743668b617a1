"""What the DIEN tests share (not a test file): the fp64 numpy reading of DIENLayer's interest extractor, auxiliary loss,
DienActivationLayer and DienGRU / CustomGRUCell (5.DIN/CustomLayers.py:292-517) with the hand-derived backward through
time, a torch transcription in the reference's operation order parametrised by dtype (autograd), the inputs of a case
from a fixed seed, the layer-level transcription and the case list.

TensorFlow is not available: the issue's text is the specification.  The numpy reading runs ONE cell for the three
recurrences (the kernels' formulation); the torch transcription writes the Keras GRU (reset_after=True, gate order z, r,
h, bias [2, 3H]) and CustomGRUCell separately, as the reference does.  Both are GIVEN one definition explicitly: a row
whose scores select nothing (the division 0 / 0 the reference turns into 0 with tf.where) scores zeros AND sends zero
gradient through the scores, where TensorFlow's gradient of the division would be NaN."""
import numpy as np
import torch

V_CASE = 200
# (B, T, C, E)
CASES = [(1, 1, 1, 1), (3, 5, 1, 8), (33, 6, 3, 16), (33, 7, 3, 5), (5, 100, 3, 32), (2, 9, 2, 64), (2049, 6, 3, 16)]
LARGEST = CASES[-1]
MASKED = (33, 6, 3, 16)
KINDS = ("AUGRU", "AGRU", "AIGRU")
PATTERNS = ("holes", "left", "all", "right", "none")
GRU_OUT, GRU_GRADS = ("gru_output", "aux"), ("dx", "dneg", "dkernel", "drecurrent_kernel", "dbias")
EVO_OUT, EVO_GRADS = ("scores", "h_final"), ("dgru_output", "dq", "dWx", "dUh", "dbx")


def rel_err(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    scale = np.abs(want).max() if want.size else 0.0
    diff = np.abs(got - want).max() if want.size else 0.0
    return diff / scale if scale > 0 else diff


def pattern_of(b):
    return PATTERNS[b % len(PATTERNS)]


def mask_series(rng, series):
    """Row b gets pattern b % 5 in its FIRST feature (the one that decides): holes anywhere (at least one valid and, with
    T > 1, one padded position), left-padded, all padded, right-padded, none padded.  The other features keep their ids:
    a padded position still reads rows."""
    B, T, _ = series.shape
    for b in range(B):
        kind = pattern_of(b)
        valid = np.ones(T, bool)
        if kind == "holes" and T > 1:
            valid = rng.random(T) < 0.5
            valid[int(rng.integers(0, T))] = True
            if valid.all():
                valid[int(rng.integers(0, T))] = False
        elif kind == "left" and T > 1:
            valid[:int(rng.integers(1, T))] = False
        elif kind == "all":
            valid[:] = False
        elif kind == "right" and T > 1:
            valid[T - int(rng.integers(1, T)):] = False
        series[b, ~valid, 0] = 0
    return series


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def ce(x, label):
    """tf.nn.sigmoid_cross_entropy_with_logits"""
    return np.maximum(x, 0) - x * label + np.log1p(np.exp(-np.abs(x)))


def lookup(table, ids):
    ok = (ids >= 0) & (ids < table.shape[0])
    rows = table[np.where(ok, ids, 0)] * ok[..., None]
    return rows.reshape(ids.shape[:-1] + (-1,))


_INPUTS = {}


def inputs(case):
    """table [200,E] (duplicate ids occur), ids, weights and upstream gradients of a case; cached, never changed.  The
    generator checks |product| < 10 for every position, so exp stays finite in fp32."""
    if case in _INPUTS:
        return _INPUTS[case]
    B, T, Cn, E = case
    H = Cn * E
    rng = np.random.default_rng(2000 + sum(p * v for p, v in zip((1, 3, 5, 7), case)))
    s = 1.0 / np.sqrt(H)
    c = {"table": rng.standard_normal((V_CASE, E)) * 0.5,
         "series": mask_series(rng, rng.integers(1, V_CASE, (B, T, Cn))),
         "negatives": rng.integers(1, V_CASE, (B, T, Cn)),
         "kernel": rng.standard_normal((H, 3 * H)) * s, "recurrent_kernel": rng.standard_normal((H, 3 * H)) * s,
         "bias": rng.standard_normal((2, 3 * H)) * 0.2,
         "Wx": rng.standard_normal((H, 3 * H)) * s, "Uh": rng.standard_normal((H, 3 * H)) * s,
         "bx": rng.standard_normal(3 * H) * 0.2, "q": rng.standard_normal((B, H)) * (2.0 * s),
         "dgru_output": rng.standard_normal((B, T, H)), "dh_final": rng.standard_normal((B, H)),
         "gaux": rng.standard_normal(1)}
    c["valid"] = c["series"][:, :, 0] != 0
    c["x"], c["xn"] = lookup(c["table"], c["series"]), lookup(c["table"], c["negatives"])
    g = cell_forward(c["x"], c["valid"], c["kernel"], c["recurrent_kernel"], c["bias"][0], c["bias"][1], "GRU")[0]
    assert np.abs(np.einsum("bth,bh->bt", g, c["q"])).max() < 10.0
    c["g"] = g                                                   # the evolution's input: the extractor's fp64 output
    _INPUTS[case] = c
    return c


def evo_weights(c, kind):
    """the packed cell weights of a kind: [z | r | h] blocks, AGRU without z"""
    H = c["q"].shape[1]
    lo = H if kind == "AGRU" else 0
    return c["Wx"][:, lo:], c["Uh"][:, lo:], c["bx"][lo:]


# ---- the fp64 reading: one cell, forward and backward through time ------------------------------------------------------
def cell_forward(x, valid, Wx, Uh, bx, bh, kind, a=None):
    """-> hs [B,T,H] and the per-step cache.  kind: GRU h' = z h + (1-z) hh; AUGRU h' = (1 - a z) h + a z hh; AGRU
    h' = (1-a) h + a hh; h' = h where valid is false."""
    B, T, H = x.shape
    ng = Wx.shape[1] // H
    h = np.zeros((B, H))
    hs, cache = np.zeros((B, T, H)), []
    for t in range(T):
        pre, rec = x[:, t] @ Wx + bx, h @ Uh + bh
        z = sigmoid(pre[:, :H] + rec[:, :H]) if ng == 3 else None
        r = sigmoid(pre[:, (ng - 2) * H:(ng - 1) * H] + rec[:, (ng - 2) * H:(ng - 1) * H])
        rc = rec[:, (ng - 1) * H:]
        hh = np.tanh(pre[:, (ng - 1) * H:] + r * rc)
        if kind == "GRU":
            hn = z * h + (1 - z) * hh
        else:
            w = a[:, t, None] * z if kind == "AUGRU" else a[:, t, None] * np.ones_like(hh)
            hn = (1 - w) * h + w * hh
        cache.append((h, z, r, rc, hh))
        h = np.where(valid[:, t, None], hn, h)
        hs[:, t] = h
    return hs, cache


def cell_backward(x, valid, Wx, Uh, kind, cache, dhs, dh_final, a=None):
    """-> dx [B,T,H], dWx, dUh, dbx, dbh, da [B,T] from the upstream of every h_t and of the final state"""
    B, T, H = x.shape
    ng = Wx.shape[1] // H
    dh = np.zeros((B, H)) if dh_final is None else dh_final.copy()
    dx, da = np.zeros((B, T, H)), np.zeros((B, T))
    dWx, dUh, dbx, dbh = np.zeros_like(Wx), np.zeros_like(Uh), np.zeros(ng * H), np.zeros(ng * H)
    for t in range(T - 1, -1, -1):
        if dhs is not None:
            dh = dh + dhs[:, t]
        h, z, r, rc, hh = cache[t]
        v = valid[:, t, None]
        if kind == "GRU":
            dhh, dz, dhold = dh * (1 - z), dh * (h - hh), dh * z
        else:
            av = a[:, t, None]
            w = av * z if kind == "AUGRU" else av * np.ones_like(hh)
            dw = dh * (hh - h)
            dhh, dhold = dh * w, dh * (1 - w)
            dz = dw * av if kind == "AUGRU" else None
            da[:, t] = np.where(v, dw * z if kind == "AUGRU" else dw, 0.0).sum(1)
        dc = np.where(v, dhh * (1 - hh * hh), 0.0)
        dr = dc * rc * r * (1 - r)
        blocks = ([np.where(v, dz * z * (1 - z), 0.0)] if ng == 3 else []) + [dr]
        dpre = np.concatenate(blocks + [dc], 1)
        drec = np.concatenate(blocks + [dc * r], 1)
        dWx += x[:, t].T @ dpre
        dUh += h.T @ drec
        dbx += dpre.sum(0)
        dbh += drec.sum(0)
        dx[:, t] = dpre @ Wx.T
        dh = np.where(v, dhold, dh) + drec @ Uh.T
    return dx, dWx, dUh, dbx, dbh, da


def extractor_numpy(c, dgru_output=None, gaux=None, negatives=True):
    """the masked Keras GRU over the looked-up series and the auxiliary loss, with the hand-derived backward"""
    x, xn, valid = c["x"], c["xn"], c["valid"]
    B, T, H = x.shape
    hs, cache = cell_forward(x, valid, c["kernel"], c["recurrent_kernel"], c["bias"][0], c["bias"][1], "GRU")
    out = {"gru_output": hs, "aux": np.zeros(1)}
    dhs = np.zeros((B, T, H)) if dgru_output is None else dgru_output.copy()
    dx_aux, dneg = np.zeros((B, T, H)), np.zeros((B, T, H))
    if negatives and T > 1:
        sp, sn = (x[:, :-1] * hs[:, 1:]).sum(-1), (x[:, :-1] * xn[:, 1:]).sum(-1)
        p, n = sigmoid(sp), sigmoid(sn)
        m = valid[:, 1:].astype(np.float64)
        out["aux"] = np.array([(ce(p, 1.0) * m).sum() + (ce(n, 0.0) * m).sum()])
        ga = 0.0 if gaux is None else float(np.asarray(gaux).reshape(-1)[0])
        gsp = ga * m * (sigmoid(p) - 1) * p * (1 - p)
        gsn = ga * m * sigmoid(n) * n * (1 - n)
        dhs[:, 1:] += gsp[..., None] * x[:, :-1]
        dx_aux[:, :-1] = gsp[..., None] * hs[:, 1:] + gsn[..., None] * xn[:, 1:]
        dneg[:, 1:] = gsn[..., None] * x[:, :-1]
    dx, dK, dU, dbx, dbh, _ = cell_backward(x, valid, c["kernel"], c["recurrent_kernel"], "GRU", cache, dhs, None)
    out.update({"dx": dx + dx_aux, "dneg": dneg, "dkernel": dK, "drecurrent_kernel": dU, "dbias": np.stack([dbx, dbh])})
    return out


def scores_numpy(g, q, valid, mask_valid):
    product = np.einsum("bth,bh->bt", g, q)
    sel = valid if mask_valid else ~valid
    e = np.where(sel, np.exp(product), 0.0)
    tot = e.sum(1, keepdims=True)
    return e / np.where(tot > 0, tot, 1.0)


def evolution_numpy(c, kind, mask_valid, dh_final=None):
    """scores, then AGRU / AUGRU over (g, scores) or -- AIGRU -- a Keras GRU over g (.) scores; the final state"""
    g, q, valid = c["g"], c["q"], c["valid"]
    a = scores_numpy(g, q, valid, mask_valid)
    if kind == "AIGRU":
        x = g * a[..., None]
        Wx, Uh, bx, bh = c["kernel"], c["recurrent_kernel"], c["bias"][0], c["bias"][1]
        hs, cache = cell_forward(x, valid, Wx, Uh, bx, bh, "GRU")
        dxin, dWx, dUh, dbx, dbh, _ = cell_backward(x, valid, Wx, Uh, "GRU", cache, None, dh_final)
        dg, da = dxin * a[..., None], (dxin * g).sum(-1)
        dbx = np.stack([dbx, dbh])
    else:
        Wx, Uh, bx = evo_weights(c, kind)
        hs, cache = cell_forward(g, valid, Wx, Uh, bx, 0.0, kind, a)
        dg, dWx, dUh, dbx, _, da = cell_backward(g, valid, Wx, Uh, kind, cache, None, dh_final, a)
    dp = a * (da - (a * da).sum(1, keepdims=True))
    return {"scores": a, "states": hs, "h_final": hs[:, -1], "dgru_output": dg + dp[..., None] * q[:, None, :],
            "dq": (dp[..., None] * g).sum(1), "dWx": dWx, "dUh": dUh, "dbx": dbx}


# ---- the torch transcription, in the reference's operation order --------------------------------------------------------
def keras_gru_torch(x, valid, kernel, recurrent_kernel, bias):
    """tf.keras.layers.GRU(H, return_sequences=True), reset_after=True, with a mask: the carried state is the output"""
    B, T, _ = x.shape
    H = recurrent_kernel.shape[0]
    h = x.new_zeros((B, H))
    outs = []
    for t in range(T):
        xi = x[:, t] @ kernel + bias[0]
        hi = h @ recurrent_kernel + bias[1]
        z = torch.sigmoid(xi[:, :H] + hi[:, :H])
        r = torch.sigmoid(xi[:, H:2 * H] + hi[:, H:2 * H])
        hh = torch.tanh(xi[:, 2 * H:] + r * hi[:, 2 * H:])
        hn = z * h + (1 - z) * hh
        h = torch.where(valid[:, t, None], hn, h)
        outs.append(h)
    return torch.stack(outs, 1)


def custom_cell_rnn_torch(x, a, valid, kind, w):
    """tf.keras.layers.RNN(CustomGRUCell, return_state=True)(concat(x, a), mask=valid): the final state"""
    B, T, H = x.shape
    h = x.new_zeros((B, H))
    for t in range(T):
        xt, at = x[:, t], a[:, t, None]
        r = torch.sigmoid(xt @ w["W_r"] + h @ w["U_r"] + w["b_r"])
        h_tilda = torch.tanh(xt @ w["W_h"] + r * (h @ w["U_h"]) + w["b_h"])
        if kind == "AGRU":
            hn = (1 - at) * h + at * h_tilda
        else:
            u = torch.sigmoid(xt @ w["W_z"] + h @ w["U_z"] + w["b_z"])
            u_hat = at * u
            hn = (1 - u_hat) * h + u_hat * h_tilda
        h = torch.where(valid[:, t, None], hn, h)
    return h


def scores_torch(product, valid, mask_valid):
    """exp, times ~mask (the mask passed in is `valid`: mask_valid = 0 is the reference), over the row sum, NaN -> 0"""
    sel = valid if mask_valid else ~valid
    masked = torch.exp(product) * sel.to(product.dtype)
    tot = masked.sum(-1, keepdim=True)
    return masked / torch.where(tot > 0, tot, torch.ones_like(tot))


def aux_torch(x, gru_output, xn, valid):
    """get_auxiliary_loss (:434-453), the double sigmoid kept"""
    xs, g, n = x[:, :-1], gru_output[:, 1:], xn[:, 1:]
    pos_logits = torch.sigmoid((xs * g).sum(-1))
    neg_logits = torch.sigmoid((xs * n).sum(-1))
    sce = lambda v, l: torch.clamp(v, min=0) - v * l + torch.log1p(torch.exp(-v.abs()))
    m = valid[:, 1:].to(x.dtype)
    return (sce(pos_logits, 1.0) * m).sum() + (sce(neg_logits, 0.0) * m).sum()


def _t(a, dtype, grad=True):
    return torch.tensor(np.asarray(a), dtype=dtype, requires_grad=grad)


def _f64(t):
    return t.detach().numpy().astype(np.float64)


def extractor_torch(c, dtype, dgru_output=None, gaux=None, negatives=True):
    x, xn = _t(c["x"], dtype), _t(c["xn"], dtype)
    valid = torch.tensor(c["valid"])
    K, U, b = _t(c["kernel"], dtype), _t(c["recurrent_kernel"], dtype), _t(c["bias"], dtype)
    g = keras_gru_torch(x, valid, K, U, b)
    aux = aux_torch(x, g, xn, valid) if negatives else g.sum() * 0
    loss = aux * 0
    if dgru_output is not None:
        loss = loss + (g * torch.tensor(dgru_output, dtype=dtype)).sum()
    if gaux is not None:
        loss = loss + aux * float(np.asarray(gaux).reshape(-1)[0])
    grads = torch.autograd.grad(loss, [x, xn, K, U, b], allow_unused=True)
    grads = [torch.zeros_like(p) if gr is None else gr for gr, p in zip(grads, (x, xn, K, U, b))]
    out = {"gru_output": _f64(g), "aux": _f64(aux).reshape(1)}
    out.update({k: _f64(v) for k, v in zip(GRU_GRADS, grads)})
    return out


def evolution_torch(c, dtype, kind, mask_valid, dh_final=None):
    g, q = _t(c["g"], dtype), _t(c["q"], dtype)
    valid = torch.tensor(c["valid"])
    H = q.shape[1]
    a = scores_torch((g * q[:, None, :]).sum(-1), valid, mask_valid)
    if kind == "AIGRU":
        ws = [_t(c["kernel"], dtype), _t(c["recurrent_kernel"], dtype), _t(c["bias"], dtype)]
        hf = keras_gru_torch(g * a[..., None], valid, *ws)[:, -1]
    else:
        Wx, Uh, bx = (_t(v, dtype) for v in evo_weights(c, kind))
        ws = [Wx, Uh, bx]
        names = ("z", "r", "h") if kind == "AUGRU" else ("r", "h")
        w = {}
        for i, n in enumerate(names):
            w["W_" + n], w["U_" + n], w["b_" + n] = Wx[:, i * H:(i + 1) * H], Uh[:, i * H:(i + 1) * H], bx[i * H:(i + 1) * H]
        hf = custom_cell_rnn_torch(g, a, valid, kind, w)
    out = {"scores": _f64(a), "h_final": _f64(hf)}
    if dh_final is not None:
        loss = (hf * torch.tensor(dh_final, dtype=dtype)).sum()
        grads = torch.autograd.grad(loss, [g, q] + ws, allow_unused=True)
        grads = [torch.zeros_like(p) if gr is None else gr for gr, p in zip(grads, [g, q] + ws)]
        out.update({k: _f64(v) for k, v in zip(EVO_GRADS, grads)})
    return out


DENSE_OUT, DENSE_GRADS = ("h_final",), ("dx", "dkernel", "drecurrent_kernel", "dbias")


def dense_numpy(c, dh_final):
    """the dense-input mode (DienGRU's AIGRU): the Keras GRU over x = g under the mask, the final state alone"""
    K, U, b = c["kernel"], c["recurrent_kernel"], c["bias"]
    hs, cache = cell_forward(c["g"], c["valid"], K, U, b[0], b[1], "GRU")
    dx, dK, dU, dbx, dbh, _ = cell_backward(c["g"], c["valid"], K, U, "GRU", cache, None, dh_final)
    return {"h_final": hs[:, -1], "states": hs, "dx": dx, "dkernel": dK, "drecurrent_kernel": dU,
            "dbias": np.stack([dbx, dbh])}


def dense_torch(c, dtype, dh_final):
    x, K, U, b = (_t(c[k], dtype) for k in ("g", "kernel", "recurrent_kernel", "bias"))
    hs = keras_gru_torch(x, torch.tensor(c["valid"]), K, U, b)
    hf = hs[:, -1]
    grads = torch.autograd.grad((hf * torch.tensor(dh_final, dtype=dtype)).sum(), [x, K, U, b])
    out = {"h_final": _f64(hf), "states": _f64(hs)}
    out.update({k: _f64(v) for k, v in zip(DENSE_GRADS, grads)})
    return out


_CACHE = {}


def cached(fn, *key):
    k = (fn.__name__,) + key
    if k not in _CACHE:
        c = inputs(key[0])
        if fn in (extractor_numpy, ):
            _CACHE[k] = fn(c, c["dgru_output"], c["gaux"])
        elif fn is extractor_torch:
            _CACHE[k] = fn(c, torch.float32, c["dgru_output"], c["gaux"])
        elif fn is evolution_numpy:
            _CACHE[k] = fn(c, key[1], key[2], c["dh_final"])
        else:
            _CACHE[k] = fn(c, torch.float32, key[1], key[2], c["dh_final"])
    return _CACHE[k]


# ---- the layer ----------------------------------------------------------------------------------------------------------
LAYER_V, LAYER_B, LAYER_E = 300, 37, 16
LAYER_TS = (6, 20)
USER = ["uid", "utag1", "utag2", "utag3", "utag4"]
ITEM = ["i_goods_id", "i_shop_id", "i_cate_id"]
SERIES = ["visited_goods_ids", "visited_shop_ids", "visited_cate_ids"]
NEGATIVE = ["negative_goods_ids", "negative_shop_ids", "negative_cate_ids"]
LAYER_H = len(ITEM) * LAYER_E
CELL = {"AUGRU": ("W_r", "U_r", "b_r", "W_h", "U_h", "b_h", "W_z", "U_z", "b_z"),
        "AGRU": ("W_r", "U_r", "b_r", "W_h", "U_h", "b_h")}


def state_shapes(kind, activation="PReLU"):
    H, Din = LAYER_H, (len(USER) + len(ITEM)) * LAYER_E + LAYER_H
    s = {"embed.embeddings": (LAYER_V, LAYER_E), "gru.kernel": (H, 3 * H), "gru.recurrent_kernel": (H, 3 * H),
         "gru.bias": (2, 3 * H), "dien_activation_layer.W": (H, H)}
    if kind == "AIGRU":
        s.update({"dien_gru.gru.kernel": (H, 3 * H), "dien_gru.gru.recurrent_kernel": (H, 3 * H),
                  "dien_gru.gru.bias": (2, 3 * H)})
    else:
        for n in CELL[kind]:
            s["dien_gru.gru_cell." + n] = (H,) if n.startswith("b") else (H, H)
    d = Din
    for i, unit in zip((0, 3), (200, 80)):
        s.update({"mlp.layers.%d.kernel" % i: (d, unit), "mlp.layers.%d.bias" % i: (unit,),
                  "mlp.layers.%d.gamma" % (i + 1): (unit,), "mlp.layers.%d.beta" % (i + 1): (unit,)})
        if activation == "PReLU":
            s["mlp.layers.%d.alpha" % (i + 2)] = (unit,)
        d = unit
    s.update({"mlp.layers.6.dense.kernel": (d, 2), "mlp.layers.6.dense.bias": (2,)})
    return s


def layer_state(seed, kind):
    rng = np.random.default_rng(seed)
    sd = {}
    for k, shape in state_shapes(kind).items():
        if k.endswith("embeddings"):
            v = rng.standard_normal(shape) * 0.3
        elif k.endswith("gamma"):
            v = 1 + 0.1 * rng.standard_normal(shape)
        elif k.endswith(".W"):
            v = rng.standard_normal(shape) * 0.3
        elif len(shape) == 2 and not k.endswith("bias"):
            v = rng.uniform(-1, 1, shape) * np.sqrt(6.0 / sum(shape))
        else:
            v = rng.standard_normal(shape) * 0.2
        sd[k] = v
    return sd


def layer_inputs(seed, B, T):
    rng = np.random.default_rng(100 + seed)
    ins = {k: rng.integers(1, LAYER_V, B) for k in USER + ITEM}
    series = mask_series(rng, rng.integers(1, LAYER_V, (B, T, len(SERIES))))
    negatives = rng.integers(1, LAYER_V, (B, T, len(NEGATIVE)))
    for i, k in enumerate(SERIES):
        ins[k] = np.ascontiguousarray(series[:, :, i])
    for i, k in enumerate(NEGATIVE):
        ins[k] = np.ascontiguousarray(negatives[:, :, i])
    ins["weight"] = rng.standard_normal((B, 2)).astype(np.float32)     # the upstream of the softmax output
    return ins


def body_torch(p, x, xn, X_item, valid, kind, mask_valid, stage):
    """DIENLayer.call between the lookups and the MLP -> (evolved interest [B,H], auxiliary loss)"""
    g = keras_gru_torch(x, valid, p["gru.kernel"], p["gru.recurrent_kernel"], p["gru.bias"])
    aux = aux_torch(x, g, xn, valid) if stage == "train" else 0
    weighted = g @ p["dien_activation_layer.W"]
    product = (weighted * X_item[:, None, :]).sum(-1)
    a = scores_torch(product, valid, mask_valid)
    if kind == "AIGRU":
        evolved = keras_gru_torch(g * a[..., None], valid, p["dien_gru.gru.kernel"], p["dien_gru.gru.recurrent_kernel"],
                                  p["dien_gru.gru.bias"])[:, -1]
    else:
        evolved = custom_cell_rnn_torch(g, a, valid, kind, {n: p["dien_gru.gru_cell." + n] for n in CELL[kind]})
    return evolved, aux


def layer_torch(sd, ins, dtype, kind, mask_valid, stage="train"):
    """DIENLayer.call (:455-517) with PReLU on the CPU at ``dtype`` under sum(output (.) weight) + auxiliary_loss ->
    X_combined, output, auxiliary_loss and the dense gradient of every state entry (zeros where autograd has none)"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    ids = lambda names: torch.stack([torch.as_tensor(np.asarray(ins[k])).long() for k in names], -1)
    table = p["embed.embeddings"]
    B = len(ins[USER[0]])
    profile = table[ids(USER + ITEM)].reshape(B, -1)
    X_item = table[ids(ITEM)].reshape(B, -1)
    series = ids(SERIES)
    x = table[series].reshape(B, series.shape[1], -1)
    xn = table[ids(NEGATIVE)].reshape(B, series.shape[1], -1) if stage == "train" else None
    valid = series[:, :, 0] != 0
    evolved, aux = body_torch(p, x, xn, X_item, valid, kind, mask_valid, stage)
    X_combined = torch.cat([profile, evolved], 1)
    h = X_combined
    for i in (0, 3):
        h = h @ p["mlp.layers.%d.kernel" % i] + p["mlp.layers.%d.bias" % i]
        mean, var = h.mean(-1, keepdim=True), h.var(-1, unbiased=False, keepdim=True)
        h = (h - mean) / torch.sqrt(var + 1e-3) * p["mlp.layers.%d.gamma" % (i + 1)] + p["mlp.layers.%d.beta" % (i + 1)]
        h = torch.clamp(h, min=0) + p["mlp.layers.%d.alpha" % (i + 2)] * torch.clamp(h, max=0)
    output = torch.softmax(h @ p["mlp.layers.6.dense.kernel"] + p["mlp.layers.6.dense.bias"], -1)
    loss = (output * torch.tensor(np.asarray(ins["weight"]), dtype=dtype)).sum() + aux
    names = list(p)
    grads = torch.autograd.grad(loss, [p[k] for k in names], allow_unused=True)
    return {"X_combined": _f64(X_combined), "output": _f64(output),
            "auxiliary_loss": float(aux.detach()) if stage == "train" else 0, "loss": float(loss.detach()),
            "grads": {k: (np.zeros(tuple(p[k].shape)) if g is None else _f64(g)) for k, g in zip(names, grads)}}
