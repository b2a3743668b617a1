"""References of the DMT family (8.DMR/CustomLayers.py:445-769), written from the definition in DESIGN 3.20 and
the reference's text read as mathematics: no program text of the reference is here.

  encoder_numpy      fp64 numpy: one Transformer encoder layer, forward and ANALYTIC backward (no autograd)
  encoder_torch      the same composed of torch ops in a given dtype, gradients by autograd (the fp32 transcription whose
                     own error against fp64 sets the tolerance of the GPU tests, and the fp64 check of the analytic backward)
  transformer_numpy, bias_network_numpy
                     fp64 numpy, forward: the decoder layer, DeepInterestTransformer and the bias network written a second
                     time, apart from the torch transcription, which tests/test_dmt_host.py holds against them
  decoder_layer_torch, transformer_torch, bias_network_torch, dmt_layer_torch
                     the decoder layer, DeepInterestTransformer, BiasDeepNeuralNetworkLayer and DMTLayer composed of torch
                     ops in a given dtype over a state dict named as dmt.py names its parameters; run in fp64 they are the
                     reference, in fp32 the transcription
  CASES, MASKS, inputs, layer_inputs, layer_state   the kernel cases (B,T,D,H,dk,dff), their four masks and the layers' inputs

Every logit of every case is asserted to stay below 32 in magnitude: the premise under which float32(l - 1e9) is -1e9
exactly, so a padded query attends uniformly.
"""
import math

import numpy as np
import torch

F64 = np.float64
WEIGHTS = ("Wq", "bq", "Wk", "bk", "Wv", "bv", "Wo", "bo", "gamma1", "beta1", "W1", "b1", "W2", "b2", "gamma2", "beta2")
GRADS = ("gx",) + tuple("d" + n for n in WEIGHTS)
LN_EPS = 1e-6

SMALLEST, TINY, DEFAULTS, ODD, LIMITS, RAGGED = ((1, 1, 2, 1, 2, 2), (3, 2, 4, 1, 2, 4), (5, 6, 48, 4, 48, 32),
                                                (7, 7, 6, 3, 4, 6), (33, 16, 64, 8, 64, 64), (70, 5, 10, 2, 6, 8))
CASES = (SMALLEST, TINY, DEFAULTS, ODD, LIMITS, RAGGED)
MASKS = ("valid", "padded", "prefix", "holes")


def rel_err(got, want):
    """max|got - want| / max|want| (the absolute error where want is zero throughout)"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    scale = np.abs(want).max() if want.size else 0.0
    return float(np.abs(got - want).max() / scale) if scale > 0 else float(np.abs(got).max() if got.size else 0.0)


def weight_shapes(D, H, dk, dff):
    return {"Wq": (D, H, dk), "bq": (H, dk), "Wk": (D, H, dk), "bk": (H, dk), "Wv": (D, H, dk), "bv": (H, dk),
            "Wo": (H, dk, D), "bo": (D,), "gamma1": (D,), "beta1": (D,), "W1": (D, dff), "b1": (dff,), "W2": (dff, D),
            "b2": (D,), "gamma2": (D,), "beta2": (D,)}


def masks_of(rng, B, T):
    """the four masks [B,T] bool: all valid; all padded; a random valid prefix per example with the lengths 1 and T
    present; holes in the middle with an example of a single valid token"""
    n = rng.integers(1, T + 1, B)
    n[0] = 1
    n[-1] = T
    prefix = np.arange(T)[None, :] < n[:, None]
    holes = rng.random((B, T)) < 0.6
    holes[:, 0] = True
    if T > 2:
        holes[:, 1] = False                      # a hole right behind the first token
        holes[:, -1] = True
    holes[0] = False
    holes[0, T // 2] = True                      # a single valid token, in the middle
    return {"valid": np.ones((B, T), bool), "padded": np.zeros((B, T), bool), "prefix": prefix, "holes": holes}


_INPUTS = {}


def inputs(case):
    """x, gz, the 16 weights (fp32 values) and the four masks of a case; computed once"""
    if case not in _INPUTS:
        B, T, D, H, dk, dff = case
        rng = np.random.default_rng(sum(case) * 7 + 1)
        f = lambda *s: rng.standard_normal(s).astype(np.float32)
        w = {}
        for name, shape in weight_shapes(D, H, dk, dff).items():
            if name.startswith("gamma"):
                w[name] = (1.0 + 0.2 * f(*shape)).astype(np.float32)
            elif name[0] == "b":                 # biases and betas: non-zero, so each is exercised
                w[name] = 0.2 * f(*shape)
            else:
                w[name] = f(*shape) * np.float32(0.7 / math.sqrt(shape[0] if name != "Wo" else shape[0] * shape[1]))
        _INPUTS[case] = {"x": f(B, T, D), "gz": f(B, T, D), "w": w, "masks": masks_of(rng, B, T)}
    return _INPUTS[case]


def _ln(v):
    mu = v.mean(-1, keepdims=True)
    var = ((v - mu) ** 2).mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(var + LN_EPS)
    return (v - mu) * rstd, rstd


def _ln_bwd(g, xhat, rstd, gamma):
    gg = g * gamma
    return rstd * (gg - gg.mean(-1, keepdims=True) - xhat * (gg * xhat).mean(-1, keepdims=True))


def encoder_numpy(x, mask, w, gz=None):
    """fp64: -> {z, probs [B,T,H,T], logits} and, with gz, the 17 gradients of GRADS by the chain rule written out"""
    x = np.asarray(x, F64)
    w = {k: np.asarray(v, F64) for k, v in w.items()}
    m = np.asarray(mask).astype(bool).astype(F64)
    dk = w["Wq"].shape[2]
    s = 1.0 / math.sqrt(dk)
    Q = (np.einsum("btd,dhk->bthk", x, w["Wq"]) + w["bq"]) * s
    K = np.einsum("btd,dhk->bthk", x, w["Wk"]) + w["bk"]
    V = np.einsum("btd,dhk->bthk", x, w["Wv"]) + w["bv"]
    l = np.einsum("bthk,buhk->bthu", Q, K)
    assert np.abs(l).max() < 32, "the premise of the exact -1e9 rounding: |logit| < 32"
    pair = m[:, :, None, None] * m[:, None, None, :]
    # float32(l + (1 - pair) * -1e9): -1e9 exactly where masked (|l| < 32 is below half an ulp of 1e9 in fp32), l otherwise
    a = np.where(pair > 0, l, -1e9)
    e = np.exp(a - a.max(-1, keepdims=True))
    p = e / e.sum(-1, keepdims=True)
    ctx = np.einsum("bthu,buhk->bthk", p, V)
    attn = np.einsum("bthk,hkd->btd", ctx, w["Wo"]) + w["bo"]
    xh1, r1 = _ln(x + attn)
    y = xh1 * w["gamma1"] + w["beta1"]
    pre = y @ w["W1"] + w["b1"]
    hid = np.maximum(pre, 0.0)
    xh2, r2 = _ln(y + hid @ w["W2"] + w["b2"])
    z = xh2 * w["gamma2"] + w["beta2"]
    out = {"z": z, "probs": p, "logits": l}
    if gz is None:
        return out
    gz = np.asarray(gz, F64)
    red = lambda t: t.reshape(-1, t.shape[-1]).sum(0)
    out["dgamma2"], out["dbeta2"] = red(gz * xh2), red(gz)
    gr2 = _ln_bwd(gz, xh2, r2, w["gamma2"])
    out["db2"] = red(gr2)
    out["dW2"] = np.einsum("btf,btd->fd", hid, gr2)
    gh = (gr2 @ w["W2"].T) * (pre > 0)
    out["db1"] = red(gh)
    out["dW1"] = np.einsum("btd,btf->df", y, gh)
    gy = gr2 + gh @ w["W1"].T
    out["dgamma1"], out["dbeta1"] = red(gy * xh1), red(gy)
    gr1 = _ln_bwd(gy, xh1, r1, w["gamma1"])
    out["dbo"] = red(gr1)
    out["dWo"] = np.einsum("bthk,btd->hkd", ctx, gr1)
    gctx = np.einsum("btd,hkd->bthk", gr1, w["Wo"])
    gp = np.einsum("bthk,buhk->bthu", gctx, V)
    gV = np.einsum("bthu,bthk->buhk", p, gctx)
    dl = p * (gp - (gp * p).sum(-1, keepdims=True))            # the softmax Jacobian, padded queries included
    gQ = np.einsum("bthu,buhk->bthk", dl, K) * s                # of the raw projection
    gK = np.einsum("bthu,bthk->buhk", dl, Q)
    out["dWq"], out["dbq"] = np.einsum("btd,bthk->dhk", x, gQ), gQ.sum((0, 1))
    out["dWk"], out["dbk"] = np.einsum("btd,bthk->dhk", x, gK), gK.sum((0, 1))
    out["dWv"], out["dbv"] = np.einsum("btd,bthk->dhk", x, gV), gV.sum((0, 1))
    out["gx"] = gr1 + np.einsum("bthk,dhk->btd", gQ, w["Wq"]) + np.einsum("bthk,dhk->btd", gK, w["Wk"]) \
        + np.einsum("bthk,dhk->btd", gV, w["Wv"])
    return out


# ---- the torch transcription ---------------------------------------------------------------------------------------------
def t_ln(v, gamma, beta, eps=LN_EPS):
    mu = v.mean(-1, keepdim=True)
    var = ((v - mu) ** 2).mean(-1, keepdim=True)
    return (v - mu) * torch.rsqrt(var + eps) * gamma + beta


def t_mha(q, kv, pair, w, want_probs=False):
    """Keras MultiHeadAttention: q [B,Tq,D] over kv [B,Tk,D], pair [B,Tq,Tk] (1 = attend), additive -1e9 in the dtype"""
    Wq, bq, Wk, bk, Wv, bv, Wo, bo = w
    dk = Wq.shape[2]
    Q = (torch.einsum("btd,dhk->bthk", q, Wq) + bq) * (1.0 / math.sqrt(float(dk)))
    K = torch.einsum("bud,dhk->buhk", kv, Wk) + bk
    V = torch.einsum("bud,dhk->buhk", kv, Wv) + bv
    l = torch.einsum("bthk,buhk->bhtu", Q, K)
    # the mask is added in float32, whatever the dtype of the rest: |l| < 32 makes the sum -1e9 exactly, and the
    # gradient of the sum still reaches l (fp64: the value -1e9, the derivative of l)
    a = torch.where(pair[:, None] > 0, l, l + (-1e9 - l).detach()) if l.dtype == torch.float64 \
        else l + (1.0 - pair[:, None].to(l.dtype)) * -1e9
    p = torch.softmax(a, -1)
    o = torch.einsum("bhtu,buhk->bthk", p, V)
    out = torch.einsum("bthk,hkd->btd", o, Wo) + bo
    return (out, p.permute(0, 2, 1, 3)) if want_probs else out


def t_encoder_layer(x, m, w, want_probs=False):
    """x [B,T,D], m [B,T] (1 = valid) and the 16 weights in the order of WEIGHTS"""
    pair = m[:, :, None] * m[:, None, :]
    attn, p = t_mha(x, x, pair, w[:8], True)
    y = t_ln(x + attn, w[8], w[9])
    f = torch.relu(y @ w[10] + w[11]) @ w[12] + w[13]
    z = t_ln(y + f, w[14], w[15])
    return (z, p) if want_probs else z


def encoder_torch(x, mask, w, gz, dtype):
    """-> {z, probs} + GRADS as numpy, computed in ``dtype`` with autograd"""
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    wt = [torch.tensor(np.asarray(w[n]), dtype=dtype, requires_grad=True) for n in WEIGHTS]
    m = torch.tensor(np.asarray(mask).astype(bool)).to(dtype)
    z, p = t_encoder_layer(xt, m, wt, True)
    out = {"z": z.detach().numpy(), "probs": p.detach().numpy()}
    if gz is not None:
        z.backward(torch.tensor(np.asarray(gz), dtype=dtype))
        for name, t in zip(GRADS, [xt] + wt):
            out[name] = t.grad.numpy()
    return out


_CACHE = {}


def cached(fn, case, mask, *extra):
    """fn's result on a case under one of its masks, computed once and shared"""
    key = (fn.__name__, case, mask) + extra
    if key not in _CACHE:
        c = inputs(case)
        _CACHE[key] = fn(c["x"], c["masks"][mask], c["w"], c["gz"], *extra)
    return _CACHE[key]


# ---- the layers ----------------------------------------------------------------------------------------------------------
LAYER_V, LAYER_B, LAYER_E = 60, 9, 4
USER_F, ITEM_F, CONT_F = ["uid", "utag1"], ["i_goods_id", "i_shop_id", "i_cate_id"], ["continuous_feature1"]
SERIES_F = {"click": ["click_goods_ids", "click_shop_ids", "click_cate_ids"],
            "cart": ["cart_goods_ids", "cart_shop_ids", "cart_cate_ids"],
            "order": ["order_goods_ids", "order_shop_ids", "order_cate_ids"]}
BIAS_F = {"position_feature": "position", "page_feature": "page",
          "neighbourhood_features": ["near_expo_seq_cate2", "near_expo_seq_cate3"]}
MAX_POSITION, MAX_PAGE, NEIGHBOURS = 12, 5, 7


def layer_inputs(seed, B, T):
    """a batch of DMTLayer: ids in [1, V) with padding 0 in the series -- a random valid prefix per example, example 1 has
    every series padded throughout, example 2 has the candidate id 0 -- plus ``weight`` [B,2] for the tests' scalar"""
    rng = np.random.default_rng(seed)
    ins = {}
    for name in USER_F + ITEM_F:
        ins[name] = rng.integers(1, LAYER_V, B)
    ins[ITEM_F[0]][2] = 0
    for name in CONT_F:
        ins[name] = rng.standard_normal(B).astype(np.float32)
    for names in SERIES_F.values():
        n = rng.integers(1, T + 1, B)
        n[0], n[1] = T, 0
        valid = np.arange(T)[None, :] < n[:, None]
        for name in names:
            ins[name] = rng.integers(1, LAYER_V, (B, T)) * valid
    ins["position"] = rng.integers(0, MAX_POSITION, B)
    ins["page"] = rng.integers(0, MAX_PAGE, B)
    for name in BIAS_F["neighbourhood_features"]:
        ins[name] = rng.integers(0, LAYER_V, (B, NEIGHBOURS))
    ins["weight"] = rng.standard_normal((B, 2)).astype(np.float32)
    return ins


def layer_state(seed, shapes):
    """a state dict of the given {name: shape}: every tensor random, so that no term hides behind a zero bias or a unit
    gamma; the scale keeps every attention logit well below 32"""
    rng = np.random.default_rng(seed + 1000)
    sd = {}
    for name, shape in shapes.items():
        v = rng.standard_normal(shape)
        if name.endswith("gamma"):
            v = 1.0 + 0.2 * v
        elif name.endswith("embeddings"):
            v = 0.5 * v
        elif len(shape) >= 2:
            v = v * (0.8 / math.sqrt(np.prod(shape[:-1]) if "_output_dense" in name else shape[0]))
        else:
            v = 0.2 * v
        sd[name] = v.astype(np.float32)
    return sd


def _mha_w(sd, prefix):
    return [sd[prefix + "." + n] for n in ("_query_dense.kernel", "_query_dense.bias", "_key_dense.kernel",
                                           "_key_dense.bias", "_value_dense.kernel", "_value_dense.bias",
                                           "_output_dense.kernel", "_output_dense.bias")]


def _enc_w(sd, prefix):
    return _mha_w(sd, prefix + ".mha") + [sd[prefix + ".layernorm1.gamma"], sd[prefix + ".layernorm1.beta"],
                                          sd[prefix + ".ffn.layers.0.kernel"], sd[prefix + ".ffn.layers.0.bias"],
                                          sd[prefix + ".ffn.layers.1.kernel"], sd[prefix + ".ffn.layers.1.bias"],
                                          sd[prefix + ".layernorm2.gamma"], sd[prefix + ".layernorm2.beta"]]


def encoder_stack_torch(sd, prefix, x, m, num_layers):
    for i in range(num_layers):
        x = t_encoder_layer(x, m, _enc_w(sd, "%s.enc_layers.%d" % (prefix, i)))
    return x


def decoder_layer_torch(sd, prefix, x, enc, look_ahead, padding):
    """x [B,1,D] the candidate token, enc [B,T,D]; look_ahead [B,1,1] and padding [B,1,T] (1 = attend)"""
    ln = lambda v, n: t_ln(v, sd["%s.layernorm%d.gamma" % (prefix, n)], sd["%s.layernorm%d.beta" % (prefix, n)])
    out1 = ln(t_mha(x, x, look_ahead, _mha_w(sd, prefix + ".mha1")) + x, 1)
    out2 = ln(t_mha(out1, enc, padding, _mha_w(sd, prefix + ".mha2")) + out1, 2)
    f = torch.relu(out2 @ sd[prefix + ".ffn.layers.0.kernel"] + sd[prefix + ".ffn.layers.0.bias"]) \
        @ sd[prefix + ".ffn.layers.1.kernel"] + sd[prefix + ".ffn.layers.1.bias"]
    return ln(f + out2, 3)


def transformer_torch(sd, prefix, enc_ids, dec_ids, x_enc, x_dec, num_layers):
    """DeepInterestTransformer: enc_ids [B,T] and dec_ids [B,1] make the masks (id != 0), x_enc [B,T,D], x_dec [B,1,D]
    -> [B,1,D]"""
    dt = x_enc.dtype
    me, md = (enc_ids != 0).to(dt), (dec_ids != 0).to(dt)
    enc = encoder_stack_torch(sd, prefix + ".encoder", x_enc, me, num_layers)
    look_ahead = md[:, :, None]                               # band_part of a 1 x 1 matrix of ones, times the padding
    padding = me[:, None, :] * md[:, :, None]
    x = x_dec
    for i in range(num_layers):
        x = decoder_layer_torch(sd, "%s.decoder.dec_layers.%d" % (prefix, i), x, enc, look_ahead, padding)
    return x


def t_mlp(sd, prefix, x, n_layers, activation, last_linear=False, softmax=False):
    """make_mlp_layer: Dense, LayerNormalization(1e-3), activation per unit; ``last_linear``: the head='linear' extension
    ends with a plain Dense after the hidden units; ``softmax``: a closing Dense + softmax"""
    i = 0
    for u in range(n_layers):
        x = x @ sd["%s.layers.%d.kernel" % (prefix, i)] + sd["%s.layers.%d.bias" % (prefix, i)]
        i += 1
        if last_linear and u == n_layers - 1:
            return x
        x = t_ln(x, sd["%s.layers.%d.gamma" % (prefix, i)], sd["%s.layers.%d.beta" % (prefix, i)], 1e-3)
        i += 1
        if activation == "PReLU":
            x = torch.relu(x) + sd["%s.layers.%d.alpha" % (prefix, i)] * torch.minimum(x, torch.zeros_like(x))
        else:
            x = torch.relu(x)
        i += 1
    if softmax:
        x = torch.softmax(x @ sd["%s.layers.%d.dense.kernel" % (prefix, i)] + sd["%s.layers.%d.dense.bias" % (prefix, i)], -1)
    return x


def bias_network_torch(sd, prefix, ins, head):
    """BiasDeepNeuralNetworkLayer: per neighbourhood feature the attention of the centre neighbour (index 3) over the 7,
    scaled by sqrt(E); the weights, the outputs, the position and the page rows feed the [8,1] ReLU MLP"""
    E = sd[prefix + ".position_embedding.embeddings"].shape[1]
    pos = sd[prefix + ".position_embedding.embeddings"][ins["position"]]
    page = sd[prefix + ".page_embedding.embeddings"][ins["page"]]
    nb = torch.stack([ins[n] for n in BIAS_F["neighbourhood_features"]], 1)                 # [B,F,N]
    xn = sd[prefix + ".neighbourhood_embedding.embeddings"][nb]                                # [B,F,N,E]
    q = xn[:, :, 3:4, :]
    wts = torch.softmax(torch.einsum("bhqe,bhke->bhqk", q, xn) / (E ** 0.5), -1)
    out = torch.einsum("bhqk,bhke->bhqe", wts, xn)
    B = pos.shape[0]
    feat = torch.cat([wts.reshape(B, -1), out.reshape(B, -1), pos, page], 1)
    return t_mlp(sd, prefix + ".mlp", feat, 2, "ReLU", last_linear=head == "linear")


def dmt_layer_torch(sd, ins, dtype, head, num_layers, expert_num=2, weight=None):
    """DMTLayer over the state dict ``sd`` (numpy) in ``dtype`` -> {'ctr_logits', 'cvr_logits'} as numpy and, with
    ``weight`` [B,2], 'grads': the gradient of sum(cat(ctr, cvr) * weight) for every parameter (zeros where none arrives)"""
    p = {k: torch.tensor(np.asarray(v), dtype=dtype, requires_grad=True) for k, v in sd.items()}
    t = {k: torch.as_tensor(np.asarray(v)) for k, v in ins.items()}
    table = p["id_embed.embeddings"]
    B = t[ITEM_F[0]].shape[0]
    flat = lambda names: torch.cat([table[t[n]] for n in names], 1)
    X_cate, X_item = flat(USER_F + ITEM_F), flat(ITEM_F)
    X_cont = torch.stack([t[n].to(dtype) for n in CONT_F], 1)
    interests = []
    for kind in ("click", "cart", "order"):
        names = SERIES_F[kind]
        x_enc = torch.cat([table[t[n]] for n in names], 2)                                     # [B,T,C E]
        interests.append(transformer_torch(p, kind + "_transformer", t[names[0]], t[ITEM_F[0]][:, None], x_enc,
                                           X_item[:, None], num_layers)[:, 0])
    X = torch.cat(interests + [X_cate, X_cont, X_item], 1)
    experts = torch.stack([t_mlp(p, "expert_model.%d" % i, X, 2, "PReLU") for i in range(expert_num)], 1)
    res = {}
    for task in ("ctr", "cvr"):
        gate = t_mlp(p, task + "_gate", X, 1, "PReLU", softmax=True)
        logits = t_mlp(p, task + "_output", (experts * gate[:, :, None]).reshape(B, -1), 2, "PReLU",
                       last_linear=head == "linear")
        res[task + "_logits"] = torch.sigmoid(logits + bias_network_torch(p, "bias_network_" + task, t, head))
    out = {k: v.detach().numpy() for k, v in res.items()}
    if weight is not None:
        (torch.cat([res["ctr_logits"], res["cvr_logits"]], 1) * torch.tensor(weight, dtype=dtype)).sum().backward()
        out["grads"] = {k: (np.zeros(v.shape) if v.grad is None else v.grad.numpy()) for k, v in p.items()}
    return out


# ---- fp64 numpy, forward: a second writing of the decoder, the transformer and the bias network ----------------------------
def _np_ln(v, gamma, beta, eps=LN_EPS):
    xh = (v - v.mean(-1, keepdims=True)) / np.sqrt(v.var(-1, keepdims=True) + eps)
    return xh * gamma + beta


def _np_mha(q, kv, pair, w):
    """q [B,Tq,D] over kv [B,Tk,D], pair [B,Tq,Tk] bool; the masked logits are -1e9 exactly, as float32 rounds them"""
    Wq, bq, Wk, bk, Wv, bv, Wo, bo = w
    out = np.zeros(q.shape[:2] + (Wo.shape[2],))
    for h in range(Wq.shape[1]):
        Q = (q @ Wq[:, h] + bq[h]) / math.sqrt(Wq.shape[2])
        l = Q @ np.swapaxes(kv @ Wk[:, h] + bk[h], 1, 2)
        assert np.abs(l).max() < 32
        a = np.where(pair, l, -1e9)
        p = np.exp(a - a.max(-1, keepdims=True))
        out += (p / p.sum(-1, keepdims=True)) @ (kv @ Wv[:, h] + bv[h]) @ Wo[h]
    return out + bo


def _np_ffn(sd, prefix, v):
    return np.maximum(v @ sd[prefix + ".ffn.layers.0.kernel"] + sd[prefix + ".ffn.layers.0.bias"], 0) \
        @ sd[prefix + ".ffn.layers.1.kernel"] + sd[prefix + ".ffn.layers.1.bias"]


def transformer_numpy(sd, prefix, enc_ids, dec_ids, x_enc, x_dec, num_layers):
    sd = {k: np.asarray(v, F64) for k, v in sd.items()}
    ln = lambda pre, n, v: _np_ln(v, sd["%s.layernorm%d.gamma" % (pre, n)], sd["%s.layernorm%d.beta" % (pre, n)])
    me, md = np.asarray(enc_ids) != 0, np.asarray(dec_ids) != 0
    x = np.asarray(x_enc, F64)
    for i in range(num_layers):
        pre = "%s.encoder.enc_layers.%d" % (prefix, i)
        y = ln(pre, 1, x + _np_mha(x, x, me[:, :, None] & me[:, None, :], _mha_w(sd, pre + ".mha")))
        x = ln(pre, 2, y + _np_ffn(sd, pre, y))
    t = np.asarray(x_dec, F64)
    for i in range(num_layers):
        pre = "%s.decoder.dec_layers.%d" % (prefix, i)
        o1 = ln(pre, 1, _np_mha(t, t, md[:, :, None], _mha_w(sd, pre + ".mha1")) + t)
        o2 = ln(pre, 2, _np_mha(o1, x, me[:, None, :] & md[:, :, None], _mha_w(sd, pre + ".mha2")) + o1)
        t = ln(pre, 3, _np_ffn(sd, pre, o2) + o2)
    return t


def bias_network_numpy(sd, prefix, ins, head):
    sd = {k: np.asarray(v, F64) for k, v in sd.items()}
    nb = np.stack([np.asarray(ins[n]) for n in BIAS_F["neighbourhood_features"]], 1)
    xn = sd[prefix + ".neighbourhood_embedding.embeddings"][nb]                                # [B,F,N,E]
    sc = np.einsum("bfe,bfke->bfk", xn[:, :, 3], xn) / math.sqrt(xn.shape[-1])
    w = np.exp(sc - sc.max(-1, keepdims=True))
    w = w / w.sum(-1, keepdims=True)
    out = np.einsum("bfk,bfke->bfe", w, xn)
    B = nb.shape[0]
    v = np.concatenate([w.reshape(B, -1), out.reshape(B, -1),
                        sd[prefix + ".position_embedding.embeddings"][np.asarray(ins["position"])],
                        sd[prefix + ".page_embedding.embeddings"][np.asarray(ins["page"])]], 1)
    m = prefix + ".mlp.layers."
    v = np.maximum(_np_ln(v @ sd[m + "0.kernel"] + sd[m + "0.bias"], sd[m + "1.gamma"], sd[m + "1.beta"], 1e-3), 0)
    v = v @ sd[m + "3.kernel"] + sd[m + "3.bias"]
    return v if head == "linear" else np.maximum(_np_ln(v, sd[m + "4.gamma"], sd[m + "4.beta"], 1e-3), 0)
