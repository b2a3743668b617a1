"""Restatements of FiBiNet++ (11.FiBiNet++/CustomLayers.py:78-242) for the tests: an fp64 numpy reading with hand-written
gradients (input stage, body, the whole layer with its head) and a torch transcription in the reference's op order (one
einsum per pair, split / stack / reduce for the groups, one LayerNormalization per key field) that autograd
differentiates, runnable in fp32 and fp64 on the CPU.  Parameters on the scale of tests/masknet_ref.py: tables
N(0, 0.5^2), continuous values and body inputs N(0, 1), glorot-uniform Dense kernels, glorot-normal bilinear matrices,
biases N(0, 0.1^2), norm gammas 1 + N(0, 0.1^2) and norm betas N(0, 0.1^2) pushed away from 0 (|beta| >= 0.01): a norm
over ONE unit returns beta, which must lie clear of the relu kink.

bn = [gamma, beta, moving_mean, moving_var] ([E] each) and ln = [gamma, beta] ([Fk, E]) describe the input stage.  A
body's parameters are the list [W, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1]: W [nW, E, E] (nW = 1 'all', F - 1
'each', P 'interaction'), Wr [P, O], S0 [2 G F, mid], S1 [mid, F E].  A head is [K0, c0, gh, bh, K1, c1]: Dense,
LayerNormalization, ReLU, Dense(1, sigmoid).  ``pre`` is, per example, the smallest |relu pre-activation| over h and A
(and the head in the layer) combined with the smallest gap between the largest and the second largest element of any
group wider than one.  An id outside [0, V) reads as a zero row, as the kernels define it."""
import itertools

import numpy as np
import torch

from tests.masknet_ref import EPS, PRE_EPS, _ln, _ln_bwd, _t, clean_seed, gather, glorot, rel_err  # noqa: F401

MOMENTUM = 0.99      # tf.keras.layers.BatchNormalization()
TYPES = ("all", "each", "interaction")


def pairs(F):
    return list(itertools.combinations(range(F), 2))


def weight_of(btype, i, t):
    return {"all": 0, "each": i, "interaction": t}[btype]


def num_weights(F, btype):
    return {"all": 1, "each": F - 1, "interaction": F * (F - 1) // 2}[btype]


def mid_units(F, G, ratio):
    return max(1, 2 * G * F // ratio)


def _beta(r, shape):
    b = r.normal(0, 0.1, shape)
    return np.where(b < 0, -1.0, 1.0) * np.maximum(np.abs(b), 0.01)


def _gamma(r, shape):
    return 1 + r.normal(0, 0.1, shape)


def make_input(r, B, Fc, Fk, E, V):
    """-> table [V,E], X [B,Fc+Fk] int64, values [B,Fk], bn, ln"""
    return (r.normal(0, 0.5, (V, E)), r.integers(0, V, (B, Fc + Fk)).astype(np.int64), r.normal(0, 1, (B, Fk)),
            [_gamma(r, E), _beta(r, E), r.normal(0, 0.2, E), 0.5 + r.uniform(0, 1, E)],
            [_gamma(r, (Fk, E)), _beta(r, (Fk, E))])


def make_block(r, F, E, G, ratio, O, btype):
    D, P, mid = F * E, F * (F - 1) // 2, mid_units(F, G, ratio)
    W = np.clip(r.normal(0, 1, (num_weights(F, btype), E, E)), -2, 2) * np.sqrt(2.0 / (E + E)) / 0.87962566
    return [W, glorot(r, P, O), r.normal(0, 0.1, O), _gamma(r, O), _beta(r, O),
            glorot(r, 2 * G * F, mid), r.normal(0, 0.1, mid), _gamma(r, mid), _beta(r, mid),
            glorot(r, mid, D), r.normal(0, 0.1, D), _gamma(r, D), _beta(r, D)]


def make_head(r, n_in, units=32):
    return [glorot(r, n_in, units), r.normal(0, 0.1, units), _gamma(r, units), _beta(r, units), glorot(r, units, 1),
            r.normal(0, 0.1, 1)]


# ---- numpy, fp64 ----------------------------------------------------------------------------------------------------
def input_stage_numpy(table, X, values, bn, ln, training=True, dx=None):
    """-> x [B, F E], moving_mean, moving_var after the call; with dx also vals [B*F, E], dtable, dbn = [dgamma, dbeta],
    dln = [dgamma, dbeta]."""
    table = np.asarray(table, np.float64)
    g_bn, b_bn, mm, mv = [np.asarray(a, np.float64) for a in bn]
    B, F = X.shape
    E = table.shape[1]
    Fk = 0 if values is None else values.shape[1]
    Fc = F - Fk
    rows = gather(table, X)
    cat = rows[:, :Fc]
    if training and Fc and B:
        mean, var = cat.mean((0, 1)), cat.var((0, 1))
        mm, mv = mm * MOMENTUM + mean * (1 - MOMENTUM), mv * MOMENTUM + var * (1 - MOMENTUM)
    else:
        mean, var = mm, mv
    rstd_bn = 1.0 / np.sqrt(var + EPS)
    xh_c = (cat - mean) * rstd_bn
    parts = [xh_c * g_bn + b_bn]
    if Fk:
        g_ln, b_ln = [np.asarray(a, np.float64) for a in ln]
        vals_in = np.asarray(values, np.float64)
        y_k, xh_k, rstd_k = _ln(rows[:, Fc:] * vals_in[:, :, None], g_ln, b_ln)
        parts.append(y_k)
    out = {"x": np.concatenate(parts, 1).reshape(B, F * E), "moving_mean": mm, "moving_var": mv}
    if dx is not None:
        dy = np.asarray(dx, np.float64).reshape(B, F, E)
        dc = dy[:, :Fc]
        dxh = dc * g_bn
        if training and Fc and B:
            dcat = rstd_bn * (dxh - dxh.mean((0, 1)) - xh_c * (dxh * xh_c).mean((0, 1)))
        else:
            dcat = rstd_bn * dxh
        vals = [dcat]
        out["dbn"] = [(dc * xh_c).sum((0, 1)), dc.sum((0, 1))]
        if Fk:
            dk = dy[:, Fc:]
            vals.append(_ln_bwd(dk, xh_k, rstd_k, g_ln) * vals_in[:, :, None])
            out["dln"] = [(dk * xh_k).sum(0), dk.sum(0)]
        else:
            out["dln"] = [np.zeros((0, E)), np.zeros((0, E))]
        vals = np.concatenate(vals, 1)
        dtable = np.zeros_like(table)
        ok = (X >= 0) & (X < table.shape[0])
        np.add.at(dtable, X[ok], vals[ok])
        out.update(vals=vals.reshape(B * F, E), dtable=dtable)
    return out


def squeeze_numpy(x, F, E, G):
    """x [B, F E] -> s [B, 2 G F] (per field: the G group means, then the G group maxima), arg-max [B,F,G], gap [B]"""
    B = x.shape[0]
    xg = x.reshape(B, F, G, E // G)
    s = np.concatenate([xg.mean(-1), xg.max(-1)], -1).reshape(B, 2 * G * F)
    gap = np.full(B, np.inf)
    if E // G > 1 and B:
        top = np.sort(xg, -1)
        gap = (top[..., -1] - top[..., -2]).reshape(B, -1).min(1)
    return s, xg.argmax(-1), gap


def block_numpy(x, params, G, btype, dout=None):
    """x [B, F E] -> out [B, O + F E], pre, s; with dout also dx and dparams (order of params)."""
    W, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1 = [np.asarray(p, np.float64) for p in params]
    x = np.asarray(x, np.float64)
    B, D = x.shape
    E = W.shape[1]
    F = D // E
    xf = x.reshape(B, F, E)
    pr = pairs(F)
    p = np.stack([np.einsum("be,ek,bk->b", xf[:, i], W[weight_of(btype, i, t)], xf[:, j])
                  for t, (i, j) in enumerate(pr)], 1)
    q, xhq, rsq = _ln(p @ Wr + br, gq, bq)
    s, arg, gap = squeeze_numpy(x, F, E, G)
    z0, xh0, rs0 = _ln(s @ S0 + b0, g0, be0)
    h = np.maximum(z0, 0)
    z1, xh1, rs1 = _ln(h @ S1 + b1, g1, be1)
    A = np.maximum(z1, 0)
    pre = np.minimum(np.minimum(np.abs(z0).min(1), np.abs(z1).min(1)), gap) if B else np.zeros(0)
    out = {"out": np.concatenate([q, x * A], 1), "pre": pre, "s": s}
    if dout is not None:
        dout = np.asarray(dout, np.float64)
        O = Wr.shape[1]
        dq, dv = dout[:, :O], dout[:, O:]
        dx = dv * A
        dy1 = dv * x * (z1 > 0)
        dz1 = _ln_bwd(dy1, xh1, rs1, g1)
        dy0 = (dz1 @ S1.T) * (z0 > 0)
        dz0 = _ln_bwd(dy0, xh0, rs0, g0)
        ds = (dz0 @ S0.T).reshape(B, F, 2 * G)
        w = E // G
        dxg = np.repeat(ds[:, :, :G, None] / w, w, -1)
        onehot = np.arange(w)[None, None, None, :] == arg[..., None]
        dxg = dxg + ds[:, :, G:, None] * onehot
        dx = dx + dxg.reshape(B, D)
        dzq = _ln_bwd(dq, xhq, rsq, gq)
        dp = dzq @ Wr.T
        dW = np.zeros_like(W)
        dxf = np.zeros((B, F, E))
        for t, (i, j) in enumerate(pr):
            wi = weight_of(btype, i, t)
            dW[wi] += np.einsum("b,be,bk->ek", dp[:, t], xf[:, i], xf[:, j])
            dxf[:, i] += dp[:, t, None] * (xf[:, j] @ W[wi].T)
            dxf[:, j] += dp[:, t, None] * (xf[:, i] @ W[wi])
        out.update(dx=dx + dxf.reshape(B, D),
                   dparams=[dW, p.T @ dzq, dzq.sum(0), (dq * xhq).sum(0), dq.sum(0),
                            s.T @ dz0, dz0.sum(0), (dy0 * xh0).sum(0), dy0.sum(0),
                            h.T @ dz1, dz1.sum(0), (dy1 * xh1).sum(0), dy1.sum(0)])
    return out


def fibinetplus_numpy(table, X, values, bn, ln, block, head, G, btype, training=True, dout=None):
    """The whole layer -> output [B,1], pre; with dout = dLoss/doutput also dtable, dbn, dln, dblock, dhead."""
    st = input_stage_numpy(table, X, values, bn, ln, training)
    o = block_numpy(st["x"], block, G, btype)
    top = o["out"]
    K0, c0, gh, bh, K1, c1 = [np.asarray(p, np.float64) for p in head]
    z, xh, rs = _ln(top @ K0 + c0, gh, bh)
    a = np.maximum(z, 0)
    prob = 1.0 / (1.0 + np.exp(-(a @ K1 + c1)))
    out = {"output": prob, "pre": np.minimum(o["pre"], np.abs(z).min(1)), "moving_mean": st["moving_mean"],
           "moving_var": st["moving_var"]}
    if dout is not None:
        dl = np.asarray(dout, np.float64) * prob * (1 - prob)
        dy = (dl @ K1.T) * (z > 0)
        dz = _ln_bwd(dy, xh, rs, gh)
        out["dhead"] = [top.T @ dz, dz.sum(0), (dy * xh).sum(0), dy.sum(0), a.T @ dl, dl.sum(0)]
        ob = block_numpy(st["x"], block, G, btype, dz @ K0.T)
        si = input_stage_numpy(table, X, values, bn, ln, training, ob["dx"])
        out.update(dtable=si["dtable"], dbn=si["dbn"], dln=si["dln"], dblock=ob["dparams"])
    return out


# ---- torch, the reference's op order --------------------------------------------------------------------------------
def input_stage_torch(table, X, values, bn, ln, training=True):
    """table [V,E], X int64 [B,F], values [B,Fk] or None, bn / ln tensors -> X_input [B,F,E] (the moving averages are not
    touched: Keras' non-fused path on 3-D input, biased variance)"""
    F = X.shape[1]
    Fk = 0 if values is None else values.shape[1]
    Fc = F - Fk
    ok = (X >= 0) & (X < table.shape[0])
    emb = table[torch.where(ok, X, torch.zeros_like(X))] * ok.unsqueeze(-1).to(table.dtype)
    g_bn, b_bn, mm, mv = bn
    cat = emb[:, :Fc]
    if training and Fc and X.shape[0]:
        mean = cat.mean(dim=(0, 1))
        var = ((cat - mean) ** 2).mean(dim=(0, 1))
    else:
        mean, var = mm, mv
    parts = [(cat - mean) * torch.rsqrt(var + EPS) * g_bn + b_bn]
    if Fk:
        cont = emb[:, Fc:] * values.unsqueeze(-1)
        normed = [torch.nn.functional.layer_norm(cont[:, i, :], (emb.shape[2],), ln[0][i], ln[1][i], EPS)
                  for i in range(Fk)]
        parts.append(torch.stack(normed, dim=1))
    return torch.cat(parts, dim=1)


def bilinear_plus_torch(x, p, btype):
    """x [B,F,E] -> [B,O]: BilinearInteractionPlusLayer.call"""
    W, Wr, br, gq, bq = p[:5]
    F = x.shape[1]
    fields = [x[:, i, :] for i in range(F)]
    ps = [torch.einsum("be,be->b", torch.tensordot(fields[i], W[weight_of(btype, i, t)], dims=([-1], [0])), fields[j])
          for t, (i, j) in enumerate(pairs(F))]
    z = torch.stack(ps, dim=1) @ Wr + br
    return torch.nn.functional.layer_norm(z, (z.shape[1],), gq, bq, EPS)


def senet_plus_torch(x, p, G):
    """x [B,F,E] -> [B,F,E]: SENetPlusLayer.call"""
    S0, b0, g0, be0, S1, b1, g1, be1 = p[5:]
    B, F, E = x.shape
    re = torch.stack(torch.split(x, E // G, dim=2), dim=2)
    info = torch.cat([re.mean(dim=-1), re.max(dim=-1).values], dim=-1).reshape(B, -1)
    h = torch.relu(torch.nn.functional.layer_norm(info @ S0 + b0, (S0.shape[1],), g0, be0, EPS))
    A = torch.relu(torch.nn.functional.layer_norm(h @ S1 + b1, (S1.shape[1],), g1, be1, EPS))
    return x * A.reshape(B, F, E)


def block_torch(x, p, G, btype):
    """x [B,F,E] -> [B, O + F E]"""
    return torch.cat([bilinear_plus_torch(x, p, btype), senet_plus_torch(x, p, G).reshape(x.shape[0], -1)], dim=1)


def fibinetplus_torch(table, X, values, bn, ln, block, head, G, btype, training=True):
    x = input_stage_torch(table, X, values, bn, ln, training)
    K0, c0, gh, bh, K1, c1 = head
    z = block_torch(x, block, G, btype) @ K0 + c0
    a = torch.relu(torch.nn.functional.layer_norm(z, (z.shape[1],), gh, bh, EPS))
    return torch.sigmoid(a @ K1 + c1)


def _n(t):
    return t.detach().double().numpy() if t is not None else None


def _tz(p, like):
    return _n(p.grad) if p.grad is not None else np.zeros(like.shape)


def _bn_ln(bn, ln, dtype):
    tbn = [_t(bn[0], dtype, True), _t(bn[1], dtype, True), _t(bn[2], dtype), _t(bn[3], dtype)]
    tln = [_t(ln[0], dtype, True), _t(ln[1], dtype, True)]
    return tbn, tln


def input_stage_torch_grads(table, X, values, bn, ln, training, dx, dtype):
    """-> x, dtable, dbn = [dgamma, dbeta], dln = [dgamma, dbeta] as numpy, in ``dtype`` arithmetic"""
    tb = _t(table, dtype, True)
    vals = None if values is None or values.shape[1] == 0 else _t(values, dtype)
    tbn, tln = _bn_ln(bn, ln, dtype)
    x = input_stage_torch(tb, torch.from_numpy(X), vals, tbn, tln, training).reshape(len(X), -1)
    (x * _t(dx, dtype)).sum().backward()
    return (_n(x), _tz(tb, tb), [_tz(tbn[0], tbn[0]), _tz(tbn[1], tbn[1])], [_tz(tln[0], tln[0]), _tz(tln[1], tln[1])])


def block_torch_grads(x, params, G, btype, dout, dtype):
    """x [B, F E] -> out, dx, dparams as numpy, in ``dtype`` arithmetic"""
    E = np.asarray(params[0]).shape[1]
    xx = _t(x, dtype, True)
    ps = [_t(p, dtype, True) for p in params]
    out = block_torch(xx.reshape(len(x), -1, E), ps, G, btype)
    (out * _t(dout, dtype)).sum().backward()
    return _n(out), _n(xx.grad), [_tz(p, p) for p in ps]


def fibinetplus_torch_grads(table, X, values, bn, ln, block, head, G, btype, training, dout, dtype):
    """-> output, dtable, dbn, dln, dblock, dhead as numpy, in ``dtype`` arithmetic"""
    tb = _t(table, dtype, True)
    vals = None if values is None or values.shape[1] == 0 else _t(values, dtype)
    tbn, tln = _bn_ln(bn, ln, dtype)
    bl = [_t(p, dtype, True) for p in block]
    hd = [_t(p, dtype, True) for p in head]
    out = fibinetplus_torch(tb, torch.from_numpy(X), vals, tbn, tln, bl, hd, G, btype, training)
    (out * _t(dout, dtype)).sum().backward()
    return (_n(out), _tz(tb, tb), [_tz(tbn[0], tbn[0]), _tz(tbn[1], tbn[1])], [_tz(tln[0], tln[0]), _tz(tln[1], tln[1])],
            [_tz(p, p) for p in bl], [_tz(p, p) for p in hd])
