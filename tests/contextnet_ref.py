"""Restatements of ContextNet (11.FiBiNet++/CustomLayers.py:412-531) for the tests: an fp64 numpy reading with
hand-written gradients (input stage, one block in both modes, the whole layer with its head) and a torch transcription in
the reference's op order (one slice, product and LayerNormalization per field) that autograd differentiates, runnable in
fp32 and fp64 on the CPU.  Parameters on the scale of tests/masknet_ref.py: tables N(0, 0.5^2), continuous values and
block inputs N(0, 1), glorot-uniform Dense kernels, glorot-normal per-field matrices (as the reference initialises them),
biases and LayerNorm betas N(0, 0.1^2), gammas 1 + N(0, 0.1^2).

A block's parameters are the list [Wa, ba, Wb, bb, W1, W2, gamma, beta] in 'pointwise' mode and [Wa, ba, Wb, bb, W1, gamma,
beta] in any other ('single'): Wa [D, R D], Wb [R D, D], W1, W2 [F, E, E], gamma, beta [F, E], D = F E.  A head is
masknet_ref's [K0, c0, alpha, K1, c1].  ``pre`` is, per example, the smallest |relu pre-activation| over both h and a
(and the head's PReLU in the layer).  An id outside [0, V) reads as a zero row, as the kernels define it."""
import numpy as np
import torch

from tests.masknet_ref import (EPS, PRE_EPS, _ln, _ln_bwd, _t, clean_seed, gather, glorot, make_head,  # noqa: F401
                               rel_err)


def glorot_normal(r, F, E):
    return np.clip(r.normal(0, 1, (F, E, E)), -2, 2) * np.sqrt(2.0 / (E + E)) / 0.87962566


def make_block(r, F, E, R, mode="pointwise"):
    D = F * E
    H = R * D
    p = [glorot(r, D, H), r.normal(0, 0.1, H), glorot(r, H, D), r.normal(0, 0.1, D), glorot_normal(r, F, E)]
    if mode == "pointwise":
        p.append(glorot_normal(r, F, E))
    return p + [1 + r.normal(0, 0.1, (F, E)), r.normal(0, 0.1, (F, E))]


def make_input(r, B, Fc, Fk, E, V):
    """-> table [V,E], X [B,Fc+Fk] int64, values [B,Fk]"""
    return r.normal(0, 0.5, (V, E)), r.integers(0, V, (B, Fc + Fk)).astype(np.int64), r.normal(0, 1, (B, Fk))


def _split(params, mode):
    p = [np.asarray(a, np.float64) for a in params]
    if mode == "pointwise":
        return p
    return p[:5] + [None] + p[5:]


# ---- numpy, fp64 ----------------------------------------------------------------------------------------------------
def input_stage_numpy(table, X, values, dx=None):
    """-> x [B, F E]; with dx also vals [B*F, E] and dtable."""
    table = np.asarray(table, np.float64)
    B, F = X.shape
    E = table.shape[1]
    Fc = F - (0 if values is None else values.shape[1])
    scale = np.ones((B, F))
    if F > Fc:
        scale[:, Fc:] = values
    out = {"x": (gather(table, X) * scale[:, :, None]).reshape(B, F * E)}
    if dx is not None:
        vals = np.asarray(dx, np.float64).reshape(B, F, E) * scale[:, :, None]
        dtable = np.zeros_like(table)
        ok = (X >= 0) & (X < table.shape[0])
        np.add.at(dtable, X[ok], vals[ok])
        out.update(vals=vals.reshape(B * F, E), dtable=dtable)
    return out


def block_numpy(x, params, mode="pointwise", dy=None):
    """x [B, F E] -> y [B, F E], pre; with dy also dx and dparams (order of params)."""
    Wa, ba, Wb, bb, W1, W2, g, be = _split(params, mode)
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    F, E, _ = W1.shape
    p1 = x @ Wa + ba
    h = np.maximum(p1, 0)
    m = h @ Wb + bb
    u = (x * m).reshape(B, F, E)
    pre = np.abs(p1).min(1) if B else np.zeros(0)
    if mode == "pointwise":
        p2 = np.einsum("bfe,fej->bfj", u, W1)
        a = np.maximum(p2, 0)
        r = np.einsum("bfe,fej->bfj", a, W2) + u
        pre = np.minimum(pre, np.abs(p2).reshape(B, -1).min(1))
    else:
        r = np.einsum("bfe,fej->bfj", u, W1)
    y, xhat, rstd = _ln(r, g, be)
    out = {"y": y.reshape(B, F * E), "pre": pre}
    if dy is not None:
        gy = np.asarray(dy, np.float64).reshape(B, F, E)
        dr = _ln_bwd(gy, xhat, rstd, g)
        if mode == "pointwise":
            da = np.einsum("bfj,fej->bfe", dr, W2) * (p2 > 0)
            dW2 = np.einsum("bfe,bfj->fej", a, dr)
            du = dr + np.einsum("bfj,fej->bfe", da, W1)
            dW = [np.einsum("bfe,bfj->fej", u, da), dW2]
        else:
            du = np.einsum("bfj,fej->bfe", dr, W1)
            dW = [np.einsum("bfe,bfj->fej", u, dr)]
        du = du.reshape(B, F * E)
        dm = du * x
        dh = (dm @ Wb.T) * (p1 > 0)
        out.update(dx=du * m + dh @ Wa.T,
                   dparams=[x.T @ dh, dh.sum(0), h.T @ dm, dm.sum(0)] + dW + [(gy * xhat).sum(0), gy.sum(0)])
    return out


def contextnet_numpy(table, X, values, blocks, head, mode="pointwise", dout=None):
    """The whole layer -> output [B,1], pre (per example, every relu / PReLU pre-activation); with dout = dLoss/doutput
    also dtable, dblocks, dhead."""
    xs, pre = [input_stage_numpy(table, X, values)["x"]], np.full(X.shape[0], np.inf)
    for bp in blocks:
        o = block_numpy(xs[-1], bp, mode)
        xs.append(o["y"])
        pre = np.minimum(pre, o["pre"])
    top = xs[-1]
    K0, c0, alpha, K1, c1 = [np.asarray(p, np.float64) for p in head]
    z1 = top @ K0 + c0
    a = np.maximum(z1, 0) + alpha * np.minimum(z1, 0)
    prob = 1.0 / (1.0 + np.exp(-(a @ K1 + c1)))
    out = {"output": prob, "pre": np.minimum(pre, np.abs(z1).min(1))}
    if dout is not None:
        dl = np.asarray(dout, np.float64) * prob * (1 - prob)
        da = dl @ K1.T
        dz1 = da * np.where(z1 > 0, 1.0, alpha)
        out["dhead"] = [top.T @ dz1, dz1.sum(0), (da * np.minimum(z1, 0)).sum(0), a.T @ dl, dl.sum(0)]
        dy, dblocks = dz1 @ K0.T, [None] * len(blocks)
        for k in reversed(range(len(blocks))):
            o = block_numpy(xs[k], blocks[k], mode, dy)
            dblocks[k], dy = o["dparams"], o["dx"]
        out.update(dtable=input_stage_numpy(table, X, values, dy)["dtable"], dblocks=dblocks)
    return out


# ---- torch, the reference's op order --------------------------------------------------------------------------------
def input_stage_torch(table, X, values):
    """table [V,E], X int64 [B,F], values [B,Fk] or None -> X [B,F,E]"""
    F = X.shape[1]
    Fc = F - (0 if values is None else values.shape[1])
    ok = (X >= 0) & (X < table.shape[0])
    emb = table[torch.where(ok, X, torch.zeros_like(X))] * ok.unsqueeze(-1).to(table.dtype)
    if F > Fc:
        emb = torch.cat([emb[:, :Fc], emb[:, Fc:] * values.unsqueeze(-1)], dim=1)
    return emb


def block_torch(x, p, mode="pointwise"):
    """x [B,F,E] -> [B,F,E]: ContextNetBlockLayer.call, field by field"""
    if mode == "pointwise":
        Wa, ba, Wb, bb, W1, W2, g, be = p
    else:
        Wa, ba, Wb, bb, W1, g, be = p
    B, F, E = x.shape
    mask = (torch.relu(x.reshape(B, F * E) @ Wa + ba) @ Wb + bb).reshape(B, F, E)
    outs = []
    for i in range(F):
        inp = x[:, i, :] * mask[:, i, :]
        o = inp @ W1[i]
        if mode == "pointwise":
            o = torch.relu(o) @ W2[i] + inp
        outs.append(torch.nn.functional.layer_norm(o, (E,), g[i], be[i], EPS))
    return torch.stack(outs, dim=1)


def contextnet_torch(table, X, values, blocks, head, mode="pointwise"):
    x = input_stage_torch(table, X, values)
    for p in blocks:
        x = block_torch(x, p, mode)
    K0, c0, alpha, K1, c1 = head
    z1 = x.reshape(x.shape[0], -1) @ K0 + c0
    a = torch.relu(z1) - alpha * torch.relu(-z1)
    return torch.sigmoid(a @ K1 + c1)


def _n(t):
    return t.detach().double().numpy()


def input_stage_torch_grads(table, X, values, dx, dtype):
    """-> x, dtable as numpy, in ``dtype`` arithmetic"""
    tb = _t(table, dtype, True)
    vals = None if values is None or values.shape[1] == 0 else _t(values, dtype)
    emb = input_stage_torch(tb, torch.from_numpy(X), vals).reshape(len(X), -1)
    (emb * _t(dx, dtype)).sum().backward()
    return _n(emb), _n(tb.grad)


def block_torch_grads(x, params, mode, dy, dtype):
    """x [B, F E] -> y, dx, dparams as numpy, in ``dtype`` arithmetic"""
    F, E, _ = np.asarray(params[4]).shape
    xx = _t(x, dtype, True)
    ps = [_t(p, dtype, True) for p in params]
    y = block_torch(xx.reshape(-1, F, E), ps, mode).reshape(len(x), -1)
    (y * _t(dy, dtype)).sum().backward()
    return _n(y), _n(xx.grad), [_n(p.grad) for p in ps]


def contextnet_torch_grads(table, X, values, blocks, head, mode, dout, dtype):
    """-> output, dtable, dblocks, dhead as numpy, in ``dtype`` arithmetic"""
    tb = _t(table, dtype, True)
    vals = None if values is None or values.shape[1] == 0 else _t(values, dtype)
    bl = [[_t(p, dtype, True) for p in bp] for bp in blocks]
    hd = [_t(p, dtype, True) for p in head]
    out = contextnet_torch(tb, torch.from_numpy(X), vals, bl, hd, mode)
    (out * _t(dout, dtype)).sum().backward()
    return _n(out), _n(tb.grad), [[_n(p.grad) for p in bp] for bp in bl], [_n(p.grad) for p in hd]
