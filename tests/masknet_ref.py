"""Restatements of MaskNet (11.FiBiNet++/CustomLayers.py:245-409) for the tests: an fp64 numpy reading with hand-written
gradients (input stage, one mask block, the whole layer) and a torch transcription in the reference's op order that
autograd differentiates, runnable in fp32 and fp64 on the CPU.  Parameter makers on the scale the tolerances of
tests/test_gpu_masknet.py were reasoned for: tables N(0, 0.5^2), continuous values and block inputs N(0, 1),
glorot-uniform kernels, biases and LayerNorm betas N(0, 0.1^2), gammas 1 + N(0, 0.1^2).

A block's parameters are the list [W1, b1, W2, b2, W3, b3, gamma, beta]; a head's [K0, c0, alpha, K1, c1] (Dense, PReLU,
Dense(1, sigmoid)).  An id outside [0, V) reads as a zero row, as the kernels define it."""
import numpy as np
import torch

EPS = 1e-3           # tf.keras.layers.LayerNormalization()
PRE_EPS = 1e-5       # an example with a relu pre-activation closer to 0 than this may take the other branch in fp32


def glorot(r, a, b):
    lim = np.sqrt(6.0 / (a + b))
    return r.uniform(-lim, lim, (a, b))


def make_input(r, B, Fc, Fk, E, V):
    """-> table [V,E], X [B,Fc+Fk] int64, values [B,Fk], gamma [F,E], beta [F,E]"""
    F = Fc + Fk
    return (r.normal(0, 0.5, (V, E)), r.integers(0, V, (B, F)).astype(np.int64), r.normal(0, 1, (B, Fk)),
            1 + r.normal(0, 0.1, (F, E)), r.normal(0, 0.1, (F, E)))


def make_block(r, D, P, O, R):
    H = R * P
    return [glorot(r, D, H), r.normal(0, 0.1, H), glorot(r, H, P), r.normal(0, 0.1, P), glorot(r, P, O),
            r.normal(0, 0.1, O), 1 + r.normal(0, 0.1, O), r.normal(0, 0.1, O)]


def make_head(r, n_in, units=32):
    return [glorot(r, n_in, units), r.normal(0, 0.1, units), r.normal(0, 0.1, units), glorot(r, units, 1),
            r.normal(0, 0.1, 1)]


def make_stack(r, F, E, O, NB, mode="serial", R=3):
    D = F * E
    return [make_block(r, D, D if (k == 0 or mode != "serial") else O, O, R) for k in range(NB)]


# ---- numpy, fp64 ----------------------------------------------------------------------------------------------------
def _ln(x, g, b):
    mean = x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt(((x - mean) ** 2).mean(-1, keepdims=True) + EPS)
    xhat = (x - mean) * rstd
    return xhat * g + b, xhat, rstd


def _ln_bwd(dy, xhat, rstd, g):
    dxh = dy * g
    return rstd * (dxh - dxh.mean(-1, keepdims=True) - xhat * (dxh * xhat).mean(-1, keepdims=True))


def gather(table, X):
    ok = (X >= 0) & (X < table.shape[0])
    return table[np.where(ok, X, 0)] * ok[..., None]


def input_stage_numpy(table, X, values, gamma, beta, dx_norm=None, dx_emb=None):
    """-> x_emb, x_norm [B, F E]; with dx_norm (and dx_emb, None: zeros) also vals [B*F, E], dgamma, dbeta, dtable."""
    table = np.asarray(table, np.float64)
    B, F = X.shape
    E = table.shape[1]
    Fc = F - (0 if values is None else values.shape[1])
    scale = np.ones((B, F))
    if F > Fc:
        scale[:, Fc:] = values
    rows = gather(table, X)
    rows[:, Fc:] = rows[:, Fc:] * scale[:, Fc:, None]
    y, xhat, rstd = _ln(rows, gamma, beta)
    out = {"x_emb": rows.reshape(B, F * E), "x_norm": y.reshape(B, F * E)}
    if dx_norm is not None:
        dy = np.asarray(dx_norm, np.float64).reshape(B, F, E)
        g = _ln_bwd(dy, xhat, rstd, gamma)
        if dx_emb is not None:
            g = g + np.asarray(dx_emb, np.float64).reshape(B, F, E)
        vals = g * scale[:, :, None]
        out.update(vals=vals.reshape(B * F, E), dgamma=(dy * xhat).sum(0), dbeta=dy.sum(0))
        dtable = np.zeros_like(table)
        ok = (X >= 0) & (X < table.shape[0])
        np.add.at(dtable, X[ok], vals[ok])
        out["dtable"] = dtable
    return out


def block_numpy(x_emb, v, params, dy=None):
    """-> y, pre = min over the units of |relu pre-activation| per example; with dy also dv, dx_emb, dparams (order of
    params)."""
    W1, b1, W2, b2, W3, b3, g, be = [np.asarray(p, np.float64) for p in params]
    x_emb, v = np.asarray(x_emb, np.float64), np.asarray(v, np.float64)
    p1 = x_emb @ W1 + b1
    h = np.maximum(p1, 0)
    m = h @ W2 + b2
    u = v * m
    p2, xhat, rstd = _ln(u @ W3 + b3, g, be)
    out = {"y": np.maximum(p2, 0), "pre": np.minimum(np.abs(p1).min(1), np.abs(p2).min(1))}
    if dy is not None:
        gy = np.asarray(dy, np.float64) * (p2 > 0)
        dz = _ln_bwd(gy, xhat, rstd, g)
        du = dz @ W3.T
        dm = du * v
        dh = (dm @ W2.T) * (p1 > 0)
        out.update(dv=du * m, dx_emb=dh @ W1.T,
                   dparams=[x_emb.T @ dh, dh.sum(0), h.T @ dm, dm.sum(0), u.T @ dz, dz.sum(0), (gy * xhat).sum(0),
                            gy.sum(0)])
    return out


def masknet_numpy(table, X, values, gamma, beta, blocks, head, mode="serial", dout=None):
    """The whole layer -> output [B,1], pre (per example, every relu / PReLU pre-activation); with dout = dLoss/doutput
    also dtable, dgamma, dbeta, dblocks, dhead."""
    st = input_stage_numpy(table, X, values, gamma, beta)
    xe, xn = st["x_emb"], st["x_norm"]
    vs, ys, pre = [], [], np.full(X.shape[0], np.inf)
    for k, bp in enumerate(blocks):
        vs.append(xn if (k == 0 or mode != "serial") else ys[-1])
        o = block_numpy(xe, vs[-1], bp)
        ys.append(o["y"])
        pre = np.minimum(pre, o["pre"])
    top = ys[-1] if mode == "serial" else np.concatenate(ys, 1)
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
        dtop = dz1 @ K0.T
        O = ys[0].shape[1]
        dxe, dxn, dblocks = np.zeros_like(xe), np.zeros_like(xn), [None] * len(blocks)
        dy = dtop if mode == "serial" else None
        for k in reversed(range(len(blocks))):
            if mode != "serial":
                dy = dtop[:, k * O:(k + 1) * O]
            o = block_numpy(xe, vs[k], blocks[k], dy)
            dblocks[k] = o["dparams"]
            dxe += o["dx_emb"]
            if k == 0 or mode != "serial":
                dxn += o["dv"]
            else:
                dy = o["dv"]
        st = input_stage_numpy(table, X, values, gamma, beta, dxn, dxe)
        out.update(dtable=st["dtable"], dgamma=st["dgamma"], dbeta=st["dbeta"], dblocks=dblocks)
    return out


# ---- torch, the reference's op order --------------------------------------------------------------------------------
def _t(a, dtype, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=dtype, requires_grad=grad)


def input_stage_torch(table, X, values, gamma, beta):
    """table [V,E], X int64 [B,F], values [B,Fk] or None, gamma / beta [F,E] tensors -> X_emb_normed, X_emb [B,F,E]"""
    F = X.shape[1]
    Fc = F - (0 if values is None else values.shape[1])
    ok = (X >= 0) & (X < table.shape[0])
    emb = table[torch.where(ok, X, torch.zeros_like(X))] * ok.unsqueeze(-1).to(table.dtype)
    if F > Fc:
        emb = torch.cat([emb[:, :Fc], emb[:, Fc:] * values.unsqueeze(-1)], dim=1)
    normed = [torch.nn.functional.layer_norm(emb[:, i, :], (emb.shape[2],), gamma[i], beta[i], EPS) for i in range(F)]
    return torch.stack(normed, dim=1), emb


def block_torch(x_emb, v, p):
    W1, b1, W2, b2, W3, b3, g, be = p
    mask = torch.relu(x_emb @ W1 + b1) @ W2 + b2
    z = (v * mask) @ W3 + b3
    return torch.relu(torch.nn.functional.layer_norm(z, (z.shape[1],), g, be, EPS))


def masknet_torch(table, X, values, gamma, beta, blocks, head, mode="serial"):
    normed, emb = input_stage_torch(table, X, values, gamma, beta)
    D = emb.shape[1] * emb.shape[2]
    normed, emb = normed.reshape(-1, D), emb.reshape(-1, D)
    if mode == "serial":
        x = block_torch(emb, normed, blocks[0])
        for p in blocks[1:]:
            x = block_torch(emb, x, p)
    else:
        x = torch.cat([block_torch(emb, normed, p) for p in blocks], dim=1)
    K0, c0, alpha, K1, c1 = head
    z1 = x @ K0 + c0
    a = torch.relu(z1) - alpha * torch.relu(-z1)
    return torch.sigmoid(a @ K1 + c1)


def input_stage_torch_grads(table, X, values, gamma, beta, dx_norm, dx_emb, dtype):
    """-> x_emb, x_norm, dtable, dgamma, dbeta as numpy, in ``dtype`` arithmetic"""
    tb, g, b = _t(table, dtype, True), _t(gamma, dtype, True), _t(beta, dtype, True)
    vals = None if values is None or values.shape[1] == 0 else _t(values, dtype)
    normed, emb = input_stage_torch(tb, torch.from_numpy(X), vals, g, b)
    loss = (normed.reshape(len(X), -1) * _t(dx_norm, dtype)).sum()
    if dx_emb is not None:
        loss = loss + (emb.reshape(len(X), -1) * _t(dx_emb, dtype)).sum()
    loss.backward()
    n = lambda t: t.detach().double().numpy()
    return n(emb).reshape(len(X), -1), n(normed).reshape(len(X), -1), n(tb.grad), n(g.grad), n(b.grad)


def block_torch_grads(x_emb, v, params, dy, dtype):
    """-> y, dv, dx_emb, dparams as numpy, in ``dtype`` arithmetic"""
    xe, vv = _t(x_emb, dtype, True), _t(v, dtype, True)
    ps = [_t(p, dtype, True) for p in params]
    y = block_torch(xe, vv, ps)
    (y * _t(dy, dtype)).sum().backward()
    n = lambda t: t.detach().double().numpy()
    return n(y), n(vv.grad), n(xe.grad), [n(p.grad) for p in ps]


def masknet_torch_grads(table, X, values, gamma, beta, blocks, head, mode, dout, dtype):
    """-> output, dtable, dgamma, dbeta, dblocks, dhead as numpy, in ``dtype`` arithmetic"""
    tb, g, b = _t(table, dtype, True), _t(gamma, dtype, True), _t(beta, dtype, True)
    vals = None if values is None or values.shape[1] == 0 else _t(values, dtype)
    bl = [[_t(p, dtype, True) for p in bp] for bp in blocks]
    hd = [_t(p, dtype, True) for p in head]
    out = masknet_torch(tb, torch.from_numpy(X), vals, g, b, bl, hd, mode)
    (out * _t(dout, dtype)).sum().backward()
    n = lambda t: t.detach().double().numpy()
    return n(out), n(tb.grad), n(g.grad), n(b.grad), [[n(p.grad) for p in bp] for bp in bl], [n(p.grad) for p in hd]


def rel_err(got, want):
    """the project's measure, per tensor: max |got - want| / max |want|"""
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / max(np.abs(want).max(), 1e-30)) if want.size else 0.0


def clean_seed(near_fn, limit=64):
    """the first seed 1, 2, 3, ... for which near_fn(seed) (fp64 reading only) reports no near-kink example"""
    for s in range(1, limit + 1):
        if not near_fn(s):
            return s
    raise AssertionError("no seed without a near-kink example among the first %d" % limit)
