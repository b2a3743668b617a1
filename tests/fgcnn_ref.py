"""Restatements of the reference's FGCNNBaseLayer / FGCNNLayer (3.DCN/CustomLayers.py:728-822) for the FGCNN tests.

* ``fgcnn_numpy``: an fp64 numpy reading of the conv / max-pool stack (everything before the Dense layers).  The
  convolution is ccpm_ref's; the pooling reshapes the kept rows to [H // pw, pw] windows and takes ``argmax``, which
  returns the FIRST maximum: on equal values the lower field.  The backward is written by hand: every level j receives
  a gradient dp_j of its own, added to what level j + 1 sends down; scatter to the arg-max, dy (1 - y^2), then dK, db
  and dx per tap; ``drows_direct`` is added to dx_0.
* ``fgcnn_torch`` / ``fgcnn_base_torch``: a transcription in the reference's op order -- expand_dims, Conv2D as ``F.pad``
  with TF's asymmetric SAME padding followed by ``conv2d``, tanh, ``max_pool2d((pw, 1))``, Flatten, Dense, reshape,
  concat -- runnable in any dtype, gradients by autograd.
* ``fgcnn_layer_torch``: the whole layer: lookup, the above, Flatten(concat[X_emb, fgcnn_output]), the continuous
  columns LAST, MLP with BatchNormalization (batch statistics), MLP([1], sigmoid).

Quirks of the reference that are kept: every Dense has dnn_maps x FIELDS x E // pooling_width units, from the original
field count and not from the height its layer pools; MaxPool2D is VALID, the trailing H mod pw rows are dropped.
"""
import numpy as np
import torch
import torch.nn.functional as TF

from tests.ccpm_ref import conv_numpy, conv_torch, same_pad


def heights(F, pws):
    out, h = [], F
    for pw in pws:
        h = h // pw
        out.append(h)
    return out


def dense_units(F, E, dnn_maps, pws):
    """FGCNNBaseLayer.build (:752-754): input_shape[1] is the ORIGINAL field count at every layer."""
    return [m * F * E // pw for m, pw in zip(dnn_maps, pws)]


def pool_numpy(y, pw, distinct_gap=False):
    """y [B,H,E,C] -> (max over windows of pw rows [B,H//pw,E,C], the position inside the window, gap [B]: the smallest
    (max - second max) of any window; ``distinct_gap``: values equal to the max are left out)."""
    B, H, E, Cn = y.shape
    Ho = H // pw
    w = y[:, :Ho * pw].reshape(B, Ho, pw, E, Cn)
    idx = np.argmax(w, axis=2)                                  # the first maximum: the lower field
    gap = np.full(B, np.inf)
    if pw > 1:
        s = -np.sort(-w, axis=2)
        d = s[:, :, :1] - s[:, :, 1:]
        if distinct_gap:
            d = np.where(d == 0.0, np.inf, d)
        gap = d.reshape(B, -1).min(axis=1)
    return np.take_along_axis(w, idx[:, :, None], axis=2)[:, :, 0], idx, gap


def fgcnn_numpy(rows, params, pws, dps=None, drows_direct=None, distinct_gap=False):
    """rows [B,F,E]; params [(K_1, b_1), ...]; pws [pw_1, ...] -> dict(pooled [p_1 .. p_L] with p_j [B, H_j E C_j],
    gap [B] [, drows = drows_direct + dx_0, dparams [(dK_1, db_1), ...]] when dps = [dp_1 .. dp_L] is given)."""
    x = np.asarray(rows, np.float64)[..., None]
    B = x.shape[0]
    gap = np.full(B, np.inf)
    saved, pooled = [], []
    for (K, b), pw in zip(params, pws):
        K, b = np.asarray(K, np.float64), np.asarray(b, np.float64)
        y, xp = conv_numpy(x, K, b)
        assert y.shape[1] // pw >= 1, "MaxPool2D leaves no row"
        x, idx, gp = pool_numpy(y, pw, distinct_gap)
        gap = np.minimum(gap, gp)
        saved.append((K, xp, y, idx, pw))
        pooled.append(x.reshape(B, -1))
    out = {"pooled": pooled, "gap": gap}
    if dps is None:
        return out
    g = None
    dparams = []
    for j in range(len(saved) - 1, -1, -1):
        K, xp, y, idx, pw = saved[j]
        Bn, H, E, Cn = y.shape
        Ho = H // pw
        gj = np.asarray(dps[j], np.float64).reshape(Bn, Ho, E, Cn)
        if g is not None:
            gj = gj + g
        dw = np.zeros((Bn, Ho, pw, E, Cn))
        np.put_along_axis(dw, idx[:, :, None], gj[:, :, None], axis=2)
        dy = np.zeros_like(y)                                    # the dropped trailing rows keep zero
        dy[:, :Ho * pw] = dw.reshape(Bn, Ho * pw, E, Cn)
        dpre = dy * (1.0 - y * y)
        kw = K.shape[0]
        top, _ = same_pad(kw)
        dK = np.zeros_like(K)
        dxp = np.zeros_like(xp)
        for t in range(kw):
            dK[t, 0] = np.einsum("bhec,bhed->cd", xp[:, t:t + H], dpre)
            dxp[:, t:t + H] += np.einsum("bhed,cd->bhec", dpre, K[t, 0])
        dparams.append((dK, dpre.sum(axis=(0, 1, 2))))
        g = dxp[:, top:top + H]
    drows = g[..., 0]
    if drows_direct is not None:
        drows = drows + np.asarray(drows_direct, np.float64)
    out.update(drows=drows, dparams=dparams[::-1])
    return out


def pool_torch(x, pw):
    """MaxPool2D(pool_size=(pw, 1)) on NHWC x [B,H,E,C]: strides = pool_size, VALID."""
    return TF.max_pool2d(x.permute(0, 3, 1, 2), (pw, 1)).permute(0, 2, 3, 1)


def fgcnn_torch(rows, params, pws):
    """The conv / pool part of FGCNNBaseLayer.call (:763-767); params is the flat list [K_1, b_1, K_2, b_2, ...]
    -> [Flatten(x_1), ..., Flatten(x_L)]."""
    x = rows.unsqueeze(-1)
    outs = []
    for i, pw in enumerate(pws):
        x = conv_torch(x, params[2 * i], params[2 * i + 1])
        x = pool_torch(x, pw)
        outs.append(x.reshape(x.shape[0], -1))
    return outs


def fgcnn_base_torch(rows, params, dense, pws):
    """FGCNNBaseLayer.call (:757-772); dense is the flat list [W_1, c_1, W_2, c_2, ...] -> [B, sum N_j, E]."""
    E = rows.shape[-1]
    outs = []
    for i, p in enumerate(fgcnn_torch(rows, params, pws)):
        out = p @ dense[2 * i] + dense[2 * i + 1]
        outs.append(out.reshape(-1, out.shape[1] // E, E))
    return torch.cat(outs, dim=1)


def fgcnn_torch_grads(rows, params, pws, dps, drows_direct, dtype):
    """The conv / pool transcription on the CPU in ``dtype``: ([p_j], drows, [dK_1, db_1, ...]); the loss is
    sum_j <dp_j, p_j> + <drows_direct, rows>."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_() for a in [rows] + [a for kb in params for a in kb]]
    outs = fgcnn_torch(t[0], t[1:], pws)
    loss = sum((torch.from_numpy(np.asarray(d)).to(dtype) * o).sum() for d, o in zip(dps, outs))
    if drows_direct is not None:
        loss = loss + (torch.from_numpy(np.asarray(drows_direct)).to(dtype) * t[0]).sum()
    g = torch.autograd.grad(loss, t)
    return [o.detach().numpy() for o in outs], g[0].numpy(), [x.numpy() for x in g[1:]]


def fgcnn_layer_torch(p, X, X_cont, pws, eps=1e-3):
    """FGCNNLayer.call (:796-822) in training mode.  p: embed [V,E], conv [K_1, b_1, ...], dense [W_1, c_1, ...], k1 /
    b1 / gamma / beta lists (MLP_layer1: MatMul, BiasAdd, BatchNormalization on batch statistics, relu), k2 / b2
    (MLP_layer2, sigmoid)."""
    emb = p["embed"][X]
    comb = torch.cat([emb, fgcnn_base_torch(emb, p["conv"], p["dense"], pws)], dim=1)
    x = comb.reshape(comb.shape[0], -1)
    if X_cont is not None:
        x = torch.cat([x, X_cont], dim=1)
    for K, b, gamma, beta in zip(p["k1"], p["b1"], p["gamma"], p["beta"]):
        x = x @ K + b
        mean = x.mean(dim=0)
        var = ((x - mean) ** 2).mean(dim=0)
        x = torch.relu((x - mean) / torch.sqrt(var + eps) * gamma + beta)
    return torch.sigmoid(x @ p["k2"] + p["b2"])
