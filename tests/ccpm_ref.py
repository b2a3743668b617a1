"""Restatements of the reference's KMaxPool / CCPMBaseLayer / CCPMLayer (3.DCN/CustomLayers.py:621-725) for the CCPM
tests.

* ``ccpm_numpy``: an fp64 numpy reading.  The convolution is a sum over the taps of padded slices, the pooling a stable
  argsort of the negated values, and the backward is written by hand: scatter to the selected positions, dy (1 - y^2),
  then dK, db and dx per tap.
* ``ccpm_torch``: a transcription in the reference's op order -- expand_dims, Conv2D as ``F.pad`` with TF's asymmetric
  SAME padding followed by ``conv2d``, tanh, KMaxPool as transpose [0,3,2,1] / sorted top k / transpose back, Flatten --
  runnable in any dtype, gradients by autograd.  The selection is ``torch.sort(descending=True, stable=True)``: like
  tf.nn.top_k it returns the values in descending order and the lower index first on equal values (torch.topk leaves
  that order unspecified).
* ``ccpm_layer_torch``: the whole layer: lookup, the above, concat with the continuous columns LAST, MLP with
  BatchNormalization (batch statistics), MLP([1], sigmoid).

Quirks of the reference that are kept: the k of the poolings is computed from the EMBEDDING width (``input_shape[-1]``),
not from the field count; the pooled values come out in descending order of VALUE, not in field order.
"""
import numpy as np
import torch
import torch.nn.functional as TF


def ccpm_k(E, L):
    """CCPMBaseLayer.build (:657-667): fields_num = input_shape[-1] = E."""
    fields_num = E
    ks = []
    for i in range(L):
        j = i + 1
        ks.append(max(1, int((1 - pow(j / L, L - j)) * fields_num)) if j < L else 3)
    return ks


def same_pad(kw):
    """TF SAME padding at stride 1: kw - 1 rows in all, the extra one at the END."""
    top = (kw - 1) // 2
    return top, kw - 1 - top


def conv_numpy(x, K, b):
    """x [B,H,E,Cin], K [kw,1,Cin,Cout], b [Cout] -> tanh(cross-correlation along H with SAME padding) [B,H,E,Cout]."""
    kw = K.shape[0]
    top, bot = same_pad(kw)
    H = x.shape[1]
    xp = np.pad(x, ((0, 0), (top, bot), (0, 0), (0, 0)))
    pre = np.zeros(x.shape[:3] + (K.shape[3],)) + b
    for t in range(kw):
        pre = pre + np.einsum("bhec,cd->bhed", xp[:, t:t + H], K[t, 0])
    return np.tanh(pre), xp


def kmax_numpy(y, k):
    """y [B,H,E,C] -> (values [B,k,E,C] descending, their positions, the whole stable descending order)."""
    order = np.argsort(-y, axis=1, kind="stable")
    idx = order[:, :k]
    return np.take_along_axis(y, idx, axis=1), idx, order


def ccpm_numpy(rows, params, ks, dout=None, distinct_gap=False):
    """rows [B,F,E]; params [(K_1, b_1), ...]; ks [k_1, ...] -> dict(out [B, k_L E C_L], gap [B] [, drows, dparams
    [(dK_1, db_1), ...]]).  gap: per example the smallest difference between neighbours among the first
    min(k, H-1) + 1 sorted values of any (e, c) column of any layer (``distinct_gap``: exact ties are left out)."""
    x = np.asarray(rows, np.float64)[..., None]
    B = x.shape[0]
    gap = np.full(B, np.inf)
    saved = []
    for (K, b), k in zip(params, ks):
        K, b = np.asarray(K, np.float64), np.asarray(b, np.float64)
        y, xp = conv_numpy(x, K, b)
        H = y.shape[1]
        assert k <= H, "top_k: k exceeds the height"
        xo, idx, order = kmax_numpy(y, k)
        n = min(k, H - 1) + 1
        ys = np.take_along_axis(y, order[:, :n], axis=1)
        d = ys[:, :-1] - ys[:, 1:]
        if distinct_gap:
            d = np.where(d == 0.0, np.inf, d)
        if d.shape[1]:
            gap = np.minimum(gap, d.reshape(B, -1).min(axis=1))
        saved.append((K, xp, y, idx))
        x = xo
    out = {"out": x.reshape(B, -1), "gap": gap}
    if dout is None:
        return out
    g = np.asarray(dout, np.float64).reshape(x.shape)
    dparams = []
    for K, xp, y, idx in reversed(saved):
        kw = K.shape[0]
        top, _ = same_pad(kw)
        H = y.shape[1]
        dy = np.zeros_like(y)
        np.put_along_axis(dy, idx, g, axis=1)                 # the selected positions only
        dpre = dy * (1.0 - y * y)
        dK = np.zeros_like(K)
        dxp = np.zeros_like(xp)
        for t in range(kw):
            dK[t, 0] = np.einsum("bhec,bhed->cd", xp[:, t:t + H], dpre)
            dxp[:, t:t + H] += np.einsum("bhed,cd->bhec", dpre, K[t, 0])
        dparams.append((dK, dpre.sum(axis=(0, 1, 2))))
        g = dxp[:, top:top + H]
    out.update(drows=g[..., 0], dparams=dparams[::-1])
    return out


def conv_torch(x, K, b):
    """Conv2D(filters, (kw, 1), strides 1, padding='same', activation='tanh') on NHWC x [B,H,E,Cin]."""
    top, bot = same_pad(K.shape[0])
    xp = TF.pad(x.permute(0, 3, 1, 2), (0, 0, top, bot))      # NCHW, H padded top / bottom
    y = TF.conv2d(xp, K.permute(3, 2, 0, 1), b)               # weight [Cout,Cin,kw,1]
    return torch.tanh(y).permute(0, 2, 3, 1)


def kmax_torch(x, k):
    """KMaxPool.call (:629-637)."""
    inputs = x.permute(0, 3, 2, 1)
    k_max = torch.sort(inputs, dim=-1, descending=True, stable=True)[0][..., :k]
    return k_max.permute(0, 3, 2, 1)


def ccpm_torch(rows, params, ks):
    """CCPMBaseLayer.call (:669-677); params is the flat list [K_1, b_1, K_2, b_2, ...]."""
    x = rows.unsqueeze(-1)
    for i, k in enumerate(ks):
        x = conv_torch(x, params[2 * i], params[2 * i + 1])
        x = kmax_torch(x, k)
    return x.reshape(x.shape[0], -1)


def ccpm_torch_grads(rows, params, ks, dout, dtype):
    """The transcription on the CPU in ``dtype``: (out, drows, [dK_1, db_1, ...])."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_() for a in [rows] + [a for kb in params for a in kb]]
    out = ccpm_torch(t[0], t[1:], ks)
    g = torch.autograd.grad(out, t, torch.from_numpy(np.asarray(dout)).to(dtype))
    return out.detach().numpy(), g[0].numpy(), [x.numpy() for x in g[1:]]


def ccpm_layer_torch(p, X, X_cont, ks, eps=1e-3):
    """CCPMLayer.call (:701-725) in training mode.  p: embed [V,E], conv [K_1, b_1, ...], k1 / b1 / gamma / beta lists
    (MLP_layer1: MatMul, BiasAdd, BatchNormalization on batch statistics, relu), k2 / b2 (MLP_layer2, sigmoid)."""
    x = torch.cat([ccpm_torch(p["embed"][X], p["conv"], ks), X_cont], dim=1) if X_cont is not None \
        else ccpm_torch(p["embed"][X], p["conv"], ks)
    for K, b, gamma, beta in zip(p["k1"], p["b1"], p["gamma"], p["beta"]):
        x = x @ K + b
        mean = x.mean(dim=0)
        var = ((x - mean) ** 2).mean(dim=0)
        x = torch.relu((x - mean) / torch.sqrt(var + eps) * gamma + beta)
    return torch.sigmoid(x @ p["k2"] + p["b2"])


def glorot_uniform_conv(shape, r):
    """Keras glorot_uniform for a conv kernel [kw,1,Cin,Cout]: the receptive field counts in both fans."""
    rf = int(np.prod(shape[:-2]))
    lim = np.sqrt(6.0 / (rf * shape[-2] + rf * shape[-1]))
    return r.uniform(-lim, lim, shape)


def make_params(filters, kernel_width, seed):
    """[(K_j, b_j)] in fp32: glorot-uniform kernels, biases ~ N(0, 0.1^2)."""
    r = np.random.default_rng(seed)
    out, cin = [], 1
    for c, kw in zip(filters, kernel_width):
        out.append((np.asarray(glorot_uniform_conv((kw, 1, cin, c), r), np.float32),
                    np.asarray(r.standard_normal(c) * 0.1, np.float32)))
        cin = c
    return out


def flat_params(params):
    return np.concatenate([np.asarray(a, np.float32).reshape(-1) for kb in params for a in kb])


def make_table(V, E, seed):
    return np.asarray(np.random.default_rng(seed).standard_normal((V, E)) * 0.5, np.float32)
