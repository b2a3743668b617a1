"""Restatements of FinalMLPLayer (8.DMR/CustomLayers.py:319-442) for the tests: an fp64 numpy reading of the body with a
hand-derived backward (the full BatchNorm backward and the moving-statistic update included), a torch transcription in
the reference's op order that autograd differentiates, runnable in fp32 and fp64 on the CPU, the whole layer with its
three lookups, and the cases the host and GPU tests share.

The body's parameters are the list of include/mi355rec.h, in its order (``shapes``):
  gate s = 1, 2: Wh_s [D_s, Hg_s], bh_s, Wo_s [Hg_s, D], bo_s;  stream s, layer l: W [in, w], b, gamma, beta;
  W_1 [d1, o], c_1, W_2 [d2, o], c_2, W_12 [n, d1 / n, d2 / n, o]
and ``moving`` is the list of the 2 L moving means (stream 1 layer 0 .., then stream 2) followed by the 2 L moving
variances.  Scale as in tests/masknet_ref.py: glorot-uniform kernels, every bias N(0, 0.1^2), gamma 1 + N(0, 0.1^2), beta
N(0, 0.1^2), moving means N(0, 0.1^2), moving variances U(0.5, 1.5), inputs N(0, 1), tables N(0, 0.5^2).

ReLU kinks.  BatchNorm couples the examples of a batch, so zeroing the upstream gradient of an example near a kink does
not isolate it.  Instead both readings take ``pin``: where an fp64 ReLU pre-activation lies within PRE_EPS of zero they
take the branch ``pin`` holds (the tests read it from what the kernel saved: hg > 0, a > 0), everywhere else their own."""
import functools

import numpy as np
import torch

from tests.masknet_ref import PRE_EPS, _t, clean_seed, glorot, rel_err  # noqa: F401

EPS, MOMENTUM = 1e-3, 0.99
SAVED = ["hg", "g", "z", "a", "stats"]

# (B, D, D1, D2, Hg1, Hg2, widths1, widths2, n, o)
DEFAULT_DIMS = (160, 80, 80, 64, 64, (64, 64, 64), (64, 64, 64), 8, 1)
BODY_CASES = [(1, 1, 1, 1, 1, 1, (1,), (1,), 1, 1), (2, 15, 5, 10, 3, 7, (5, 7), (12, 4), 1, 2),
              (33,) + DEFAULT_DIMS, (31,) + DEFAULT_DIMS, (32,) + DEFAULT_DIMS,
              (17, 416, 208, 208, 128, 128, (128, 64), (64, 128), 64, 1),
              (33, 160, 80, 80, 64, 64, (64,), (64,), 8, 4), (2049,) + DEFAULT_DIMS]
# the default shape with one constant column and one large-mean column in layer 0 of stream 1 (``special_case``)
SPECIAL_BATCHES = (33, 2049)
CONST_COL, BIG_COL, BIG_BIAS, BIG_BETA = 3, 5, 1e3, 5.0


def f32_exact(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def shapes(D, D1, D2, Hg1, Hg2, w1, w2, n, o):
    """[(name, shape)] in the packed order"""
    out = []
    for s, (Dx, Hg) in enumerate(((D1, Hg1), (D2, Hg2)), 1):
        out += [("Wh_%d" % s, (Dx, Hg)), ("bh_%d" % s, (Hg,)), ("Wo_%d" % s, (Hg, D)), ("bo_%d" % s, (D,))]
    for s, ws in enumerate((w1, w2), 1):
        d = D
        for l, w in enumerate(ws):
            out += [("W_%d_%d" % (s, l), (d, w)), ("b_%d_%d" % (s, l), (w,)), ("gamma_%d_%d" % (s, l), (w,)),
                    ("beta_%d_%d" % (s, l), (w,))]
            d = w
    return out + [("W_1", (w1[-1], o)), ("c_1", (o,)), ("W_2", (w2[-1], o)), ("c_2", (o,)),
                  ("W_12", (n, w1[-1] // n, w2[-1] // n, o))]


def w12_limit(n, h1, h2, o):
    """Keras' glorot-uniform bound of a rank-4 variable: the leading dims are the receptive field"""
    return np.sqrt(6.0 / (n * h1 * h2 + n * h1 * o))


def make_body(r, D, D1, D2, Hg1, Hg2, w1, w2, n, o):
    """-> (params, moving)"""
    params = []
    for name, shape in shapes(D, D1, D2, Hg1, Hg2, w1, w2, n, o):
        if name == "W_12":
            lim = w12_limit(*shape)
            params.append(r.uniform(-lim, lim, shape))
        elif len(shape) == 2:
            params.append(glorot(r, *shape))
        elif name.startswith("gamma"):
            params.append(1 + r.normal(0, 0.1, shape))
        else:
            params.append(r.normal(0, 0.1, shape))
    widths = list(w1) + list(w2)
    return params, [r.normal(0, 0.1, w) for w in widths] + [r.uniform(0.5, 1.5, w) for w in widths]


def pack(params):
    return np.concatenate([np.asarray(p).reshape(-1) for p in params])


def unpack(flat, dims):
    out, at = [], 0
    for _, shape in shapes(*dims):
        cnt = int(np.prod(shape))
        out.append(np.asarray(flat[at:at + cnt]).reshape(shape))
        at += cnt
    assert at == len(flat)
    return out


def _zcols(w1, w2):
    """column of (stream, layer) in z / a / stats: layer-major, stream 1 first"""
    cols, at = {}, 0
    for l in range(len(w1)):
        cols[(0, l)] = at
        at += w1[l]
        cols[(1, l)] = at
        at += w2[l]
    return cols, at


def _branch(pre, pin):
    """the relu branch: pre > 0, but where |pre| < PRE_EPS (fp64 reading) the branch ``pin`` holds"""
    act = pre > 0
    if pin is not None:
        near = np.abs(pre) < PRE_EPS
        act = np.where(near, pin, act)
    return act


# ---- numpy, fp64 ----------------------------------------------------------------------------------------------------
def body_numpy(xs, x1, x2, params, moving, w1, w2, n, training, dout=None, pin=None):
    """-> out [B, o], the save buffers, ``pre_h`` [B, Hg1 + Hg2] and ``pre_y`` [B, Z] (the relu pre-activations),
    ``moving`` after the call; with dout also dxs, dx1, dx2 and dparams (order of params).  ``pin``: dict(h=, y=) of
    boolean branches for the near-kink entries."""
    P = [np.asarray(a, np.float64) for a in params]
    xs, xg = np.asarray(xs, np.float64), [np.asarray(x1, np.float64), np.asarray(x2, np.float64)]
    B, L, ws = xs.shape[0], len(w1), (list(w1), list(w2))
    zc, Z = _zcols(w1, w2)
    mm, mv = [np.asarray(a, np.float64) for a in moving[:2 * L]], [np.asarray(a, np.float64) for a in moving[2 * L:]]
    gate, stream, head = P[:8], P[8:8 + 8 * L], P[8 + 8 * L:]
    hgs, gs, parts, pre_h, hact = [], [], [], [], []
    Hoff = [0, gate[0].shape[1]]
    for s in range(2):
        Wh, bh, Wo, bo = gate[4 * s:4 * s + 4]
        ph = xg[s] @ Wh + bh
        act = _branch(ph, None if pin is None else pin["h"][:, Hoff[s]:Hoff[s] + Wh.shape[1]])
        h = np.where(act, ph, 0.0)
        g = 2.0 / (1.0 + np.exp(-(h @ Wo + bo)))
        pre_h.append(ph), hact.append(act), hgs.append(h), gs.append(g), parts.append(g * xs)
    z, a, pre_y = np.zeros((B, Z)), np.zeros((B, Z)), np.zeros((B, Z))
    stats, yact = np.zeros((2, Z)), np.zeros((B, Z), bool)
    new_mm, new_mv = [m.copy() for m in mm], [v.copy() for v in mv]
    keep = {}
    m = []
    for s in range(2):
        cur = parts[s]
        for l in range(L):
            W, b, gamma, beta = stream[4 * (s * L + l):4 * (s * L + l) + 4]
            c0, w = zc[(s, l)], ws[s][l]
            zl = cur @ W + b
            if training:
                mean, var = zl.mean(0), zl.var(0)
                new_mm[s * L + l] = mm[s * L + l] * MOMENTUM + mean * (1 - MOMENTUM)
                new_mv[s * L + l] = mv[s * L + l] * MOMENTUM + var * (1 - MOMENTUM)
            else:
                mean, var = mm[s * L + l], mv[s * L + l]
            rstd = 1.0 / np.sqrt(var + EPS)
            xhat = (zl - mean) * rstd
            y = xhat * gamma + beta
            act = _branch(y, None if pin is None else pin["y"][:, c0:c0 + w])
            al = np.where(act, y, 0.0)
            z[:, c0:c0 + w], a[:, c0:c0 + w], pre_y[:, c0:c0 + w], yact[:, c0:c0 + w] = zl, al, y, act
            stats[0, c0:c0 + w], stats[1, c0:c0 + w] = mean, rstd
            keep[(s, l)] = (cur, xhat, rstd)
            cur = al
        m.append(cur)
    W_1, c_1, W_2, c_2, W_12 = head
    o = W_1.shape[1]
    h1, h2 = W_12.shape[1], W_12.shape[2]
    m1h, m2h = m[0].reshape(B, n, h1), m[1].reshape(B, n, h2)
    logit = m[0] @ W_1 + c_1 + m[1] @ W_2 + c_2 + np.einsum("bnx,nxyo,bny->bo", m1h, W_12, m2h)
    out = 1.0 / (1.0 + np.exp(-logit))
    res = dict(out=out, hg=np.concatenate(hgs, 1), g=np.concatenate(gs, 1), z=z, a=a, stats=stats,
               pre_h=np.concatenate(pre_h, 1), pre_y=pre_y, moving=new_mm + new_mv)
    if dout is None:
        return res
    dl = np.asarray(dout, np.float64) * out * (1 - out)
    dhead = [m[0].T @ dl, dl.sum(0), m[1].T @ dl, dl.sum(0), np.einsum("bnx,bny,bo->nxyo", m1h, m2h, dl)]
    dm = [dl @ W_1.T + np.einsum("bo,nxyo,bny->bnx", dl, W_12, m2h).reshape(B, -1),
          dl @ W_2.T + np.einsum("bo,nxyo,bnx->bny", dl, W_12, m1h).reshape(B, -1)]
    dstream, dgate, dxs, dxg = [None] * (8 * L), [None] * 8, np.zeros_like(xs), []
    bias_scale = {}                                          # sum_b |dz| of the biases whose gradient is identically 0
    for s in range(2):
        da = dm[s]
        for l in reversed(range(L)):
            W, b, gamma, beta = stream[4 * (s * L + l):4 * (s * L + l) + 4]
            c0, w = zc[(s, l)], ws[s][l]
            inp, xhat, rstd = keep[(s, l)]
            dy = da * yact[:, c0:c0 + w]
            dgamma, dbeta = (dy * xhat).sum(0), dy.sum(0)
            if training:                                     # the full backward across the batch
                dz = gamma * rstd * (dy - dy.mean(0) - xhat * (dy * xhat).mean(0))
                db = np.zeros(w)                             # sum_b dz = 0 identically
                bias_scale["b_%d_%d" % (s + 1, l)] = np.abs(dz).sum(0).max()
            else:
                dz = gamma * rstd * dy
                db = dz.sum(0)
            dstream[4 * (s * L + l):4 * (s * L + l) + 4] = [inp.T @ dz, db, dgamma, dbeta]
            da = dz @ W.T
        Wh, bh, Wo, bo = gate[4 * s:4 * s + 4]
        g = gs[s]
        dxs += da * g
        dpre = (da * xs) * (g * (1 - g / 2))
        dh = (dpre @ Wo.T) * hact[s]
        dgate[4 * s:4 * s + 4] = [xg[s].T @ dh, dh.sum(0), hgs[s].T @ dpre, dpre.sum(0)]
        dxg.append(dh @ Wh.T)
    res.update(dxs=dxs, dx1=dxg[0], dx2=dxg[1], dparams=dgate + dstream + dhead, bias_scale=bias_scale)
    return res


# ---- torch, the reference's op order --------------------------------------------------------------------------------
def _relu_pinned(y, near, pin):
    """relu with the near-kink entries on the pinned branch (near, pin: boolean arrays or None)"""
    if near is None:
        return torch.relu(y)
    act = torch.where(torch.from_numpy(near), torch.from_numpy(pin), y > 0)
    return torch.where(act, y, torch.zeros_like(y))


def body_torch(xs, x1, x2, params, moving, w1, w2, n, training, saved=None, near=None, pin=None):
    """tensors -> out [B, o]: Dense, BatchNormalization, Activation per unit, as make_mlp_layer strings them.  ``saved``
    receives the intermediates under the names of SAVED and the moved statistics under 'moving'; ``near`` / ``pin``:
    dict(h=, y=) of numpy boolean arrays (the near-kink entries of the fp64 reading and their branch)."""
    L, ws, xg = len(w1), (list(w1), list(w2)), (x1, x2)
    zc, Z = _zcols(w1, w2)
    gate, stream, head = params[:8], params[8:8 + 8 * L], params[8 + 8 * L:]
    hgs, gs, m, zs, as_, mean_, rstd_ = [], [], [], {}, {}, {}, {}
    new_mm, new_mv = list(moving[:2 * L]), list(moving[2 * L:])
    hoff = [0, gate[0].shape[1]]
    for s in range(2):
        Wh, bh, Wo, bo = gate[4 * s:4 * s + 4]
        sl = slice(hoff[s], hoff[s] + Wh.shape[1])
        h = _relu_pinned(xg[s] @ Wh + bh, None if near is None else near["h"][:, sl], None if pin is None else pin["h"][:, sl])
        g = torch.sigmoid(h @ Wo + bo) * 2
        hgs.append(h), gs.append(g)
        cur = g * xs
        for l in range(L):
            W, b, gamma, beta = stream[4 * (s * L + l):4 * (s * L + l) + 4]
            c0, w = zc[(s, l)], ws[s][l]
            zl = cur @ W + b
            if training:
                mean = zl.mean(0)
                var = ((zl - mean) ** 2).mean(0)
                new_mm[s * L + l] = moving[s * L + l] * MOMENTUM + mean * (1 - MOMENTUM)
                new_mv[s * L + l] = moving[2 * L + s * L + l] * MOMENTUM + var * (1 - MOMENTUM)
            else:
                mean, var = moving[s * L + l], moving[2 * L + s * L + l]
            rstd = 1.0 / torch.sqrt(var + EPS)
            y = (zl - mean) * rstd * gamma + beta
            ysl = slice(c0, c0 + w)
            cur = _relu_pinned(y, None if near is None else near["y"][:, ysl], None if pin is None else pin["y"][:, ysl])
            zs[(s, l)], as_[(s, l)], mean_[(s, l)], rstd_[(s, l)] = zl, cur, mean, rstd
        m.append(cur)
    W_1, c_1, W_2, c_2, W_12 = head
    B, h1, h2 = xs.shape[0], W_12.shape[1], W_12.shape[2]
    t = torch.einsum("bnx,nxyo->bnyo", m[0].reshape(B, n, h1), W_12)
    t = torch.einsum("bnyo,bny->bno", t, m[1].reshape(B, n, h2)).sum(1)
    out = torch.sigmoid((m[0] @ W_1 + c_1) + (m[1] @ W_2 + c_2) + t)
    if saved is not None:
        order = [(s, l) for l in range(L) for s in range(2)]
        cat = lambda d: torch.cat([d[k] for k in order], dim=-1)
        saved.update(hg=torch.cat(hgs, 1), g=torch.cat(gs, 1), z=cat(zs), a=cat(as_),
                     stats=torch.stack([cat(mean_), cat(rstd_)]), moving=new_mm + new_mv)
    return out


def body_torch_grads(xs, x1, x2, params, moving, w1, w2, n, training, dout, dtype, near=None, pin=None):
    """-> (out, (dxs, dx1, dx2), dparams, saved) as fp64 numpy, computed in ``dtype`` on the CPU"""
    xt = [_t(a, dtype, True) for a in (xs, x1, x2)]
    pt = [_t(a, dtype, True) for a in params]
    mt = [_t(a, dtype) for a in moving]
    saved = {}
    out = body_torch(*xt, pt, mt, w1, w2, n, training, saved, near, pin)
    out.backward(_t(dout, dtype))
    n64 = lambda t: t.detach().double().numpy()
    sv = {k: ([n64(a) for a in v] if k == "moving" else n64(v)) for k, v in saved.items()}
    return n64(out), [n64(a.grad) for a in xt], [n64(a.grad) for a in pt], sv


def layer_torch_grads(tables, X_user, X_item, params, moving, w1, w2, n, training, gout, dtype, near=None, pin=None):
    """The whole layer: the three lookups (shared rows of [user | item] ids, gate 1 from the item ids through tables[1],
    gate 2 from the user ids through tables[2]), flatten, body -> (out, dtables, dparams, moving) as fp64 numpy"""
    tt = [_t(a, dtype, True) for a in tables]
    pt = [_t(a, dtype, True) for a in params]
    mt = [_t(a, dtype) for a in moving]
    Xu, Xi = torch.from_numpy(np.asarray(X_user, np.int64)), torch.from_numpy(np.asarray(X_item, np.int64))
    saved = {}
    out = body_torch(tt[0][torch.cat([Xu, Xi], 1)].flatten(1), tt[1][Xi].flatten(1), tt[2][Xu].flatten(1), pt, mt, w1, w2,
                     n, training, saved, near, pin)
    out.backward(_t(gout, dtype))
    n64 = lambda t: t.detach().double().numpy()
    return n64(out), [n64(a.grad) for a in tt], [n64(a.grad) for a in pt], [n64(a) for a in saved["moving"]]


def state_dict_of(tables, params, moving, L):
    """arrays -> {state-dict name of FinalMLPLayer: array}; ``moving`` may be None (parameters only)"""
    out = {"shared_embedding.embeddings": tables[0], "fs_layer.fs1_embedding.embeddings": tables[1],
           "fs_layer.fs2_embedding.embeddings": tables[2]}
    for s in range(2):
        Wh, bh, Wo, bo = params[4 * s:4 * s + 4]
        pre = "fs_layer.mlp_gate%d_" % (s + 1)
        out.update({pre + "hidden.layers.0.kernel": Wh, pre + "hidden.layers.0.bias": bh,
                    pre + "output.layers.0.kernel": Wo, pre + "output.layers.0.bias": bo})
        for l in range(L):
            W, b, gamma, beta = params[8 + 4 * (s * L + l):8 + 4 * (s * L + l) + 4]
            pre = "mlp%d.layers." % (s + 1)
            out.update({pre + "%d.kernel" % (3 * l): W, pre + "%d.bias" % (3 * l): b, pre + "%d.gamma" % (3 * l + 1): gamma,
                        pre + "%d.beta" % (3 * l + 1): beta})
            if moving is not None:
                out.update({pre + "%d.moving_mean" % (3 * l + 1): moving[s * L + l],
                            pre + "%d.moving_variance" % (3 * l + 1): moving[2 * L + s * L + l]})
    W_1, c_1, W_2, c_2, W_12 = params[8 + 8 * L:]
    out.update({"interaction_layer.W_1.kernel": W_1, "interaction_layer.W_1.bias": c_1,
                "interaction_layer.W_2.kernel": W_2, "interaction_layer.W_2.bias": c_2, "interaction_layer.W_12": W_12})
    return out


# ---- the cases of the host and GPU tests ----------------------------------------------------------------------------
def _gen(case, seed, special=False):
    B, dims = case[0], case[1:]
    D, D1, D2 = dims[:3]
    r = np.random.default_rng(seed)
    params, moving = make_body(r, *dims)
    if special:          # stream 1, layer 0: a constant column, and one whose mean is far above its spread
        names = [nm for nm, _ in shapes(*dims)]
        W, b, beta = (params[names.index(k)] for k in ("W_1_0", "b_1_0", "beta_1_0"))
        W[:, CONST_COL] = 0.0
        b[BIG_COL] = BIG_BIAS
        beta[BIG_COL] = BIG_BETA     # that column's relu stays open: the case is about the statistic, not about kinks
    params, moving = [f32_exact(p) for p in params], [f32_exact(p) for p in moving]
    xs, x1, x2 = (f32_exact(r.normal(0, 1, (B, d))) for d in (D, D1, D2))
    return r, params, moving, xs, x1, x2


def near_of(ref):
    return dict(h=np.abs(ref["pre_h"]) < PRE_EPS, y=np.abs(ref["pre_y"]) < PRE_EPS)


@functools.lru_cache(maxsize=None)
def body_case(case, training=True, special=False):
    """-> dict(params, moving, xs, x1, x2, dout, near, seed, ...): fp32-exact inputs and the near-kink entries of the fp64
    reading.  Under 100 examples the first seed 1, 2, 3, ... without a near-kink entry, on the fp64 reading alone."""
    B, w1, w2, n, o = case[0], case[6], case[7], case[8], case[9]

    def near(seed):
        _, params, moving, xs, x1, x2 = _gen(case, seed, special)
        return near_of(body_numpy(xs, x1, x2, params, moving, w1, w2, n, training))

    seed = clean_seed(lambda s: any(v.any() for v in near(s).values())) if B < 100 else 1
    r, params, moving, xs, x1, x2 = _gen(case, seed, special)
    return dict(params=params, moving=moving, xs=xs, x1=x1, x2=x2, dout=f32_exact(r.uniform(-1, 1, (B, o))),
                near=near(seed), seed=seed, w1=w1, w2=w2, n=n, training=training)


def case_ref(c, pin=None):
    """the fp64 reading of a body_case, with the near-kink entries on the branches of ``pin``"""
    return body_numpy(c["xs"], c["x1"], c["x2"], c["params"], c["moving"], c["w1"], c["w2"], c["n"], c["training"],
                      c["dout"], pin)


def case_t32(c, pin=None):
    """the fp32 CPU transcription on the same inputs: (out, (dxs, dx1, dx2), dparams, saved)"""
    return body_torch_grads(c["xs"], c["x1"], c["x2"], c["params"], c["moving"], c["w1"], c["w2"], c["n"], c["training"],
                            c["dout"], torch.float32, c["near"] if pin is not None else None, pin)


def pinned_share(c):
    """the share of a case's relu entries that lie within PRE_EPS of the kink on the fp64 reading"""
    n = sum(int(v.sum()) for v in c["near"].values())
    return n / sum(v.size for v in c["near"].values())
