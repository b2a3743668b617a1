"""Reference readings of the CAN co-action (csrc/can.hip, layers.CoActionUnit), written from the formulas of
include/mi355rec.h: an fp64 numpy forward with a hand-derived backward, a torch-CPU transcription of the reference layer
(7.SIM/CustomLayers.py:285-378, read line by line) whose gradients come from autograd (fp32: the error floor of the
tolerance; fp64: the check of the hand-derived backward), and the generators of the test cases.

Generators: feed table ~ N(0, 0.5), induction tables ~ N(0, 1 / sqrt(E)), upstream gradients ~ U(-1, 1), every value
fp32-exact; V = 97, so ids repeat.  The first four examples have 0, 1, 2 and T padded positions (at most T), padding sits
anywhere; the others have a random number of them.  T = 0 in a case means the 1-D feed [B].

relu has a kink: a pre-activation that is near zero in fp64 may take the other branch in fp32.  The relu generator
re-draws the feed id of every position that takes part (its id is not the padding id: a padded position is zeroed after
the MLP and contributes to no output and no gradient) and has a pre-activation with |z| < KINK_EPS in fp64, at any order
and any layer; the induction id stays.  At most KINK_ROUNDS rounds, then it asserts that none is left: nothing is ever
left out of a comparison."""
import functools

import numpy as np
import torch

from tests.masknet_ref import rel_err  # noqa: F401

V_CASE = 97
PAD = 0
KINK_EPS, KINK_ROUNDS = 1e-4, 20
ACTS = ("tanh", "relu", "sigmoid", "linear")

# (B, T, E, coefs, order); T = 0: the 1-D feed
CASES = [(1, 1, 1, (1,), 1), (3, 5, 4, (1, 1, 1), 3), (33, 6, 16, (1, 1, 1), 3), (33, 50, 16, (1, 1, 1), 3),
         (33, 65, 8, (2, 1), 3), (17, 33, 16, (1, 1, 1), 1), (17, 6, 16, (1, 1, 1), 2), (5, 9, 32, (1, 1, 1), 3),
         (5, 9, 16, (2, 2, 1), 3), (5, 3, 64, (1, 1), 2), (2049, 10, 16, (1, 1, 1), 3), (33, 0, 16, (1, 1, 1), 3)]
EXTRA_CASES = [(7, 7, 6, (3, 2), 2), (9, 5, 3, (1, 5, 7), 4)]   # widths that are no powers of two; four orders
OTHER_ACT_CASES = [CASES[2], CASES[4], CASES[9]]            # cases 3, 5 and 10 of the list, with relu, sigmoid and linear
LAYER_CASES = [CASES[2], CASES[3], CASES[11]]               # cases 3, 4 and 12


def case_id(c):
    return "%dx%dx%dx%sx%d" % (c[0], c[1], c[2], "-".join(map(str, c[3])), c[4])


def f32_exact(a):
    return np.asarray(a, np.float32).astype(np.float64)


def widths(E, coefs):
    return [E] + [E * c for c in coefs]


def row_floats(E, coefs):
    w = widths(E, coefs)
    return sum(a * b + b for a, b in zip(w[:-1], w[1:]))


def layer_slices(E, coefs):
    """[(W start, W end = B start, B end, (w_in, w_out))] of every layer in an induction row"""
    w, at, out = widths(E, coefs), 0, []
    for a, b in zip(w[:-1], w[1:]):
        out.append((at, at + a * b, at + a * b + b, (a, b)))
        at += a * b + b
    return out


def rows(table, ids):
    """table[ids]; an id outside the table is a zero row"""
    V = table.shape[0]
    ok = (ids >= 0) & (ids < V)
    return np.where(ok[..., None], table[np.clip(ids, 0, V - 1)], 0.0)


def _act(name, z):
    if name == "tanh":
        return np.tanh(z)
    if name == "relu":
        return np.maximum(z, 0.0)
    if name == "sigmoid":
        return 1.0 / (1.0 + np.exp(-z))
    assert name in ("linear", None)
    return z


def _dact(name, z, y):
    if name == "tanh":
        return 1.0 - y * y
    if name == "relu":
        return (z > 0).astype(np.float64)
    if name == "sigmoid":
        return y * (1.0 - y)
    return np.ones_like(z)


def can_numpy(feed, inds, iid, fid, coefs, order, act, pad=PAD, gout=None, gpool=None):
    """fp64.  feed [Vf,E]; inds: `order` tables [Vi,P], or one that every order reads; iid [B]; fid [B,T].
    -> out [order,B,T,Eo], pool [B,Eo], zmin [B,T] (the smallest |pre-activation| of a position over orders and layers)
    and, with gout [order,B,T,Eo] or gpool [B,Eo], gfeed [B,T,E] and gind [order,B,P]."""
    E = feed.shape[1]
    La = min(len(coefs), order)
    sl = layer_slices(E, coefs)
    f = rows(feed, fid)                                               # [B,T,E]
    padded = (fid == pad)[..., None]
    B, T = fid.shape
    P = row_floats(E, coefs)
    outs, saved = [], []
    zmin = np.full((B, T), np.inf)
    for o in range(1, order + 1):
        v = rows(inds[0 if len(inds) == 1 else o - 1], iid)           # [B,P]
        x, xs, zs, Ws = f ** o, [], [], []
        for l in range(La):
            w0, w1, b1, shape = sl[l]
            W, Bv = v[:, w0:w1].reshape((B,) + shape), v[:, w1:b1]
            z = np.einsum("bti,bij->btj", x, W) + Bv[:, None, :]
            xs.append(x)
            zs.append(z)
            Ws.append(W)
            zmin = np.minimum(zmin, np.abs(z).min(-1))
            x = _act(act, z)
        outs.append(np.where(padded, 0.0, x))
        saved.append((xs, zs, Ws, x))
    out = np.stack(outs)
    res = dict(out=out, pool=out.sum((0, 2)), zmin=zmin)
    if gout is None and gpool is None:
        return res
    gfeed, gind = np.zeros((B, T, E)), np.zeros((order, B, P))
    for o in range(1, order + 1):
        xs, zs, Ws, y = saved[o - 1]
        g = gout[o - 1] if gout is not None else np.broadcast_to(gpool[:, None, :], y.shape)
        g = np.where(padded, 0.0, g)
        for l in range(La - 1, -1, -1):
            w0, w1, b1, _ = sl[l]
            dz = g * _dact(act, zs[l], y)
            gind[o - 1, :, w0:w1] = np.einsum("bti,btj->bij", xs[l], dz).reshape(B, -1)
            gind[o - 1, :, w1:b1] = dz.sum(1)
            g = np.einsum("btj,bij->bti", dz, Ws[l])
            y = xs[l]                                                 # the output of layer l - 1
        gfeed += g * (o * f ** (o - 1) if o > 1 else 1.0)
    res.update(gfeed=gfeed, gind=gind)
    return res


# ---- the torch-CPU transcription -------------------------------------------------------------------------------------
_T_ACT = {"tanh": torch.tanh, "relu": torch.relu, "sigmoid": torch.sigmoid, "linear": lambda x: x, None: lambda x: x}


class CoActionUnitTorch:
    """CoActionUnit of 7.SIM/CustomLayers.py:285-378 line by line; the two Embedding calls of basic_call are the two
    arguments feed_rows (= self.feed_embedding(feed_feature)) and induction_vector (= embedding(induction_feature)), so
    that a caller can make either the looked-up rows or the tables the leaves of the graph."""

    def __init__(self, feed_feature_dim=16, layer_unit_coef=None, order=3, activation="tanh", padding_index=0):
        if layer_unit_coef is None:
            layer_unit_coef = [1, 1, 1]
        layer_unit_coef = list(layer_unit_coef)
        num_layers = len(layer_unit_coef)
        self.W_indexes, self.B_indexes, self.W_shapes = [], [], []
        start = 0
        base = feed_feature_dim ** 2
        all_coefs = [1] + layer_unit_coef
        for i in range(num_layers):
            start_coef, end_coef = all_coefs[i], all_coefs[i + 1]
            self.W_shapes.append((-1, feed_feature_dim * start_coef, feed_feature_dim * end_coef))
            W_params = base * start_coef * end_coef
            B_params = feed_feature_dim * end_coef
            self.W_indexes.append([start, start + W_params])
            self.B_indexes.append([start + W_params, start + W_params + B_params])
            start = start + W_params + B_params
        self.induction_feature_dim = start
        self.activation = [_T_ACT[activation] for _ in range(order)]
        self.order = order
        self.padding_index = padding_index

    def basic_call(self, induction_vector, feed_feature, feed_rows, order):
        feed_mask = feed_feature == self.padding_index
        feed_vector = feed_rows ** order
        W_matrixes = [induction_vector[:, start:end] for start, end in self.W_indexes]
        B_matrixes = [induction_vector[:, start:end] for start, end in self.B_indexes]
        rank = feed_vector.dim()
        for W, B, W_shape, activation in zip(W_matrixes, B_matrixes, self.W_shapes, self.activation):
            W = W.reshape(W_shape)
            if rank == 2:
                feed_vector = feed_vector.unsqueeze(1)
                feed_vector = torch.matmul(feed_vector, W).squeeze(1) + B
            elif rank == 3:
                B = B.unsqueeze(1)
                feed_vector = torch.matmul(feed_vector, W) + B
            else:
                raise ValueError("feed_vector维度必须是2维或者3维")
            feed_vector = activation(feed_vector)
        feed_mask = feed_mask.unsqueeze(-1)
        return torch.where(feed_mask, torch.zeros((), dtype=feed_vector.dtype), feed_vector)

    def call(self, induction_vectors, feed_feature, feed_rows):
        """induction_vectors: the looked-up row of every order (the same tensor `order` times for a shared table)"""
        return [self.basic_call(v, feed_feature, feed_rows, i + 1) for i, v in enumerate(induction_vectors)]


def can_torch_grads(feed, inds, iid, fid, coefs, order, act, dtype, pad=PAD, gout=None, gpool=None):
    """The transcription with the looked-up rows as leaves -> out, pool and, with an upstream gradient, gfeed and gind in
    the layout of can_numpy.  fid [B,T] or [B]."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    E = feed.shape[1]
    unit = CoActionUnitTorch(E, list(coefs), order, act, pad)
    x = t(rows(feed, fid)).requires_grad_()
    vs = [t(rows(inds[0 if len(inds) == 1 else o], iid)).requires_grad_() for o in range(order)]
    outs = unit.call(vs, torch.from_numpy(np.asarray(fid)), x)
    out = torch.stack(outs)
    pool = out.sum((0, 2)) if out.dim() == 4 else out.sum(0)
    res = dict(out=out.detach().numpy(), pool=pool.detach().numpy())
    if gout is not None or gpool is not None:
        ((out * t(gout)).sum() if gout is not None else (pool * t(gpool)).sum()).backward()
        res.update(gfeed=x.grad.numpy(), gind=np.stack([v.grad.numpy() for v in vs]))
    return res


# ---- cases -------------------------------------------------------------------------------------------------------------
def feed_ids(r, B, T, V, pad=PAD):
    """[B,T]: the first four examples have 0, 1, 2 and T padded positions, the others a random number; anywhere"""
    n_pad = r.integers(0, T + 1, B)
    n_pad[:4] = np.minimum([0, 1, 2, T], T)[:B]
    ids = r.integers(1, V, (B, T))
    for b in range(B):
        ids[b, r.permutation(T)[:n_pad[b]]] = pad
    return ids.astype(np.int64)


def near_kink(c, act):
    """[B,T] bool: the positions that take part and have a pre-activation within KINK_EPS of zero in fp64"""
    ref = can_numpy(c["feed"], c["inds"], c["iid"], c["fid"], c["coefs"], c["order"], act)
    return (ref["zmin"] < KINK_EPS) & (c["fid"] != PAD)


@functools.lru_cache(maxsize=None)
def can_case(case, act="tanh", shared=False):
    """The inputs of a case (fid always [B,T]; `flat` says that the case means the 1-D feed [B]) and how many positions
    the relu generator still finds near the kink (`kink_left`: asserted zero without a GPU)."""
    B, T, E, coefs, order = case
    flat, T = T == 0, max(T, 1)
    r = np.random.default_rng(7)
    P = row_floats(E, coefs)
    Eo = widths(E, coefs)[min(len(coefs), order)]
    c = dict(feed=f32_exact(r.normal(0, 0.5, (V_CASE, E))),
             inds=[f32_exact(r.normal(0, 1 / np.sqrt(E), (V_CASE, P))) for _ in range(1 if shared else order)],
             iid=r.integers(0, V_CASE, B).astype(np.int64), fid=feed_ids(r, B, T, V_CASE),
             gout=f32_exact(r.uniform(-1, 1, (order, B, T, Eo))), gpool=f32_exact(r.uniform(-1, 1, (B, Eo))),
             coefs=coefs, order=order, flat=flat, P=P, Eo=Eo, kink_left=0, redrawn=0)
    if act == "relu":
        for _ in range(KINK_ROUNDS):
            near = near_kink(c, act)
            if not near.any():
                break
            c["redrawn"] += int(near.sum())
            c["fid"][near] = r.integers(1, V_CASE, int(near.sum()))
        c["kink_left"] = int(near_kink(c, act).sum())
    return c


@functools.lru_cache(maxsize=None)
def can_ref(case, act="tanh", shared=False):
    c = can_case(case, act, shared)
    return can_numpy(c["feed"], c["inds"], c["iid"], c["fid"], c["coefs"], c["order"], act, PAD, c["gout"]), \
        can_numpy(c["feed"], c["inds"], c["iid"], c["fid"], c["coefs"], c["order"], act, PAD, None, c["gpool"])


@functools.lru_cache(maxsize=None)
def can_case_t(case, act, dtype, shared=False):
    """(unpooled, pooled) results of the transcription in `dtype`"""
    c = can_case(case, act, shared)
    args = (c["feed"], c["inds"], c["iid"], c["fid"], c["coefs"], c["order"], act, dtype, PAD)
    return can_torch_grads(*args, gout=c["gout"]), can_torch_grads(*args, gpool=c["gpool"])


def dense_grad(V, ids, vals):
    """IndexedSlices values -> the dense gradient of a table with V rows"""
    vals = np.asarray(vals, np.float64)
    g = np.zeros((V, vals.shape[-1]))
    np.add.at(g, np.asarray(ids).reshape(-1), vals.reshape(-1, vals.shape[-1]))
    return g


# ---- the layer ---------------------------------------------------------------------------------------------------------
def layer_state(case, order_independent=True, seed=3):
    """state dict of layers.CoActionUnit for a case: Keras' uniform(-0.05, 0.05) would give outputs near zero, so the
    tables are the body generators' (as loaded weights would be)"""
    B, T, E, coefs, order = case
    r = np.random.default_rng(seed)
    sd = {"feed_embedding.embeddings": f32_exact(r.normal(0, 0.5, (V_CASE, E)))}
    for i in range(order if order_independent else 1):
        sd["induction_embedding.%d.embeddings" % i] = f32_exact(r.normal(0, 1 / np.sqrt(E),
                                                                         (V_CASE, row_floats(E, coefs))))
    return sd


def layer_inputs(case, seed=3, same_item=False):
    """(induction_feature [B,1] -- the shape a Model's input dict delivers --, feed_feature [B,T] or [B])"""
    B, T, E, coefs, order = case
    r = np.random.default_rng(100 + seed)
    iid = r.integers(0, V_CASE, (B, 1)).astype(np.int64)
    if same_item:
        iid[:] = 5
    fid = feed_ids(r, B, max(T, 1), V_CASE)
    return iid, (fid[:, 0].copy() if T == 0 else fid)


def layer_upstream(case, seed=3):
    B, T, E, coefs, order = case
    r = np.random.default_rng(200 + seed)
    Eo = widths(E, coefs)[min(len(coefs), order)]
    shape = (B, Eo) if T == 0 else (B, T, Eo)
    return [f32_exact(r.uniform(-1, 1, shape)) for _ in range(order)], f32_exact(r.uniform(-1, 1, (B, Eo)))


def layer_torch(sd, case, inputs, dtype, gouts=None, gpool=None, activation="tanh", order_independent=True):
    """The transcription with the TABLES as leaves (torch's own embedding lookup) -> outputs (the list), pooled and, with
    an upstream gradient for the list or for pooled, grads {state-dict key: dense gradient}."""
    B, T, E, coefs, order = case
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    p = {k: t(v).requires_grad_() for k, v in sd.items()}
    iid, fid = (torch.from_numpy(np.asarray(a)) for a in inputs)
    unit = CoActionUnitTorch(E, list(coefs), order, activation, PAD)
    if iid.dim() == 2 and iid.shape[1] == 1:
        iid = iid.squeeze(1)
    tables = [p["induction_embedding.%d.embeddings" % (i if order_independent else 0)] for i in range(order)]
    outs = unit.call([tab[iid] for tab in tables], fid, p["feed_embedding.embeddings"][fid])
    pooled = sum(o.sum(1) if o.dim() == 3 else o for o in outs)
    res = dict(outputs=[o.detach().numpy() for o in outs], pooled=pooled.detach().numpy())
    if gouts is not None or gpool is not None:
        loss = sum((o * t(g)).sum() for o, g in zip(outs, gouts)) if gouts is not None else (pooled * t(gpool)).sum()
        loss.backward()
        res["grads"] = {k: v.grad.numpy() for k, v in p.items()}
    return res
