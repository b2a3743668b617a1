"""Restatements of MMOELayer / ESMMLayer (4.MMOE/CustomLayers.py:107-245) for the tests: an fp64 numpy reading of the body
with hand-written gradients, a torch transcription in the reference's op order (one MLP per expert, gate and tower, a
softmax per gate, stack, multiply, flatten) that autograd differentiates, runnable in fp32 and fp64 on the CPU, the whole
layer with its lookup, and the cases the host and GPU tests share.

The body's parameters are the packed list of include/mi355rec.h:
  [W1 [D, (n+T) H1], b1, We2 [n, H1, O], be2 [n, O], Wg2 [T, H1, n], bg2 [T, n], Wt1 [T, n O, H2], bt1 [T, H2],
   Wt2 [T, H2, O2], bt2 [T, O2], Wt3 [T, O2], bt3 [T]]
column block i < n of W1 being expert i's first kernel and block n + t gate t's.  Scale as in tests/masknet_ref.py:
glorot-uniform kernels (each sub-layer's own fan-in / fan-out), every bias N(0, 0.1^2) -- the gates' too, so that not
every gate is the uniform one -- inputs N(0, 1), tables N(0, 0.5^2).  ``pre`` is, per example, the smallest |relu
pre-activation| over h, e, z, a1 and a2."""
import functools

import numpy as np
import torch

from tests.masknet_ref import PRE_EPS, _t, clean_seed, glorot, rel_err  # noqa: F401

NAMES = ["W1", "b1", "We2", "be2", "Wg2", "bg2", "Wt1", "bt1", "Wt2", "bt2", "Wt3", "bt3"]
SAVED = ["h", "e", "z", "g", "a1", "a2", "p"]
TASKS = ("ctr", "cvr")

# (B, D, n, T, H1, O, H2, O2, gate_softmax_passes, ctcvr)
BODY_CASES = [(1, 1, 1, 1, 1, 1, 1, 1, 1, 0), (2, 15, 3, 2, 5, 3, 7, 2, 1, 0), (33, 144, 3, 2, 64, 8, 64, 8, 1, 0),
              (33, 144, 3, 2, 64, 8, 64, 8, 2, 1), (17, 144, 1, 2, 64, 8, 64, 8, 1, 0), (17, 64, 4, 4, 64, 8, 32, 4, 1, 0),
              (17, 512, 2, 1, 32, 16, 128, 8, 1, 0), (2049, 144, 3, 2, 64, 8, 64, 8, 1, 0),
              (2049, 144, 3, 2, 64, 8, 64, 8, 2, 1),
              # the slice edges of the small weight-gradient launch (csrc/tile_ops.h), at the smallest non-trivial widths:
              # B = 513 two slices of unequal length, B = 4097 sixteen of 288 examples, the last one empty
              (513, 15, 3, 2, 5, 3, 7, 2, 1, 0), (4097, 15, 3, 2, 5, 3, 7, 2, 1, 0), (4097, 15, 3, 2, 5, 3, 7, 2, 2, 1)]


def f32_exact(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def make_body(r, D, n, T, H1, O, H2, O2):
    b = lambda *s: r.normal(0, 0.1, s)
    W1 = np.concatenate([glorot(r, D, H1) for _ in range(n + T)], axis=1)
    We2 = np.stack([glorot(r, H1, O) for _ in range(n)])
    Wg2 = np.stack([glorot(r, H1, n) for _ in range(T)])
    Wt1 = np.stack([glorot(r, n * O, H2) for _ in range(T)])
    Wt2 = np.stack([glorot(r, H2, O2) for _ in range(T)])
    Wt3 = np.stack([glorot(r, O2, 1).reshape(-1) for _ in range(T)])
    return [W1, b(W1.shape[1]), We2, b(n, O), Wg2, b(T, n), Wt1, b(T, H2), Wt2, b(T, O2), Wt3, b(T)]


def _softmax(z):
    ex = np.exp(z - z.max(-1, keepdims=True))
    return ex / ex.sum(-1, keepdims=True)


# ---- numpy, fp64 ----------------------------------------------------------------------------------------------------
def body_numpy(x, params, passes=1, ctcvr=0, dout=None):
    """x [B, D] -> out [B, T], the save buffers and pre; with dout also dx and dparams (order of params)."""
    W1, b1, We2, be2, Wg2, bg2, Wt1, bt1, Wt2, bt2, Wt3, bt3 = [np.asarray(a, np.float64) for a in params]
    x = np.asarray(x, np.float64)
    B = x.shape[0]
    n, H1, O = We2.shape
    T, H2, O2 = Wt2.shape
    ph = x @ W1 + b1
    h = np.maximum(ph, 0)
    hb = h.reshape(B, n + T, H1)
    pe = np.einsum("bik,iko->bio", hb[:, :n], We2) + be2
    e = np.maximum(pe, 0)
    pz = np.einsum("btk,tkj->btj", hb[:, n:], Wg2) + bg2
    z = np.maximum(pz, 0)
    gs = [_softmax(z)]
    for _ in range(passes - 1):
        gs.append(_softmax(gs[-1]))
    g = gs[-1]
    u = (e[:, None, :, :] * g[:, :, :, None]).reshape(B, T, n * O)          # flattened, not summed over the experts
    pa1 = np.einsum("btk,tkc->btc", u, Wt1) + bt1
    a1 = np.maximum(pa1, 0)
    pa2 = np.einsum("btk,tkc->btc", a1, Wt2) + bt2
    a2 = np.maximum(pa2, 0)
    p = 1.0 / (1.0 + np.exp(-(np.einsum("btk,tk->bt", a2, Wt3) + bt3)))
    out = p.copy()
    if ctcvr:
        out[:, 1] = p[:, 0] * p[:, 1]
    pre = np.min([np.abs(a).reshape(B, -1).min(1) for a in (ph, pe, pz, pa1, pa2)], axis=0)
    res = dict(out=out, pre=pre, h=h, e=e.reshape(B, -1), z=z.reshape(B, -1), g=g.reshape(B, -1),
               a1=a1.reshape(B, -1), a2=a2.reshape(B, -1), p=p)
    if dout is None:
        return res
    dout = np.asarray(dout, np.float64)
    dp = dout.copy()
    if ctcvr:
        dp[:, 0] = dout[:, 0] + dout[:, 1] * p[:, 1]
        dp[:, 1] = dout[:, 1] * p[:, 0]
    dl = dp * p * (1 - p)
    dWt3, dbt3 = np.einsum("bt,btk->tk", dl, a2), dl.sum(0)
    da2 = dl[:, :, None] * Wt3[None] * (pa2 > 0)
    dWt2, dbt2 = np.einsum("btk,btc->tkc", a1, da2), da2.sum(0)
    da1 = np.einsum("btc,tkc->btk", da2, Wt2) * (pa1 > 0)
    dWt1, dbt1 = np.einsum("btk,btc->tkc", u, da1), da1.sum(0)
    du = np.einsum("btc,tkc->btk", da1, Wt1).reshape(B, T, n, O)
    de = (du * g[:, :, :, None]).sum(1)
    dg = (du * e[:, None]).sum(3)
    for gk in reversed(gs):
        dg = gk * (dg - (dg * gk).sum(-1, keepdims=True))
    dzz, dze = dg * (pz > 0), de * (pe > 0)
    dWe2, dbe2 = np.einsum("bik,bio->iko", hb[:, :n], dze), dze.sum(0)
    dWg2, dbg2 = np.einsum("btk,btj->tkj", hb[:, n:], dzz), dzz.sum(0)
    dh = np.concatenate([np.einsum("bio,iko->bik", dze, We2), np.einsum("btj,tkj->btk", dzz, Wg2)], axis=1)
    dz1 = dh.reshape(B, -1) * (ph > 0)
    res.update(dx=dz1 @ W1.T,
               dparams=[x.T @ dz1, dz1.sum(0), dWe2, dbe2, dWg2, dbg2, dWt1, dbt1, dWt2, dbt2, dWt3, dbt3])
    return res


# ---- torch, the reference's op order --------------------------------------------------------------------------------
def body_torch(x, params, passes=1, ctcvr=0, saved=None):
    """tensors -> out [B, T]: one MLP per expert, gate and tower, as the reference calls them.  ``saved``: a dict that
    receives the intermediates under the names of SAVED."""
    W1, b1, We2, be2, Wg2, bg2, Wt1, bt1, Wt2, bt2, Wt3, bt3 = params
    n, H1, _ = We2.shape
    T = Wt2.shape[0]
    relu = torch.relu
    hs = [relu(x @ W1[:, i * H1:(i + 1) * H1] + b1[i * H1:(i + 1) * H1]) for i in range(n + T)]
    experts = torch.stack([relu(hs[i] @ We2[i] + be2[i]) for i in range(n)], dim=1)             # [B, n, O]
    zs, gs, a1s, a2s, ps = [], [], [], [], []
    for t in range(T):
        gate = relu(hs[n + t] @ Wg2[t] + bg2[t])                 # MLPLayer: the activation on the last layer too
        zs.append(gate)
        for _ in range(passes):
            gate = torch.softmax(gate, dim=-1)
        gs.append(gate)
        tower_in = (experts * gate.unsqueeze(2)).flatten(1)
        a1s.append(relu(tower_in @ Wt1[t] + bt1[t]))
        a2s.append(relu(a1s[-1] @ Wt2[t] + bt2[t]))
        ps.append(torch.sigmoid(a2s[-1] @ Wt3[t].reshape(-1, 1) + bt3[t]))
    if saved is not None:
        cat = lambda ts: torch.cat(ts, dim=1)
        saved.update(h=cat(hs), e=experts.flatten(1), z=cat(zs), g=cat(gs), a1=cat(a1s), a2=cat(a2s), p=cat(ps))
    outs = list(ps)
    if ctcvr:
        outs[1] = ps[0] * ps[1]
    return torch.cat(outs, dim=1)


def body_torch_grads(x, params, passes, ctcvr, dout, dtype):
    """-> (out, dx, dparams, saved) as fp64 numpy, computed in ``dtype`` on the CPU"""
    xt = _t(x, dtype, True)
    pt = [_t(a, dtype, True) for a in params]
    saved = {}
    out = body_torch(xt, pt, passes, ctcvr, saved)
    out.backward(_t(dout, dtype))
    n64 = lambda t: t.detach().double().numpy()
    return n64(out), n64(xt.grad), [n64(a.grad) for a in pt], {k: n64(v) for k, v in saved.items()}


def layer_torch_grads(table, X, params, passes, ctcvr, gout, dtype):
    """The whole layer: lookup, flatten, body -> (out [B, 2], dtable, dparams) as fp64 numpy"""
    tt = _t(table, dtype, True)
    pt = [_t(a, dtype, True) for a in params]
    Xt = torch.from_numpy(np.asarray(X, np.int64))
    out = body_torch(tt[Xt].flatten(1), pt, passes, ctcvr)
    out.backward(_t(gout, dtype))
    n64 = lambda t: t.detach().double().numpy()
    return n64(out), n64(tt.grad), [n64(a.grad) for a in pt]


def state_dict_of(table, params):
    """packed arrays -> {state-dict name of MMOELayer / ESMMLayer: array}"""
    W1, b1, We2, be2, Wg2, bg2, Wt1, bt1, Wt2, bt2, Wt3, bt3 = params
    n, H1, _ = We2.shape
    out = {"embedding_layer.embeddings": table}
    blk = lambda a, i: a[..., i * H1:(i + 1) * H1]
    for i in range(n):
        pre = "expert_model.%d." % i
        out.update({pre + "kernel_0": blk(W1, i), pre + "bias_0": blk(b1, i), pre + "kernel_1": We2[i],
                    pre + "bias_1": be2[i]})
    for t, task in enumerate(TASKS):
        pre = task + "_gate."
        out.update({pre + "kernel_0": blk(W1, n + t), pre + "bias_0": blk(b1, n + t), pre + "kernel_1": Wg2[t],
                    pre + "bias_1": bg2[t]})
        pre = task + "_output."
        out.update({pre + "0.kernel_0": Wt1[t], pre + "0.bias_0": bt1[t], pre + "0.kernel_1": Wt2[t],
                    pre + "0.bias_1": bt2[t], pre + "1.kernel_0": Wt3[t].reshape(-1, 1), pre + "1.bias_0": bt3[t:t + 1]})
    return out


# ---- the cases of the host and GPU tests ----------------------------------------------------------------------------
def _gen(case, seed):
    B, D, n, T, H1, O, H2, O2 = case[:8]
    r = np.random.default_rng(seed)
    params = [f32_exact(p) for p in make_body(r, D, n, T, H1, O, H2, O2)]
    return r, params, f32_exact(r.normal(0, 1, (B, D)))


@functools.lru_cache(maxsize=None)
def body_case(*case):
    """-> dict(params, x, dout, ref, near, seed): fp32-exact inputs, the fp64 reading, the near-kink examples (their dout
    rows are zero).  Under 100 examples the first seed 1, 2, 3, ... without a near-kink example, on the fp64 reading."""
    B, passes, ctcvr = case[0], case[8], case[9]

    def near_of(s):
        _, params, x = _gen(case, s)
        return body_numpy(x, params, passes, ctcvr)["pre"] < PRE_EPS

    seed = clean_seed(lambda s: near_of(s).any()) if B < 100 else 1
    r, params, x = _gen(case, seed)
    near = near_of(seed)
    dout = f32_exact(r.uniform(-1, 1, (B, case[3])))
    dout[near] = 0.0
    return dict(params=params, x=x, dout=dout, near=near, seed=seed, passes=passes, ctcvr=ctcvr,
                ref=body_numpy(x, params, passes, ctcvr, dout))


@functools.lru_cache(maxsize=None)
def body_case_t32(*case):
    """the fp32 CPU transcription on the inputs of body_case: (out, dx, dparams, saved)"""
    c = body_case(*case)
    return body_torch_grads(c["x"], c["params"], c["passes"], c["ctcvr"], c["dout"], torch.float32)
