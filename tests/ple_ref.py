"""Restatements of PLELayer (4.MMOE/CustomLayers.py:248-384) for the tests: an fp64 numpy reading of one CGC level and of
the whole body with hand-written gradients, a torch transcription in the reference's op order (one MLP per expert and
gate, a softmax dense layer, the second softmax of the task gates, stack, expand_dims, multiply, reduce_sum) that
autograd differentiates, runnable in fp32 and fp64 on the CPU, the whole layer with its lookup, and the cases the host
and GPU tests share.

A level's parameters are the packed list of include/mi355rec.h:
  [W1 [Din, M H1], b1, We2 [ne, H1, O], be2 [ne, O], Wg2 [Gout, H1, Og], bg2 [Gout, Og], Wg3s [T, Og, S + Sh],
   Wg3h [Og, ne] or None (last), Wtw [T, O] or None, btw [T] or None (not last)]
with ne = T S + Sh, Gout = T (last) or T + 1, M = ne + Gout; column block m < ne of W1 is expert m's first kernel
(specific experts task-major, then the shared ones), block ne + g gate g's (task gates, then the shared gate).

Scale: inputs N(0, 1), every kernel N(0, 2 / fan_in), every bias N(0, 0.5^2), incoming gradients U(-1, 1), tables
N(0, 0.5^2).  With glorot-uniform kernels and 0.1 biases the 8-wide inputs of later levels shrink and 10-14 % of 2049
examples sit within 1e-5 of a relu kink at three levels on the fp64 reading alone; these scales give 1.2-3.5 %.
``pre`` is, per example, the smallest |relu pre-activation| over h, e and q."""
import functools

import numpy as np
import torch

from tests.masknet_ref import PRE_EPS, _t, clean_seed, rel_err  # noqa: F401

NAMES = ["W1", "b1", "We2", "be2", "Wg2", "bg2", "Wg3s", "Wg3h", "Wtw", "btw"]
SAVED = ["h", "e", "q", "g"]

# (B, Din, Gin, T, S, Sh, H1, O, Og, last)
LEVEL_CASES = [(1, 1, 1, 1, 1, 1, 1, 1, 1, 1), (2, 15, 1, 2, 2, 1, 5, 3, 2, 0), (33, 72, 1, 3, 3, 3, 64, 8, 8, 0),
               (33, 8, 4, 3, 3, 3, 64, 8, 8, 1), (17, 8, 4, 3, 3, 3, 64, 8, 8, 0), (17, 72, 1, 3, 3, 3, 64, 8, 8, 1),
               (17, 40, 1, 2, 3, 2, 48, 4, 6, 0), (17, 512, 1, 4, 2, 2, 128, 12, 8, 0),
               (2049, 72, 1, 3, 3, 3, 64, 8, 8, 0), (2049, 8, 4, 3, 3, 3, 64, 8, 8, 1),
               # the slice edges of the small weight-gradient launch (csrc/tile_ops.h), at the smallest non-trivial
               # widths, a level before the last and a last one with Gin = T + 1: B = 513 two slices of unequal length,
               # B = 4097 sixteen of 288 examples, the last one empty
               (513, 15, 1, 2, 2, 1, 5, 3, 2, 0), (4097, 15, 1, 2, 2, 1, 5, 3, 2, 0), (513, 3, 3, 2, 2, 1, 5, 3, 2, 1),
               (4097, 3, 3, 2, 2, 1, 5, 3, 2, 1)]
# (B, D, T, S, Sh, L): whole bodies at the reference's widths H1 = 64, O = Og = 8
BODY_CASES = [(33, 72, 3, 3, 3, 1), (33, 72, 3, 3, 3, 2), (33, 72, 3, 3, 3, 3)]
H1_REF, O_REF, OG_REF = 64, 8, 8


def f32_exact(a):
    return None if a is None else np.asarray(a).astype(np.float32).astype(np.float64)


def he(r, a, b):
    return r.normal(0, np.sqrt(2.0 / a), (a, b))


def make_level(r, Din, T, S, Sh, H1, O, Og, last):
    ne, ns, Gout = T * S + Sh, S + Sh, T if last else T + 1
    b = lambda *s: r.normal(0, 0.5, s)
    W1 = np.concatenate([he(r, Din, H1) for _ in range(ne + Gout)], axis=1)
    We2 = np.stack([he(r, H1, O) for _ in range(ne)])
    Wg2 = np.stack([he(r, H1, Og) for _ in range(Gout)])
    Wg3s = np.stack([he(r, Og, ns) for _ in range(T)])
    return [W1, b(W1.shape[1]), We2, b(ne, O), Wg2, b(Gout, Og), Wg3s, None if last else he(r, Og, ne),
            np.stack([he(r, O, 1).reshape(-1) for _ in range(T)]) if last else None, b(T) if last else None]


def make_body(r, D, T, S, Sh, L, H1=H1_REF, O=O_REF, Og=OG_REF):
    return [make_level(r, D if lv == 0 else O, T, S, Sh, H1, O, Og, lv == L - 1) for lv in range(L)]


def groups(T, S, Sh, last):
    """the input group that each of the M first layers reads"""
    ne, Gout = T * S + Sh, T if last else T + 1
    return [m // S if m < T * S else (T if m < ne else m - ne) for m in range(ne + Gout)]


def task_experts(T, S, Sh):
    """[T, S + Sh]: the experts task gate t mixes, its own first, then the shared ones"""
    return np.array([list(range(t * S, (t + 1) * S)) + list(range(T * S, T * S + Sh)) for t in range(T)])


def _softmax(z):
    ex = np.exp(z - z.max(-1, keepdims=True))
    return ex / ex.sum(-1, keepdims=True)


def _softmax_bwd(g, dg):
    return g * (dg - (dg * g).sum(-1, keepdims=True))


# ---- numpy, fp64 ----------------------------------------------------------------------------------------------------
def level_numpy(xin, params, T, S, Sh, last, dy=None, dout=None):
    """xin [B, Gin, Din] -> y [B, Gout, O], out [B, T] (last), the save buffers and pre; with dy and / or dout also dxin
    and dparams (order of params, None where the parameter is None)."""
    W1, b1, We2, be2, Wg2, bg2, Wg3s, Wg3h, Wtw, btw = [None if a is None else np.asarray(a, np.float64) for a in params]
    xin = np.asarray(xin, np.float64)
    B, Gin, Din = xin.shape
    ne, Gout = T * S + Sh, T if last else T + 1
    M = ne + Gout
    H1 = We2.shape[1]
    grp = groups(T, S, Sh, last)
    xg = xin[:, [g if Gin > 1 else 0 for g in grp], :]                        # [B, M, Din]
    W1b = W1.reshape(Din, M, H1)
    ph = np.einsum("bmk,kmj->bmj", xg, W1b) + b1.reshape(M, H1)
    h = np.maximum(ph, 0)
    pe = np.einsum("bik,iko->bio", h[:, :ne], We2) + be2
    e = np.maximum(pe, 0)
    pq = np.einsum("bgk,gko->bgo", h[:, ne:], Wg2) + bg2
    q = np.maximum(pq, 0)
    idx = task_experts(T, S, Sh)
    g1 = _softmax(np.einsum("btk,tkj->btj", q[:, :T], Wg3s))
    g2 = _softmax(g1)                                                         # the softmax applied twice (:304, :341)
    et = e[:, idx]                                                            # [B, T, ns, O]
    ys = [(g2[..., None] * et).sum(2)]                                        # a SUM over the experts (:343)
    gcols = [g2.reshape(B, -1)]
    if not last:
        gh = _softmax(q[:, T] @ Wg3h)                                         # once (:351-353), over all ne experts
        ys.append((gh[..., None] * e).sum(1)[:, None])
        gcols.append(gh)
    y = np.concatenate(ys, axis=1)
    res = dict(y=y, out=None, h=h.reshape(B, -1), e=e.reshape(B, -1), q=q.reshape(B, -1), g=np.concatenate(gcols, 1),
               pre=np.min([np.abs(a).reshape(B, -1).min(1) for a in (ph, pe, pq)], axis=0))
    if last:
        p = 1.0 / (1.0 + np.exp(-(np.einsum("bto,to->bt", y, Wtw) + btw)))
        res["out"] = p
    if dy is None and dout is None:
        return res
    dyt = np.zeros_like(y) if dy is None else np.asarray(dy, np.float64).copy()
    dWtw = dbtw = dWg3h = None
    if last:
        dl = np.asarray(dout, np.float64) * p * (1 - p)
        dWtw, dbtw = np.einsum("bt,bto->to", dl, y), dl.sum(0)
        dyt = dyt + dl[:, :, None] * Wtw[None]
    de = np.zeros_like(e)
    dg2 = (dyt[:, :T, None, :] * et).sum(3)
    for t in range(T):
        de[:, idx[t]] += g2[:, t, :, None] * dyt[:, t, None, :]
    dls = _softmax_bwd(g1, _softmax_bwd(g2, dg2))                             # through both passes
    dWg3s = np.einsum("btk,btj->tkj", q[:, :T], dls)
    dq = np.zeros_like(q)
    dq[:, :T] = np.einsum("btj,tkj->btk", dls, Wg3s)
    if not last:
        de += gh[..., None] * dyt[:, T, None, :]
        dlh = _softmax_bwd(gh, (dyt[:, T, None, :] * e).sum(2))
        dWg3h = q[:, T].T @ dlh
        dq[:, T] = dlh @ Wg3h.T
    dzq, dze = dq * (pq > 0), de * (pe > 0)
    dWe2, dbe2 = np.einsum("bik,bio->iko", h[:, :ne], dze), dze.sum(0)
    dWg2, dbg2 = np.einsum("bgk,bgo->gko", h[:, ne:], dzq), dzq.sum(0)
    dh = np.concatenate([np.einsum("bio,iko->bik", dze, We2), np.einsum("bgo,gko->bgk", dzq, Wg2)], axis=1)
    dz1 = dh * (ph > 0)
    dxg = np.einsum("bmj,kmj->bmk", dz1, W1b)
    dxin = np.zeros_like(xin)
    for m, g in enumerate(grp):                                               # a group's dxin sums its own MLPs only
        dxin[:, g if Gin > 1 else 0] += dxg[:, m]
    res.update(dxin=dxin, dparams=[np.einsum("bmk,bmj->kmj", xg, dz1).reshape(Din, -1), dz1.sum(0).reshape(-1), dWe2,
                                   dbe2, dWg2, dbg2, dWg3s, dWg3h, dWtw, dbtw])
    return res


def body_numpy(x, levels, T, S, Sh, dout=None):
    """x [B, D] and the packed parameters of every level -> out [B, T], pre, the level results; with dout also dx and
    dparams (a list per level)."""
    L = len(levels)
    cur = np.asarray(x, np.float64)[:, None, :]
    fwd = []
    for lv, params in enumerate(levels):
        fwd.append((cur, level_numpy(cur, params, T, S, Sh, lv == L - 1)))
        cur = fwd[-1][1]["y"]
    res = dict(out=fwd[-1][1]["out"], pre=np.min([f[1]["pre"] for f in fwd], axis=0), levels=[f[1] for f in fwd])
    if dout is None:
        return res
    dparams, dy = [None] * L, None
    for lv in reversed(range(L)):
        r = level_numpy(fwd[lv][0], levels[lv], T, S, Sh, lv == L - 1, dy=dy, dout=dout if lv == L - 1 else None)
        dparams[lv], dy = r["dparams"], r["dxin"]
    res.update(dx=dy[:, 0], dparams=dparams)
    return res


# ---- torch, the reference's op order --------------------------------------------------------------------------------
def level_torch(inputs, params, T, S, Sh, last, saved=None):
    """call_cgc_net (:315-358): ``inputs`` a list of T + 1 tensors [B, Din] -> the list of T (last) or T + 1 outputs.
    ``saved``: a dict that receives the intermediates under the names of SAVED."""
    W1, b1, We2, be2, Wg2, bg2, Wg3s, Wg3h, Wtw, btw = params
    ne, H1 = T * S + Sh, We2.shape[1]
    relu = torch.relu
    hs = {}

    def first(x, m):
        hs[m] = relu(x @ W1[:, m * H1:(m + 1) * H1] + b1[m * H1:(m + 1) * H1])
        return hs[m]

    expert = lambda x, i: relu(first(x, i) @ We2[i] + be2[i])
    specific = [expert(inputs[i], i * S + j) for i in range(T) for j in range(S)]
    shared = [expert(inputs[-1], T * S + k) for k in range(Sh)]
    outputs, qs, gs = [], [], []
    for t in range(T):
        cur = specific[t * S:(t + 1) * S] + shared
        expert_concat = torch.stack(cur, dim=1)
        gate = relu(first(inputs[t], ne + t) @ Wg2[t] + bg2[t])
        qs.append(gate)
        gate = torch.softmax(gate @ Wg3s[t], dim=-1)      # MLPLayer(units=[S + Sh], use_bias=False, activation='softmax')
        gate = torch.softmax(gate, dim=-1)                # tf.nn.softmax(gate_output, axis=-1)
        gs.append(gate)
        outputs.append((expert_concat * gate.unsqueeze(-1)).sum(1))
    if not last:
        expert_concat = torch.stack(specific + shared, dim=1)
        gate = relu(first(inputs[-1], ne + T) @ Wg2[T] + bg2[T])
        qs.append(gate)
        gate = torch.softmax(gate @ Wg3h, dim=-1)
        gs.append(gate)
        outputs.append((expert_concat * gate.unsqueeze(-1)).sum(1))
    if saved is not None:
        cat = lambda ts: torch.cat(ts, dim=1)
        saved.update(h=cat([hs[m] for m in sorted(hs)]), e=cat(specific + shared), q=cat(qs), g=cat(gs))
    return outputs


def towers_torch(ys, Wtw, btw):
    return torch.cat([torch.sigmoid(y @ Wtw[t].reshape(-1, 1) + btw[t]) for t, y in enumerate(ys)], dim=1)


def _n64(t):
    return None if t is None else t.detach().double().numpy()


def _grads(ts):
    return [None if t is None else _n64(t.grad) for t in ts]


def _params_t(params, dtype):
    return [None if a is None else _t(a, dtype, True) for a in params]


def level_torch_grads(xin, params, T, S, Sh, last, dy, dout, dtype):
    """-> (y, out, dxin, dparams, saved) as fp64 numpy, computed in ``dtype`` on the CPU"""
    xt, pt = _t(xin, dtype, True), _params_t(params, dtype)
    Gin = xt.shape[1]
    saved = {}
    ys = level_torch([xt[:, g if Gin > 1 else 0] for g in range(T + 1)], pt, T, S, Sh, last, saved)
    y = torch.stack(ys, dim=1)
    loss = (y * _t(dy, dtype)).sum() if dy is not None else 0
    out = None
    if last:
        out = towers_torch(ys, pt[8], pt[9])
        loss = loss + (out * _t(dout, dtype)).sum()
    loss.backward()
    return _n64(y), _n64(out), _n64(xt.grad), _grads(pt), {k: _n64(v) for k, v in saved.items()}


def body_torch(x, levels, T, S, Sh):
    """PLELayer.call after the lookup (:371-382): tensors -> out [B, T]"""
    inputs = [x] * (T + 1)
    for lv, params in enumerate(levels):
        inputs = level_torch(inputs, params, T, S, Sh, lv == len(levels) - 1)
    return towers_torch(inputs, levels[-1][8], levels[-1][9])


def body_torch_grads(x, levels, T, S, Sh, dout, dtype):
    """-> (out, dx, dparams per level) as fp64 numpy"""
    xt, pt = _t(x, dtype, True), [_params_t(p, dtype) for p in levels]
    out = body_torch(xt, pt, T, S, Sh)
    out.backward(_t(dout, dtype))
    return _n64(out), _n64(xt.grad), [_grads(p) for p in pt]


def layer_torch_grads(table, X, levels, T, S, Sh, gout, dtype):
    """The whole layer: lookup, flatten, body -> (out [B, T], dtable, dparams per level) as fp64 numpy"""
    tt, pt = _t(table, dtype, True), [_params_t(p, dtype) for p in levels]
    out = body_torch(tt[torch.from_numpy(np.asarray(X, np.int64))].flatten(1), pt, T, S, Sh)
    out.backward(_t(gout, dtype))
    return _n64(out), _n64(tt.grad), [_grads(p) for p in pt]


def state_dict_of(table, levels, T, S, Sh):
    """packed arrays of every level -> {state-dict name of PLELayer: array}"""
    L = len(levels)
    out = {"embedding_layer.embeddings": table}
    for lv, (W1, b1, We2, be2, Wg2, bg2, Wg3s, Wg3h, Wtw, btw) in enumerate(levels):
        ne, H1 = T * S + Sh, We2.shape[1]
        blk = lambda a, i: a[..., i * H1:(i + 1) * H1]
        for i in range(ne):
            pre = ("specific_expert_networks.%d.%d." % (lv, i)) if i < T * S else \
                ("shared_expert_networks.%d.%d." % (lv, i - T * S))
            out.update({pre + "kernel_0": blk(W1, i), pre + "bias_0": blk(b1, i), pre + "kernel_1": We2[i],
                        pre + "bias_1": be2[i]})
        for g in range(Wg2.shape[0]):
            pre = ("specific_gates.%d.%d." % (lv, g)) if g < T else ("shared_gates.%d." % lv)
            out.update({pre + "0.kernel_0": blk(W1, ne + g), pre + "0.bias_0": blk(b1, ne + g), pre + "0.kernel_1": Wg2[g],
                        pre + "0.bias_1": bg2[g], pre + "1.kernel_0": Wg3s[g] if g < T else Wg3h})
        if lv == L - 1:
            for t in range(T):
                out.update({"tower_outputs.%d.kernel_0" % t: Wtw[t].reshape(-1, 1), "tower_outputs.%d.bias_0" % t: btw[t:t + 1]})
    return out


# ---- the cases of the host and GPU tests ----------------------------------------------------------------------------
def _gen_level(case, seed):
    B, Din, Gin, T, S, Sh, H1, O, Og, last = case
    r = np.random.default_rng(seed)
    params = [f32_exact(p) for p in make_level(r, Din, T, S, Sh, H1, O, Og, last)]
    return r, params, f32_exact(r.normal(0, 1, (B, Gin, Din)))


@functools.lru_cache(maxsize=None)
def level_case(*case):
    """-> dict(params, xin, dy, dout, ref, near, seed): fp32-exact inputs, the fp64 reading, the near-kink examples (their
    dy and dout rows are zero).  Under 100 examples the first seed 1, 2, 3, ... without a near-kink example, on the fp64
    reading.  The last level takes a gradient on y AND on out, so that both reach dy inside the kernel."""
    B, _, _, T, S, Sh, _, O, _, last = case

    def near_of(s):
        _, params, xin = _gen_level(case, s)
        return level_numpy(xin, params, T, S, Sh, last)["pre"] < PRE_EPS

    seed = clean_seed(lambda s: near_of(s).any()) if B < 100 else 1
    r, params, xin = _gen_level(case, seed)
    near = near_of(seed)
    dy = f32_exact(r.uniform(-1, 1, (B, T if last else T + 1, O)))
    dout = f32_exact(r.uniform(-1, 1, (B, T))) if last else None
    dy[near] = 0.0
    if last:
        dout[near] = 0.0
    return dict(params=params, xin=xin, dy=dy, dout=dout, near=near, seed=seed, cfg=(T, S, Sh, last),
                ref=level_numpy(xin, params, T, S, Sh, last, dy, dout))


@functools.lru_cache(maxsize=None)
def level_case_t32(*case):
    """the fp32 CPU transcription on the inputs of level_case: (y, out, dxin, dparams, saved)"""
    c = level_case(*case)
    return level_torch_grads(c["xin"], c["params"], *c["cfg"], c["dy"], c["dout"], torch.float32)


def _gen_body(case, seed):
    B, D, T, S, Sh, L = case
    r = np.random.default_rng(seed)
    levels = [[f32_exact(p) for p in lv] for lv in make_body(r, D, T, S, Sh, L)]
    return r, levels, f32_exact(r.normal(0, 1, (B, D)))


@functools.lru_cache(maxsize=None)
def body_case(*case):
    """-> dict(levels, x, dout, ref, near, seed) of a whole body, chosen like level_case"""
    B, _, T, S, Sh, _ = case

    def near_of(s):
        _, levels, x = _gen_body(case, s)
        return body_numpy(x, levels, T, S, Sh)["pre"] < PRE_EPS

    seed = clean_seed(lambda s: near_of(s).any()) if B < 100 else 1
    r, levels, x = _gen_body(case, seed)
    near = near_of(seed)
    dout = f32_exact(r.uniform(-1, 1, (B, T)))
    dout[near] = 0.0
    return dict(levels=levels, x=x, dout=dout, near=near, seed=seed, cfg=(T, S, Sh),
                ref=body_numpy(x, levels, T, S, Sh, dout))


LAYER_B, LAYER_V, LAYER_F, LAYER_E = 32, 1000, 9, 8


def _gen_layer(seed):
    r = np.random.default_rng(seed)
    table = f32_exact(r.normal(0, 0.5, (LAYER_V, LAYER_E)))
    levels = [[f32_exact(p) for p in lv] for lv in make_body(r, LAYER_F * LAYER_E, 3, 3, 3, 2)]
    return table, r.integers(0, LAYER_V, (LAYER_B, LAYER_F)).astype(np.int64), levels


@functools.lru_cache(maxsize=None)
def layer_case():
    """-> (seed, table, X int64 [32, 9], levels) of the default PLELayer over a table of 1000 rows: the first seed without
    a near-kink example"""
    def near(seed):
        table, X, levels = _gen_layer(seed)
        return (body_numpy(table[X].reshape(LAYER_B, -1), levels, 3, 3, 3)["pre"] < PRE_EPS).any()

    seed = clean_seed(near)
    return (seed,) + _gen_layer(seed)


@functools.lru_cache(maxsize=None)
def body_case_t32(*case):
    c = body_case(*case)
    return body_torch_grads(c["x"], c["levels"], *c["cfg"], c["dout"], torch.float32)
