"""Reference readings of the ComiRec kernels and layers (csrc/comirec.hip, layers.ComiRecLayer), written from the formulas
of include/mi355rec.h: an fp64 numpy forward with a hand-derived backward of the dynamic routing, the self-attentive
extractor and the hard attention + sampled-softmax loss, a torch-CPU transcription of each and of the whole layer whose
gradients come from autograd (fp32: the error floor of the tolerance; fp64: the check of the hand-derived backward), the
generators of the test cases and the kink rule of the argmax.

Generators: table ~ N(0, 0.5), W ~ N(0, 1 / sqrt(D)), W1 and W2 glorot, B0 ~ N(0, 0.05) (non-zero: a kernel that ignored it
would fail), m ~ N(0, 0.5), every value fp32-exact.  The first four examples of a series case have 0, 1, 2 and T padded
positions (at most T), the others are mind_ref.series_ids'; only the FIRST series feature carries the padding id.
Position t takes part iff (series[b,t,0] == pad) == keep_padding, and every series case runs with keep_padding 0 and 1.

The argmax of the hard attention is a kink: an example is NEAR A TIE when any of its items has a top-two gap of p in fp64
below GAP_EPS (1e-4 for the body cases, 1e-5 for the layer cases, whose capsules are small).  Near-tie examples of a body
case are left out of the comparison (their rows skipped, their upstream gradients zeroed on both sides) and may be at
most 10 % of the batch; the seed of a layer case is the first of 1, 2, 3, ... with none at all."""
import functools

import numpy as np
import torch

from tests import mind_ref as MR
from tests.mind_ref import FMIN, V_CASE, f32_exact, gather, rel_err, series_ids  # noqa: F401
from tests.masknet_ref import clean_seed, glorot

# (B, T, C, E, Dc, K, R)
DR_CASES = [(1, 1, 1, 1, 1, 1, 1), (3, 5, 1, 8, 8, 4, 3), (33, 6, 3, 16, 48, 4, 3), (33, 50, 3, 16, 48, 4, 3),
            (33, 65, 3, 8, 40, 16, 3), (17, 6, 3, 16, 48, 4, 1), (17, 6, 3, 16, 48, 4, 5), (17, 33, 3, 16, 48, 1, 3),
            (5, 9, 4, 64, 256, 16, 3), (2049, 10, 3, 16, 48, 4, 3)]
# (B, T, C, E, Dc, K): the distinct shapes of the above
SA_CASES = list(dict.fromkeys(c[:6] for c in DR_CASES))
# (B, Ns, C, E, K)
SELECT_CASES = MR.LAA_CASES
SELECT_WAYS = MR.LAA_WAYS
GAP_EPS_BODY, GAP_EPS_LAYER = 1e-4, 1e-5


def _softmax(z, axis):
    e = np.exp(z - z.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def comirec_series(r, B, T, C, V, pad=0):
    ids = series_ids(r, B, T, C, V, pad)
    for b, n in enumerate(np.minimum([0, 1, 2, T], T)[:B]):
        ids[b, :, 0] = r.integers(1, V, T)
        ids[b, r.permutation(T)[:n], 0] = pad
    return ids


def takes_part(series, keep, pad=0):
    return (series[:, :, 0] == pad) == bool(keep)


def positional_table(T, D):
    """the float32 reading of ComiRecSelfAttentiveLayer.positional_encoding / get_angles"""
    pos = np.arange(T).astype(np.float32)[:, None]
    i = np.arange(D).astype(np.float32)[None, :]
    angle_rates = np.float32(1) / np.power(np.float32(10000.0), (np.float32(2) * (i // np.float32(2))) / np.float32(D))
    angle = pos * angle_rates
    out = np.where((np.arange(D) % 2 == 0)[None, :], np.sin(angle), np.cos(angle))
    assert out.dtype == np.float32
    return out


# ---- (a) dynamic routing ---------------------------------------------------------------------------------------------
def dr_numpy(table, series, W, B0, R, keep, pad=0, gout=None):
    """fp64.  -> out [B,K,Dc], W (the weights of the last round), valid (who takes part) and, with gout, gkeys [B,T,D] and
    dW [K,T,D,Dc]"""
    x = gather(table, series)
    part = takes_part(series, keep, pad)[:, None, :]
    u = np.einsum("btd,ktdc->bktc", x, W)
    L = np.broadcast_to(B0, (len(x),) + B0.shape).copy()
    Cs, ss = [], []
    for r in range(R):
        C = _softmax(np.where(part, L, FMIN), axis=2)
        s = np.einsum("bkt,bktc->bkc", C, u)
        n2 = (s * s).sum(-1, keepdims=True)
        c = s * np.sqrt(n2) / (1 + n2)
        Cs.append(C)
        ss.append(s)
        if r < R - 1:
            L = L + np.einsum("bkc,bktc->bkt", c, u)
    res = dict(out=c, W=Cs[-1], valid=part[:, 0, :])
    if gout is None:
        return res
    du, dL = np.zeros_like(u), np.zeros_like(L)
    for r in range(R - 1, -1, -1):
        C, s = Cs[r], ss[r]
        n2 = (s * s).sum(-1, keepdims=True)
        n = np.sqrt(n2)
        f = n / (1 + n2)
        dc = gout if r == R - 1 else np.einsum("bkt,bktc->bkc", dL, u)
        if r < R - 1:
            du += dL[..., None] * (s * f)[:, :, None, :]
        g = np.where(n > 0, (1 - n2) / ((1 + n2) ** 2 * np.where(n > 0, n, 1.0)), 0.0)
        ds = f * dc + s * g * (s * dc).sum(-1, keepdims=True)
        dC = np.einsum("bkc,bktc->bkt", ds, u)
        du += C[..., None] * ds[:, :, None, :]
        dL = dL + np.where(part, C * (dC - (dC * C).sum(-1, keepdims=True)), 0.0)
    res["gkeys"] = np.einsum("bktc,ktdc->btd", du, W)
    res["dW"] = np.einsum("btd,bktc->ktdc", x, du)
    return res


def dr_torch(x, part, W, B0, R):
    """x [B,T,D] looked-up rows, part [B,T] bool -> the capsules [B,K,Dc]: ComiRecDynamicRoutingLayer.call with the squash
    written as c n / (1 + n^2)"""
    u = torch.einsum("bse,nsec->bnsc", x, W)
    L = B0[None].expand(x.shape[0], -1, -1)
    drop = torch.full_like(L, FMIN)
    for i in range(R):
        C = torch.softmax(torch.where(part[:, None, :], L, drop), dim=2)
        s = torch.einsum("bns,bnsc->bnc", C, u)
        n = torch.linalg.vector_norm(s, dim=2, keepdim=True)
        c = s * n / (1 + n * n)
        if i < R - 1:
            L = L + torch.einsum("bnc,bnsc->bns", c, u)
    return c


def dr_torch_grads(table, series, W, B0, R, keep, gout, dtype, pad=0):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x, Wt = t(gather(table, series)).requires_grad_(), t(W).requires_grad_()
    out = dr_torch(x, torch.from_numpy(takes_part(series, keep, pad)), Wt, t(B0), R)
    (out * t(gout)).sum().backward()
    return dict(out=out.detach().numpy(), gkeys=x.grad.numpy(), dW=Wt.grad.numpy())


@functools.lru_cache(maxsize=None)
def dr_inputs(*case):
    B, T, C, E, Dc, K, R = case
    r = np.random.default_rng(1)
    D = C * E
    return dict(table=f32_exact(r.normal(0, 0.5, (V_CASE, E))), W=f32_exact(r.normal(0, 1 / np.sqrt(D), (K, T, D, Dc))),
                B0=f32_exact(r.normal(0, 0.05, (K, T))), series=comirec_series(r, B, T, C, V_CASE),
                gout=f32_exact(r.uniform(-1, 1, (B, K, Dc))), R=R)


@functools.lru_cache(maxsize=None)
def dr_ref(case, keep):
    c = dr_inputs(*case)
    return dr_numpy(c["table"], c["series"], c["W"], c["B0"], c["R"], keep, 0, c["gout"])


@functools.lru_cache(maxsize=None)
def dr_case_t(case, keep, dtype):
    c = dr_inputs(*case)
    return dr_torch_grads(c["table"], c["series"], c["W"], c["B0"], c["R"], keep, c["gout"], dtype)


routed_share = MR.routed_share


# ---- (b) self-attentive extractor --------------------------------------------------------------------------------------
def sa_numpy(table, series, W1, W2, pos, keep, pad=0, gout=None):
    """fp64; pos [T,D] or None.  -> out [B,K,Dc] and, with gout, gkeys [B,T,D], dW1 [D,Dc] and dW2 [K,Dc]"""
    x = gather(table, series)
    if pos is not None:
        x = x + np.asarray(pos, np.float64)
    part = takes_part(series, keep, pad)[:, None, :]
    h = np.tanh(x @ W1)
    sc = np.einsum("btc,kc->bkt", h, W2)
    A = _softmax(np.where(part, sc, FMIN), axis=2)
    res = dict(out=np.einsum("bkt,btc->bkc", A, h), A=A)
    if gout is None:
        return res
    dA = np.einsum("bkc,btc->bkt", gout, h)
    dsc = np.where(part, A * (dA - (A * dA).sum(-1, keepdims=True)), 0.0)
    dh = np.einsum("bkt,bkc->btc", A, gout) + np.einsum("bkt,kc->btc", dsc, W2)
    dz = dh * (1 - h * h)
    res.update(gkeys=dz @ W1.T, dW1=np.einsum("btd,btc->dc", x, dz), dW2=np.einsum("bkt,btc->kc", dsc, h))
    return res


def sa_torch(x, part, W1, W2, pos):
    """ComiRecSelfAttentiveLayer.call on looked-up rows x [B,T,D]"""
    if pos is not None:
        x = x + pos
    mids = torch.tanh(torch.einsum("bse,ec->bsc", x, W1))
    score = torch.einsum("bsc,nc->bns", mids, W2)
    score = torch.softmax(torch.where(part[:, None, :], score, torch.full_like(score, FMIN)), dim=-1)
    return torch.einsum("bsc,bns->bnc", mids, score)


def sa_torch_grads(table, series, W1, W2, pos, keep, gout, dtype, pad=0):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x, W1t, W2t = t(gather(table, series)).requires_grad_(), t(W1).requires_grad_(), t(W2).requires_grad_()
    out = sa_torch(x, torch.from_numpy(takes_part(series, keep, pad)), W1t, W2t, None if pos is None else t(pos))
    (out * t(gout)).sum().backward()
    return dict(out=out.detach().numpy(), gkeys=x.grad.numpy(), dW1=W1t.grad.numpy(), dW2=W2t.grad.numpy())


@functools.lru_cache(maxsize=None)
def sa_inputs(*case):
    B, T, C, E, Dc, K = case
    r = np.random.default_rng(3)
    D = C * E
    return dict(table=f32_exact(r.normal(0, 0.5, (V_CASE, E))), W1=f32_exact(glorot(r, D, Dc)),
                W2=f32_exact(glorot(r, K, Dc)), series=comirec_series(r, B, T, C, V_CASE),
                gout=f32_exact(r.uniform(-1, 1, (B, K, Dc))), pos=positional_table(T, D).astype(np.float64))


def sa_pos(c, with_pos):
    return c["pos"] if with_pos else None


@functools.lru_cache(maxsize=None)
def sa_ref(case, keep, with_pos):
    c = sa_inputs(*case)
    return sa_numpy(c["table"], c["series"], c["W1"], c["W2"], sa_pos(c, with_pos), keep, 0, c["gout"])


@functools.lru_cache(maxsize=None)
def sa_case_t(case, keep, with_pos, dtype):
    c = sa_inputs(*case)
    return sa_torch_grads(c["table"], c["series"], c["W1"], c["W2"], sa_pos(c, with_pos), keep, c["gout"], dtype)


# ---- (c) hard attention + sampled-softmax loss -------------------------------------------------------------------------
def select_numpy(table, items, m, ginner=None, gloss=None, gsel=None):
    """fp64.  -> chosen [B,Ns] (the smallest index of the maximum), inner [B,Ns], loss [B], gap [B] (the smallest top-two
    gap of p over the example's items; inf at K = 1) and, with any upstream gradient, gm [B,K,Dc] and gitems [B,Ns,Dc]"""
    x = gather(table, items)
    B, K = m.shape[:2]
    p = np.einsum("bkd,bsd->bsk", m, x)
    chosen = p.argmax(-1)                                        # numpy: the first occurrence
    inner = p.max(-1)
    top = np.sort(p, axis=-1)
    gap = (top[..., -1] - top[..., -2]).min(1) if K > 1 else np.full(B, np.inf)
    mx = inner.max(1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(inner - mx).sum(1))
    res = dict(chosen=chosen.astype(np.int32), inner=inner, loss=lse - inner[:, 0], gap=gap)
    if ginner is None and gloss is None and gsel is None:
        return res
    g = np.zeros_like(inner) if ginner is None else ginner.copy()
    if gloss is not None:
        q = np.exp(inner - lse[:, None])
        q[:, 0] -= 1.0
        g = g + gloss[:, None] * q
    dsel = g[..., None] * x + (0.0 if gsel is None else gsel)     # the gradient of the selected capsules
    onehot = chosen[..., None] == np.arange(K)
    res["gm"] = np.einsum("bsk,bsd->bkd", onehot.astype(np.float64), dsel)
    res["gitems"] = g[..., None] * np.take_along_axis(m, chosen[..., None], axis=1)
    return res


def first_argmax(p):
    K = p.shape[-1]
    return torch.where(p == p.max(-1, keepdim=True).values, torch.arange(K), K).min(-1).values


def select_torch(x, m):
    """x [B,Ns,Dc] looked-up items, m [B,K,Dc] -> (selected [B,Ns,Dc], inner [B,Ns], loss [B], chosen [B,Ns]):
    ComiRecLayer.manually_negative_sampled_call after the capsules"""
    p = (m[:, None, :, :] * x[:, :, None, :]).sum(-1)
    chosen = first_argmax(p.detach())
    selected = torch.gather(m, 1, chosen[:, :, None].expand(-1, -1, m.shape[2]))
    inner = (selected * x).sum(-1)
    return selected, inner, torch.logsumexp(inner, dim=1) - inner[:, 0], chosen


def select_torch_grads(table, items, m, ginner, gloss, gsel, dtype):
    t = lambda a: torch.tensor(np.asarray(a), dtype=dtype)
    x, mt = t(gather(table, items)).requires_grad_(), t(m).requires_grad_()
    selected, inner, loss, chosen = select_torch(x, mt)
    tot = 0
    for out, g in ((inner, ginner), (loss, gloss), (selected, gsel)):
        if g is not None:
            tot = tot + (out * t(g)).sum()
    tot.backward()
    return dict(chosen=chosen.numpy().astype(np.int32), inner=inner.detach().numpy(), loss=loss.detach().numpy(),
                gm=mt.grad.numpy(), gitems=x.grad.numpy())


@functools.lru_cache(maxsize=None)
def select_case(*case):
    """-> inputs and near [B] bool (the near-tie examples on the fp64 reading); the upstream gradients of those examples
    are zero already"""
    B, Ns, C, E, K = case
    r = np.random.default_rng(2)
    c = dict(table=f32_exact(r.normal(0, 0.5, (V_CASE, E))), items=r.integers(0, V_CASE, (B, Ns, C)).astype(np.int64),
             m=f32_exact(r.normal(0, 0.5, (B, K, C * E))), ginner=f32_exact(r.uniform(-1, 1, (B, Ns))),
             gloss=f32_exact(r.uniform(-1, 1, B)), gsel=f32_exact(r.uniform(-1, 1, (B, Ns, C * E))))
    c["near"] = select_numpy(c["table"], c["items"], c["m"])["gap"] < GAP_EPS_BODY
    for k in ("ginner", "gloss", "gsel"):
        c[k][c["near"]] = 0.0
    return c


def select_way(c, way, with_gsel=False):
    use_inner, use_loss = SELECT_WAYS[way]
    return (c["ginner"] if use_inner else None), (c["gloss"] if use_loss else None), (c["gsel"] if with_gsel else None)


# ---- the layer ---------------------------------------------------------------------------------------------------------
ITEM, SERIES = MR.ITEM, MR.SERIES
LAYER_V, LAYER_E, LAYER_K, LAYER_R, LAYER_NS = MR.LAYER_V, MR.LAYER_E, MR.LAYER_K, MR.LAYER_R, MR.LAYER_NS
LAYER_B, LAYER_TS = MR.LAYER_B, MR.LAYER_TS
LAYER_D = LAYER_E * len(SERIES)
STATE_SHAPES = {
    "DR": lambda T: {"embed.embeddings": (LAYER_V, LAYER_E), "interest_extractor.W": (LAYER_K, T, LAYER_D, LAYER_D),
                     "interest_extractor.B": (LAYER_K, T)},
    "SA": lambda T: {"embed.embeddings": (LAYER_V, LAYER_E), "interest_extractor.W1": (LAYER_D, LAYER_D),
                     "interest_extractor.W2": (LAYER_K, LAYER_D)}}
BUFFERS = ("interest_extractor.B",)


def layer_state(seed, T, mode):
    r = np.random.default_rng(seed)
    D = LAYER_D
    sd = {"embed.embeddings": r.normal(0, 0.5, (LAYER_V, LAYER_E))}
    if mode == "DR":
        sd["interest_extractor.W"] = r.normal(0, 1 / np.sqrt(D), (LAYER_K, T, D, D))
        sd["interest_extractor.B"] = r.normal(0, 0.05, (LAYER_K, T))
    else:
        sd["interest_extractor.W1"] = glorot(r, D, D)
        sd["interest_extractor.W2"] = glorot(r, LAYER_K, D)
    assert {k: v.shape for k, v in sd.items()} == STATE_SHAPES[mode](T)
    return {k: f32_exact(v) for k, v in sd.items()}


def layer_inputs(seed, B, T, mode="DR"):
    """mind_ref's batch with the series' first feature re-drawn.  DR: the first four rows get 0, 1, 2 and T padded
    positions.  SA: every row gets between 2 and T - 2 of them, so that two or more positions take part under either mask
    sense: with fewer, every head of the self-attentive extractor returns the SAME capsule -- an exact tie of the hard
    attention by construction, which the body cases and a test of their own cover, not a near tie a seed could avoid."""
    ins = MR.layer_inputs(seed, B, T)
    r = np.random.default_rng(3000 + seed)
    n_pad = np.minimum([0, 1, 2, T], T)[:B] if mode == "DR" else r.integers(2, T - 1, B)
    for b, n in enumerate(n_pad):
        ins[SERIES[0]][b] = r.integers(1, LAYER_V, T)
        ins[SERIES[0]][b, r.permutation(T)[:n]] = 0
    return ins


def layer_torch(sd, ins, dtype, mode, reference_mask, gsel=None, gloss=None):
    """ComiRecLayer.call / generate_interest_capsules on the CPU.  -> dict(output [B,Ns,Dc], loss, capsules, chosen, gap
    [B]: the example's smallest top-two gap of the inner products) and, with gsel / gloss, grads of every trainable
    parameter"""
    P = {k: torch.tensor(v, dtype=dtype) for k, v in sd.items()}
    for k in P:
        if k not in BUFFERS:
            P[k].requires_grad_()
    series = torch.from_numpy(np.stack([ins[n] for n in SERIES], axis=2))
    items = torch.from_numpy(np.stack([ins[n] for n in ITEM], axis=2))
    B, T, C = series.shape
    tab = P["embed.embeddings"]
    part = (series[:, :, 0] == 0) == bool(reference_mask)
    x = tab[series].reshape(B, T, -1)
    if mode == "DR":
        caps = dr_torch(x, part, P["interest_extractor.W"], P["interest_extractor.B"], LAYER_R)
    else:
        caps = sa_torch(x, part, P["interest_extractor.W1"], P["interest_extractor.W2"],
                        torch.tensor(positional_table(T, x.shape[2]), dtype=dtype))
    xi = tab[items].reshape(B, items.shape[1], -1)
    selected, inner, loss, chosen = select_torch(xi, caps)
    p = torch.einsum("bkd,bsd->bsk", caps.detach(), xi.detach())
    top = torch.sort(p, dim=-1).values
    res = dict(output=selected.detach().numpy(), loss=loss.detach().numpy(), capsules=caps.detach().numpy(),
               chosen=chosen.numpy(), gap=(top[..., -1] - top[..., -2]).min(1).values.numpy())
    if gsel is not None:
        ((selected * torch.tensor(gsel, dtype=dtype)).sum() + (loss * torch.tensor(gloss, dtype=dtype)).sum()).backward()
        res["grads"] = {k: p.grad.numpy() for k, p in P.items() if k not in BUFFERS}
    return res


@functools.lru_cache(maxsize=None)
def layer_seed(T, mode, reference_mask, B=LAYER_B):
    """the first seed 1, 2, 3, ... whose fp64 reading has no near-tie example at all"""
    def near(seed):
        res = layer_torch(layer_state(seed, T, mode), layer_inputs(seed, B, T, mode), torch.float64, mode, reference_mask)
        return bool((res["gap"] < GAP_EPS_LAYER).any())
    return clean_seed(near)


def layer_upstream(seed, B=LAYER_B):
    r = np.random.default_rng(2000 + seed)
    return f32_exact(r.uniform(-1, 1, (B, LAYER_NS, LAYER_D))), f32_exact(r.uniform(-1, 1, B))
