"""Restatements of the reference's InteractionLayer / AttentionLayer / AttentionalFactorizationMachine
(3.DCN/CustomLayers.py:825-885) for the AFM tests.

* ``afm_numpy``: an fp64 numpy reading.  The pair list comes from index arithmetic (row-major upper triangle), the
  softmax is explicit with the max subtracted, and the backward is derived by hand with c = do . o:
  ds_k = a_k (do . p_k - c).
* ``afm_torch``: a transcription in the reference's op order -- python double loop over the fields, stack, transpose,
  Dense-relu, Dense, softmax(dim=1), transpose, matmul, reshape -- runnable in any dtype, gradients by autograd (fp64 is
  checked against the numpy reading, fp32 measures what a float32 evaluation of the same ops loses).
* ``afm_torch_indexed``: the same ops with the pairs taken by two index tensors instead of the python loop (what a torch
  user would run on the GPU; used by scripts/exp/afm_time.py).
* ``afm_batchaxis``: the softmax over the batch axis, which the reference does NOT compute; the tests use it to show
  that their inputs can tell the two apart.
* ``afm_layer_torch``: the whole layer: lookup, interaction, attention, MLPLayer([1], sigmoid).
"""
import numpy as np
import torch


def pair_index(F):
    """(I, J): the pairs i < j with i outer and j inner, by index arithmetic."""
    I, J = np.triu_indices(F, k=1)
    return I.astype(np.int64), J.astype(np.int64)


def afm_numpy(rows, Wa, ba, hv, bh, do=None):
    """rows [B,F,E], Wa [E,A], ba [A], hv [A] or [A,1], bh [1] -> dict(o, a, pre_min [, drows, dWa, dba, dhv, dbh])."""
    rows, Wa, ba, bh = (np.asarray(t, np.float64) for t in (rows, Wa, ba, bh))
    hv = np.asarray(hv, np.float64).reshape(-1)
    B, F, E = rows.shape
    I, J = pair_index(F)
    p = rows[:, I, :] * rows[:, J, :]                             # [B,P,E]
    pre = p @ Wa + ba                                             # [B,P,A]
    h = np.maximum(pre, 0.0)
    s = h @ hv + bh.reshape(())                                   # [B,P]
    w = np.exp(s - s.max(axis=1, keepdims=True))                  # softmax over the PAIR axis
    a = w / w.sum(axis=1, keepdims=True)
    o = np.einsum("bk,bke->be", a, p)
    out = {"o": o, "a": a, "pre_min": np.abs(pre).min(axis=(1, 2))}
    if do is None:
        return out
    do = np.asarray(do, np.float64)
    c = (do * o).sum(axis=1)
    ds = a * ((do[:, None, :] * p).sum(axis=2) - c[:, None])      # the same summation as c: exactly 0 at P = 1
    dpre = ds[:, :, None] * hv[None, None, :] * (pre > 0)
    dp = a[:, :, None] * do[:, None, :] + dpre @ Wa.T
    drows = np.zeros_like(rows)
    for k in range(len(I)):
        drows[:, I[k], :] += dp[:, k, :] * rows[:, J[k], :]
        drows[:, J[k], :] += dp[:, k, :] * rows[:, I[k], :]
    out.update(drows=drows, dWa=np.einsum("bke,bka->ea", p, dpre), dba=dpre.sum(axis=(0, 1)),
               dhv=np.einsum("bk,bka->a", ds, h), dbh=np.array([ds.sum()]))
    return out


def interaction_torch(x):
    """3.DCN/CustomLayers.py:829-838."""
    result = []
    fields_cnt = x.shape[1]
    for i in range(fields_cnt - 1):
        for j in range(i + 1, fields_cnt):
            result.append(x[:, i, :] * x[:, j, :])
    return torch.stack(result).permute(1, 0, 2)                  # convert_to_tensor + transpose [1,0,2]


def attention_torch(x, Wa, ba, hv, bh, axis=1):
    """3.DCN/CustomLayers.py:847-853; hv [A,1]."""
    s = torch.relu(x @ Wa + ba) @ hv + bh                         # (B, P, 1)
    score = torch.softmax(s, dim=axis)
    out = torch.matmul(score.permute(0, 2, 1), x)                 # (B, 1, E)
    return out.reshape(-1, x.shape[2])


def afm_torch(rows, Wa, ba, hv, bh):
    return attention_torch(interaction_torch(rows), Wa, ba, hv.reshape(-1, 1), bh)


def afm_torch_indexed(rows, I, J, Wa, ba, hv, bh):
    return attention_torch(rows[:, I, :] * rows[:, J, :], Wa, ba, hv.reshape(-1, 1), bh)


def afm_batchaxis(rows, Wa, ba, hv, bh):
    return attention_torch(interaction_torch(rows), Wa, ba, hv.reshape(-1, 1), bh, axis=0)


def afm_layer_torch(p, X):
    """p: embed [V,E], Wa, ba, hv [A,1], bh, out_k [E,1], out_b [1]; X int64 [B,F] -> sigmoid [B,1]."""
    o = afm_torch(p["embed"][X], p["Wa"], p["ba"], p["hv"], p["bh"])
    return torch.sigmoid(o @ p["out_k"] + p["out_b"])


def afm_torch_grads(rows, Wa, ba, hv, bh, do, dtype):
    """The transcription on the CPU in ``dtype``: (o, [drows, dWa, dba, dhv, dbh])."""
    t = [torch.from_numpy(np.asarray(a)).to(dtype).requires_grad_() for a in (rows, Wa, ba, hv, bh)]
    o = afm_torch(*t)
    g = torch.autograd.grad(o, t, torch.from_numpy(np.asarray(do)).to(dtype))
    return o.detach().numpy(), [x.detach().numpy() for x in g]


def make_params(E, A, seed, hv_scale=4.0):
    """Values on the scale the tolerances were reasoned for: Wa glorot-scaled normal, ba ~ N(0, 0.1^2), hv ~ N(0, 1)
    scaled up so that the softmax is far from uniform; fp32 arrays."""
    r = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32)
    Wa = f32(r.standard_normal((E, A)) * np.sqrt(2.0 / (E + A)))
    ba = f32(r.standard_normal(A) * 0.1)
    hv = f32(r.standard_normal((A, 1)) * hv_scale)
    hv[0, 0] = np.float32(hv_scale) * (1 if hv[0, 0] >= 0 else -1)     # never a vanishing attention vector at A = 1
    bh = f32(r.standard_normal(1) * 0.1)
    return Wa, ba, hv, bh


def make_table(V, E, seed):
    return np.asarray(np.random.default_rng(seed).standard_normal((V, E)) * 0.5, np.float32)


def reference_main_input():
    """ids 0 .. 29 in ten columns (the arange-style input of the reference's docstring examples)."""
    names = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
    return names, np.arange(30, dtype=np.int64).reshape(10, 3).T.copy()
