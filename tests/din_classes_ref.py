"""The kernel classes of DIN's attention (csrc/din.hip) restated for the tests, the table of shapes that reaches every one
of them, and the references the GPU tests compare with.  No GPU and no package import here: numpy and torch on the CPU.

kernel_class() restates the four dispatch rules of rec_din_attn_fwd_f32 / _bwd_f32 and of the kernels' own run-time
switches, read off din.hip:
  NT     = ceil(H / 16), 1..4                                     (template argument, H <= 64)
  ND     = 2 (D <= 32), 6 (D <= 96), 8 (D <= 128), 16 (D <= 256)  (template argument, padded D / 16)
  NPASS  = 2 at ND = 16 (the backward walks the series twice, 8 d tiles of gEff per pass), else 1
  fast   = E a power of two >= 4, ld % 4 == 0 and 4 C E <= 384: 16-byte row pieces with prefetch; else attn_rows_slow
  vec    = D H % 4 == 0, (D H + H) % 4 == 0 and Mext, Wkd 16-byte aligned: float4 loads of Eff with the h_magic division;
           else the scalar loop of attn_load_eff
D > 128 with H > 48 is refused by both directions (the backward's LDS), so (NT, ND) = (4, 16) is no class.

The references: literal_attention() is oracle.torch_ref.din_activation_unit -- the materialised concat unit -- per time
step, then the mask in either mask_valid mode, then the pooling; factorised_attention() is the formula the kernels
implement, pre = c_b + k_t . Eff_b, in plain torch at any dtype: in fp64 it is proved equal to the literal unit by
tests/test_din_classes_host.py, in fp32 it measures what a correct fp32 evaluation loses (the tolerance of the wide
classes).  An id outside [0, V) is a zero key row, as the kernels define it.
"""
import collections
import functools

import numpy as np
import torch

from oracle import torch_ref as T
from tests import helpers as H_

ACTS = ("none", "relu", "tanh", "sigmoid", "dice", "prelu")
OUT_TOL, GRAD_TOL = 1e-5, 3e-5          # tests/test_gpu_din.py: relative to max(1, |ref|max), set at D <= 96
KINK_MARGIN = 1e-4                      # relu / prelu: no reference pre-activation closer to 0 than this


def kernel_class(E, C, H, ld, aligned=True):
    """(NT, ND, NPASS, fast, vec_eff) of a call with embedding width E, C series features, H hidden units and table row
    stride ld; ``aligned``: Mext and Wkd start on 16-byte boundaries."""
    D = E * C
    if not (1 <= D <= 256 and 1 <= H <= 64) or (D > 128 and H > 48):
        raise ValueError("outside the envelope of the DIN attention kernels: D=%d, H=%d" % (D, H))
    NT = (H + 15) // 16
    nd = (D + 15) // 16
    ND = 2 if nd <= 2 else 6 if nd <= 6 else 8 if nd <= 8 else 16
    NPASS = 2 if ND == 16 else 1
    fast = E >= 4 and E & (E - 1) == 0 and ld % 4 == 0 and 4 * C * E <= 384
    vec_eff = bool(aligned) and (D * H) % 4 == 0 and (D * H + H) % 4 == 0
    return NT, ND, NPASS, fast, vec_eff


Case = collections.namedtuple("Case", "name E C H T B V act mask_valid padding_index seed")


def _c(name, E, C, H=36, T=7, B=3, V=97, act="dice", mv=1, pad=0, seed=0):
    return Case(name, E, C, H, T, B, V, act, mv, pad, seed)


def _cases():
    out = [
        # ND = 8: D = 128 exactly, and D = 100 padded to 128
        _c("nd8_d128", 32, 4, T=20, B=4, V=300), _c("nd8_d100", 20, 5, T=7, mv=0),
        # ND = 16, the two-pass backward: one, two tiles and wave 0 with two tiles per pass; a second pass of 8 rows;
        # D no multiple of 16; the largest corner
        _c("nd16_t5", 64, 3, T=5, mv=0), _c("nd16_t20", 64, 3, T=20), _c("nd16_t70", 64, 3, T=70, act="prelu", seed=2),
        _c("nd16_d136", 8, 17, T=18), _c("nd16_d132_h20", 12, 11, H=20, T=9, mv=0), _c("nd16_d256_h48", 64, 4, H=48, T=18),
        # the two (NT, ND) pairs the rows above and below leave out
        _c("nd8_h17", 32, 4, H=17, T=6), _c("nd16_h5", 48, 3, H=5, T=6),
    ]
    for h in (1, 16, 17, 32, 48, 49, 64):                      # NT classes at ND = 2 and ND = 6, fast rows
        out.append(_c("nt_e4_h%d" % h, 4, 3, H=h, T=7, mv=h & 1))
        out.append(_c("nt_e32_h%d" % h, 32, 3, H=h, T=20, mv=1 - (h & 1)))
    out += [_c("nt_nd8_h16", 32, 4, H=16, T=6), _c("nt_nd8_h64", 32, 4, H=64, T=6, mv=0)]
    # the scalar Eff path: D H or D H + H no multiple of 4
    out += [_c("eff_scalar_e3_h6", 3, 3, H=6), _c("eff_scalar_e32_h37", 32, 3, H=37, T=20, mv=0),
            _c("eff_scalar_e2_h2", 2, 3, H=2)]
    # C other than 3 on the fast path (c_magic), two shapes with exactly 384 pieces, and one just past (slow, ND = 8)
    out += [_c("c1_e32", 32, 1), _c("c12_e8", 8, 12, T=18), _c("c24_e4", 4, 24, T=18, mv=0), _c("c5_e16", 16, 5, T=18),
            _c("c25_e4", 4, 25, T=18)]
    # slow rows with E a multiple of 4 that is no power of two
    out.append(_c("slow_e12_t33", 12, 3, T=33, mv=0))
    # tile edges of the slow path (16 steps per wave tile, 64 per round of the workgroup) at ND = 2 and ND = 16
    for t in (1, 15, 16, 17, 63, 65, 129):
        out.append(_c("edge_e3_t%d" % t, 3, 3, T=t, mv=t & 1))
        out.append(_c("edge_e64_t%d" % t, 64, 3, T=t, mv=1 - (t & 1)))
    # every activation at one fast shape and one ND = 16 shape; the seeds of relu / prelu keep the kink margin
    seeds = {("relu", 8): 1, ("prelu", 8): 0, ("relu", 64): 0, ("prelu", 64): 0}
    for act in ACTS:
        out.append(_c("act_%s_e8" % act, 8, 3, T=18, act=act, seed=seeds.get((act, 8), 0)))
        out.append(_c("act_%s_e64" % act, 64, 3, T=18, act=act, mv=0, seed=seeds.get((act, 64), 0)))
    # a padding id other than 0, both mask modes
    out += [_c("pad7_valid", 8, 3, T=18, pad=7, mv=1), _c("pad7_reference", 8, 3, T=18, pad=7, mv=0)]
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}


def series_of(r, B, T_, C, V, padding_index):
    """[B,T,C] ids in [0, V) without the padding id; example 0 is a full series, example 1 all padding, example 2 ends
    inside the last 16-step tile, the others at random (the padding fills all C columns, as padded_batch does)."""
    ids = r.integers(0, V - 1, size=(B, T_, C)).astype(np.int64)
    ids[ids >= padding_index] += 1
    lens = r.integers(1, T_ + 1, size=B)
    lens[0] = T_
    if B > 1:
        lens[1] = 0
    if B > 2:
        last = 16 * ((T_ - 1) // 16)
        lens[2] = last + max(1, (T_ - last) // 2)
    for b in range(B):
        ids[b, lens[b]:, :] = padding_index
    return ids, lens


def make(case):
    """The inputs of one case as numpy arrays (fp32 values, int64 ids), from its seed alone."""
    r = H_.rng(1000 + case.seed)
    E, C, Hh = case.E, case.C, case.H
    D = E * C
    act = {"kind": case.act}
    if case.act in ("dice", "prelu"):
        act["alpha"] = r.uniform(-0.2, 0.3, size=Hh).astype(np.float32)
    if case.act == "dice":
        act["mean"] = r.uniform(-0.1, 0.1, size=Hh).astype(np.float32)
        act["var"] = r.uniform(0.5, 1.5, size=Hh).astype(np.float32)
    if case.act == "none":
        act["kind"] = None
    att = {"W1": H_.glorot(r, 3 * D + D * D, Hh), "b1": r.uniform(-0.1, 0.1, size=Hh).astype(np.float32), "act": act,
           "W2": H_.glorot(r, Hh, 1), "b2": r.uniform(-0.1, 0.1, size=1).astype(np.float32)}
    series, lens = series_of(r, case.B, case.T, C, case.V, case.padding_index)
    return {"embed": r.uniform(-0.5, 0.5, size=(case.V, E)).astype(np.float32), "att": att, "series": series,
            "lens": lens, "q": r.normal(size=(case.B, D)).astype(np.float32),
            "g": r.normal(size=(case.B, D)).astype(np.float32)}


def _keys(embed_t, series, zero_rows):
    """[B,T,D] key rows; zero_rows [B,T,C] bool marks lookups that read as a zero row (ids outside the table)."""
    B, T_, C = series.shape
    ids = torch.from_numpy(series.reshape(B, T_ * C))
    if zero_rows is None:
        return T.lookup(embed_t, ids).reshape(B, T_, C * embed_t.shape[1])
    z = torch.from_numpy(zero_rows.reshape(B, T_ * C))
    rows = T.lookup(embed_t, torch.where(z, torch.zeros_like(ids), ids))
    return (rows * (~z).unsqueeze(-1).to(rows.dtype)).reshape(B, T_, C * embed_t.shape[1])


def _mask(series, padding_index, mask_valid, dtype):
    pad = torch.from_numpy(series[:, :, 0] == padding_index)
    return (~pad if mask_valid else pad).to(dtype)


def literal_attention(embed_t, q_t, series, att_t, padding_index, mask_valid, zero_rows=None):
    """The literal concat unit per time step, the (quirky) mask, the pooling -> (scores [B,T], pooled [B,D], keys)."""
    keys = _keys(embed_t, series, zero_rows)
    sc = torch.stack([T.din_activation_unit(q_t, keys[:, t, :], att_t) for t in range(series.shape[1])],
                     dim=1).squeeze(-1)
    m = _mask(series, padding_index, mask_valid, sc.dtype)
    pooled = (keys * (sc * m).unsqueeze(-1)).sum(1)
    return sc, pooled, keys


def factorised_attention(embed_t, q_t, series, att_t, padding_index, mask_valid, zero_rows=None):
    """pre[b,t,:] = c_b + k_t . Eff_b with Eff_b = (W_k - W_d) + M_b, M_b[i,o] = sum_j q_j W_o[i,j,o] and
    c_b = q (W_q + W_d) + b1, at the dtype of its arguments -> (scores, pooled, keys, pre [B,T,H], Mext [B, D H + H])."""
    B, D = q_t.shape
    W1 = att_t["W1"]
    Hh = W1.shape[1]
    Wq, Wd, Wk, Wo = W1[:D], W1[D:2 * D], W1[2 * D:3 * D], W1[3 * D:].reshape(D, D, Hh)
    M = torch.einsum("bj,ijo->bio", q_t, Wo)
    c = q_t @ (Wq + Wd) + att_t["b1"]
    Mext = torch.cat([M.reshape(B, D * Hh), c], dim=1)
    Eff = (Wk - Wd).unsqueeze(0) + Mext[:, :D * Hh].reshape(B, D, Hh)
    keys = _keys(embed_t, series, zero_rows)
    pre = Mext[:, D * Hh:].unsqueeze(1) + torch.einsum("btd,bdo->bto", keys, Eff)
    sc = (T._din_act(att_t["act"], pre) @ att_t["W2"] + att_t["b2"]).squeeze(-1)
    m = _mask(series, padding_index, mask_valid, sc.dtype)
    pooled = (keys * (sc * m).unsqueeze(-1)).sum(1)
    return sc, pooled, keys, pre, Mext


GRADS = ("q", "embed", "W1", "b1", "W2", "b2", "alpha")


def evaluate(data, padding_index, mask_valid, dtype=torch.float64, form="literal", zero_rows=None):
    """Forward and the gradients of sum(pooled * g) -> {scores, pooled, q, embed, W1, b1, W2, b2, alpha (or None), keys
    (the gradient at the key rows [B,T,D])} as fp64 numpy; the factorised form adds pre and Mext (its gradient)."""
    att = H_.to_torch(data["att"], dtype, True)
    emb = torch.from_numpy(data["embed"]).to(dtype).requires_grad_()
    q = torch.from_numpy(data["q"]).to(dtype).requires_grad_()
    extra = {}
    if form == "literal":
        sc, pooled, keys = literal_attention(emb, q, data["series"], att, padding_index, mask_valid, zero_rows)
    else:
        sc, pooled, keys, pre, Mext = factorised_attention(emb, q, data["series"], att, padding_index, mask_valid,
                                                           zero_rows)
        Mext.retain_grad()
        extra = {"pre": pre, "Mext": Mext}
    keys.retain_grad()
    (pooled * torch.from_numpy(data["g"]).to(dtype)).sum().backward()
    alpha = att["act"].get("alpha")
    out = {"scores": sc, "pooled": pooled, "q": q.grad, "embed": emb.grad, "W1": att["W1"].grad, "b1": att["b1"].grad,
           "W2": att["W2"].grad, "b2": att["b2"].grad, "alpha": None if alpha is None else alpha.grad,
           "keys": keys.grad}
    if extra:
        out["pre"] = extra["pre"]
        out["Mext"] = extra["Mext"].grad
    return {k: None if v is None else v.detach().double().numpy() for k, v in out.items()}


@functools.lru_cache(maxsize=None)
def reference(name, form="literal", dtype=torch.float64):
    """evaluate() of a row of CASES, computed once per process; the arrays are shared: do not write to them."""
    case = BY_NAME[name]
    out = evaluate(make(case), case.padding_index, case.mask_valid, dtype, form)
    for v in out.values():
        if v is not None:
            v.setflags(write=False)
    return out


def rel_err(got, want):
    """max |got - want| relative to max(1, |want|max): the measure of tests/test_gpu_din.py."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / max(1.0, np.abs(want).max()))


def fp32_error(name):
    """(outputs, gradients): the worst rel_err of the fp32 factorised restatement against the fp64 literal unit."""
    ref, f32 = reference(name), reference(name, "factorised", torch.float32)
    out = max(rel_err(f32[k], ref[k]) for k in ("scores", "pooled"))
    grad = max(rel_err(f32[k], ref[k]) for k in GRADS if ref[k] is not None)
    return out, grad


def wide(case):
    """The classes beyond the D <= 96 at which the project's tolerances were set: ND = 8 and ND = 16."""
    return kernel_class(case.E, case.C, case.H, case.E)[1] >= 8


def tolerances(name):
    """(outputs, gradients) bound of a case.  For a wide case it is the larger of the project's figure and 4 x
    fp32_error(); measured (the table in tests/test_gpu_din_classes.py), 4 x the fp32 error stays below the project's
    figures in every case, which tests/test_din_classes_host.py asserts, so the figures are the bound everywhere."""
    assert name in BY_NAME
    return OUT_TOL, GRAD_TOL
