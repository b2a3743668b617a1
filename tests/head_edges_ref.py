"""Inputs and restatements for the tests of the saturated, clipped and clamped model heads
(tests/test_gpu_head_edges.py on the GPU, tests/test_head_edges_host.py without one).  numpy / torch-CPU only.

Every construction is deterministic (fixed seeds).  Ordinary ids of an example are redrawn until the fp64 oracle puts
the example where the test wants it, so that an fp32 kernel and the fp64 oracle take the same branch everywhere:

  clip band   fp64 p is "live" (1e-4 <= p <= 1 - 1e-4) or "clipped" (p <= 1e-8 or 1 - p <= 1e-8), nothing in between:
              fl32(1 - 1e-7) = 1 - 2^-23, so the fp32 and fp64 clip edges differ, and fp32 p (1 - p) loses its digits
              for 9 < |z| < 17 -- in TF's fp32 as much as in the kernels';
  ReLU kinks  a hidden pre-activation is >= 2e-5 away from 0, or exactly 0.0 by construction (zero weights and bias);
              the pre-activations of a "dead" example are <= -1 (or exactly 0.0);
  norm clamp  sum x^2 of a tower output is >= 1e-6, exactly 0, or in [1e-16, 1e-14]: nothing near 1e-12.
"""
import functools

import numpy as np

from oracle import layers_np as L
from tests import helpers as H

KINK = 2e-5                     # the margin avoid_kinks of tests/test_gpu_dssm_fused.py uses
LIVE_P, CLIP_P = 1e-4, 1e-8
Z_LIVE, Z_CLIP = 9.2, 18.5      # |z| <= 9.2 <=> live, |z| >= 18.5 <=> clipped
NSPEC = 8                       # ids 0..7 of every field (DeepFM) / table (DSSM) are reserved for the special rows

# ------------------------------------------------------------------------------------------------
# fused DeepFM step
# ------------------------------------------------------------------------------------------------
DFM_F, DFM_E, DFM_V = 5, 16, 3000
DFM_NAMES = ["f%d" % i for i in range(DFM_F)]
DFM_DIMS = [DFM_V // DFM_F] * DFM_F
DFM_OFFS = H.field_offsets(DFM_DIMS)
DFM_SETS = ("mixed", "dead2", "zero1")
W_SAT, W_CONF, C_DEAD = 25.0, 6.5, 2.0
# categories of the mixed batch
LIVE, SAT_HI, SAT_LO, DEAD1 = 0, 1, 2, 3
# special ids (local to their field): column 0 -- w rows; column 1 -- embedding rows of -C_DEAD
SAT_HI_IDS, SAT_LO_IDS, CONF_HI_ID, CONF_LO_ID = (0, 1), (2, 3), 4, 5
DEAD1_IDS = (0, 1)


@functools.lru_cache(maxsize=None)
def deepfm_params(kind):
    """'mixed': K0 >= 0 entrywise, special rows.  'dead2': also K1 = 0 and b1 <= -1 (h2 = 0 exactly).  'zero1': K0 = 0 and
    b0 = 0 (every first-layer pre-activation is exactly 0.0; relu'(0) = 0)."""
    assert kind in DFM_SETS
    p = H.deepfm_params(7, DFM_V, DFM_F, DFM_E)
    p["embed"] = p["embed"] * np.float32(6.0)
    p["k1"][0] = np.abs(p["k1"][0])
    o0, o1 = DFM_OFFS[0], DFM_OFFS[1]
    for j in SAT_HI_IDS:
        p["w"][o0 + j] = W_SAT
    for j in SAT_LO_IDS:
        p["w"][o0 + j] = -W_SAT
    p["w"][o0 + CONF_HI_ID] = W_CONF
    p["w"][o0 + CONF_LO_ID] = -W_CONF
    for j in DEAD1_IDS:
        p["embed"][o1 + j] = -C_DEAD
    if kind == "dead2":
        p["k1"][1] = np.zeros_like(p["k1"][1])
        p["b1"][1] = (-1.0 - np.abs(p["b1"][1])).astype(np.float32)
    if kind == "zero1":
        p["k1"][0] = np.zeros_like(p["k1"][0])
        p["b1"][0] = np.zeros_like(p["b1"][0])
    return p


def deepfm_state(p):
    """The parameters under the names DeepFMRankingLayer gives them."""
    return {"embed.embeddings": p["embed"], "w.embeddings": p["w"], "bias": p["bias"],
            "MLP_layer1.kernel_0": p["k1"][0], "MLP_layer1.bias_0": p["b1"][0],
            "MLP_layer1.kernel_1": p["k1"][1], "MLP_layer1.bias_1": p["b1"][1],
            "MLP_layer2.kernel_0": p["k2"][0], "MLP_layer2.bias_0": p["b2"][0]}


def deepfm_fp64(p, X):
    """fp64 oracle: z [B], p [B], first- and second-layer pre-activations [B,32], [B,8]."""
    prob, z, (_, _, s1, _) = L.deepfm_forward(p, X, np.float64, keep=True)
    return z[:, 0], prob[:, 0], s1[0][1], s1[1][1]


def _kink_ok(pre):
    return ((np.abs(pre) >= KINK) | (pre == 0.0)).all(axis=1)


def _deepfm_settle(p, X, special, ok_z, seed):
    """Redraw the ordinary ids (``~special``) of the examples the fp64 oracle does not put where ``ok_z(z)`` wants them
    or puts within KINK of a ReLU kink."""
    r = H.rng(seed)
    for _ in range(200):
        z, _, pre1, pre2 = deepfm_fp64(p, X)
        bad = ~(ok_z(z) & _kink_ok(pre1) & _kink_ok(pre2))
        if not bad.any():
            return X
        for f in range(DFM_F):
            m = bad & ~special[:, f]
            X[m, f] = DFM_OFFS[f] + r.integers(NSPEC, DFM_DIMS[f], size=int(m.sum()))
    raise AssertionError("could not settle the batch")


def _as_batch(X, y):
    b = {n: X[:, f:f + 1].copy() for f, n in enumerate(DFM_NAMES)}
    b["label"] = y.reshape(-1, 1).astype(np.float32)
    return b


@functools.lru_cache(maxsize=None)
def deepfm_mixed(kind, B):
    """The mixed batch: example e has category e % 4 (live, saturated high, saturated low, dead first layer); the last
    three examples -- the partial half of the last workgroup -- are saturated low, dead, saturated high.  Saturated
    examples alternate their label, so all four (sign, label) combinations occur.  Returns (batch, X, cat)."""
    p = deepfm_params(kind)
    r = H.rng(100 + B)
    cat = np.arange(B) % 4
    cat[B - 3:] = (SAT_LO, DEAD1, SAT_HI)
    X = np.stack([DFM_OFFS[f] + r.integers(NSPEC, DFM_DIMS[f], size=B) for f in range(DFM_F)], axis=1).astype(np.int64)
    special = np.zeros((B, DFM_F), bool)
    alt = (np.arange(B) // 4) % 2
    X[cat == SAT_HI, 0] = DFM_OFFS[0] + np.take(SAT_HI_IDS, alt[cat == SAT_HI])
    X[cat == SAT_LO, 0] = DFM_OFFS[0] + np.take(SAT_LO_IDS, alt[cat == SAT_LO])
    X[cat == DEAD1, 1] = DFM_OFFS[1] + np.take(DEAD1_IDS, alt[cat == DEAD1])
    special[(cat == SAT_HI) | (cat == SAT_LO), 0] = True
    special[cat == DEAD1, 1] = True
    y = (r.random(B) < 0.3).astype(np.float32)
    sat = (cat == SAT_HI) | (cat == SAT_LO)
    y[sat] = ((np.arange(B) // 8) % 2)[sat]
    y[B - 3], y[B - 1] = 1.0, 0.0                      # the tail: a clipped example on the wrong side of its label, each way
    ok = lambda z: np.where(cat == SAT_HI, z >= Z_CLIP, np.where(cat == SAT_LO, z <= -Z_CLIP, np.abs(z) <= Z_LIVE))  # noqa: E731
    X = _deepfm_settle(p, X, special, ok, 200 + B)
    return _as_batch(X, y), X, cat


@functools.lru_cache(maxsize=None)
def deepfm_confident(B):
    """4 <= |z| <= 9.2 for every example and label = (z > 0): a loss of order 1e-3."""
    p = deepfm_params("mixed")
    r = H.rng(300 + B)
    X = np.stack([DFM_OFFS[f] + r.integers(NSPEC, DFM_DIMS[f], size=B) for f in range(DFM_F)], axis=1).astype(np.int64)
    X[:, 0] = DFM_OFFS[0] + np.where(r.random(B) < 0.5, CONF_HI_ID, CONF_LO_ID)
    special = np.zeros((B, DFM_F), bool)
    special[:, 0] = True
    X = _deepfm_settle(p, X, special, lambda z: (np.abs(z) >= 4.0) & (np.abs(z) <= Z_LIVE), 400 + B)
    z = deepfm_fp64(p, X)[0]
    return _as_batch(X, (z > 0).astype(np.float32)), X


def gz_fp32(y, prob):
    """The fused kernel's d loss / d z restated op for op in fp32 on the kernel's OWN probabilities."""
    y = np.asarray(y, np.float32).reshape(-1)
    p = np.asarray(prob, np.float32).reshape(-1)
    return L.bce_backward(y, p, np.float32) * p * (np.float32(1) - p)


# ------------------------------------------------------------------------------------------------
# fused DSSM step
# ------------------------------------------------------------------------------------------------
UN, IN = ["user_tag1", "user_tag2"], ["item_tag1", "item_tag2", "item_tag3"]
DSSM_E, DSSM_VU, DSSM_VI = 16, 1500, 2500
DSSM_CASES = ("equal", "opposite", "u_zero", "u_tiny", "both_zero")
DD, DL, LD, LL = 0, 1, 2, 3      # dead user / dead item, dead / live, live / dead, live / live
DD_ID, DX_ID = 0, 1              # special id of the dead/dead examples; of a dead tower beside a live one


@functools.lru_cache(maxsize=None)
def dssm_params(case):
    """Both towers: K0 >= 0, K1 >= 0, b1 <= -1, embedding rows 0..NSPEC-1 = -C_DEAD, ordinary rows in (-0.5, 1): an
    example whose every field picks a special id has h1 = 0, h2 = 0 and tower output bf exactly."""
    assert case in DSSM_CASES
    out = []
    for seed, V, F in ((5, DSSM_VU, len(UN)), (6, DSSM_VI, len(IN))):
        p = H.tower_params(seed, V, F, DSSM_E)
        r = H.rng(50 + seed)
        p["embed"] = r.uniform(-0.5, 1.0, size=(V, DSSM_E)).astype(np.float32)
        p["embed"][:NSPEC] = -C_DEAD
        p["mlp_k"] = [np.abs(k) for k in p["mlp_k"]]
        p["mlp_b"][1] = (-1.0 - np.abs(p["mlp_b"][1])).astype(np.float32)
        out.append(p)
    r = H.rng(60)
    v = r.uniform(0.2, 1.0, size=8) * np.where(r.random(8) < 0.5, -1, 1)
    bu, bi = {"equal": (v, v), "opposite": (v, -v), "u_zero": (0 * v, v),
              "u_tiny": (1e-8 * r.normal(size=8), v), "both_zero": (0 * v, 0 * v)}[case]
    out[0]["final_b"] = [bu.astype(np.float32)]
    out[1]["final_b"] = [bi.astype(np.float32)]
    return tuple(out)


def dssm_state(pu, pi):
    """The parameters under the names DSSMTwoTowerRetrievalLayer gives them."""
    sd = {}
    for t, p in (("u_tower", pu), ("i_tower", pi)):
        sd[t + ".embed.embeddings"] = p["embed"]
        for n, v in zip(["mlp.kernel_0", "mlp.bias_0", "mlp.kernel_1", "mlp.bias_1", "final.kernel_0", "final.bias_0"],
                        [p["mlp_k"][0], p["mlp_b"][0], p["mlp_k"][1], p["mlp_b"][1], p["final_k"][0], p["final_b"][0]]):
            sd[t + "." + n] = v
    return sd


def dssm_fp64(p, X):
    """One tower in fp64: pre-activations [B,64], [B,32] and the output [B,8]."""
    x = p["embed"][X].astype(np.float64).reshape(X.shape[0], -1)
    z1 = x @ p["mlp_k"][0].astype(np.float64) + p["mlp_b"][0]
    z2 = np.maximum(z1, 0) @ p["mlp_k"][1].astype(np.float64) + p["mlp_b"][1]
    return z1, z2, np.maximum(z2, 0) @ p["final_k"][0].astype(np.float64) + p["final_b"][0]


def dssm_X(batch):
    return (np.stack([batch[n].reshape(-1) for n in UN], axis=1), np.stack([batch[n].reshape(-1) for n in IN], axis=1))


@functools.lru_cache(maxsize=None)
def dssm_batch(case, B):
    """Example e has category e % 4 (DD, DL, LD, LL); the last example -- alone in its workgroup tail -- is dead/dead.
    Returns (batch, cat)."""
    pu, pi = dssm_params(case)
    r = H.rng(500 + B)
    cat = np.arange(B) % 4
    cat[B - 1] = DD
    dead_u, dead_i = (cat == DD) | (cat == DL), (cat == DD) | (cat == LD)
    Xu = r.integers(NSPEC, DSSM_VU, size=(B, len(UN))).astype(np.int64)
    Xi = r.integers(NSPEC, DSSM_VI, size=(B, len(IN))).astype(np.int64)
    Xu[dead_u], Xi[dead_i] = DX_ID, DX_ID
    Xu[cat == DD], Xi[cat == DD] = DD_ID, DD_ID
    y = (r.random((B, 1)) < 0.3).astype(np.float32)
    y[cat == DD] = ((np.arange(B) // 4) % 2).reshape(B, 1)[cat == DD]      # clipped examples on both sides of their label
    for _ in range(200):
        z1u, z2u, ou = dssm_fp64(pu, Xu)
        z1i, z2i, oi = dssm_fp64(pi, Xi)
        s = L.two_tower_score(ou, oi, np.float64)
        bad_u = ~(_kink_ok(z1u) & _kink_ok(z2u)) & ~dead_u
        bad_i = ~(_kink_ok(z1i) & _kink_ok(z2i)) & ~dead_i
        band = ~((s >= LIVE_P) & (s <= 1 - LIVE_P))              # (a dead/dead example is never redrawn)
        bad_u |= band & ~dead_u
        bad_i |= band & ~dead_i
        if not (bad_u.any() or bad_i.any()):
            break
        Xu[bad_u] = r.integers(NSPEC, DSSM_VU, size=(int(bad_u.sum()), len(UN)))
        Xi[bad_i] = r.integers(NSPEC, DSSM_VI, size=(int(bad_i.sum()), len(IN)))
    else:
        raise AssertionError("could not settle the batch")
    b = {n: Xu[:, j].copy() for j, n in enumerate(UN)}
    b.update({n: Xi[:, j].copy() for j, n in enumerate(IN)})
    b["label"] = y
    return b, cat


# ------------------------------------------------------------------------------------------------
# the unfused kernels
# ------------------------------------------------------------------------------------------------
GRID = np.array([0.0] + [s * v for v in (1e-6, 1.0, 9.0, 17.0, 20.0, 88.0, 89.0, 104.0, 1e4) for s in (1, -1)], np.float32)
COS_GROUPS = ("u_zero", "i_zero", "both_zero", "u_tiny", "parallel", "antiparallel", "ordinary", "mixed")


def sigmoid64(x):
    """fp64 sigmoid without overflow warnings."""
    x = np.asarray(x, np.float64)
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1 / (1 + e), e / (1 + e))


def cosine_rows(d, seed=0):
    """64 rows in 8 groups of 8 (COS_GROUPS): u = 0, i = 0, both 0, |u|^2 ~ 1e-15, u = 3 i, u = -2 i, ordinary, and one
    row of each of the other seven kinds plus an ordinary one."""
    r = H.rng(1000 + d + seed)
    u = r.normal(size=(64, d)).astype(np.float32)
    i = r.normal(size=(64, d)).astype(np.float32)

    def put(row, kind):
        if kind in ("u_zero", "both_zero"):
            u[row] = 0
        if kind in ("i_zero", "both_zero"):
            i[row] = 0
        if kind == "u_tiny":
            u[row] = (u[row] / np.linalg.norm(u[row].astype(np.float64)) * 3e-8).astype(np.float32)
        if kind == "parallel":
            u[row] = 3 * i[row]
        if kind == "antiparallel":
            u[row] = -2 * i[row]
    for g, kind in enumerate(COS_GROUPS[:7]):
        for row in range(8 * g, 8 * g + 8):
            put(row, kind)
    for j, kind in enumerate(COS_GROUPS[:7]):
        put(56 + j, kind)
    return u, i


def softmax_rows(N, seed=0):
    """5 rows: x + 1e4, x - 1e4, spread 200, all equal, one entry 1e3 above the rest."""
    r = H.rng(2000 + N + seed)
    x = r.normal(size=(5, N)).astype(np.float32)
    x[0] += 1e4
    x[1] -= 1e4
    x[2] = r.uniform(-100, 100, size=N)
    if N >= 2:
        x[2, 0], x[2, -1] = 100, -100
    x[3] = 0.37
    x[4, N // 2] += 1e3
    return x


def norm_conditioning(x, axis):
    """max|x| / std along ``axis`` (1 where the std is 0), at least 1: the conditioning of x -> (x - mean) / std.  One
    fp32 rounding of a value of size max|x| is a relative error of 2^-24 * max|x| / std in x - mean, so a tolerance that
    holds for well-conditioned rows (max|x| ~ std) holds for an ill-conditioned one when it is scaled by this factor."""
    x = np.asarray(x, np.float64)
    sd = x.std(axis=axis)
    return np.maximum(1.0, np.abs(x).max(axis=axis) / np.where(sd > 0, sd, np.abs(x).max(axis=axis) + 1e-300))
