"""Host tests of the constructions of tests/head_edges_ref.py (the conditions under which comparing an fp32 kernel
with the fp64 oracle is meaningful: both take the same branch for every example) and of the corrected
oracle.layers_np.two_tower_score_backward against torch fp64 autograd."""
import numpy as np
import pytest
import torch

from oracle import layers_np as L
from oracle import torch_ref as T
from tests import head_edges_ref as R


def _band(p):
    live = (p >= R.LIVE_P) & (p <= 1 - R.LIVE_P)
    clipped = (p <= R.CLIP_P) | (1 - p <= R.CLIP_P)
    return live, clipped


def _kinks(pre):
    return ((np.abs(pre) >= R.KINK) | (pre == 0.0)).all()


@pytest.mark.parametrize("B", [200, 33])
@pytest.mark.parametrize("kind", R.DFM_SETS)
def test_deepfm_mixed_batch_conditions(kind, B):
    p = R.deepfm_params(kind)
    batch, X, cat = R.deepfm_mixed(kind, B)
    y = batch["label"][:, 0]
    assert X.shape == (B, R.DFM_F)
    for f in range(R.DFM_F):                                    # every id inside its field
        assert X[:, f].min() >= R.DFM_OFFS[f] and X[:, f].max() < R.DFM_OFFS[f] + R.DFM_DIMS[f]
    z, prob, pre1, pre2 = R.deepfm_fp64(p, X)
    live, clipped = _band(prob)
    assert (live | clipped).all()
    sat = (cat == R.SAT_HI) | (cat == R.SAT_LO)
    assert np.array_equal(clipped, sat) and (np.abs(z[sat]) >= R.Z_CLIP).all() and (np.abs(z[~sat]) <= R.Z_LIVE).all()
    assert (z[cat == R.SAT_HI] > 0).all() and (z[cat == R.SAT_LO] < 0).all()
    assert _kinks(pre1) and _kinks(pre2)
    if kind == "zero1":
        assert not pre1.any()
    else:
        assert (pre1[cat == R.DEAD1] <= -1).all()
        assert (pre1[cat == R.LIVE] > 0).any(axis=1).sum() >= 8    # (K0 >= 0: a few ordinary examples are dead as well)
    if kind == "dead2":
        assert (pre2 <= -1).all()
    # at least 8 examples of every category, all four (saturation sign, label) combinations, a degenerate tail
    for c in (R.LIVE, R.SAT_HI, R.SAT_LO, R.DEAD1):
        assert (cat == c).sum() >= 8
    for c in (R.SAT_HI, R.SAT_LO):
        for lab in (0.0, 1.0):
            assert ((cat == c) & (y == lab)).sum() >= 2
    assert list(cat[B - 3:]) == [R.SAT_LO, R.DEAD1, R.SAT_HI] and B % 16 != 0      # the last half of 16 is partial
    assert y[B - 3] == 1.0 and y[B - 1] == 0.0                   # clipped on the wrong side of the label, both ways
    # the special ids of column 0 are touched by clipped examples only, those of column 1 by dead examples only
    spec0 = X[:, 0] - R.DFM_OFFS[0] < 4
    spec1 = X[:, 1] - R.DFM_OFFS[1] < R.NSPEC
    assert np.array_equal(spec0, sat) and np.array_equal(spec1, cat == R.DEAD1)
    assert ((X - np.asarray(R.DFM_OFFS))[:, 2:] >= R.NSPEC).all()


def test_deepfm_confident_batch_conditions():
    p = R.deepfm_params("mixed")
    batch, X = R.deepfm_confident(200)
    z, prob, pre1, pre2 = R.deepfm_fp64(p, X)
    assert (np.abs(z) >= 4.0).all() and (np.abs(z) <= R.Z_LIVE).all()
    assert np.array_equal(batch["label"][:, 0], (z > 0).astype(np.float32))
    assert (z > 0).sum() >= 8 and (z < 0).sum() >= 8
    assert _kinks(pre1) and _kinks(pre2)
    loss = L.bce_forward(batch["label"], prob.reshape(-1, 1), np.float64)
    assert 1e-4 <= loss <= 5e-3


@pytest.mark.parametrize("B", [200, 33])
@pytest.mark.parametrize("case", R.DSSM_CASES)
def test_dssm_batch_conditions(case, B):
    pu, pi = R.dssm_params(case)
    batch, cat = R.dssm_batch(case, B)
    Xu, Xi = R.dssm_X(batch)
    assert Xu.min() >= 0 and Xu.max() < R.DSSM_VU and Xi.min() >= 0 and Xi.max() < R.DSSM_VI
    for c in (R.DD, R.DL, R.LD, R.LL):
        assert (cat == c).sum() >= 8
    assert cat[B - 1] == R.DD
    assert set(batch["label"][cat == R.DD, 0]) == {0.0, 1.0}
    dead_u, dead_i = (cat == R.DD) | (cat == R.DL), (cat == R.DD) | (cat == R.LD)
    outs = []
    for p, X, dead in ((pu, Xu, dead_u), (pi, Xi, dead_i)):
        for k in p["mlp_k"]:
            assert (k >= 0).all()
        assert (p["mlp_b"][1] <= -1).all()
        z1, z2, o = R.dssm_fp64(p, X)
        assert (z1[dead] <= -1).all() and (z2[dead] <= -1).all()
        assert np.array_equal(o[dead], np.broadcast_to(p["final_b"][0].astype(np.float64), o[dead].shape))
        assert _kinks(z1[~dead]) and _kinks(z2[~dead])
        assert (z2[~dead] > 0).any(axis=1).all()                # a live example has live units in front of its output
        ss = np.square(o).sum(axis=1)
        assert ((ss >= 1e-6) | (ss == 0) | ((ss >= 1e-16) & (ss <= 1e-14))).all()
        assert (ss[~dead] >= 1e-6).all()
        outs.append((o, ss))
        # the special ids: DD_ID by dead/dead examples only, DX_ID by the other dead examples only
        assert np.array_equal((X == R.DD_ID).any(axis=1), cat == R.DD)
        assert np.array_equal((X == R.DX_ID).any(axis=1), dead & (cat != R.DD))
    s = L.two_tower_score(outs[0][0], outs[1][0], np.float64)
    live, clipped = _band(s)
    assert (live | clipped).all()
    dd = cat == R.DD
    assert live[~dd].all()
    ssu, ssi = outs[0][1][dd], outs[1][1][dd]
    if case == "equal":
        assert (s[dd] <= R.CLIP_P).all()
    elif case == "opposite":
        assert (1 - s[dd] <= R.CLIP_P).all()
    elif case == "u_zero":
        assert not ssu.any() and (ssi >= 1e-6).all() and (s[dd] == 0.5).all()
    elif case == "u_tiny":
        assert ((ssu >= 1e-16) & (ssu <= 1e-14)).all() and live[dd].all()
    else:
        assert not ssu.any() and not ssi.any() and (s[dd] == 0.5).all()


def test_cosine_rows_hold_what_they_claim():
    for d in (8, 5, 64):
        u, i = R.cosine_rows(d)
        su = np.square(u.astype(np.float64)).sum(1)
        si = np.square(i.astype(np.float64)).sum(1)
        assert not su[0:8].any() and not si[8:16].any() and not su[16:24].any() and not si[16:24].any()
        assert ((su[24:32] >= 1e-16) & (su[24:32] <= 1e-14)).all()
        assert np.array_equal(u[32:40], 3 * i[32:40]) and np.array_equal(u[40:48], -2 * i[40:48])
        assert (su[32:56] >= 1e-6).all() and (si[24:56] >= 1e-6).all() and (si[0:8] >= 1e-6).all()
        # the mixed group: one row of each kind, then an ordinary one
        assert not su[56] and not si[57] and not su[58] and not si[58] and 1e-16 <= su[59] <= 1e-14
        assert np.array_equal(u[60], 3 * i[60]) and np.array_equal(u[61], -2 * i[61]) and min(su[62:].min(), si[59:].min()) >= 1e-6


def _torch_score_grads(u, i, g):
    ut = torch.from_numpy(u).double().requires_grad_()
    it = torch.from_numpy(i).double().requires_grad_()
    (T.two_tower_score(ut, it) * torch.from_numpy(g).double()).sum().backward()
    return ut.grad.numpy(), it.grad.numpy()


@pytest.mark.parametrize("d", [8, 5, 64])
def test_two_tower_score_backward_matches_autograd_under_the_clamp(d):
    """Zero, tiny (0 < |u|^2 < 1e-12: clamp active with a non-zero vector -- no projection term), parallel, antiparallel
    and ordinary rows, group by group so that the 1e6-scaled rows do not hide the ordinary ones."""
    u, i = R.cosine_rows(d)
    g = R.H.rng(d).normal(size=64).astype(np.float32)
    gu, gi = L.two_tower_score_backward(u, i, g, np.float64)
    ru, ri = _torch_score_grads(u, i, g)
    for k in range(8):
        rows = slice(8 * k, 8 * k + 8)
        for got, want in ((gu[rows], ru[rows]), (gi[rows], ri[rows])):
            if R.COS_GROUPS[k] in ("parallel", "antiparallel"):
                # cos = +-1 up to rounding: the exact gradient is 0 and both sides return rounding residue of their own
                # -- bounded by a few fp64 ulps of the terms that cancel, |g| / (2 |u|)
                assert np.abs(got - want).max() <= 1e-12 * np.abs(g[rows]).max() / np.sqrt(np.square(u[rows]).sum(1)).min()
            else:
                assert np.abs(got - want).max() <= 1e-12 * max(np.abs(want).max(), 1e-300)
    # the tiny rows are where the two forms differ: the projection term would change the gradient
    t = slice(24, 32)
    nu = 1e-6
    c = ((u[t].astype(np.float64) / nu) * (i[t] / np.linalg.norm(i[t].astype(np.float64), axis=1, keepdims=True))).sum(1)
    assert np.abs(c).max() > 1e-3
