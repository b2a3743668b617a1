"""Every kernel family of ``ops`` under the allocation seam of tests/guarded.py: kernels stay inside their buffers and read
only what they wrote.

A DRIVER builds the device inputs of one family outside the guarded block (the generators of tests/*_ref.py and of the
family's GPU test file) and, inside it, calls only ``ops.*``: the forward, then the backward fed from the forward's saved
tensors; it returns every tensor handed back to the caller, saved ones included, and declares the
``rec_*_workspace_bytes`` queries it must be seen to call (tests/test_guarded_host.py holds their union to the text of
ops.py).  Per driver and case, test_guards_and_poison:

  1. runs plain                              -> want
  2. runs under guarded(ops, 0xFF)           -> guards intact, the declared queries called, at least one allocation seen,
                                                every float finite, everything bit-equal to want
  3. runs under guarded(ops, 0x7F)           -> guards intact, bit-equal to 2.
  4. the inputs are bit-equal to clones taken before 1.

The cases are the smallest at which bounds or slice logic can go wrong: a family's smallest listed case, its tile + 1
batches (17 and 33: both, whatever the family's tile), T = 65 / Ns = 65 for the series kernels, and B = 513 and B = 4097 at
the family's smallest non-trivial widths wherever a backward adds partials over the batch.  513 gives the small
weight-gradient launch of csrc/tile_ops.h two slices of unequal length (288 + 225) and the split-K GEMM two of 257 + 256;
4097 gives it mb_small_split = 16 slices of per = 288 examples, 15 x 288 = 4320 >= 4097: slice 14 holds 65 examples and
slice 15 none.  4097 = 17 x 241 has no factor 2, so every other family's scheme, which cuts the batch into tiles of 16 or
32 examples or strides a capped grid over it (MIND / ComiRec: at most 1024 workgroups, none of them without an example
once B >= 1024), gets a partial trailing tile; no family has a formula under which a smaller batch than 4097 is needed for
that.

Elements a call leaves unspecified are masked only where include/mi355rec.h says so:
  FiBiNet++ input stage: with Fk = 0 ops hands back a placeholder rstd_ln [B, 1], with Fc = 0 an rstd_bn [E] nothing
  fills; the header (the paragraph above rec_emb_fibinetplus_in_workspace_bytes: "rstd_bn [E] (Fc > 0) and rstd_ln
  [B, Fk] (Fk > 0)") has no such buffer then.

Measured on the MI355X: 176 passed in 3.6 s; the slowest test 0.60 s (the first one, which loads the library), every
other at most 0.12 s.  With `small_dw_kernel` of csrc/tile_ops.h changed, in a scratch build, to skip its store where the
slice is empty (`b0 >= b1`), the four B = 4097 cases of mmoe and ple fail step 2 ("returned tensor 11 (3, 5, 3) holds
poison or a non-finite value": dWe2) and the other 43 cases of the five csrc/tile_ops.h families pass; the fp64 parity
tests then fail at B = 4097 as well (dWe2 off by 0.57 against a bound of 3e-05) and pass at every B <= 2049.
"""
import numpy as np
import pytest
import torch

from tests import guarded as G

pytestmark = pytest.mark.gpu

F32 = np.float32


def cu(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


class Driver:
    """``build(case)`` -> the inputs (a tree of device tensors and plain values), ``run(ops, inputs, case)`` -> the tree
    of returned tensors; ``queries`` the workspace queries a run must call"""

    def __init__(self, name, queries, cases, build, run):
        self.name, self.queries, self.cases, self.build, self.run = name, tuple(queries), list(cases), build, run


def case_id(case):
    def s(v):
        if isinstance(v, (tuple, list)):
            return "-".join(s(x) for x in v)
        return str(int(v)) if isinstance(v, (bool, np.integer)) else str(v)
    return "x".join(s(v) for v in case)


# ---- CIN --------------------------------------------------------------------------------------------------------------
def cin_build(case):
    from tests.test_gpu_xdeepfm import make_inputs
    B, F, E, cin = case
    x0, Ws, g = make_inputs(B, F, E, list(cin), seed=B + F + E)
    return cu(x0), [cu(w) for w in Ws], cu(g)


def cin_run(ops, inp, case):
    x0, Ws, g = inp
    part, states = ops.cin_fwd(x0, Ws)
    return part, states, ops.cin_bwd(x0, states, g, Ws)


# ---- FiBiNet ----------------------------------------------------------------------------------------------------------
def fibinet_build(case):
    from tests.test_gpu_fibinet import make_inputs
    B, F, E, C, mid, btype = case
    return [cu(a) for a in make_inputs(B, F, E, C, mid, btype, seed=B + F + E)]


def fibinet_run(ops, inp, case):
    x, xc, S0, S1, W, g = inp
    code = ops.FIBINET_TYPES[case[5]]
    out, A, H1 = ops.fibinet_fwd(x, xc, S0, S1, W, code)
    return out, A, H1, ops.fibinet_bwd(x, g, A, H1, S0, S1, W, code)


# ---- AutoInt ----------------------------------------------------------------------------------------------------------
def autoint_build(case):
    from tests.test_gpu_autoint import make_inputs
    B, Fc, C, E, H, res, scaling = case
    return [cu(a) for a in make_inputs(B, Fc, C, E, H, res, seed=B + Fc + E)]


def autoint_run(ops, inp, case):
    x, xc, ce, Wq, Wk, Wv, Wr, dy = inp
    B, Fc, C, E, H, res, scaling = case
    xc, ce = (xc, ce) if C else (None, None)
    Wr = Wr if res == 2 else None
    y, stats, o = ops.autoint_fwd(x, Wq, Wk, Wv, Wr, H, res, scaling, xc, ce, want_o=True)
    return y, stats, o, ops.autoint_bwd(x, Wq, Wk, Wv, Wr, y, dy, stats, H, res, scaling, xc, ce)


# ---- AFM --------------------------------------------------------------------------------------------------------------
def afm_build(case):
    from tests.test_gpu_afm import make_inputs
    B, F, E, A = case
    table, X, Wa, ba, hv, bh, do = make_inputs(B, F, E, A, 5000, seed=B + F + E + A)
    return cu(table), cu(X, np.int64), cu(Wa), cu(ba), cu(hv), cu(bh), cu(do)


def afm_run(ops, inp, case):
    table, X, Wa, ba, hv, bh, do = inp
    flag = ops.new_flag(table.device)
    o, stats, rows = ops.emb_afm_fwd(table, X, Wa, ba, hv, bh, flag, want_rows=True)
    return flag, o, stats, rows, ops.emb_afm_bwd(table, X, Wa, ba, hv, bh, o, stats, do, rows)


# ---- CCPM / FGCNN -----------------------------------------------------------------------------------------------------
def ccpm_build(case):
    from tests import ccpm_ref as CR
    from tests.test_gpu_ccpm import make_inputs
    B, F, E, filters, kw = case
    table, X, params, filters, kw, dout = make_inputs(B, F, E, list(filters), list(kw), 5000, seed=B + F)
    return cu(table), cu(X, np.int64), cu(CR.flat_params(params)), cu(dout)


def ccpm_run(ops, inp, case):
    table, X, flat, dout = inp
    filters, kw = list(case[3]), list(case[4])
    flag = ops.new_flag(table.device)
    out, rows = ops.emb_ccpm_fwd(table, X, flat, filters, kw, flag, want_rows=True)
    return flag, out, rows, ops.emb_ccpm_bwd(table, X, flat, filters, kw, dout, rows)


def fgcnn_build(case):
    from tests import ccpm_ref as CR
    from tests.test_gpu_fgcnn import make_inputs
    B, F, E, filters, kw, pws = case
    table, X, params, _, _, _, dps, dd = make_inputs(B, F, E, list(filters), list(kw), list(pws), 5000, seed=B + F)
    return cu(table), cu(X, np.int64), cu(CR.flat_params(params)), [cu(d) for d in dps], cu(dd)


def fgcnn_run(ops, inp, case):
    table, X, flat, dps, dd = inp
    filters, kw, pws = list(case[3]), list(case[4]), list(case[5])
    flag = ops.new_flag(table.device)
    rows, pooled = ops.emb_fgcnn_fwd(table, X, flat, filters, kw, pws, flag)
    return flag, rows, pooled, ops.emb_fgcnn_bwd(rows, flat, filters, kw, pws, dps, dd)


# ---- MaskNet ----------------------------------------------------------------------------------------------------------
def _uniform(r, *shape):
    return r.uniform(-1, 1, shape)


def masknet_ln_build(case):
    from tests import masknet_ref as MR
    B, Fc, Fk, E = case
    r = np.random.default_rng(B * 7 + Fc)
    table, X, values, gamma, beta = MR.make_input(r, B, Fc, Fk, E, 5000)
    F = Fc + Fk
    return (cu(table), cu(X, np.int64), cu(values) if Fk else None, cu(gamma), cu(beta), cu(_uniform(r, B, F * E)),
            cu(_uniform(r, B, F * E)))


def masknet_ln_run(ops, inp, case):
    table, X, values, gamma, beta, dn, de = inp
    flag = ops.new_flag(table.device)
    x_emb, x_norm, stats = ops.emb_masknet_ln_fwd(table, X, values, gamma, beta, flag)
    return flag, x_emb, x_norm, stats, ops.emb_masknet_ln_bwd(x_emb, stats, values, gamma, dn, de)


def masknet_block_build(case):
    from tests import masknet_ref as MR
    B, D, P, O, R = case
    r = np.random.default_rng(B + D)
    p = [cu(a) for a in MR.make_block(r, D, P, O, R)]
    return cu(r.normal(0, 0.5, (B, D))), cu(r.normal(0, 1, (B, P))), p, cu(_uniform(r, B, O))


def masknet_block_run(ops, inp, case):
    xe, v, p, dy = inp
    y, saved = ops.mask_block_fwd(xe, v, *p)
    return y, saved, ops.mask_block_bwd(xe, v, p[0], p[2], p[4], p[6], y, saved, dy)


# ---- ContextNet -------------------------------------------------------------------------------------------------------
def contextnet_in_build(case):
    from tests import contextnet_ref as CR
    B, Fc, Fk, E = case
    r = np.random.default_rng(B * 7 + Fc)
    table, X, values = CR.make_input(r, B, Fc, Fk, E, 5000)
    return cu(table), cu(X, np.int64), cu(values) if Fk else None, cu(_uniform(r, B, (Fc + Fk) * E))


def contextnet_in_run(ops, inp, case):
    table, X, values, dx = inp
    flag = ops.new_flag(table.device)
    return flag, ops.emb_contextnet_in_fwd(table, X, values, flag), ops.emb_contextnet_in_bwd(dx, values, X.shape[1])


def contextnet_block_build(case):
    from tests import contextnet_ref as CR
    B, F, E, R, mode = case
    r = np.random.default_rng(B + F)
    p = [cu(a) for a in CR.make_block(r, F, E, R, mode)]
    if mode != "pointwise":
        p = p[:5] + [None] + p[5:]                        # W2 is None in single mode
    return cu(r.normal(0, 1, (B, F * E))), p, cu(_uniform(r, B, F * E))


def contextnet_block_run(ops, inp, case):
    x, p, dy = inp
    y, saved = ops.contextnet_block_fwd(x, *p)
    return y, saved, ops.contextnet_block_bwd(x, p[0], p[2], p[4], p[5], p[6], saved, dy)


# ---- FiBiNet++ --------------------------------------------------------------------------------------------------------
def fibinetplus_in_build(case):
    from tests import fibinetplus_ref as FR
    B, Fc, Fk, E, training = case
    r = np.random.default_rng(B * 7 + Fc)
    table, X, values, bn, ln = FR.make_input(r, B, Fc, Fk, E, 5000)
    return (cu(table), cu(X, np.int64), cu(values) if Fk else None, [cu(a) for a in bn],
            [cu(a) if Fk else None for a in ln], cu(_uniform(r, B, (Fc + Fk) * E)))


def fibinetplus_in_run(ops, inp, case):
    table, X, values, (g_bn, b_bn, mm0, mv0), (g_ln, b_ln), dx = inp
    training, Fk = case[4], case[2]
    mm, mv = mm0.clone(), mv0.clone()                     # the call's in / out state: a fresh copy per run, returned
    flag = ops.new_flag(table.device)
    x, saved = ops.emb_fibinetplus_in_fwd(table, X, values, g_bn, b_bn, g_ln, b_ln, mm, mv, training, flag)
    back = ops.emb_fibinetplus_in_bwd(dx, values, saved, g_bn, g_ln, X.shape[1], training)
    xhat, rstd_bn, rstd_ln = saved                        # rstd_bn exists for Fc > 0, rstd_ln for Fk > 0 (module docstring)
    saved = (xhat, rstd_bn if case[1] > 0 else None, rstd_ln if Fk > 0 else None)
    return flag, mm, mv, x, saved, back


def fibinetplus_block_build(case):
    from tests import fibinetplus_ref as FR
    B, F, E, Gr, ratio, O, btype = case
    r = np.random.default_rng(B + F)
    p = [cu(a) for a in FR.make_block(r, F, E, Gr, ratio, O, btype)]
    return cu(r.normal(0, 1, (B, F * E))), p, cu(_uniform(r, B, O + F * E))


def fibinetplus_block_run(ops, inp, case):
    x, p, dout = inp
    Gr, code = case[3], ops.FIBINET_TYPES[case[6]]
    out, saved = ops.fibinetplus_block_fwd(x, *p, Gr, code)
    W, Wr, br, gq, bq, S0, b0, g0, be0, S1, b1, g1, be1 = p
    return out, saved, ops.fibinetplus_block_bwd(x, W, Wr, gq, S0, g0, be0, S1, g1, be1, Gr, code, saved, dout)


# ---- MMOE / PLE: the inputs of the parity tests (and their cached fp64 readings) ------------------------------------
def mmoe_build(case):
    from tests.test_gpu_mmoe import dev_case
    return dev_case(*case)


def mmoe_run(ops, inp, case):
    x, w, dout = inp
    out, saved = ops.mmoe_fwd(x, w, case[8], case[9])
    return out, saved, ops.mmoe_bwd(x, w, saved, dout, case[8], case[9])


def ple_build(case):
    from tests.test_gpu_ple import dev_case
    return dev_case(*case)


def ple_run(ops, inp, case):
    from tests import ple_ref as PR
    xin, w, dy, dout = inp
    cfg = PR.level_case(*case)["cfg"]
    y, out, saved = ops.ple_cgc_fwd(xin, w, *cfg)
    return y, out, saved, ops.ple_cgc_bwd(xin, w, saved, y, out, dy, dout, *cfg)


# ---- MIND / ComiRec / CAN ---------------------------------------------------------------------------------------------
def mind_routing_build(case):
    from tests.test_gpu_mind import dev_routing
    return dev_routing(*case)


def mind_routing_run(ops, inp, case):
    tab, ser, S, B0, gout = inp
    flag = ops.new_flag(tab.device)
    return flag, ops.mind_routing_fwd(tab, ser, S, B0, case[6], 0, flag), \
        ops.mind_routing_bwd(tab, ser, S, B0, gout, case[6], 0)


def mind_laa_build(case):
    from tests.test_gpu_mind import dev_laa
    return dev_laa(*case)


def mind_laa_run(ops, inp, case):
    tab, it, m, kv, gout, gloss = inp
    flag = ops.new_flag(tab.device)
    return flag, ops.mind_laa_fwd(tab, it, m, kv, flag), ops.mind_laa_bwd(tab, it, m, kv, gout, gloss)


def comirec_dr_build(case):
    from tests.test_gpu_comirec import dev_dr
    return dev_dr(*case)


def comirec_dr_run(ops, inp, case):
    tab, ser, W, B0, gout = inp
    flag = ops.new_flag(tab.device)
    return flag, ops.comirec_dr_fwd(tab, ser, W, B0, case[6], 0, True, flag), \
        ops.comirec_dr_bwd(tab, ser, W, B0, gout, case[6], 0, True)


def comirec_sa_build(case):
    from tests.test_gpu_comirec import dev_sa
    return dev_sa(*case)


def comirec_sa_run(ops, inp, case):
    tab, ser, W1, W2, pos, gout = inp
    flag = ops.new_flag(tab.device)
    return flag, ops.comirec_sa_fwd(tab, ser, W1, W2, pos, 0, True, flag), \
        ops.comirec_sa_bwd(tab, ser, W1, W2, gout, pos, 0, True)


def comirec_select_build(case):
    from tests.test_gpu_comirec import dev_select
    return dev_select(*case)


def comirec_select_run(ops, inp, case):
    tab, it, m, ginner, gloss, gsel = inp
    flag = ops.new_flag(tab.device)
    chosen, inner, loss = ops.comirec_select_fwd(tab, it, m, flag)
    return flag, chosen, inner, loss, ops.comirec_select_bwd(tab, it, m, chosen, ginner, gloss, gsel)


def can_build(case):
    from tests.test_gpu_can import dev_case
    return dev_case(case[:5])


def can_run(ops, inp, case):
    from tests import can_ref as CR
    feed, inds, iid, fid, gout, gpool = inp
    pooled = bool(case[5])
    flag = ops.new_flag(feed.device)
    res = ops.can_fwd(feed, inds, iid, fid, case[3], case[4], ops.ACT_TANH, CR.PAD, pooled, flag)
    return flag, res, ops.can_bwd(feed, inds, iid, fid, case[3], case[4], ops.ACT_TANH, gpool if pooled else gout, CR.PAD,
                                  pooled)


# ---- the older entry points with a workspace --------------------------------------------------------------------------
def crossnet_build(case):
    B, D, L = case
    r = np.random.default_rng(D + B)
    return cu(r.normal(size=(B, D))), cu(r.normal(0, 0.05, (L, D))), cu(r.normal(0, 0.05, (L, D))), cu(r.normal(size=(B, D)))


def crossnet_run(ops, inp, case):
    x0, w, b, gy = inp
    y, xs = ops.crossnet_vec_fwd(x0, w, b)
    return y, xs, ops.crossnet_vec_bwd(x0, w, xs, gy)


def batchnorm_build(case):
    B, N, training = case
    r = np.random.default_rng(B + N)
    return (cu(r.normal(size=(B, N))), cu(1 + r.normal(0, 0.1, N)), cu(r.normal(0, 0.1, N)), cu(r.normal(0, 0.2, N)),
            cu(0.5 + r.uniform(0, 1, N)), cu(_uniform(r, B, N)))


def batchnorm_run(ops, inp, case):
    x, gamma, beta, mm0, mv0, g = inp
    training = bool(case[2])
    mm, mv = mm0.clone(), mv0.clone()                     # updated in place when training: a fresh copy per run, returned
    y, xhat, rstd = ops.batchnorm_fwd(x, gamma, beta, mm, mv, training)
    return mm, mv, y, xhat, rstd, ops.batchnorm_bwd(g, xhat, rstd, gamma, training)


def l2_rows_build(case):
    from explicit_tf2_recommendation_amd import ops
    n, V, E = case
    r = np.random.default_rng(n + V)
    plan = ops.DedupPlan(cu(r.integers(0, V, n), np.int64), V)
    return cu(r.normal(size=(V, E))), plan, [plan.uniq_ids, plan.seg_start, plan.perm, plan.n_uniq]


def l2_rows_run(ops, inp, case):
    table, plan, _ = inp
    return ops.l2_used_rows(table, plan, 0.01)


def topk_build(case):
    nq, n, d, k = case
    r = np.random.default_rng(nq + n)
    return cu(r.normal(size=(nq, d))), cu(r.normal(size=(n, d)))


def topk_run(ops, inp, case):
    return ops.topk_l2(inp[0], inp[1], case[3])


def shard_build(case):
    n, V, P = case
    return [cu(np.random.default_rng(n + P).integers(0, V, n), np.int64)]


def shard_run(ops, inp, case):
    n, V, P = case
    return ops.shard_bucketize(inp[0], -(-V // P), P)


def dedup_build(case):
    """X [B, F] with ascending duplicate-free rows: its flat ids are B sorted lists of F ids laid end to end"""
    B, F, V, E = case
    r = np.random.default_rng(B + F)
    X = np.stack([np.sort(r.choice(V, F, replace=False)) for _ in range(B)]).astype(np.int64)
    return (cu(r.normal(0, 0.5, (V, E))), cu(r.normal(0, 0.5, (V, 1))), cu(r.normal(size=1)), cu(X, np.int64),
            cu(np.full(B, F), np.int64), cu(_uniform(r, B)))


def dedup_run(ops, inp, case):
    embed, w, bias, X, counts, gz = inp
    z, _, rows, sumvec = ops.emb_fm_fwd(embed, w, bias, X, want_rows=True)
    vals = ops.emb_fm_bwd_vals(embed, X, gz, sumvec, rows)
    plan = ops.DedupPlan(X.reshape(-1), embed.shape[0], list_counts=counts)
    return z, vals, plan.uniq_ids, plan.seg_start, plan.perm, plan.n_uniq, plan.segment_sum(vals, embed.shape[1])


def _batches(small, *rest, at=0):
    """``small`` with its batch (element ``at``) replaced by each of ``rest``"""
    return [small[:at] + (b,) + small[at + 1:] for b in rest]


SLICED = (17, 33, 513, 4097)
MMOE_SMALL = (2, 15, 3, 2, 5, 3, 7, 2, 1, 0)
PLE_MID, PLE_LAST = (2, 15, 1, 2, 2, 1, 5, 3, 2, 0), (2, 3, 3, 2, 2, 1, 5, 3, 2, 1)    # Gin = 1; last level, Gin = T + 1
ROUTE_SMALL = (3, 5, 1, 8, 8, 4, 3)

DRIVERS = [
    Driver("cin", ["rec_cin_workspace_bytes"],
           [(1, 1, 1, (1,))] + _batches((33, 3, 5, (7, 13)), *SLICED), cin_build, cin_run),
    Driver("fibinet", ["rec_fibinet_workspace_bytes"],
           [(53, 5, 1, 1, 1, "interaction"), (37, 2, 16, 0, 1, "all")]
           + [c for t in ("all", "each", "interaction") for c in _batches((53, 5, 3, 4, 2, t), *SLICED)],
           fibinet_build, fibinet_run),
    Driver("autoint", ["rec_autoint_workspace_bytes"],
           [(2, 1, 0, 1, 1, 0, False), (17, 4, 1, 3, 1, 1, True)]
           + [c for res in (0, 2) for c in _batches((17, 4, 1, 6, 2, res, False), *SLICED)],
           autoint_build, autoint_run),
    Driver("afm", ["rec_afm_workspace_bytes"], [(1, 2, 1, 1)] + _batches((2, 3, 3, 3), 2, *SLICED), afm_build, afm_run),
    Driver("ccpm", ["rec_ccpm_workspace_bytes"],
           [(1, 3, 1, (1,), (1,))] + _batches((2, 3, 6, (4, 6), (4, 2)), 2, *SLICED), ccpm_build, ccpm_run),
    Driver("fgcnn", ["rec_fgcnn_workspace_bytes"],
           [(1, 3, 1, (1,), (1,), (3,))] + _batches((2, 3, 6, (4, 6), (4, 2), (1, 3)), 2, *SLICED),
           fgcnn_build, fgcnn_run),
    Driver("masknet_ln", ["rec_masknet_ln_workspace_bytes"],
           [(1, 1, 0, 1)] + _batches((2, 1, 1, 3), 2, *SLICED) + [(4097, 3, 0, 5)], masknet_ln_build, masknet_ln_run),
    Driver("masknet_block", ["rec_masknet_block_workspace_bytes"],
           [(1, 1, 1, 1, 1)] + _batches((2, 3, 3, 5, 2), 2, *SLICED), masknet_block_build, masknet_block_run),
    Driver("contextnet_in", [], [(1, 1, 0, 1)] + _batches((2, 1, 1, 3), 2, 17, 33, 4097),
           contextnet_in_build, contextnet_in_run),
    Driver("contextnet_block", ["rec_contextnet_block_workspace_bytes"],
           [(1, 1, 1, 1, "pointwise")] + _batches((2, 3, 5, 2, "pointwise"), 2, *SLICED)
           + _batches((2, 3, 5, 2, "single"), *SLICED), contextnet_block_build, contextnet_block_run),
    Driver("fibinetplus_in", ["rec_emb_fibinetplus_in_workspace_bytes"],
           [(1, 1, 0, 1, True)] + _batches((2, 1, 1, 3, True), 2, *SLICED) + _batches((2, 1, 1, 3, False), 17, 4097)
           + [(4097, 0, 2, 3, True)], fibinetplus_in_build, fibinetplus_in_run),
    Driver("fibinetplus_block", ["rec_fibinetplus_block_workspace_bytes"],
           [(1, 2, 1, 1, 3, 1, "all")] + _batches((2, 3, 6, 3, 2, 4, "each"), 2, *SLICED)
           + _batches((2, 3, 6, 3, 2, 4, "interaction"), 513, 4097) + _batches((2, 3, 6, 3, 2, 4, "all"), 513, 4097),
           fibinetplus_block_build, fibinetplus_block_run),
    Driver("mmoe", ["rec_mmoe_workspace_bytes"],
           [(1, 1, 1, 1, 1, 1, 1, 1, 1, 0), MMOE_SMALL] + _batches(MMOE_SMALL, *SLICED)
           + _batches(MMOE_SMALL[:8] + (2, 1), 33, 513, 4097), mmoe_build, mmoe_run),
    Driver("ple", ["rec_ple_cgc_workspace_bytes"],
           [(1, 1, 1, 1, 1, 1, 1, 1, 1, 1), PLE_MID] + _batches(PLE_MID, *SLICED) + _batches(PLE_LAST, 2, *SLICED),
           ple_build, ple_run),
    Driver("mind_routing", ["rec_mind_routing_workspace_bytes"],
           [(1, 1, 1, 1, 1, 1, 1), ROUTE_SMALL, (33, 6, 3, 16, 48, 4, 3), (33, 65, 3, 8, 40, 16, 3)]
           + _batches(ROUTE_SMALL, 513, 4097), mind_routing_build, mind_routing_run),
    Driver("mind_laa", [], [(1, 1, 1, 1, 1), (3, 2, 1, 8, 4), (33, 11, 3, 16, 4), (33, 65, 3, 16, 16)],
           mind_laa_build, mind_laa_run),
    Driver("comirec_dr", ["rec_comirec_dr_workspace_bytes"],
           [(1, 1, 1, 1, 1, 1, 1), ROUTE_SMALL, (33, 6, 3, 16, 48, 4, 3), (33, 65, 3, 8, 40, 16, 3)]
           + _batches(ROUTE_SMALL, 513, 4097), comirec_dr_build, comirec_dr_run),
    Driver("comirec_sa", ["rec_comirec_sa_workspace_bytes"],
           [(1, 1, 1, 1, 1, 1), ROUTE_SMALL[:6], (33, 6, 3, 16, 48, 4), (33, 65, 3, 8, 40, 16)]
           + _batches(ROUTE_SMALL[:6], 513, 4097), comirec_sa_build, comirec_sa_run),
    Driver("comirec_select", [], [(1, 1, 1, 1, 1), (3, 2, 1, 8, 4), (33, 11, 3, 16, 4), (33, 65, 3, 16, 16)],
           comirec_select_build, comirec_select_run),
    Driver("can", [], [(1, 1, 1, (1,), 1, 0), (3, 5, 4, (1, 1, 1), 3, 0), (3, 5, 4, (1, 1, 1), 3, 1),
                       (33, 6, 16, (1, 1, 1), 3, 0), (33, 65, 8, (2, 1), 3, 0), (33, 65, 8, (2, 1), 3, 1)],
           can_build, can_run),
    Driver("crossnet_vec", ["rec_crossnet_vec_bwd_workspace_bytes"], [(5, 7, 1)] + _batches((5, 7, 2), *SLICED),
           crossnet_build, crossnet_run),
    Driver("batchnorm", ["rec_batchnorm_workspace_bytes"],
           [(2, 1, True)] + _batches((2, 5, True), *SLICED) + _batches((2, 5, False), 33, 4097),
           batchnorm_build, batchnorm_run),
    Driver("l2_rows", ["rec_l2_rows_workspace_bytes"], [(1, 1, 1), (33, 50, 3), (513, 50, 3), (4097, 50, 3), (4097, 9000, 3)],
           l2_rows_build, l2_rows_run),
    Driver("topk_l2", ["rec_topk_l2_workspace_bytes"], [(1, 1, 1, 1), (3, 33, 5, 4), (17, 513, 5, 8), (5, 4097, 3, 8)],
           topk_build, topk_run),
    Driver("shard_bucketize", ["rec_shard_bucketize_workspace_bytes"],
           [(1, 10, 1), (33, 1000, 2), (513, 1000, 4), (4097, 1000, 8)], shard_build, shard_run),
    Driver("dedup_lists", ["rec_dedup_workspace_bytes"], [(1, 1, 10, 16), (33, 3, 50, 16), (64, 5, 40, 16)],
           dedup_build, dedup_run),
]

PARAMS = [pytest.param(d, c, id="%s-%s" % (d.name, case_id(c))) for d in DRIVERS for c in d.cases]


def _compare(what, got, want):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert G.bit_equal(a, b), "%s: returned tensor %d %s %s differs" % (what, i, tuple(a.shape), a.dtype)


@pytest.mark.parametrize("driver,case", PARAMS)
def test_guards_and_poison(driver, case):
    from explicit_tf2_recommendation_amd import ops
    inputs = driver.build(case)
    flat_in = G.flatten(inputs)
    before = [t.clone() for t in flat_in]
    want = G.flatten(driver.run(ops, inputs, case))
    assert want, "the driver hands nothing back"
    with G.guarded(ops, G.POISON_NAN) as g:
        nan_run = G.flatten(driver.run(ops, inputs, case))
    print("%s %s: %d allocations, %d bytes through the seam; queries %s"
          % (driver.name, case_id(case), len(g.allocations), g.total_bytes(), g.queries))
    assert g.allocations, "the driver bypassed the seam"
    assert set(driver.queries) <= set(g.queries), (driver.queries, g.queries)
    for i, t in enumerate(nan_run):
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), "returned tensor %d %s holds poison or a non-finite value" \
                % (i, tuple(t.shape))
    _compare("0xFF poison against the plain run", nan_run, want)
    with G.guarded(ops, G.POISON_FINITE):
        fin_run = G.flatten(driver.run(ops, inputs, case))
    _compare("0x7F poison against 0xFF poison", fin_run, nan_run)
    _compare("the inputs after the runs", flat_in, before)


SHORT_BY = 32


@pytest.mark.parametrize("name,case", [("mmoe", _batches(MMOE_SMALL, 513)[0]), ("mind_routing", ROUTE_SMALL)],
                         ids=["mmoe", "mind_routing"])
def test_a_short_workspace_view_trips_the_guard(name, case):
    """The detector fires on the GPU, with unmodified kernels and no access outside an allocation: the workspace's trailing
    guard starts SHORT_BY bytes early, inside the view, and the kernels that fill the workspace to its end "damage" it.
    Both queries answer with 4 floats more than their entry point consumes (``total + 4`` in rec_mmoe_workspace_bytes,
    ``grid D Dc + 4`` in rec_mind_routing_workspace_bytes, against the sizes rec_mmoe_bwd_f32 and rec_mind_routing_bwd_f32
    check): a view 16 bytes short would end exactly on that slack, which no kernel touches, so the view is 16 bytes
    shorter still.  MMOE at B = 513: the last region of the carve is the two split-K slices of dW1, 2 x 375 floats rounded
    up to 752, two of its last four floats written.  MIND routing at B = 3: the last four floats of the third dS
    partial."""
    from explicit_tf2_recommendation_amd import ops
    driver = {d.name: d for d in DRIVERS}[name]
    inputs = driver.build(case)
    with pytest.raises(G.GuardError) as e:
        with G.guarded(ops, G.POISON_NAN, short_by=SHORT_BY, short_if=lambda a: a.frames[0].startswith("_workspace:")):
            driver.run(ops, inputs, case)
    msg = str(e.value)
    print(msg)
    assert "after the view" in msg and "_workspace:" in msg and "before the view" not in msg
    assert msg.count("\n") == 1, "one allocation, the workspace, and no other"
