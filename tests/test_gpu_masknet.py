"""MaskNet on the GPU: the fused lookup + per-field LayerNorm kernels and the mask-block kernels (csrc/masknet.hip) against
the fp64 numpy reading of tests/masknet_ref.py, the layers against the torch-CPU transcription, graph capture, bit identity
run to run, error paths and ModelManager(layer='MaskNet').

Tolerance, per tensor: max|got - want| / max|want| against fp64 must stay within 4 x the error of the fp32 CPU
transcription on the same inputs, never below 1e-5 (forward tensors) / 3e-5 (gradients).  An example whose smallest
|relu pre-activation| in fp64 is below PRE_EPS = 1e-5 may take the other branch in fp32: the upstream-gradient rows of
those examples are zeroed before either side runs, every case asserts they are at most 10 % of its examples, and cases
under 100 examples use the first seed 1, 2, 3, ... without any (chosen on the fp64 reading alone).

Measured on the MI355X, the first run's printout (28 passed in 5 s).  Where the fp64 value of a tensor is zero
throughout (dgamma at E = 1 or O = 1) the fp32 transcription's relative error, and with it the bound, is meaningless;
the kernels return exact zeros there.
  input stage (4099, 10, 3, 16)                                block (4099, 208, 208, 32, 3), near-kink examples: 55 of 4099
    x_norm       error/bound 1.59e-07 / 1.00e-05 = 0.02           y            error/bound 6.81e-07 / 1.00e-05 = 0.07
    dtable       error/bound 8.74e-08 / 3.00e-05 = 0.00           dv           error/bound 5.60e-07 / 3.00e-05 = 0.02
    vals         error/bound 1.86e-07 / 3.00e-05 = 0.01           dx_emb       error/bound 8.73e-07 / 3.00e-05 = 0.03
    dgamma       error/bound 1.35e-07 / 3.00e-05 = 0.00           dW1          error/bound 5.04e-07 / 3.00e-05 = 0.02
    dbeta        error/bound 9.79e-08 / 3.00e-05 = 0.00           db1          error/bound 3.44e-07 / 3.00e-05 = 0.01
  input stage (17, 61, 3, 64)                                     dW2          error/bound 4.36e-07 / 3.00e-05 = 0.01
    x_norm       error/bound 1.44e-07 / 1.00e-05 = 0.01           db2          error/bound 2.48e-07 / 3.00e-05 = 0.01
    dtable       error/bound 1.23e-07 / 3.00e-05 = 0.00           dW3          error/bound 4.93e-07 / 3.00e-05 = 0.02
    vals         error/bound 1.47e-07 / 3.00e-05 = 0.00           db3          error/bound 2.34e-07 / 3.00e-05 = 0.01
    dgamma       error/bound 1.05e-07 / 3.00e-05 = 0.00           dgamma       error/bound 4.19e-07 / 3.00e-05 = 0.01
    dbeta        error/bound 6.61e-08 / 3.00e-05 = 0.00           dbeta        error/bound 9.23e-08 / 3.00e-05 = 0.00
  block (17, 512, 512, 128, 4), near-kink examples: 0 of 17    block (2049, 416, 416, 32, 3), near-kink examples: 54 of 2049
    y            error/bound 8.91e-07 / 1.00e-05 = 0.09           y            error/bound 9.27e-07 / 1.00e-05 = 0.09
    dv           error/bound 1.33e-06 / 3.00e-05 = 0.04           dv           error/bound 8.28e-07 / 3.00e-05 = 0.03
    dx_emb       error/bound 1.33e-06 / 3.00e-05 = 0.04           dx_emb       error/bound 8.67e-07 / 3.00e-05 = 0.03
    dW1          error/bound 5.21e-07 / 3.00e-05 = 0.02           dW1          error/bound 5.90e-07 / 3.00e-05 = 0.02
    db1          error/bound 5.89e-07 / 3.00e-05 = 0.02           db1          error/bound 5.57e-07 / 3.00e-05 = 0.02
    dW2          error/bound 6.12e-07 / 3.00e-05 = 0.02           dW2          error/bound 4.71e-07 / 3.00e-05 = 0.02
    db2          error/bound 2.42e-07 / 3.00e-05 = 0.01           db2          error/bound 2.98e-07 / 3.00e-05 = 0.01
    dW3          error/bound 6.84e-07 / 3.00e-05 = 0.02           dW3          error/bound 5.53e-07 / 3.00e-05 = 0.02
    db3          error/bound 1.47e-07 / 3.00e-05 = 0.00           db3          error/bound 3.52e-07 / 3.00e-05 = 0.01
    dgamma       error/bound 8.66e-07 / 3.00e-05 = 0.03           dgamma       error/bound 4.96e-07 / 3.00e-05 = 0.02
    dbeta        error/bound 7.08e-08 / 3.00e-05 = 0.00           dbeta        error/bound 1.66e-07 / 3.00e-05 = 0.01
  block (4099, 208, 32, 32, 3): 7 of 4099 near a kink, y 4.91e-07 / 1.00e-05, the largest gradient ratio dx_emb
  6.25e-07 / 3.00e-05; the other cases lie below the ones shown, and (1, 1, 1, 1, 1) is exact in every tensor.
  layer, serial at the defaults: output 2.21e-07 / 1.00e-05, largest gradient ratio 2.83e-06 / 3.00e-05 (a ln_hid gamma);
  parallel with block_num = 2: output 2.21e-07 / 1.00e-05, largest gradient ratio 8.42e-07 / 3.00e-05 (a field's gamma).
"""
import functools

import numpy as np
import pytest
import torch

from tests import masknet_ref as MR

pytestmark = pytest.mark.gpu

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]
F32 = np.float32


def cu(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def check(name, got, want, t32, floor):
    err, bound = MR.rel_err(got, want), max(floor, 4 * MR.rel_err(t32, want))
    print("%-12s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    assert err <= bound, (name, err, bound)


# ---- input stage ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def input_case(B, Fc, Fk, E, V=5000, special=False):
    r = np.random.default_rng(B * 7 + Fc)
    table, X, values, gamma, beta = MR.make_input(r, B, Fc, Fk, E, V)
    if special and Fk:                                   # values exactly 0 and negative ones
        values[::3, 0] = 0.0
        values[1::3, -1] = -np.abs(values[1::3, -1]) - 0.5
    table, values, gamma, beta = (a.astype(F32).astype(np.float64) for a in (table, values, gamma, beta))
    F = Fc + Fk
    dn, de = (r.uniform(-1, 1, (B, F * E)).astype(F32).astype(np.float64) for _ in range(2))
    ref = MR.input_stage_numpy(table, X, values, gamma, beta, dn, de)
    t32 = MR.input_stage_torch_grads(table, X, values, gamma, beta, dn, de, torch.float32)
    return dict(table=table, X=X, values=values, gamma=gamma, beta=beta, dn=dn, de=de, ref=ref, t32=t32)


def run_input(c, direct="given"):
    from explicit_tf2_recommendation_amd import ops
    Fk = c["values"].shape[1]
    table, X, gamma, beta, dn = cu(c["table"]), cu(c["X"], np.int64), cu(c["gamma"]), cu(c["beta"]), cu(c["dn"])
    values = cu(c["values"]) if Fk else None
    de = {"given": cu(c["de"]), "none": None, "zeros": torch.zeros_like(dn)}[direct]
    flag = ops.new_flag(table.device)
    x_emb, x_norm, stats = ops.emb_masknet_ln_fwd(table, X, values, gamma, beta, flag)
    vals, dg, db = ops.emb_masknet_ln_bwd(x_emb, stats, values, gamma, dn, de)
    return x_emb, x_norm, vals, dg, db, int(flag.item())


INPUT_CASES = [(1, 1, 0, 1), (2, 1, 1, 3), (17, 10, 3, 16), (33, 3, 2, 40), (17, 61, 3, 64), (1000, 26, 0, 16),
               (4099, 10, 3, 16), (1000, 10, 3, 16, 7), (100, 10, 3, 16, 5000, True)]


@pytest.mark.parametrize("case", INPUT_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_input_stage_matches_fp64(case):
    c = input_case(*case)
    x_emb, x_norm, vals, dg, db, flag = run_input(c)
    assert flag == 0
    ref, (te, tn, tt, tg, tb) = c["ref"], c["t32"]
    B, F = c["X"].shape
    Fc = F - c["values"].shape[1]
    rows = c["table"].astype(F32)[c["X"]]
    rows[:, Fc:] *= c["values"].astype(F32)[:, :, None]
    assert np.array_equal(x_emb.cpu().numpy(), rows.reshape(B, -1))           # table[X] times the value, bit for bit
    check("x_norm", x_norm.cpu().numpy(), ref["x_norm"], tn, 1e-5)
    dtable = np.zeros_like(c["table"])
    np.add.at(dtable, c["X"], vals.cpu().numpy().astype(np.float64).reshape(B, F, -1))
    check("dtable", dtable, ref["dtable"], tt, 3e-5)
    check("vals", vals.cpu().numpy(), ref["vals"], ref["vals"], 3e-5)
    check("dgamma", dg.cpu().numpy(), ref["dgamma"], tg, 3e-5)
    check("dbeta", db.cpu().numpy(), ref["dbeta"], tb, 3e-5)
    none, zeros = run_input(c, "none"), run_input(c, "zeros")
    for a, b in zip(none[:5], zeros[:5]):
        assert torch.equal(a, b)                                              # no direct gradient == zeros, bitwise


@pytest.mark.parametrize("col", [2, 11], ids=["categorical", "key"])
def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows(col):
    c = dict(input_case(17, 10, 3, 16))
    X = c["X"].copy()
    X[3, col], X[9, col] = 5000, -1
    c["X"] = X
    x_emb, x_norm, vals, dg, db, flag = run_input(c)
    assert flag == 1
    ref = MR.input_stage_numpy(c["table"], X, c["values"], c["gamma"], c["beta"], c["dn"], c["de"])
    e = x_emb.cpu().numpy().reshape(17, 13, 16)
    assert np.count_nonzero(e[3, col]) == 0 and np.count_nonzero(e[9, col]) == 0
    np.testing.assert_allclose(x_norm.cpu().numpy().reshape(17, 13, 16)[3, col], c["beta"][col], rtol=0, atol=1e-7)
    assert MR.rel_err(x_norm.cpu().numpy(), ref["x_norm"]) <= 1e-5 and MR.rel_err(vals.cpu().numpy(), ref["vals"]) <= 3e-5


# ---- mask block -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_case(B, D, P, O, R):
    def gen(seed):
        r = np.random.default_rng(seed)
        params = [p.astype(F32).astype(np.float64) for p in MR.make_block(r, D, P, O, R)]
        xe, v = (r.normal(0, s, shp).astype(F32).astype(np.float64) for s, shp in ((0.5, (B, D)), (1.0, (B, P))))
        return r, params, xe, v

    near_of = lambda s: MR.block_numpy(*[gen(s)[i] for i in (2, 3, 1)])["pre"] < MR.PRE_EPS
    seed = MR.clean_seed(lambda s: near_of(s).any()) if B < 100 else 1      # on the fp64 reading alone
    r, params, xe, v = gen(seed)
    near = near_of(seed)
    assert near.mean() <= 0.10 and (B >= 100 or not near.any())
    dy = r.uniform(-1, 1, (B, O)).astype(F32).astype(np.float64)
    dy[near] = 0.0
    ref = MR.block_numpy(xe, v, params, dy)
    t32 = MR.block_torch_grads(xe, v, params, dy, torch.float32)
    return dict(params=params, xe=xe, v=v, dy=dy, ref=ref, t32=t32, near=near)


def run_block(c, save=True):
    from explicit_tf2_recommendation_amd import ops
    xe, v, dy = cu(c["xe"]), cu(c["v"]), cu(c["dy"])
    p = [cu(a) for a in c["params"]]
    y, saved = ops.mask_block_fwd(xe, v, *p, save=save)
    if not save:
        return y
    dv, dx, g = ops.mask_block_bwd(xe, v, p[0], p[2], p[4], p[6], y, saved, dy)
    return y, dv, dx, g, (xe, v, p, saved, dy)


BLOCK_CASES = [(1, 1, 1, 1, 1), (2, 3, 3, 5, 2), (5, 130, 130, 33, 3), (17, 208, 208, 32, 3), (17, 208, 32, 32, 3),
               (33, 200, 7, 7, 3), (17, 512, 512, 128, 4), (4099, 208, 208, 32, 3), (4099, 208, 32, 32, 3),
               (2049, 416, 416, 32, 3),
               # slice edges of the small weight-gradient launch (csrc/tile_ops.h): two unequal slices; sixteen, the last empty
               (513, 3, 3, 5, 2), (4097, 3, 3, 5, 2)]
GRAD_NAMES = ["dW1", "db1", "dW2", "db2", "dW3", "db3", "dgamma", "dbeta"]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_block_matches_fp64(case):
    from explicit_tf2_recommendation_amd import ops
    c = block_case(*case)
    print("near-kink examples: %d of %d" % (c["near"].sum(), len(c["near"])))
    y, dv, dx, g, (xe, v, p, saved, dy) = run_block(c)
    ref, (ty, tdv, tdx, tg) = c["ref"], c["t32"]
    check("y", y.cpu().numpy(), ref["y"], ty, 1e-5)
    check("dv", dv.cpu().numpy(), ref["dv"], tdv, 3e-5)
    check("dx_emb", dx.cpu().numpy(), ref["dx_emb"], tdx, 3e-5)
    for name, got, want, t in zip(GRAD_NAMES, g, ref["dparams"], tg):
        check(name, got.cpu().numpy(), want, t, 3e-5)
    assert torch.equal(run_block(c, save=False), y)      # inference writes the same y, bitwise
    pre = torch.from_numpy(np.random.default_rng(5).uniform(-1, 1, tuple(dx.shape)).astype(F32)).cuda()
    acc = pre.clone()
    ops.mask_block_bwd(xe, v, p[0], p[2], p[4], p[6], y, saved, dy, dx_emb=acc, accumulate=True)
    assert float((acc - (dx + pre)).abs().max()) <= 1e-6


def test_every_output_is_bit_identical_run_to_run():
    c = block_case(4099, 208, 208, 32, 3)
    a, b = run_block(c), run_block(c)
    for x, y in zip([a[0], a[1], a[2], *a[3], *a[4][3]], [b[0], b[1], b[2], *b[3], *b[4][3]]):
        assert torch.equal(x, y)
    ci = input_case(4099, 10, 3, 16)
    for x, y in zip(run_input(ci)[:5], run_input(ci)[:5]):
        assert torch.equal(x, y)


def test_graph_replay_equals_eager():
    """Forward + backward of the input stage and two blocks captured in one hipGraph, replayed twice."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    ci, c1, c2 = input_case(1000, 10, 3, 16), block_case(4099, 208, 208, 32, 3), block_case(4099, 208, 32, 32, 3)
    table, X, values, gamma, beta = cu(ci["table"]), cu(ci["X"], np.int64), cu(ci["values"]), cu(ci["gamma"]), cu(ci["beta"])
    p1, p2 = [cu(a) for a in c1["params"]], [cu(a) for a in c2["params"]]
    dy = cu(c2["dy"][:1000])

    def step():
        x_emb, x_norm, stats = ops.emb_masknet_ln_fwd(table, X, values, gamma, beta)
        y1, s1 = ops.mask_block_fwd(x_emb, x_norm, *p1)
        y2, s2 = ops.mask_block_fwd(x_emb, y1, *p2)
        dv2, dx, g2 = ops.mask_block_bwd(x_emb, y1, p2[0], p2[2], p2[4], p2[6], y2, s2, dy)
        dv1, dx, g1 = ops.mask_block_bwd(x_emb, x_norm, p1[0], p1[2], p1[4], p1[6], y1, s1, dv2, dx_emb=dx,
                                         accumulate=True)
        return [y2, dx, *g1, *g2, *ops.emb_masknet_ln_bwd(x_emb, stats, values, gamma, dv1, dx)]

    eager = [t.clone() for t in step()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        static = step()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    c = block_case(2, 3, 3, 5, 2)
    xe, v, dy = cu(c["xe"]), cu(c["v"]), cu(c["dy"])
    p = [cu(a) for a in c["params"]]
    with pytest.raises(RuntimeError):
        ops.mask_block_fwd(xe.cpu(), v, *p)                                   # no CPU fallback
    with pytest.raises(ValueError):
        ops.mask_block_fwd(xe, v[:, :2].contiguous(), *p)
    with pytest.raises(ValueError):
        ops.mask_block_fwd(xe, v, p[0], p[1][:-1].contiguous(), *p[2:])
    y, saved = ops.mask_block_fwd(xe, v, *p)
    with pytest.raises(ValueError):
        ops.mask_block_bwd(xe, v, p[0], p[2], p[4], p[6], y, saved, dy[:, :3].contiguous())
    with pytest.raises(RuntimeError):
        ops.mask_block_bwd(xe, v, p[0], p[2], p[4], p[6], y, saved, dy.cpu())
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(NotImplementedError):                                  # D = 513
        ops.mask_block_fwd(z(2, 513), z(2, 8), z(513, 24), z(24), z(24, 8), z(8), z(8, 4), z(4), z(4), z(4))
    with pytest.raises(NotImplementedError):                                  # R = 5
        ops.mask_block_fwd(z(2, 8), z(2, 8), z(8, 40), z(40), z(40, 8), z(8), z(8, 4), z(4), z(4), z(4))
    ye, se = ops.mask_block_fwd(xe[:0], v[:0], *p)
    assert tuple(ye.shape) == (0, 5) and tuple(se[0].shape) == (0, 6)
    dv, dx, g = ops.mask_block_bwd(xe[:0], v[:0], p[0], p[2], p[4], p[6], ye, se, dy[:0])
    assert tuple(dv.shape) == (0, 3) and tuple(dx.shape) == (0, 3) and all(float(t.abs().sum()) == 0 for t in g)

    ci = input_case(2, 1, 1, 3)
    table, X, values, gamma, beta = cu(ci["table"]), cu(ci["X"], np.int64), cu(ci["values"]), cu(ci["gamma"]), cu(ci["beta"])
    with pytest.raises(RuntimeError):
        ops.emb_masknet_ln_fwd(table.cpu(), X, values, gamma, beta)
    with pytest.raises(ValueError):
        ops.emb_masknet_ln_fwd(table, X, values, gamma[:1].contiguous(), beta)
    with pytest.raises(ValueError):
        ops.emb_masknet_ln_fwd(table, X, values[:1].contiguous(), gamma, beta)
    with pytest.raises(NotImplementedError):
        ops.emb_masknet_ln_fwd(table, torch.zeros(2, 65, dtype=torch.int64, device="cuda"), None, z(65, 3), z(65, 3))
    x_emb, x_norm, stats = ops.emb_masknet_ln_fwd(table, X[:0], values[:0], gamma, beta)
    assert tuple(x_emb.shape) == (0, 6) and tuple(stats.shape) == (0, 2, 2)
    vals, dg, db = ops.emb_masknet_ln_bwd(x_emb, stats, values[:0], gamma, x_norm)
    assert tuple(vals.shape) == (0, 3) and float(dg.abs().sum()) == 0 and float(db.abs().sum()) == 0
    x_emb, x_norm, stats = ops.emb_masknet_ln_fwd(table, X, values, gamma, beta)
    with pytest.raises(ValueError):
        ops.emb_masknet_ln_bwd(x_emb, stats, values, gamma, z(2, 5))


# ---- layers ---------------------------------------------------------------------------------------------------------
LAYER_B, LAYER_V = 64, 1000
KEYS = [c + "_key" for c in CONT]
VALS = [c + "_value" for c in CONT]


def _ref_params(sd, mode, NB):
    """state dict (name -> array) -> (table, gamma, beta, blocks, head) in the layout of tests/masknet_ref.py"""
    ln = "mask_net.norm_embedding_layer.emb_layernorm_list.%d.%s"
    names = (["mask_net.mask_block_on_feature."] + ["mask_net.mask_block_on_block_list.%d." % k for k in range(NB - 1)]
             if mode == "serial" else ["mask_net.mask_block_on_feature_list.%d." % k for k in range(NB)])
    suffix = ["instance_guided_mask.layers.0.kernel", "instance_guided_mask.layers.0.bias",
              "instance_guided_mask.layers.2.kernel", "instance_guided_mask.layers.2.bias", "ln_hid.layers.0.kernel",
              "ln_hid.layers.0.bias", "ln_hid.layers.1.gamma", "ln_hid.layers.1.beta"]
    head = ["final_mlp.layers.0.kernel", "final_mlp.layers.0.bias", "final_mlp.layers.1.alpha", "final_mlp.layers.2.kernel",
            "final_mlp.layers.2.bias"]
    return (["mask_net.norm_embedding_layer.embedding_layer.embeddings"], [ln % (f, "gamma") for f in range(13)],
            [ln % (f, "beta") for f in range(13)], [[n + s for s in suffix] for n in names], head)


def _layer_setup(mode, NB, seed):
    """parameters on the test scale and a batch, all from ``seed`` -> (state dict of numpy fp32 arrays, batch)"""
    from explicit_tf2_recommendation_amd import data
    r = np.random.default_rng(seed)
    table, _, _, gamma, beta = MR.make_input(r, 1, 10, 3, 16, LAYER_V)
    blocks = MR.make_stack(r, 13, 16, 32, NB, mode)
    head = MR.make_head(r, 32 if mode == "serial" else NB * 32)
    nt, ng, nb, nbl, nh = _ref_params(None, mode, NB)
    sd = {nt[0]: table, **{n: gamma[f] for f, n in enumerate(ng)}, **{n: beta[f] for f, n in enumerate(nb)},
          **{n: a for ns, bp in zip(nbl, blocks) for n, a in zip(ns, bp)},
          **{n: a.reshape(-1) if n.endswith(("bias", "alpha")) else a for n, a in zip(nh, head)}}
    batch = data.SyntheticGenerator(CAT + KEYS, LAYER_V, continuous=VALS, seed=seed).batch(LAYER_B)
    return {k: np.asarray(v, F32) for k, v in sd.items()}, batch


def _layer_ref_inputs(sd, batch, mode, NB):
    nt, ng, nb, nbl, nh = _ref_params(None, mode, NB)
    d = lambda n: sd[n].astype(np.float64)
    X = np.stack([np.asarray(batch[n]).reshape(-1) for n in CAT + KEYS], axis=1).astype(np.int64)
    values = np.stack([np.asarray(batch[n], np.float64).reshape(-1) for n in VALS], axis=1)
    head = [d(n) for n in nh]
    head[1], head[2], head[4] = head[1].reshape(-1), head[2].reshape(-1), head[4].reshape(-1)
    return (d(nt[0]), X, values, np.stack([d(n) for n in ng]), np.stack([d(n) for n in nb]),
            [[d(n) for n in ns] for ns in nbl], head)


@pytest.mark.parametrize("mode,NB", [("serial", 6), ("parallel", 2)])
def test_layer_parity_with_the_torch_cpu_transcription(mode, NB):
    from explicit_tf2_recommendation_amd import data, layers

    def near(seed):
        sd, batch = _layer_setup(mode, NB, seed)
        return (MR.masknet_numpy(*_layer_ref_inputs(sd, batch, mode, NB), mode)["pre"] < MR.PRE_EPS).any()

    seed = MR.clean_seed(near)                           # under 100 examples: a seed without a near-kink example
    sd, batch = _layer_setup(mode, NB, seed)
    lay = layers.MaskNetLayer(feature_dims=LAYER_V, block_num=NB, stacking_mode=mode).cuda()
    with torch.no_grad():
        for k, p in lay.named_parameters():
            p.copy_(torch.from_numpy(sd[k]).reshape(p.shape))
    lay.train()
    out = lay(data.to_device(batch))["output"]
    assert tuple(out.shape) == (LAYER_B, 1)
    gout = np.random.default_rng(0).uniform(-1, 1, (LAYER_B, 1)).astype(F32)
    out.backward(torch.from_numpy(gout).cuda())
    args = _layer_ref_inputs(sd, batch, mode, NB)
    ref = MR.masknet_numpy(*args, mode, gout)
    assert not (ref["pre"] < MR.PRE_EPS).any()
    t64 = MR.masknet_torch_grads(*args, mode, gout, torch.float64)
    t32 = MR.masknet_torch_grads(*args, mode, gout, torch.float32)
    assert MR.rel_err(t64[0], ref["output"]) < 1e-12
    check("output", out.detach().cpu().numpy(), t64[0], t32[0], 1e-5)
    nt, ng, nb, nbl, nh = _ref_params(None, mode, NB)
    flat = lambda t: ([(nt[0], t[1])] + [(n, t[2][f]) for f, n in enumerate(ng)] + [(n, t[3][f]) for f, n in enumerate(nb)]
                      + [(n, a) for ns, bp in zip(nbl, t[4]) for n, a in zip(ns, bp)] + list(zip(nh, t[5])))
    grads = {k: (p.grad.to_dense() if p.grad.is_sparse else p.grad).cpu().numpy() for k, p in lay.named_parameters()}
    assert grads.keys() == {n for n, _ in flat(t64)}
    for (name, want), (_, w32) in zip(flat(t64), flat(t32)):
        check(name.replace("mask_net.", "")[-40:], grads[name].reshape(want.shape), want, w32, 3e-5)


def test_out_of_range_key_raises():
    from explicit_tf2_recommendation_amd import data, layers
    lay = layers.MaskNetLayer(feature_dims=100, block_num=2).cuda()
    batch = data.SyntheticGenerator(CAT + KEYS, 100, continuous=VALS, seed=1).batch(16)
    lay(data.to_device(batch))
    bad = dict(batch)
    ids = np.array(bad["itag4_square_key"]).copy()
    ids.reshape(-1)[5] = 100
    bad["itag4_square_key"] = ids
    with pytest.raises(IndexError):
        lay(data.to_device(bad))


def _manager(engine, V=5000, B=512, lr=0.01):
    from explicit_tf2_recommendation_amd import data
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    return ModelManager(feature_names=CAT, continuous_features=CONT, data_info=data.data_info(V, len(CAT) + len(CONT)),
                        embedding_dims=16, lr=lr, batch=B, layer="MaskNet", engine=engine)


def test_model_manager_trains_masknet_graphed_like_eager():
    from explicit_tf2_recommendation_amd import data, layers
    a, b = _manager("eager"), _manager("auto")
    assert isinstance(a.layer, layers.MaskNetLayer)
    b.model.load_state_dict(a.model.state_dict())
    gen = data.SyntheticGenerator(CAT + KEYS, 5000, continuous=VALS, dist="zipf", seed=9)
    for _ in range(3):
        batch = gen.batch(512)
        la, lb = a.train_loop(dict(batch)), b.train_loop(dict(batch))
        assert np.isfinite(la.item()) and np.isfinite(lb.item())
        assert la.item() == lb.item()
    assert b._eng[0] == "graphed"
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k
