"""ContextNet on the GPU: the lookup x value kernels and the block kernels (csrc/contextnet.hip) against the fp64 numpy
reading of tests/contextnet_ref.py, the layers against the torch-CPU transcription, graph capture, bit identity run to
run, error paths and ModelManager(layer='ContextNet').

Tolerance, per tensor (MaskNet's rule): max|got - want| / max|want| against fp64 must stay within 4 x the error of the
fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors) / 3e-5 (gradients).  An example whose
smallest |relu pre-activation| in fp64, over both h and a, is below PRE_EPS = 1e-5 may take the other branch in fp32: the
upstream-gradient rows of those examples are zeroed before either side runs, every case asserts they are at most 10 % of
its examples, and cases under 100 examples use the first seed 1, 2, 3, ... without any (chosen on the fp64 reading alone).
Where the fp64 value of a tensor is zero throughout (E = 1: every gradient but dbeta) the kernels return exact zeros.

Measured on the MI355X: the first run's printout (27 passed in 5 s), every tensor of every input-stage and block case
as `name error / bound`, three to a line; the two layer cases check 119 and 136 tensors and are given as a DIGEST (the
output, the three largest error / bound ratios and the number of tensors).  The test of the sub-layers' direct calls was added
after that run and prints nothing.
  input stage (B, Fc, Fk, E); x is table[X] times the value bit for bit in every case
    (1, 1, 0, 1)                         dtable 0.00e+00 / 3.00e-05; vals 0.00e+00 / 3.00e-05
    (2, 1, 1, 3)                         dtable 5.94e-09 / 3.00e-05; vals 5.94e-09 / 3.00e-05
    (17, 10, 3, 16)                      dtable 3.91e-08 / 3.00e-05; vals 3.91e-08 / 3.00e-05
    (17, 61, 3, 8)                       dtable 2.53e-08 / 3.00e-05; vals 2.74e-08 / 3.00e-05
    (4099, 10, 3, 16)                    dtable 1.70e-08 / 3.00e-05; vals 3.11e-08 / 3.00e-05
    (100, 10, 3, 16), values 0 and < 0   dtable 3.58e-08 / 3.00e-05; vals 3.61e-08 / 3.00e-05
  block (1, 1, 1, 1, 'pointwise'), near-kink examples: 0 of 1
    y 0.00e+00 / 1.00e-05; dx 0.00e+00 / 3.00e-05; dWa 0.00e+00 / 3.00e-05
    dba 0.00e+00 / 3.00e-05; dWb 0.00e+00 / 3.00e-05; dbb 0.00e+00 / 3.00e-05
    dW1 0.00e+00 / 3.00e-05; dW2 0.00e+00 / 3.00e-05; dgamma 0.00e+00 / 4.26e+22
    dbeta 0.00e+00 / 3.00e-05
  block (2, 3, 5, 2, 'pointwise'), near-kink examples: 0 of 2
    y 1.18e-07 / 1.00e-05; dx 1.58e-07 / 3.00e-05; dWa 3.08e-07 / 3.00e-05
    dba 2.86e-07 / 3.00e-05; dWb 1.75e-07 / 3.00e-05; dbb 1.14e-07 / 3.00e-05
    dW1 1.19e-07 / 3.00e-05; dW2 3.37e-07 / 3.00e-05; dgamma 2.77e-08 / 3.00e-05
    dbeta 3.09e-08 / 3.00e-05
  block (5, 13, 10, 3, 'pointwise'), near-kink examples: 0 of 5
    y 5.56e-07 / 1.00e-05; dx 3.49e-07 / 3.00e-05; dWa 4.93e-07 / 3.00e-05
    dba 3.31e-07 / 3.00e-05; dWb 5.98e-07 / 3.00e-05; dbb 3.52e-07 / 3.00e-05
    dW1 2.91e-07 / 3.00e-05; dW2 7.23e-07 / 3.00e-05; dgamma 3.35e-07 / 3.00e-05
    dbeta 6.71e-08 / 3.00e-05
  block (17, 13, 16, 3, 'pointwise'), near-kink examples: 0 of 17
    y 9.46e-07 / 1.00e-05; dx 7.04e-07 / 3.00e-05; dWa 5.33e-07 / 3.00e-05
    dba 8.18e-07 / 3.00e-05; dWb 6.87e-07 / 3.00e-05; dbb 5.50e-07 / 3.00e-05
    dW1 6.12e-07 / 3.00e-05; dW2 5.92e-07 / 3.00e-05; dgamma 2.86e-07 / 3.00e-05
    dbeta 1.30e-07 / 3.00e-05
  block (17, 13, 16, 3, 'single'), near-kink examples: 0 of 17
    y 1.35e-06 / 1.00e-05; dx 7.48e-07 / 3.00e-05; dWa 6.44e-07 / 3.00e-05
    dba 6.59e-07 / 3.00e-05; dWb 7.44e-07 / 3.00e-05; dbb 5.47e-07 / 3.00e-05
    dW1 6.14e-07 / 3.00e-05; dgamma 4.85e-07 / 3.00e-05; dbeta 8.95e-08 / 3.00e-05
  block (33, 7, 33, 1, 'pointwise'), near-kink examples: 0 of 33
    y 4.69e-07 / 1.00e-05; dx 4.70e-07 / 3.00e-05; dWa 4.09e-07 / 3.00e-05
    dba 3.63e-07 / 3.00e-05; dWb 3.97e-07 / 3.00e-05; dbb 1.99e-07 / 3.00e-05
    dW1 5.33e-07 / 3.00e-05; dW2 3.25e-07 / 3.00e-05; dgamma 3.25e-07 / 3.00e-05
    dbeta 1.18e-07 / 3.00e-05
  block (17, 8, 64, 4, 'pointwise'), near-kink examples: 0 of 17
    y 8.14e-07 / 1.00e-05; dx 1.11e-06 / 3.00e-05; dWa 6.31e-07 / 3.00e-05
    dba 5.64e-07 / 3.00e-05; dWb 6.06e-07 / 3.00e-05; dbb 4.98e-07 / 3.00e-05
    dW1 8.32e-07 / 3.00e-05; dW2 7.20e-07 / 3.00e-05; dgamma 6.39e-07 / 3.00e-05
    dbeta 1.43e-07 / 3.00e-05
  block (17, 64, 8, 4, 'single'), near-kink examples: 0 of 17
    y 2.98e-06 / 1.00e-05; dx 1.73e-06 / 3.00e-05; dWa 1.78e-06 / 3.00e-05
    dba 1.87e-06 / 3.00e-05; dWb 3.79e-06 / 3.00e-05; dbb 3.41e-06 / 3.00e-05
    dW1 1.88e-06 / 3.00e-05; dgamma 9.28e-07 / 3.00e-05; dbeta 1.29e-07 / 3.00e-05
  block (33, 64, 1, 3, 'pointwise'), near-kink examples: 0 of 33
    y 0.00e+00 / 1.00e-05; dx 0.00e+00 / 4.32e+25; dWa 0.00e+00 / 9.47e+25
    dba 0.00e+00 / 5.16e+25; dWb 0.00e+00 / 3.56e+26; dbb 0.00e+00 / 8.00e+25
    dW1 0.00e+00 / 3.72e+25; dW2 0.00e+00 / 5.07e+25; dgamma 0.00e+00 / 4.86e+25
    dbeta 2.20e-07 / 3.00e-05
  block (4099, 13, 16, 3, 'pointwise'), near-kink examples: 45 of 4099
    y 1.39e-06 / 1.00e-05; dx 9.15e-07 / 3.00e-05; dWa 6.61e-07 / 3.00e-05
    dba 4.81e-07 / 3.00e-05; dWb 7.18e-07 / 3.00e-05; dbb 4.38e-07 / 3.00e-05
    dW1 5.07e-07 / 3.00e-05; dW2 5.63e-07 / 3.00e-05; dgamma 5.30e-07 / 3.00e-05
    dbeta 1.31e-07 / 3.00e-05
  block (4099, 13, 16, 3, 'single'), near-kink examples: 34 of 4099
    y 1.25e-06 / 1.00e-05; dx 9.73e-07 / 3.00e-05; dWa 6.55e-07 / 3.00e-05
    dba 4.96e-07 / 3.00e-05; dWb 6.73e-07 / 3.00e-05; dbb 4.17e-07 / 3.00e-05
    dW1 5.03e-07 / 3.00e-05; dgamma 4.33e-07 / 3.00e-05; dbeta 1.06e-07 / 3.00e-05
  block (2049, 26, 16, 3, 'pointwise'), near-kink examples: 45 of 2049
    y 2.88e-06 / 1.00e-05; dx 1.63e-06 / 3.00e-05; dWa 7.17e-07 / 3.00e-05
    dba 6.42e-07 / 3.00e-05; dWb 8.60e-07 / 3.00e-05; dbb 5.80e-07 / 3.00e-05
    dW1 8.22e-07 / 3.00e-05; dW2 5.19e-07 / 3.00e-05; dgamma 4.91e-07 / 3.00e-05
    dbeta 1.25e-07 / 3.00e-05
  layer pointwise, block_num = 2, B = 32 (digest): output 7.27e-07 / 1.00e-05; 118 gradients, the largest ratios:
    0.nonlinear_layer_list.9.W1 2.04e-06 / 3.00e-05
    0.nonlinear_layer_list.2.ln.gamma 2.24e-06 / 3.00e-05
    0.nonlinear_layer_list.4.ln.gamma 1.98e-06 / 3.00e-05
  layer single, block_num = 3, B = 32 (digest): output 1.41e-06 / 1.00e-05; 135 gradients, the largest ratios:
    final_mlp.layers.2.bias 1.59e-05 / 4.86e-05
    1.nonlinear_layer_list.9.ln.beta 3.80e-06 / 3.00e-05
    0.nonlinear_layer_list.5.ln.gamma 3.52e-06 / 3.00e-05
"""
import functools

import numpy as np
import pytest
import torch

from tests import contextnet_ref as CR

pytestmark = pytest.mark.gpu

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]
KEYS = [c + "_key" for c in CONT]
VALS = [c + "_value" for c in CONT]
F32 = np.float32
PW, SINGLE = "pointwise", "single"


def cu(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def f32_exact(a):
    return np.asarray(a).astype(F32).astype(np.float64)


def check(name, got, want, t32, floor):
    err, bound = CR.rel_err(got, want), max(floor, 4 * CR.rel_err(t32, want))
    print("%-12s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    assert err <= bound, (name, err, bound)


# ---- input stage ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def input_case(B, Fc, Fk, E, V=5000, special=False):
    r = np.random.default_rng(B * 7 + Fc)
    table, X, values = CR.make_input(r, B, Fc, Fk, E, V)
    if special and Fk:                                   # values exactly 0 and negative ones
        values[::3, 0] = 0.0
        values[1::3, -1] = -np.abs(values[1::3, -1]) - 0.5
    table, values = f32_exact(table), f32_exact(values)
    dx = f32_exact(r.uniform(-1, 1, (B, (Fc + Fk) * E)))
    ref = CR.input_stage_numpy(table, X, values, dx)
    t32 = CR.input_stage_torch_grads(table, X, values, dx, torch.float32)
    return dict(table=table, X=X, values=values, dx=dx, ref=ref, t32=t32)


def run_input(c):
    from explicit_tf2_recommendation_amd import ops
    Fk = c["values"].shape[1]
    table, X, dx = cu(c["table"]), cu(c["X"], np.int64), cu(c["dx"])
    values = cu(c["values"]) if Fk else None
    flag = ops.new_flag(table.device)
    x = ops.emb_contextnet_in_fwd(table, X, values, flag)
    vals = ops.emb_contextnet_in_bwd(dx, values, c["X"].shape[1])
    return x, vals, int(flag.item())


INPUT_CASES = [(1, 1, 0, 1), (2, 1, 1, 3), (17, 10, 3, 16), (17, 61, 3, 8), (4099, 10, 3, 16),
               (100, 10, 3, 16, 5000, True)]


@pytest.mark.parametrize("case", INPUT_CASES, ids=lambda c: "x".join(str(int(v)) for v in c))
def test_input_stage_matches_fp64(case):
    c = input_case(*case)
    x, vals, flag = run_input(c)
    assert flag == 0
    ref, (tx, tt) = c["ref"], c["t32"]
    B, F = c["X"].shape
    Fc = F - c["values"].shape[1]
    rows = c["table"].astype(F32)[c["X"]]
    rows[:, Fc:] *= c["values"].astype(F32)[:, :, None]
    assert np.array_equal(x.cpu().numpy(), rows.reshape(B, -1))               # table[X] times the value, bit for bit
    dtable = np.zeros_like(c["table"])
    np.add.at(dtable, c["X"], vals.cpu().numpy().astype(np.float64).reshape(B, F, -1))
    check("dtable", dtable, ref["dtable"], tt, 3e-5)
    check("vals", vals.cpu().numpy(), ref["vals"], ref["vals"], 3e-5)
    if len(case) == 6:
        assert np.count_nonzero(vals.cpu().numpy().reshape(B, F, -1)[::3, Fc]) == 0    # value 0: no gradient


@pytest.mark.parametrize("col", [2, 11], ids=["categorical", "key"])
def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows(col):
    c = dict(input_case(17, 10, 3, 16))
    X = c["X"].copy()
    X[3, col], X[9, col] = 5000, -1
    c["X"] = X
    x, vals, flag = run_input(c)
    assert flag == 1
    ref = CR.input_stage_numpy(c["table"], X, c["values"], c["dx"])
    e = x.cpu().numpy().reshape(17, 13, 16)
    assert np.count_nonzero(e[3, col]) == 0 and np.count_nonzero(e[9, col]) == 0
    assert CR.rel_err(x.cpu().numpy(), ref["x"]) <= 1e-5 and CR.rel_err(vals.cpu().numpy(), ref["vals"]) <= 3e-5


# ---- block ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def block_case(B, F, E, R, mode):
    def gen(seed):
        r = np.random.default_rng(seed)
        params = [f32_exact(p) for p in CR.make_block(r, F, E, R, mode)]
        return r, params, f32_exact(r.normal(0, 1, (B, F * E)))

    def near_of(s):
        _, params, x = gen(s)
        return CR.block_numpy(x, params, mode)["pre"] < CR.PRE_EPS

    seed = CR.clean_seed(lambda s: near_of(s).any()) if B < 100 else 1      # on the fp64 reading alone
    r, params, x = gen(seed)
    near = near_of(seed)
    assert near.mean() <= 0.10 and (B >= 100 or not near.any())
    dy = f32_exact(r.uniform(-1, 1, (B, F * E)))
    dy[near] = 0.0
    ref = CR.block_numpy(x, params, mode, dy)
    t32 = CR.block_torch_grads(x, params, mode, dy, torch.float32)
    return dict(params=params, x=x, dy=dy, ref=ref, t32=t32, near=near, mode=mode)


def dev_params(c):
    """the device operands in the order of ops.contextnet_block_fwd: W2 is None in single mode"""
    p = [cu(a) for a in c["params"]]
    return p if c["mode"] == PW else p[:5] + [None] + p[5:]


def run_block(c, save=True):
    from explicit_tf2_recommendation_amd import ops
    x, dy, p = cu(c["x"]), cu(c["dy"]), dev_params(c)
    y, saved = ops.contextnet_block_fwd(x, *p, save=save)
    if not save:
        return y
    dx, g = ops.contextnet_block_bwd(x, p[0], p[2], p[4], p[5], p[6], saved, dy)
    return y, dx, g, saved


BLOCK_CASES = [(1, 1, 1, 1, PW), (2, 3, 5, 2, PW), (5, 13, 10, 3, PW), (17, 13, 16, 3, PW), (17, 13, 16, 3, SINGLE),
               (33, 7, 33, 1, PW), (17, 8, 64, 4, PW), (17, 64, 8, 4, SINGLE), (33, 64, 1, 3, PW), (4099, 13, 16, 3, PW),
               (4099, 13, 16, 3, SINGLE), (2049, 26, 16, 3, PW),
               # slice edges of the small weight-gradient launch (csrc/tile_ops.h): two unequal slices; sixteen, the last empty
               (513, 3, 5, 2, PW), (4097, 3, 5, 2, PW), (4097, 3, 5, 2, SINGLE)]
GRAD_NAMES = ["dWa", "dba", "dWb", "dbb", "dW1", "dW2", "dgamma", "dbeta"]


@pytest.mark.parametrize("case", BLOCK_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_block_matches_fp64(case):
    c = block_case(*case)
    print("near-kink examples: %d of %d" % (c["near"].sum(), len(c["near"])))
    y, dx, g, saved = run_block(c)
    ref, (ty, tdx, tg) = c["ref"], c["t32"]
    names = [n for n in GRAD_NAMES if n != "dW2" or c["mode"] == PW]
    got = [t for t in g if t is not None]
    assert len(got) == len(names) == len(ref["dparams"]) and (g[5] is None) == (c["mode"] != PW)
    if case[:4] == (1, 1, 1, 1):                          # LayerNorm over one element: exact in every tensor
        assert np.array_equal(y.cpu().numpy(), ref["y"].astype(F32))
        assert np.count_nonzero(dx.cpu().numpy()) == 0 and np.count_nonzero(ref["dx"]) == 0
        for t, want in zip(got, ref["dparams"]):
            assert np.array_equal(t.cpu().numpy().reshape(want.shape), want.astype(F32))
    check("y", y.cpu().numpy(), ref["y"], ty, 1e-5)
    check("dx", dx.cpu().numpy(), ref["dx"], tdx, 3e-5)
    for name, t, want, w32 in zip(names, got, ref["dparams"], tg):
        check(name, t.cpu().numpy().reshape(want.shape), want, w32, 3e-5)
    assert torch.equal(run_block(c, save=False), y)      # inference writes the same y, bitwise


def test_every_output_is_bit_identical_run_to_run():
    c = block_case(4099, 13, 16, 3, PW)
    a, b = run_block(c), run_block(c)
    flat = lambda o: [o[0], o[1], *[t for t in o[2] if t is not None], *[t for t in o[3] if t is not None]]
    assert len(flat(a)) == 2 + 8 + 5
    for s, t in zip(flat(a), flat(b)):
        assert torch.equal(s, t)
    ci = input_case(4099, 10, 3, 16)
    for s, t in zip(run_input(ci)[:2], run_input(ci)[:2]):
        assert torch.equal(s, t)


def test_graph_replay_equals_eager():
    """Forward + backward of the input stage and two blocks captured in one hipGraph, replayed twice."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    ci, c1, c2 = input_case(4099, 10, 3, 16), block_case(4099, 13, 16, 3, PW), block_case(4099, 13, 16, 3, SINGLE)
    table, X, values = cu(ci["table"]), cu(ci["X"], np.int64), cu(ci["values"])
    p1, p2 = dev_params(c1), dev_params(c2)
    dy = cu(c2["dy"])

    def step():
        x = ops.emb_contextnet_in_fwd(table, X, values)
        y1, s1 = ops.contextnet_block_fwd(x, *p1)
        y2, s2 = ops.contextnet_block_fwd(y1, *p2)
        dx2, g2 = ops.contextnet_block_bwd(y1, p2[0], p2[2], p2[4], p2[5], p2[6], s2, dy)
        dx1, g1 = ops.contextnet_block_bwd(x, p1[0], p1[2], p1[4], p1[5], p1[6], s1, dx2)
        vals = ops.emb_contextnet_in_bwd(dx1, values, 13)
        return [y2, dx1, vals, *[t for t in g1 + g2 if t is not None]]

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
    c = block_case(2, 3, 5, 2, PW)
    x, dy, p = cu(c["x"]), cu(c["dy"]), dev_params(c)
    bwd = lambda xx, sv, g: ops.contextnet_block_bwd(xx, p[0], p[2], p[4], p[5], p[6], sv, g)
    with pytest.raises(RuntimeError):
        ops.contextnet_block_fwd(x.cpu(), *p)                                 # no CPU fallback
    with pytest.raises(ValueError):
        ops.contextnet_block_fwd(x[:, :14].contiguous(), *p)
    with pytest.raises(ValueError):
        ops.contextnet_block_fwd(x, p[0], p[1][:-1].contiguous(), *p[2:])
    with pytest.raises(ValueError):
        ops.contextnet_block_fwd(x, *p[:5], p[5][:2].contiguous(), *p[6:])    # W2 of another shape than W1
    y, saved = ops.contextnet_block_fwd(x, *p)
    with pytest.raises(ValueError):
        bwd(x, saved, dy[:, :3].contiguous())
    with pytest.raises(ValueError):
        bwd(x, saved[:4] + (None,), dy)                                       # pointwise needs a
    with pytest.raises(RuntimeError):
        bwd(x, saved, dy.cpu())
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(NotImplementedError):                                  # F E = 513
        ops.contextnet_block_fwd(z(2, 513), z(513, 513), z(513), z(513, 513), z(513), z(27, 19, 19), None, z(27, 19),
                                 z(27, 19))
    with pytest.raises(NotImplementedError):                                  # R = 5
        ops.contextnet_block_fwd(z(2, 8), z(8, 40), z(40), z(40, 8), z(8), z(2, 4, 4), None, z(2, 4), z(2, 4))
    with pytest.raises(NotImplementedError):                                  # E = 65
        ops.contextnet_block_fwd(z(2, 65), z(65, 65), z(65), z(65, 65), z(65), z(1, 65, 65), None, z(1, 65), z(1, 65))
    ye, se = ops.contextnet_block_fwd(x[:0], *p)
    assert tuple(ye.shape) == (0, 15) and tuple(se[0].shape) == (0, 30) and tuple(se[3].shape) == (0, 3)
    dx, g = bwd(x[:0], se, dy[:0])
    assert tuple(dx.shape) == (0, 15) and all(float(t.abs().sum()) == 0 for t in g)
    assert [tuple(t.shape) for t in g] == [(15, 30), (30,), (30, 15), (15,), (3, 5, 5), (3, 5, 5), (3, 5), (3, 5)]

    ci = input_case(2, 1, 1, 3)
    table, X, values = cu(ci["table"]), cu(ci["X"], np.int64), cu(ci["values"])
    with pytest.raises(RuntimeError):
        ops.emb_contextnet_in_fwd(table.cpu(), X, values)
    with pytest.raises(ValueError):
        ops.emb_contextnet_in_fwd(table, X, values[:1].contiguous())
    with pytest.raises(ValueError):
        ops.emb_contextnet_in_fwd(table, X.reshape(-1), values)
    with pytest.raises(NotImplementedError):
        ops.emb_contextnet_in_fwd(table, torch.zeros(2, 65, dtype=torch.int64, device="cuda"), None)
    xe = ops.emb_contextnet_in_fwd(table, X[:0], values[:0])
    assert tuple(xe.shape) == (0, 6)
    assert tuple(ops.emb_contextnet_in_bwd(xe, values[:0], 2).shape) == (0, 3)
    with pytest.raises(ValueError):
        ops.emb_contextnet_in_bwd(z(2, 5), values, 2)


# ---- layers ---------------------------------------------------------------------------------------------------------
LAYER_B, LAYER_V = 32, 1000


def _ref_names(mode, NB):
    """(table, blocks, head) parameter names in the layout of tests/contextnet_ref.py: per block the Dense kernels and
    biases, then the lists of the 13 fields' W1, (W2,) gamma, beta"""
    blocks = []
    for k in range(NB):
        ce = "context_block_list.%d.ce_layer.contextual_embedding_transform.layers." % k
        nl = "context_block_list.%d.nonlinear_layer_list.%%d.%%s" % k
        per_field = ["W1"] + (["W2"] if mode == PW else []) + ["ln.gamma", "ln.beta"]
        blocks.append([ce + "0.kernel", ce + "0.bias", ce + "2.kernel", ce + "2.bias"]
                      + [[nl % (f, s) for f in range(13)] for s in per_field])
    head = ["final_mlp.layers.0.kernel", "final_mlp.layers.0.bias", "final_mlp.layers.1.alpha", "final_mlp.layers.2.kernel",
            "final_mlp.layers.2.bias"]
    return "embedding_layer.embeddings", blocks, head


def _named(mode, NB, table, blocks, head):
    """reference-layout arrays -> {state-dict name: array}"""
    nt, nbl, nh = _ref_names(mode, NB)
    out = {nt: table}
    for names, bp in zip(nbl, blocks):
        for n, a in zip(names, bp):
            if isinstance(n, list):
                out.update({nf: a[f] for f, nf in enumerate(n)})
            else:
                out[n] = a
    out.update({n: a.reshape(-1) if n.endswith(("bias", "alpha")) else a for n, a in zip(nh, head)})
    return out


@functools.lru_cache(maxsize=None)
def _layer_setup(mode, NB, seed):
    """parameters on the test scale and a batch, all from ``seed`` -> (table, X, values, blocks, head), fp32-exact"""
    from explicit_tf2_recommendation_amd import data
    r = np.random.default_rng(seed)
    table = f32_exact(r.normal(0, 0.5, (LAYER_V, 16)))
    blocks = [[f32_exact(p) for p in CR.make_block(r, 13, 16, 3, mode)] for _ in range(NB)]
    head = [f32_exact(p) for p in CR.make_head(r, 208)]
    batch = data.SyntheticGenerator(CAT + KEYS, LAYER_V, continuous=VALS, seed=seed).batch(LAYER_B)
    X = np.stack([np.asarray(batch[n]).reshape(-1) for n in CAT + KEYS], axis=1).astype(np.int64)
    values = np.stack([np.asarray(batch[n], np.float64).reshape(-1) for n in VALS], axis=1)
    return batch, (table, X, values, blocks, head)


@pytest.mark.parametrize("mode,NB", [(PW, 2), (SINGLE, 3)])
def test_layer_parity_with_the_torch_cpu_transcription(mode, NB):
    from explicit_tf2_recommendation_amd import data, layers

    def near(seed):
        return (CR.contextnet_numpy(*_layer_setup(mode, NB, seed)[1], mode)["pre"] < CR.PRE_EPS).any()

    seed = CR.clean_seed(near)                           # under 100 examples: a seed without a near-kink example
    batch, args = _layer_setup(mode, NB, seed)
    sd = _named(mode, NB, args[0], args[3], args[4])
    lay = layers.ContextNetLayer(feature_dims=LAYER_V, block_num=NB, nonlinear_type=mode).cuda()
    with torch.no_grad():
        for k, p in lay.named_parameters():
            p.copy_(torch.from_numpy(sd[k].astype(F32)).reshape(p.shape))
    lay.train()
    out = lay(data.to_device(batch))["output"]
    assert tuple(out.shape) == (LAYER_B, 1)
    gout = np.random.default_rng(0).uniform(-1, 1, (LAYER_B, 1)).astype(F32)
    out.backward(torch.from_numpy(gout).cuda())
    ref = CR.contextnet_numpy(*args, mode, gout)
    assert not (ref["pre"] < CR.PRE_EPS).any()
    t64 = CR.contextnet_torch_grads(*args, mode, gout, torch.float64)
    t32 = CR.contextnet_torch_grads(*args, mode, gout, torch.float32)
    assert CR.rel_err(t64[0], ref["output"]) < 1e-12
    check("output", out.detach().cpu().numpy(), t64[0], t32[0], 1e-5)
    want, w32 = _named(mode, NB, *t64[1:]), _named(mode, NB, *t32[1:])
    grads = {k: (p.grad.to_dense() if p.grad.is_sparse else p.grad).cpu().numpy() for k, p in lay.named_parameters()}
    assert grads.keys() == want.keys()
    for name in want:
        check(name.replace("context_block_list.", "").replace("contextual_embedding_transform.", "")[-40:],
              grads[name].reshape(want[name].shape), want[name], w32[name], 3e-5)


@pytest.mark.parametrize("mode", [PW, SINGLE])
def test_direct_calls_of_the_sub_layers_match_the_transcription(mode):
    """NonLinearFeedforwardLayer and ContextualEmbeddingLayer called on their own (the block layer runs them inside its
    kernel): composed from the GEMM, activation and LayerNorm kernels, against fp64."""
    from explicit_tf2_recommendation_amd import layers
    c = block_case(17, 13, 16, 3, mode)
    p, x = c["params"], c["x"]
    x3 = torch.from_numpy(x).reshape(17, 13, 16)
    nl = layers.NonLinearFeedforwardLayer(embedding_dims=16, mode=mode).cuda()
    assert hasattr(nl, "W2") == (mode == PW)
    ce = layers.ContextualEmbeddingLayer(fields_num=13, embedding_dims=16).cuda()
    f = 5
    with torch.no_grad():
        nl.W1.copy_(cu(p[4][f]))
        if mode == PW:
            nl.W2.copy_(cu(p[5][f]))
        nl.ln.gamma.copy_(cu(p[-2][f]))
        nl.ln.beta.copy_(cu(p[-1][f]))
        d1, _, d2 = ce.contextual_embedding_transform.layers
        for dst, src in ((d1.kernel, p[0]), (d1.bias, p[1]), (d2.kernel, p[2]), (d2.bias, p[3])):
            dst.copy_(cu(src))
    xin = cu(x3[:, f, :].numpy()).requires_grad_()
    out = nl(xin)
    g = np.random.default_rng(1).uniform(-1, 1, (17, 16)).astype(F32)
    out.backward(cu(g))
    xr = x3[:, f, :].clone().requires_grad_()
    o = xr @ torch.from_numpy(p[4][f])
    if mode == PW:
        o = torch.relu(o) @ torch.from_numpy(p[5][f]) + xr
    want = torch.nn.functional.layer_norm(o, (16,), torch.from_numpy(p[-2][f]), torch.from_numpy(p[-1][f]), CR.EPS)
    want.backward(torch.from_numpy(g).double())
    assert CR.rel_err(out.detach().cpu().numpy(), want.detach().numpy()) <= 1e-5
    assert CR.rel_err(xin.grad.cpu().numpy(), xr.grad.numpy()) <= 3e-5
    mask = ce(cu(x3.numpy()))
    assert tuple(mask.shape) == (17, 13, 16)
    m64 = np.maximum(x @ p[0] + p[1], 0) @ p[2] + p[3]
    assert CR.rel_err(mask.detach().cpu().numpy().reshape(17, -1), m64) <= 1e-5


def test_out_of_range_key_raises():
    from explicit_tf2_recommendation_amd import data, layers
    lay = layers.ContextNetLayer(feature_dims=100, block_num=2).cuda()
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
                        embedding_dims=16, lr=lr, batch=B, layer="ContextNet", engine=engine)


def test_model_manager_trains_contextnet_graphed_like_eager():
    from explicit_tf2_recommendation_amd import data, layers
    a, b = _manager("eager"), _manager("auto")
    assert isinstance(a.layer, layers.ContextNetLayer)
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
