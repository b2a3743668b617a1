"""PLE on the GPU: the CGC-level kernels (csrc/ple.hip) against the fp64 numpy reading of tests/ple_ref.py, whole bodies
chained through functional.PLELevel, the layer against the torch-CPU transcription, inference, bit identity run to run,
graph capture, engine.GraphedTrainStep with three labels, and the error paths.

Tolerance, per tensor (the project's rule, as tests/test_gpu_mmoe.py restates it): max|got - want| / max|want| against
fp64 must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors:
y, out and the four save buffers) / 3e-5 (gradients).  An example whose smallest |relu pre-activation| in fp64, over h,
e and q, is below PRE_EPS = 1e-5 may take the other branch in fp32: its dy and dout rows are zeroed before either side
runs, every case asserts such examples are at most 10 % (tests/test_ple_host.py checks the same without a GPU), and
cases under 100 examples use the first seed 1, 2, 3, ... without any (chosen on the fp64 reading alone).  Where the fp64
value of a tensor is zero throughout, the kernels must return exact zeros.

Measured on the MI355X (21 passed in 5 s): the printout of the kernels as committed, every tensor of every level case as
`name error / bound`, three to a line; the three body cases and the layer case are given as a DIGEST (the output, the
three largest error / bound ratios and the number of gradients).
  level (1, 1, 1, 1, 1, 1, 1, 1, 1, 1), near-kink examples: 0 of 1
    y 0.00e+00 / 1.00e-05; out 2.02e-09 / 1.00e-05; h 2.40e-08 / 1.00e-05
    e 0.00e+00 / 1.00e-05; q 0.00e+00 / 1.00e-05; g 0.00e+00 / 1.00e-05
    dxin 0.00e+00 / 3.00e-05; dW1 0.00e+00 / 3.00e-05; db1 0.00e+00 / 3.00e-05
    dWe2 0.00e+00 / 3.00e-05; dbe2 0.00e+00 / 3.00e-05; dWg2 0.00e+00 / 3.00e-05
    dbg2 0.00e+00 / 3.00e-05; dWg3s 0.00e+00 / 3.00e-05; dWtw 0.00e+00 / 3.00e-05
    dbtw 9.88e-09 / 3.00e-05
  level (2, 15, 1, 2, 2, 1, 5, 3, 2, 0), near-kink examples: 0 of 2
    y 8.77e-08 / 1.00e-05; h 9.56e-08 / 1.00e-05; e 8.29e-08 / 1.00e-05
    q 2.67e-07 / 1.00e-05; g 3.18e-08 / 1.00e-05; dxin 1.40e-07 / 3.00e-05
    dW1 1.18e-07 / 3.00e-05; db1 1.77e-07 / 3.00e-05; dWe2 1.30e-07 / 3.00e-05
    dbe2 7.72e-08 / 3.00e-05; dWg2 9.39e-08 / 3.00e-05; dbg2 1.58e-07 / 3.00e-05
    dWg3s 3.65e-07 / 3.00e-05; dWg3h 0.00e+00 / 3.00e-05
  level (33, 72, 1, 3, 3, 3, 64, 8, 8, 0), near-kink examples: 0 of 33
    y 2.26e-07 / 1.00e-05; h 2.54e-07 / 1.00e-05; e 1.75e-07 / 1.00e-05
    q 1.61e-07 / 1.00e-05; g 2.33e-07 / 1.00e-05; dxin 4.61e-07 / 3.00e-05
    dW1 2.69e-07 / 3.00e-05; db1 2.45e-07 / 3.00e-05; dWe2 2.58e-07 / 3.00e-05
    dbe2 2.33e-07 / 3.00e-05; dWg2 2.76e-07 / 3.00e-05; dbg2 3.45e-07 / 3.00e-05
    dWg3s 5.93e-07 / 3.00e-05; dWg3h 3.95e-07 / 3.00e-05
  level (33, 8, 4, 3, 3, 3, 64, 8, 8, 1), near-kink examples: 0 of 33
    y 1.28e-07 / 1.00e-05; out 1.16e-07 / 1.00e-05; h 9.51e-08 / 1.00e-05
    e 1.35e-07 / 1.00e-05; q 1.16e-07 / 1.00e-05; g 1.14e-07 / 1.00e-05
    dxin 3.86e-07 / 3.00e-05; dW1 1.54e-07 / 3.00e-05; db1 1.34e-07 / 3.00e-05
    dWe2 2.64e-07 / 3.00e-05; dbe2 8.16e-08 / 3.00e-05; dWg2 6.81e-07 / 3.00e-05
    dbg2 3.83e-07 / 3.00e-05; dWg3s 4.30e-07 / 3.00e-05; dWtw 1.13e-07 / 3.00e-05
    dbtw 5.60e-08 / 3.00e-05
  level (17, 8, 4, 3, 3, 3, 64, 8, 8, 0), near-kink examples: 0 of 17
    y 1.73e-07 / 1.00e-05; h 8.94e-08 / 1.00e-05; e 1.41e-07 / 1.00e-05
    q 1.64e-07 / 1.00e-05; g 1.50e-07 / 1.00e-05; dxin 3.16e-07 / 3.00e-05
    dW1 2.16e-07 / 3.00e-05; db1 2.11e-07 / 3.00e-05; dWe2 1.54e-07 / 3.00e-05
    dbe2 1.01e-07 / 3.00e-05; dWg2 2.34e-07 / 3.00e-05; dbg2 3.31e-07 / 3.00e-05
    dWg3s 1.96e-07 / 3.00e-05; dWg3h 3.52e-07 / 3.00e-05
  level (17, 72, 1, 3, 3, 3, 64, 8, 8, 1), near-kink examples: 0 of 17
    y 2.00e-07 / 1.00e-05; out 1.13e-07 / 1.00e-05; h 2.44e-07 / 1.00e-05
    e 2.59e-07 / 1.00e-05; q 2.41e-07 / 1.00e-05; g 2.30e-07 / 1.00e-05
    dxin 6.05e-07 / 3.00e-05; dW1 1.40e-07 / 3.00e-05; db1 1.29e-07 / 3.00e-05
    dWe2 1.27e-07 / 3.00e-05; dbe2 1.03e-07 / 3.00e-05; dWg2 2.13e-07 / 3.00e-05
    dbg2 1.92e-07 / 3.00e-05; dWg3s 2.41e-07 / 3.00e-05; dWtw 2.92e-07 / 3.00e-05
    dbtw 1.25e-07 / 3.00e-05
  level (17, 40, 1, 2, 3, 2, 48, 4, 6, 0), near-kink examples: 0 of 17
    y 2.50e-07 / 1.00e-05; h 2.03e-07 / 1.00e-05; e 2.00e-07 / 1.00e-05
    q 2.03e-07 / 1.00e-05; g 2.22e-07 / 1.00e-05; dxin 3.81e-07 / 3.00e-05
    dW1 4.20e-07 / 3.00e-05; db1 2.99e-07 / 3.00e-05; dWe2 1.83e-07 / 3.00e-05
    dbe2 1.78e-07 / 3.00e-05; dWg2 3.35e-07 / 3.00e-05; dbg2 4.27e-07 / 3.00e-05
    dWg3s 7.70e-08 / 3.00e-05; dWg3h 2.06e-07 / 3.00e-05
  level (17, 512, 1, 4, 2, 2, 128, 12, 8, 0), near-kink examples: 0 of 17
    y 5.08e-07 / 1.00e-05; h 5.97e-07 / 1.00e-05; e 5.40e-07 / 1.00e-05
    q 3.14e-07 / 1.00e-05; g 3.11e-07 / 1.00e-05; dxin 9.28e-07 / 3.00e-05
    dW1 3.51e-07 / 3.00e-05; db1 2.93e-07 / 3.00e-05; dWe2 4.52e-07 / 3.00e-05
    dbe2 1.67e-07 / 3.00e-05; dWg2 5.92e-07 / 3.00e-05; dbg2 5.83e-07 / 3.00e-05
    dWg3s 1.60e-06 / 3.00e-05; dWg3h 2.25e-07 / 3.00e-05
  level (2049, 72, 1, 3, 3, 3, 64, 8, 8, 0), near-kink examples: 16 of 2049
    y 3.35e-07 / 1.00e-05; h 4.10e-07 / 1.00e-05; e 2.73e-07 / 1.00e-05
    q 3.49e-07 / 1.00e-05; g 6.10e-07 / 1.00e-05; dxin 6.06e-07 / 3.00e-05
    dW1 5.19e-07 / 3.00e-05; db1 4.12e-07 / 3.00e-05; dWe2 5.58e-07 / 3.00e-05
    dbe2 1.87e-07 / 3.00e-05; dWg2 7.63e-07 / 3.00e-05; dbg2 7.07e-07 / 3.00e-05
    dWg3s 6.61e-07 / 3.00e-05; dWg3h 3.39e-07 / 3.00e-05
  level (2049, 8, 4, 3, 3, 3, 64, 8, 8, 1), near-kink examples: 15 of 2049
    y 2.87e-07 / 1.00e-05; out 1.54e-07 / 1.00e-05; h 1.04e-07 / 1.00e-05
    e 2.27e-07 / 1.00e-05; q 2.50e-07 / 1.00e-05; g 2.33e-07 / 1.00e-05
    dxin 3.56e-07 / 3.00e-05; dW1 2.18e-07 / 3.00e-05; db1 1.14e-07 / 3.00e-05
    dWe2 3.30e-07 / 3.00e-05; dbe2 1.78e-07 / 3.00e-05; dWg2 3.62e-07 / 3.00e-05
    dbg2 1.51e-07 / 3.00e-05; dWg3s 3.16e-07 / 3.00e-05; dWtw 3.72e-07 / 3.00e-05
    dbtw 1.50e-07 / 3.00e-05
  body (33, 72, 3, 3, 3, 1) (digest): out 1.13e-07 / 1.00e-05; 10 gradients, the largest ratios:
    dx 1.05e-06 / 3.00e-05; L0 db1 1.56e-07 / 3.00e-05; L0 dWe2 2.10e-07 / 3.00e-05
  body (33, 72, 3, 3, 3, 2) (digest): out 1.02e-07 / 1.00e-05; 18 gradients, the largest ratios:
    L0 dWg3h 1.18e-06 / 3.00e-05; L0 dWg2 7.61e-07 / 3.00e-05; L0 dbg2 9.32e-07 / 3.00e-05
  body (33, 72, 3, 3, 3, 3) (digest): out 9.51e-08 / 1.00e-05; 26 gradients, the largest ratios:
    L2 dbtw 1.08e-06 / 3.00e-05; dx 9.91e-07 / 3.00e-05; L0 dW1 1.04e-06 / 3.00e-05
  layer PLELayer, B = 32 (digest): output 8.82e-08 / 1.00e-05; 138 gradients, the largest ratios:
    specific_gates.1.2.0.kernel_1 1.25e-06 / 3.00e-05; specific_gates.1.2.0.bias_1 1.06e-06 / 3.00e-05; specific_gates.1.2.1.kernel_0 1.28e-06 / 3.00e-05
"""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import ple_ref as PR

pytestmark = pytest.mark.gpu

CAT = ["sdk_type", "remote_host", "device_type", "dtu", "click_goods_num", "buy_click_num", "goods_show_num",
       "goods_click_num", "brand_name"]
F32 = np.float32
BIG0 = (2049, 72, 1, 3, 3, 3, 64, 8, 8, 0)
BIG1 = (2049, 8, 4, 3, 3, 3, 64, 8, 8, 1)


def cu(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def check(name, got, want, t32, floor):
    err, bound = PR.rel_err(got, want), max(floor, 4 * PR.rel_err(t32, want))
    print("%-12s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


@functools.lru_cache(maxsize=None)
def dev_case(*case):
    c = PR.level_case(*case)
    return cu(c["xin"]), [cu(p) for p in c["params"]], cu(c["dy"]), cu(c["dout"])


def run_level(case, save=True):
    from explicit_tf2_recommendation_amd import ops
    xin, w, dy, dout = dev_case(*case)
    cfg = PR.level_case(*case)["cfg"]
    y, out, saved = ops.ple_cgc_fwd(xin, w, *cfg, save=save)
    if not save:
        return y, out
    dxin, grads = ops.ple_cgc_bwd(xin, w, saved, y, out, dy, dout, *cfg)
    return y, out, saved, dxin, grads


def flat(res):
    y, out, saved, dxin, grads = res
    return [t for t in [y, out, *saved, dxin, *grads] if t is not None]


@pytest.mark.parametrize("case", PR.LEVEL_CASES, ids=lambda c: "x".join(map(str, c)))
def test_level_matches_fp64(case):
    c = PR.level_case(*case)
    near, last = c["near"], case[9]
    print("near-kink examples: %d of %d" % (near.sum(), len(near)))
    assert near.mean() <= 0.10 and (case[0] >= 100 or not near.any())
    ref, (ty, tout, tdx, tg, tsaved) = c["ref"], PR.level_case_t32(*case)
    y, out, saved, dxin, grads = run_level(case)
    check("y", y.cpu().numpy(), ref["y"], ty, 1e-5)
    assert (out is not None) == bool(last)
    if last:
        check("out", out.cpu().numpy(), ref["out"], tout, 1e-5)
    assert len(saved) == len(PR.SAVED)
    for name, t in zip(PR.SAVED, saved):
        check(name, t.cpu().numpy(), ref[name], tsaved[name], 1e-5)
    check("dxin", dxin.cpu().numpy(), ref["dxin"], tdx, 3e-5)
    assert len(grads) == len(PR.NAMES)
    for name, t, want, w32 in zip(PR.NAMES, grads, ref["dparams"], tg):
        assert (t is None) == (want is None), name
        if t is not None:
            check("d" + name, t.cpu().numpy().reshape(want.shape), want, w32, 3e-5)
    yi, oi = run_level(case, save=False)                  # inference (NULL save buffers) writes the same bits
    assert torch.equal(yi, y) and (oi is None if not last else torch.equal(oi, out))


def test_last_level_without_a_gradient_on_y_equals_a_zero_one():
    from explicit_tf2_recommendation_amd import ops
    case = (33, 8, 4, 3, 3, 3, 64, 8, 8, 1)
    xin, w, dy, dout = dev_case(*case)
    cfg = PR.level_case(*case)["cfg"]
    y, out, saved = ops.ple_cgc_fwd(xin, w, *cfg)
    a = ops.ple_cgc_bwd(xin, w, saved, y, out, None, dout, *cfg)
    b = ops.ple_cgc_bwd(xin, w, saved, y, out, torch.zeros_like(dy), dout, *cfg)
    assert torch.equal(a[0], b[0])
    for s, t in zip(a[1], b[1]):
        assert (s is None and t is None) or torch.equal(s, t)


@pytest.mark.parametrize("case", [BIG0, BIG1], ids=["first", "last"])
def test_every_output_is_bit_identical_run_to_run(case):
    a, b = flat(run_level(case)), flat(run_level(case))
    assert len(a) == len(b) == (1 + 1 + 4 + 1 + 9 if case[9] else 1 + 4 + 1 + 8)
    for s, t in zip(a, b):
        assert torch.equal(s, t)


# ---- whole bodies chained through functional.PLELevel ----------------------------------------------------------------
def run_body(case, grad=True):
    from explicit_tf2_recommendation_amd import functional as Fn
    c = PR.body_case(*case)
    T, S, Sh = c["cfg"]
    x = cu(c["x"]).requires_grad_(grad)
    levels = [[None if p is None else cu(p).requires_grad_(grad) for p in lv] for lv in c["levels"]]
    y = x.reshape(x.shape[0], 1, -1)
    for lv, w in enumerate(levels[:-1]):
        y = Fn.PLELevel.apply(y, T, S, Sh, False, *w)
        assert tuple(y.shape) == (case[0], T + 1, PR.O_REF)
    y, out = Fn.PLELevel.apply(y, T, S, Sh, True, *levels[-1])
    assert tuple(y.shape) == (case[0], T, PR.O_REF)
    if grad:
        out.backward(cu(c["dout"]))
    return out.detach(), x, levels


@pytest.mark.parametrize("case", PR.BODY_CASES, ids=lambda c: "x".join(map(str, c)))
def test_body_chained_through_the_levels_matches_fp64(case):
    c = PR.body_case(*case)
    assert not c["near"].any()
    ref, (tout, tdx, tg) = c["ref"], PR.body_case_t32(*case)
    out, x, levels = run_body(case)
    check("out", out.cpu().numpy(), ref["out"], tout, 1e-5)
    check("dx", x.grad.cpu().numpy(), ref["dx"], tdx, 3e-5)              # through every level
    for lv, w in enumerate(levels):
        for name, t, want, w32 in zip(PR.NAMES, w, ref["dparams"][lv], tg[lv]):
            assert (t is None) == (want is None), name
            if t is not None:
                check("L%d d%s" % (lv, name), t.grad.cpu().numpy().reshape(want.shape), want, w32, 3e-5)
    with torch.no_grad():                                 # nothing requires grad: nothing is saved, the same bits
        assert torch.equal(run_body(case, grad=False)[0], out)


@functools.lru_cache(maxsize=None)
def _two_level_inputs():
    c = PR.body_case(*PR.BODY_CASES[1])
    w0, w1 = [[cu(p) for p in lv] for lv in c["levels"]]
    return cu(c["x"]).reshape(33, 1, 72), cu(c["dout"]), w0, w1, c["cfg"]


def _two_levels():
    """forward and backward of a two-level body through the ops: every tensor either direction writes"""
    from explicit_tf2_recommendation_amd import ops
    x, dout, w0, w1, (T, S, Sh) = _two_level_inputs()
    y0, _, s0 = ops.ple_cgc_fwd(x, w0, T, S, Sh, False)
    y1, out, s1 = ops.ple_cgc_fwd(y0, w1, T, S, Sh, True)
    dy0, g1 = ops.ple_cgc_bwd(y0, w1, s1, y1, out, None, dout, T, S, Sh, True)
    dx, g0 = ops.ple_cgc_bwd(x, w0, s0, y0, None, dy0, None, T, S, Sh, False)
    return [t for t in [y0, *s0, y1, out, *s1, dy0, *g1, dx, *g0] if t is not None]


def test_graph_replay_equals_eager():
    """Forward + backward of both levels captured in one hipGraph, replayed twice."""
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    eager = [t.clone() for t in _two_levels()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _two_levels()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        static = _two_levels()
    assert len(static) == len(eager) == 2 * (1 + 4) + 1 + 2 + 9 + 8
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)


# ---- the layer --------------------------------------------------------------------------------------------------------
def _layer(V=PR.LAYER_V, **kw):
    from explicit_tf2_recommendation_amd import layers
    return layers.PLELayer(feature_dims=V, **kw).cuda()


def _batch_of(X):
    return {n: torch.from_numpy(np.ascontiguousarray(X[:, i:i + 1])).cuda() for i, n in enumerate(CAT)}


def test_layer_parity_with_the_torch_cpu_transcription():
    seed, table, X, levels = PR.layer_case()
    sd = PR.state_dict_of(table, levels, 3, 3, 3)
    lay = _layer()
    assert sd.keys() == dict(lay.named_parameters()).keys()
    with torch.no_grad():
        for k, p in lay.named_parameters():
            p.copy_(torch.from_numpy(np.asarray(sd[k], F32)).reshape(p.shape))
    res = lay(_batch_of(X))
    assert res.keys() == {"task_0", "task_1", "task_2"}
    assert all(tuple(v.shape) == (PR.LAYER_B, 1) for v in res.values())
    both = lay.task_outputs(_batch_of(X))
    assert tuple(both.shape) == (PR.LAYER_B, 3)
    assert all(torch.equal(both[:, i:i + 1], res["task_%d" % i]) for i in range(3))
    gout = np.random.default_rng(0).uniform(-1, 1, (PR.LAYER_B, 3)).astype(F32)
    sum((res["task_%d" % i] * cu(gout[:, i:i + 1])).sum() for i in range(3)).backward()
    t64 = PR.layer_torch_grads(table, X, levels, 3, 3, 3, gout, torch.float64)
    t32 = PR.layer_torch_grads(table, X, levels, 3, 3, 3, gout, torch.float32)
    ref = PR.body_numpy(table[X].reshape(PR.LAYER_B, -1), levels, 3, 3, 3)
    assert PR.rel_err(t64[0], ref["out"]) < 1e-12
    out = torch.cat([res["task_%d" % i] for i in range(3)], dim=1).detach().cpu().numpy()
    check("output", out, t64[0], t32[0], 1e-5)
    want, w32 = PR.state_dict_of(t64[1], t64[2], 3, 3, 3), PR.state_dict_of(t32[1], t32[2], 3, 3, 3)
    grads = {k: (p.grad.to_dense() if p.grad.is_sparse else p.grad).cpu().numpy() for k, p in lay.named_parameters()}
    assert grads.keys() == want.keys() and len(want) == 1 + 2 * 48 + 2 * 15 + 5 + 6
    for k in want:
        check(k[-30:], grads[k].reshape(np.shape(want[k])), want[k], w32[k], 3e-5)


def test_one_level_layer_and_out_of_range_ids():
    from explicit_tf2_recommendation_amd import data
    lay = _layer(V=100, level_num=1, specific_expert_num=2, shared_expert_num=1)
    batch = data.SyntheticGenerator(CAT, 100, seed=1).batch(16)
    batch.pop("label", None)
    res = lay(data.to_device(batch))
    assert res.keys() == {"task_0", "task_1", "task_2"} and all(torch.isfinite(v).all() for v in res.values())
    bad = dict(batch)
    ids = np.array(bad["dtu"]).copy()
    ids.reshape(-1)[5] = 100
    bad["dtu"] = ids
    with pytest.raises(IndexError):
        lay(data.to_device(bad))


def test_graphed_train_step_with_three_labels_trains_like_the_eager_loop():
    from explicit_tf2_recommendation_amd import data, engine
    from explicit_tf2_recommendation_amd import functional as Fn
    from explicit_tf2_recommendation_amd.model_manager import KerasAdam
    labels, B, V = ("l0", "l1", "l2"), 256, 500
    a = _layer(V=V)
    b = copy.deepcopy(a)
    gen = data.SyntheticGenerator(CAT, V, dist="zipf", seed=7)
    r = np.random.default_rng(7)
    batches = []
    for _ in range(3):
        bt = gen.batch(B)
        bt.pop("label", None)
        for n, pr in zip(labels, (0.5, 0.3, 0.1)):
            bt[n] = (r.random((B, 1)) < pr).astype(F32)
        batches.append(data.to_device(bt))
    step = engine.GraphedTrainStep(a, batches[0], label_name=labels, output_fn=lambda l, ins: l.task_outputs(ins))
    oa, ob = KerasAdam(a.parameters(), 0.01), KerasAdam(b.parameters(), 0.01)
    for bt in batches:
        la = step(bt).clone()
        oa.apply_gradients()
        ins = {k: v for k, v in bt.items() if k not in labels}
        target = torch.stack([bt[n].to(torch.float32).reshape(-1) for n in labels], dim=1)
        lb = Fn.KerasBCE.apply(b.task_outputs(ins), target)
        lb.backward()
        ob.apply_gradients()
        assert np.isfinite(la.item()) and la.item() == lb.item()
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k


# ---- error paths ------------------------------------------------------------------------------------------------------
def test_cpu_tensors_bad_shapes_limits_workspace_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd._lib import lib
    case = (2, 15, 1, 2, 2, 1, 5, 3, 2, 0)
    xin, w, dy, _ = dev_case(*case)
    cfg = (2, 2, 1, False)
    with pytest.raises(RuntimeError):
        ops.ple_cgc_fwd(xin.cpu(), w, *cfg)                                       # no CPU fallback
    with pytest.raises(RuntimeError):
        ops.ple_cgc_fwd(xin, [w[0].cpu()] + w[1:], *cfg)
    with pytest.raises(ValueError):
        ops.ple_cgc_fwd(xin[:, :, :14].contiguous(), w, *cfg)
    with pytest.raises(ValueError):
        ops.ple_cgc_fwd(xin, w[:1] + [w[1][:-1].contiguous()] + w[2:], *cfg)      # b1 one short
    with pytest.raises(ValueError):
        ops.ple_cgc_fwd(xin, w[:6] + [w[6][:, :, :2].contiguous()] + w[7:], *cfg)  # a gate over two of three experts
    with pytest.raises(ValueError):
        ops.ple_cgc_fwd(xin, w, 2, 2, 1, True)                                    # a last level with a shared gate
    with pytest.raises(ValueError):
        ops.ple_cgc_fwd(xin.expand(2, 2, 15).contiguous(), w, *cfg)               # Gin neither 1 nor T + 1
    y, out, saved = ops.ple_cgc_fwd(xin, w, *cfg)
    assert out is None
    with pytest.raises(ValueError):
        ops.ple_cgc_bwd(xin, w, saved, y, None, dy[:, :2].contiguous(), None, *cfg)
    with pytest.raises(ValueError):
        ops.ple_cgc_bwd(xin, w, saved[:3] + (None,), y, None, dy, None, *cfg)     # partial saves
    with pytest.raises(ValueError):
        ops.ple_cgc_bwd(xin, w, saved, y, None, None, None, *cfg)                 # dy is optional for the last level only
    with pytest.raises(RuntimeError):
        ops.ple_cgc_bwd(xin, w, saved, y, None, dy.cpu(), None, *cfg)
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(NotImplementedError):                                      # Din = 513
        ops.ple_cgc_fwd(z(2, 1, 513), [z(513, 4), z(4), z(2, 1, 1), z(2, 1), z(2, 1, 1), z(2, 1), z(1, 1, 2), z(1, 2),
                                       None, None], 1, 1, 1)
    with pytest.raises(NotImplementedError):                                      # five tasks
        ops.ple_cgc_fwd(z(2, 1, 4), [z(4, 12), z(12), z(6, 1, 1), z(6, 1), z(6, 1, 1), z(6, 1), z(5, 1, 2), z(1, 6),
                                     None, None], 5, 1, 1)
    # the ABI itself: partial save buffers and a workspace that is too small, on device pointers, nothing launched
    p = lambda t: None if t is None else t.data_ptr()
    dims = (2, 15, 1, 2, 2, 1, 5, 3, 2, 0)
    assert lib.rec_ple_cgc_fwd_f32(p(xin), *[p(t) for t in w], *dims, p(y), None, p(saved[0]), None, p(saved[2]),
                                   p(saved[3]), None) == -1
    need = lib.rec_ple_cgc_workspace_bytes(*dims)
    ws, gr = z(need // 4 + 1), [None if t is None else torch.zeros_like(t) for t in w]
    args = [p(xin), *[p(w[i]) for i in (0, 2, 4, 6, 7, 8)], *[p(t) for t in saved], p(y), None, p(dy), None, *dims,
            p(torch.zeros_like(xin)), *[p(t) for t in gr], p(ws)]
    assert lib.rec_ple_cgc_bwd_f32(*args, need - 32, None) == -3
    # empty batches: nothing is launched, the gradients are zeros of the weights' shapes
    ye, oe, se = ops.ple_cgc_fwd(xin[:0], w, *cfg)
    assert tuple(ye.shape) == (0, 3, 3) and oe is None
    assert [tuple(t.shape) for t in se] == [(0, 8 * 5), (0, 5 * 3), (0, 3 * 2), (0, 2 * 3 + 5)]
    dx, g = ops.ple_cgc_bwd(xin[:0], w, se, ye, None, dy[:0], None, *cfg)
    assert tuple(dx.shape) == (0, 1, 15) and all(t is None or float(t.abs().sum()) == 0 for t in g)
    assert [None if t is None else tuple(t.shape) for t in g] == [None if t is None else tuple(t.shape) for t in w]
