"""FinalMLP on the GPU: the body kernels (csrc/finalmlp.hip) against the fp64 numpy reading of tests/finalmlp_ref.py, the
fused layer against the torch-CPU transcription and against its own composed path, graph capture, and
ModelManager(layer='FinalMLP').

Tolerance, per tensor (the project's rule, as tests/test_gpu_mmoe.py states it): max|got - want| / max|want| against fp64
is at most 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 for forward tensors (out and
every save buffer) and 3e-5 for gradients; where the fp64 tensor is zero throughout the kernel's is exactly zero (the
gradient of a Dense bias in front of a batch-statistics BatchNorm is: sum_b dz = 0 identically).  The moving statistics
after one training call: the same 4 x, floor 1e-6 (the figure tests/test_gpu_head_edges.py quotes for test_batchnorm).
The mean row and the rstd row of ``stats`` are judged apart: a column mean of 1e3 would hide every rstd.

ReLU kinks: BatchNorm couples the examples, so no example can be taken out of a case.  Both CPU readings instead take the
branch the kernel took (read from its save buffers: hg > 0, a > 0) wherever the fp64 pre-activation lies within PRE_EPS
= 1e-5 of zero; such entries are at most 1 % of a case's relu entries, and cases under 100 examples use the first seed
without one (tests/test_finalmlp_host.py checks both on the fp64 reading alone).  The large-mean column of the special
case keeps its relu open (beta = 5): it is about the tile merge, and its xhat carries the rounding of z near 1e3.

First run (one MI355X), ``name error / bound`` (830 lines; per tensor group the largest error and the largest ratio to
its bound over all 27 tests, then the lines above a ratio of 0.2):
  out        max error 4.63e-06, max ratio 0.23
  saves      max error 4.97e-06, max ratio 0.26   (hg, g, z, a, stats.mean, stats.rstd)
  gradients  max error 9.14e-06, max ratio 0.25   (dxs, dx1, dx2 and the 29 / 21 / 13 packed gradients)
  moving     max error 1.15e-07, max ratio 0.09   (floor 1e-6)
  pinned relu entries: 3.81e-06 of the two 2049-example cases (3 of 786816), 0 of every other case
  a              error/bound 3.25e-06 / 1.27e-05 = 0.26      (large-mean column, B = 2049)
  dW_1_1         error/bound 9.14e-06 / 3.73e-05 = 0.25
  dgamma_1_0     error/bound 8.20e-06 / 3.32e-05 = 0.25
  dxs            error/bound 7.28e-06 / 3.00e-05 = 0.24
  out            error/bound 4.63e-06 / 2.02e-05 = 0.23
  dx1            error/bound 6.92e-06 / 3.00e-05 = 0.23
  out            error/bound 2.08e-06 / 1.00e-05 = 0.21
  guard bands: 12 allocations through the seam in training (11 in evaluation), 564 B at B = 1 to 5.8 MB at B = 4097
An earlier build computed 1 - momentum in fp32 (1 - 0.99f is 9.5e-7 off 0.01, relatively): the moving mean of the
large-mean column then stood at 9.34e-07 against the 1e-6 floor; eps and momentum are doubles in the ABI since.
"""
import functools

import numpy as np
import pytest
import torch

from tests import finalmlp_ref as FR
from tests import guarded as G

pytestmark = pytest.mark.gpu
F32 = np.float32
SMALL = (2, 15, 5, 10, 3, 7, (5, 7), (12, 4), 1, 2)
DEFAULT33 = (33,) + FR.DEFAULT_DIMS
USER = ["uid", "utag1", "utag2", "utag3", "utag4"]
ITEM = ["iid", "itag1", "itag2", "itag3", "itag4"]


def cu(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def check(name, got, want, t32, floor):
    err, bound = FR.rel_err(got, want), max(floor, 4 * FR.rel_err(t32, want))
    print("%-14s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


def dims_of(case):
    return (case[4], case[5], list(case[6]), list(case[7]), case[8], case[9])


@functools.lru_cache(maxsize=None)
def dev_case(case, training=True, special=False):
    c = FR.body_case(case, training, special)
    return (cu(c["xs"]), cu(c["x1"]), cu(c["x2"]), cu(FR.pack(c["params"])), [cu(m) for m in c["moving"]], cu(c["dout"]))


def run_body(case, training=True, special=False, ops=None, backward=True, save=True):
    """-> (out, saved, (dxs, dx1, dx2, dparams), moving after the call); the cached moving statistics stay untouched"""
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    xs, x1, x2, params, moving, dout = dev_case(case, training, special)
    moving = [m.clone() for m in moving]
    half = len(moving) // 2
    out, saved = ops.finalmlp_fwd(xs, x1, x2, params, moving[:half], moving[half:], dims_of(case), training, save=save)
    if not backward:
        return out, saved, None, moving
    return out, saved, ops.finalmlp_bwd(xs, x1, x2, params, saved, out, dout, dims_of(case), training), moving


def compare_with_readings(case, training, special, res):
    c = FR.body_case(case, training, special)
    share = FR.pinned_share(c)
    print("pinned relu entries: %.2e of the case" % share)
    assert share <= 0.01 and (case[0] >= 100 or share == 0.0)
    out, saved, (dxs, dx1, dx2, dparams), moving = res
    n = lambda t: t.cpu().numpy()
    pin = dict(h=n(saved[0]) > 0, y=n(saved[3]) > 0)        # the branch the kernel took, from what it saved
    ref, (tout, tdx, tdp, tsaved) = FR.case_ref(c, pin), FR.case_t32(c, pin)
    check("out", n(out), ref["out"], tout, 1e-5)
    for name, t in zip(FR.SAVED[:4], saved):
        check(name, n(t), ref[name], tsaved[name], 1e-5)
    for row, name in enumerate(("stats.mean", "stats.rstd")):
        check(name, n(saved[4])[row], ref["stats"][row], tsaved["stats"][row], 1e-5)
    for k, (got, want, w32) in enumerate(zip(moving, ref["moving"], tsaved["moving"])):
        check("moving[%d]" % k, n(got), want, w32, 1e-6)
    for name, got, want, w32 in zip(("dxs", "dx1", "dx2"), (dxs, dx1, dx2), (ref["dxs"], ref["dx1"], ref["dx2"]), tdx):
        check(name, n(got), want, w32, 3e-5)
    names = [nm for nm, _ in FR.shapes(*case[1:])]
    for name, got, want, w32 in zip(names, FR.unpack(n(dparams), case[1:]), ref["dparams"], tdp):
        check("d" + name, got, want, w32, 3e-5)
    return c, ref


@pytest.mark.parametrize("case", FR.BODY_CASES, ids=lambda c: "B%d-D%d-L%d-n%d-o%d" % (c[0], c[1], len(c[6]), c[8], c[9]))
def test_body_matches_fp64(case):
    res = run_body(case)
    c, ref = compare_with_readings(case, True, False, res)
    if case[0] == 1:             # one row: xhat is exactly 0, every BatchNorm output equals beta, bitwise
        a = res[1][3].cpu().numpy()
        names = [nm for nm, _ in FR.shapes(*case[1:])]
        betas = [c["params"][names.index("beta_%d_%d" % (s, l))] for l in range(len(case[6])) for s in (1, 2)]
        assert np.array_equal(a[0], np.maximum(np.concatenate(betas), 0).astype(F32))
        assert np.array_equal(res[1][4].cpu().numpy()[1], np.full(a.shape[1], F32(1.0) / np.sqrt(F32(1e-3)), F32))


@pytest.mark.parametrize("B", FR.SPECIAL_BATCHES)
def test_constant_and_large_mean_columns(B):
    """One constant column (variance 0) and one column with a layer-0 bias of 1e3: the tile merge does not cancel."""
    case = (B,) + FR.DEFAULT_DIMS
    res = run_body(case, special=True)
    compare_with_readings(case, True, True, res)
    z, a, stats = (t.cpu().numpy() for t in res[1][2:5])
    assert np.ptp(z[:, FR.CONST_COL]) == 0 and stats[0, FR.CONST_COL] == z[0, FR.CONST_COL]      # mean exact, variance 0
    assert stats[1, FR.CONST_COL] == F32(1.0) / np.sqrt(F32(1e-3)) and np.ptp(a[:, FR.CONST_COL]) == 0
    assert abs(stats[0, FR.BIG_COL] - 1e3) < 1 and 0.5 < 1 / stats[1, FR.BIG_COL] < 2


@pytest.mark.parametrize("case", [SMALL, DEFAULT33], ids=["small", "default33"])
def test_evaluation_mode_uses_the_moving_statistics_in_one_launch(case):
    from explicit_tf2_recommendation_amd import ops
    res = run_body(case, training=False)
    compare_with_readings(case, False, False, res)
    before = dev_case(case, False)[4]
    assert all(torch.equal(a, b) for a, b in zip(res[3], before))            # nothing moved
    out_only = run_body(case, training=False, backward=False, save=False)
    assert out_only[1] is None and torch.equal(out_only[0], res[0])           # NULL save buffers: the same out, bitwise
    xs, x1, x2, params, moving, _ = dev_case(case, False)
    half, L = len(moving) // 2, len(case[6])

    def kernels(training):
        mv = [m.clone() for m in moving]
        torch.cuda.synchronize()
        with torch.profiler.profile(activities=[torch.profiler.ProfilerActivity.CUDA]) as prof:
            ops.finalmlp_fwd(xs, x1, x2, params, mv[:half], mv[half:], dims_of(case), training)
            torch.cuda.synchronize()
        return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "finalmlp" in e.name)

    assert kernels(False) == 1 and kernels(True) == 2 * L + 1


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_every_output_is_bit_identical_run_to_run(training):
    case = (2049,) + FR.DEFAULT_DIMS
    flat = lambda r: [r[0], *r[1], *r[2], *r[3]]
    a, b = flat(run_body(case, training)), flat(run_body(case, training))
    assert len(a) == 1 + 5 + 4 + 12
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_cpu_tensors_strides_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import functional as Fn, ops
    xs, x1, x2, params, moving, dout = dev_case(SMALL)
    dims, half = dims_of(SMALL), len(moving) // 2
    mm, mv = moving[:half], moving[half:]
    fwd = lambda *a, **k: ops.finalmlp_fwd(*a, **k)
    with pytest.raises(RuntimeError):
        fwd(xs.cpu(), x1, x2, params, mm, mv, dims, True)                    # no CPU fallback
    with pytest.raises(RuntimeError):
        fwd(xs, x1, x2, params.cpu(), mm, mv, dims, True)
    wide = torch.zeros(2, 30, device="cuda")
    wide[:, ::2] = xs
    with pytest.raises(ValueError):                                          # strided: rejected like the siblings'
        fwd(wide[:, ::2], x1, x2, params, mm, mv, dims, True)
    mv2 = [m.clone() for m in moving]
    out = Fn.FinalMLPBody.apply(wide[:, ::2], x1, x2, params, mv2, dims, True, 1e-3, 0.99)   # the Function makes it so
    assert torch.equal(out, run_body(SMALL)[0])
    with pytest.raises(ValueError):
        fwd(xs, x1[:1].contiguous(), x2, params, mm, mv, dims, True)
    with pytest.raises(ValueError):
        fwd(xs, x1, x2, params[:-1].contiguous(), mm, mv, dims, True)
    with pytest.raises(ValueError):
        fwd(xs, x1, x2, params, mm[:-1], mv, dims, True)
    with pytest.raises(ValueError):
        fwd(xs, x1, x2, params, mm, mv, dims[:4] + (5, 2), True)             # five heads do not divide 7 and 4
    with pytest.raises(ValueError):
        fwd(xs, x1, x2, params, mm, mv, dims, True, save=False)
    out, saved = fwd(xs, x1, x2, params, [m.clone() for m in mm], [m.clone() for m in mv], dims, True)
    with pytest.raises(ValueError):
        ops.finalmlp_bwd(xs, x1, x2, params, saved, out, dout[:, :1].contiguous(), dims, True)
    with pytest.raises(ValueError):
        ops.finalmlp_bwd(xs, x1, x2, params, saved[:4] + (None,), out, dout, dims, True)
    z = lambda *s: torch.zeros(*s, device="cuda")

    def past(D=4, D1=4, D2=4, Hg1=2, Hg2=2, w1=(4,), w2=(4,), n=2, o=1):
        total = sum(int(np.prod(s)) for _, s in FR.shapes(D, D1, D2, Hg1, Hg2, w1, w2, n, o))
        wm = [z(w) for w in list(w1) + list(w2)]
        with pytest.raises(NotImplementedError):
            fwd(z(2, D), z(2, D1), z(2, D2), z(total), wm, wm, (Hg1, Hg2, list(w1), list(w2), n, o), True)

    past(D=513), past(D1=513), past(D2=513), past(Hg1=129), past(Hg2=129), past(w1=(130,)), past(w2=(4, 130, 4), w1=(4,) * 3)
    past(w1=(4,) * 5, w2=(4,) * 5), past(o=5), past(w2=(128,), n=1, o=2)
    oe, se = fwd(xs[:0], x1[:0], x2[:0], params, mm, mv, dims, True)
    assert tuple(oe.shape) == (0, 2) and [tuple(t.shape) for t in se] == [(0, 10), (0, 30), (0, 28), (0, 28), (2, 28)]
    g = ops.finalmlp_bwd(xs[:0], x1[:0], x2[:0], params, se, oe, dout[:0], dims, True)
    assert [tuple(t.shape) for t in g] == [(0, 15), (0, 5), (0, 10), tuple(params.shape)] and float(g[3].abs().sum()) == 0


# ---- guard bands and poison under every allocation of the wrappers --------------------------------------------------
def _driver(ops, case, training):
    out, saved, grads, moving = run_body(case, training, ops=ops)
    return out, saved, grads, moving


GUARD_CASES = [(FR.BODY_CASES[0], True), (SMALL, True), (SMALL, False), (DEFAULT33, True),
               ((513,) + SMALL[1:], True), ((4097,) + SMALL[1:], True), ((4097,) + SMALL[1:], False)]


@pytest.mark.parametrize("case,training", GUARD_CASES, ids=lambda v: "B%d" % v[0] if isinstance(v, tuple) else str(v))
def test_guards_and_poison(case, training):
    from explicit_tf2_recommendation_amd import ops
    want = G.flatten(_driver(ops, case, training))
    with G.guarded(ops, G.POISON_NAN) as g:
        nan_run = G.flatten(_driver(ops, case, training))
    print("%d allocations, %d bytes through the seam, queries %s" % (len(g.allocations), g.total_bytes(), g.queries))
    assert len(g.allocations) >= 11
    for i, t in enumerate(nan_run):
        assert bool(torch.isfinite(t).all()), "returned tensor %d %s holds poison or a non-finite value" % (i, tuple(t.shape))
    for i, (a, b) in enumerate(zip(nan_run, want)):
        assert G.bit_equal(a, b), "0xFF poison against the plain run: tensor %d %s differs" % (i, tuple(a.shape))
    with G.guarded(ops, G.POISON_FINITE):
        fin_run = G.flatten(_driver(ops, case, training))
    for i, (a, b) in enumerate(zip(fin_run, nan_run)):
        assert G.bit_equal(a, b), "0x7F poison against 0xFF poison: tensor %d %s differs" % (i, tuple(a.shape))


# ---- graph capture --------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_moves_the_statistics_alike():
    """Forward + backward in one hipGraph: every replay gives the eager bits, and after k replays the moving statistics
    are those after k eager calls."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    case = DEFAULT33
    xs, x1, x2, params, moving0, dout = dev_case(case)
    dims, half = dims_of(case), len(moving0) // 2

    def step(moving):
        out, saved = ops.finalmlp_fwd(xs, x1, x2, params, moving[:half], moving[half:], dims, True)
        return [out, *saved, *ops.finalmlp_bwd(xs, x1, x2, params, saved, out, dout, dims, True)]

    K = 3
    eager_mv = [m.clone() for m in moving0]
    eager = [[t.clone() for t in step(eager_mv)] for _ in range(K)]
    graph_mv = [m.clone() for m in moving0]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        step(graph_mv)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        static = step(graph_mv)
    for m, m0 in zip(graph_mv, moving0):
        m.copy_(m0)                                          # the warm-up moved them; capturing does not
    for k in range(K):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager[k]):
            assert torch.equal(a, b)
    for a, b, m0 in zip(graph_mv, eager_mv, moving0):
        assert torch.equal(a, b) and not torch.equal(a, m0)


# ---- layers ---------------------------------------------------------------------------------------------------------
LAYER_B, LAYER_V = 32, 1000
LAYER_DIMS = FR.DEFAULT_DIMS


@functools.lru_cache(maxsize=None)
def _layer_setup(seed):
    r = np.random.default_rng(seed)
    tables = [FR.f32_exact(r.normal(0, 0.5, (LAYER_V, 16))) for _ in range(3)]
    params, moving = FR.make_body(r, *LAYER_DIMS)
    params, moving = [FR.f32_exact(p) for p in params], [FR.f32_exact(m) for m in moving]
    Xu, Xi = r.integers(0, LAYER_V, (LAYER_B, 5)), r.integers(0, LAYER_V, (LAYER_B, 5))
    return tables, params, moving, Xu.astype(np.int64), Xi.astype(np.int64)


def _layer_ref(seed, training, gout=None, dtype=None):
    tables, params, moving, Xu, Xi = _layer_setup(seed)
    w1, w2, n = LAYER_DIMS[5], LAYER_DIMS[6], LAYER_DIMS[7]
    if gout is not None:
        return FR.layer_torch_grads(tables, Xu, Xi, params, moving, w1, w2, n, training, gout, dtype)
    rows = lambda t, X: t[X].reshape(LAYER_B, -1)
    return FR.body_numpy(rows(tables[0], np.concatenate([Xu, Xi], 1)), rows(tables[1], Xi), rows(tables[2], Xu), params,
                         moving, w1, w2, n, training)


def _clean_layer_seed(training):
    return FR.clean_seed(lambda s: any(v.any() for v in FR.near_of(_layer_ref(s, training)).values()))


def _make_layer(seed, fused):
    from explicit_tf2_recommendation_amd import layers
    tables, params, moving, Xu, Xi = _layer_setup(seed)
    lay = layers.FinalMLPLayer(feature_dims=LAYER_V, fs1_feature_dims=LAYER_V, fs2_feature_dims=LAYER_V, fused=fused).cuda()
    sd = FR.state_dict_of(tables, params, moving, 3)
    assert sd.keys() == lay.state_dict().keys()
    lay.load_state_dict({k: torch.from_numpy(np.asarray(v, F32)) for k, v in sd.items()})
    inputs = {k: cu(Xu[:, i], np.int64) for i, k in enumerate(USER)}
    inputs.update({k: cu(Xi[:, i], np.int64) for i, k in enumerate(ITEM)})
    return lay, inputs


def _layer_run(lay, inputs, training, gout):
    lay.train(training)
    lay.zero_grad(set_to_none=True)
    res = lay(inputs)
    assert res.keys() == {"output"} and tuple(res["output"].shape) == (LAYER_B, 1)
    (res["output"] * cu(gout)).sum().backward()
    grads = {k: (p.grad.to_dense() if p.grad.is_sparse else p.grad).cpu().numpy() for k, p in lay.named_parameters()}
    buffers = {k: b.cpu().numpy().copy() for k, b in lay.named_buffers()}
    return res["output"].detach().cpu().numpy(), grads, buffers


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_layer_parity_with_the_torch_cpu_transcription_and_the_composed_path(training):
    seed = _clean_layer_seed(training)                       # under 100 examples: a seed without a near-kink entry
    tables, params, moving, Xu, Xi = _layer_setup(seed)
    gout = np.random.default_rng(0).uniform(-1, 1, (LAYER_B, 1)).astype(F32)
    t64, t32 = (_layer_ref(seed, training, gout, dt) for dt in (torch.float64, torch.float32))
    assert FR.rel_err(t64[0], _layer_ref(seed, training)["out"]) < 1e-12
    L = 3
    want, w32 = FR.state_dict_of(t64[1], t64[2], t64[3], L), FR.state_dict_of(t32[1], t32[2], t32[3], L)
    zero = [k for k, v in want.items() if k.startswith("mlp") and k.endswith(".bias")] if training else []
    results = {}
    for fused in (True, False):
        lay, inputs = _make_layer(seed, fused)
        assert lay.fused is fused
        out, grads, buffers = results[fused] = _layer_run(lay, inputs, training, gout)
        print("fused" if fused else "composed")
        check("output", out, t64[0], t32[0], 1e-5)
        assert grads.keys() | buffers.keys() == want.keys() and len(grads) == 40 and len(buffers) == 12
        for k in grads:
            if k in zero and fused:                          # autograd's fp64 leaves 1e-17 there, the hand reading zero
                assert not np.any(grads[k]), (k, "identically zero: the kernel writes exact zeros")
                continue
            if k in zero:
                # identically zero; the composed path adds B roundings of dz: at most the gradient floor of sum_b |dz|
                scale = _layer_body64(seed, training)["bias_scale"]["b_%s_%d" % (k[3], int(k.split(".")[2]) // 3)]
                assert np.abs(grads[k]).max() <= 3e-5 * scale, k
                continue
            check(k[-30:], grads[k].reshape(np.shape(want[k])), want[k], w32[k], 3e-5)
        for k in buffers:
            check(k[-30:], buffers[k], want[k], w32[k], 1e-6)
    # and the two paths against each other, under the same rule: each within its bound of the fp64 reading was shown
    # above; the distance between them is at most the sum
    for k in results[True][1]:
        if k in zero:
            continue
        a, b = results[True][1][k], results[False][1][k]
        bound = 2 * max(3e-5, 4 * FR.rel_err(w32[k], want[k]))
        assert FR.rel_err(a.reshape(np.shape(want[k])), b.reshape(np.shape(want[k]))) <= bound, k


@functools.lru_cache(maxsize=None)
def _layer_body64(seed, training):
    tables, params, moving, Xu, Xi = _layer_setup(seed)
    rows = lambda t, X: t[X].reshape(LAYER_B, -1)
    gout = np.random.default_rng(0).uniform(-1, 1, (LAYER_B, 1)).astype(F32)
    return FR.body_numpy(rows(tables[0], np.concatenate([Xu, Xi], 1)), rows(tables[1], Xi), rows(tables[2], Xu), params,
                         moving, LAYER_DIMS[5], LAYER_DIMS[6], LAYER_DIMS[7], training, gout)


def test_ids_as_vectors_and_as_columns_give_the_same_bits():
    lay, inputs = _make_layer(1, True)
    lay.eval()
    with torch.no_grad():
        a = lay(inputs)["output"]
        b = lay({k: v.reshape(-1, 1) for k, v in inputs.items()})["output"]
    assert torch.equal(a, b)
    bad = dict(inputs)
    bad["itag2"] = inputs["itag2"].clone()
    bad["itag2"][5] = LAYER_V
    with pytest.raises(IndexError):
        lay(bad)


# ---- ModelManager ---------------------------------------------------------------------------------------------------
def _manager(engine, V=5000, B=512):
    from explicit_tf2_recommendation_amd import data
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    return ModelManager(feature_names=USER + ITEM, data_info=data.data_info(V, 10), embedding_dims=16, lr=0.01, batch=B,
                        layer="FinalMLP", engine=engine)


def test_model_manager_trains_graphed_like_eager():
    from explicit_tf2_recommendation_amd import data, layers
    a, b = _manager("eager"), _manager("auto")
    assert type(a.layer) is layers.FinalMLPLayer and a.layer.fused and a.layer.user_features == USER
    b.model.load_state_dict(a.model.state_dict())
    a._metric_reset()
    b._metric_reset()
    gen = data.SyntheticGenerator(USER + ITEM, 5000, dist="zipf", seed=9)
    for _ in range(4):
        batch = gen.batch(512)
        la, lb = a.train_loop(dict(batch)), b.train_loop(dict(batch))
        assert np.isfinite(la.item()) and la.item() == lb.item()
    assert b._eng[0] == "graphed"
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k
    moved = 0
    for (k, p), (_, q) in zip(a.model.named_buffers(), b.model.named_buffers()):
        assert torch.equal(p, q), k
        moved += int(k.endswith("moving_mean") and bool(p.abs().max() > 0))
    assert moved == 6
    ra, rb = a._metric_result(), b._metric_result()
    assert ra.keys() == rb.keys() == {"auc", "loss"} and ra == rb and all(np.isfinite(v) for v in ra.values())
