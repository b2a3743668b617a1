"""GPU tests of the model heads where they saturate, clip and clamp: the fused DeepFM step (csrc/deepfm_fused3.hip) and
the fused DSSM step (csrc/dssm_fused.hip) on batches with saturated predictions, dead ReLU layers, zero / tiny /
parallel / antiparallel tower outputs and confident labels, and the unfused kernels that hold the same formulas
(cosine, activations, GEMM epilogues, Dice, softmax, layer and batch norm) at large arguments and degenerate rows.

The inputs and the conditions that make an fp32-vs-fp64 comparison meaningful there are built and checked without a
GPU: tests/head_edges_ref.py, tests/test_head_edges_host.py.  Exact assertions (== 0, == 1, == 0.5) are deliberate: they
tell a masked gradient from a merely small one."""
import functools

import numpy as np
import pytest
import torch

from oracle import layers_np as L
from oracle import torch_ref as T
from tests import head_edges_ref as R
from tests import helpers as H
from tests import test_gpu_dssm_fused as D
from tests.test_gpu_engine import close, oracle_grads

pytestmark = pytest.mark.gpu

DFM_DENSE = ("MLP_layer1.kernel_0", "MLP_layer1.bias_0", "MLP_layer1.kernel_1", "MLP_layer1.bias_1",
             "MLP_layer2.kernel_0", "MLP_layer2.bias_0", "bias")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    from explicit_tf2_recommendation_amd import ops as _ops
    return _ops


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


# ------------------------------------------------------------------------------------------------
# 1. fused DeepFM step
# ------------------------------------------------------------------------------------------------
def deepfm_layer(kind):
    from explicit_tf2_recommendation_amd import layers
    layer = layers.DeepFMRankingLayer(feature_names=R.DFM_NAMES, feature_dims=R.DFM_V, embedding_dims=R.DFM_E,
                                      mlp_dims=[32, 8]).cuda()
    sd = dict(layer.named_parameters())
    with torch.no_grad():
        for n, v in R.deepfm_state(R.deepfm_params(kind)).items():
            sd[n].copy_(torch.from_numpy(v).reshape(sd[n].shape))
    return layer


class _HostLayer:
    """What oracle_grads reads of a layer, over the numpy parameters."""

    def __init__(self, state):
        self.state = state

    def named_parameters(self):
        return [(k, torch.from_numpy(v)) for k, v in self.state.items()]


@functools.lru_cache(maxsize=None)
def deepfm_ref(kind, B):
    """fp64 oracle of the mixed batch, computed once per (parameter set, B) and shared by the eager and graph runs"""
    batch, X, _ = R.deepfm_mixed(kind, B)
    loss, g = oracle_grads(_HostLayer(R.deepfm_state(R.deepfm_params(kind))), R.DFM_NAMES, batch)
    return loss, g, R.deepfm_fp64(R.deepfm_params(kind), X)[1]


def run_step(step, dbatch, use_graph):
    for _ in range(3 if use_graph else 1):                       # eager, eager + capture, replay
        loss = step(dbatch)
    if use_graph:
        assert len(step._graphs) == 1
    step.check_flags()
    return loss.item()


def deepfm_grads(step):
    g = step.gradients()
    ids, rows, nu = g["embed.embeddings"]
    nu = int(nu.item())
    out = {n: g[n].clone() for n in DFM_DENSE}
    out["ids"], out["embed"], out["w"] = ids[:nu].clone(), rows[:nu].clone(), g["w.embeddings"][1][:nu].clone()
    out["gz"], out["loss"] = step.gz.clone(), step.loss.clone()
    return out


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("B", [200, 33])
@pytest.mark.parametrize("kind", R.DFM_SETS)
def test_deepfm_mixed_batch(kind, B, use_graph):
    """Saturated (both signs, both labels), dead-first-layer and ordinary examples in one batch, the tail of the last
    workgroup included; parameter sets 'dead2' (h2 = 0 for every example) and 'zero1' (first-layer pre-activations
    exactly 0.0)."""
    from explicit_tf2_recommendation_amd import engine, data
    layer = deepfm_layer(kind)
    batch, X, cat = R.deepfm_mixed(kind, B)
    y = batch["label"][:, 0]
    step = engine.DeepFMFusedStep(layer, B, R.DFM_DIMS, R.DFM_OFFS, use_graph=use_graph, want_prob=True)
    loss = run_step(step, data.to_device(batch), use_graph)
    ref_loss64, ref, p64 = deepfm_ref(kind, B)
    prob, gz = host(step.prob), host(step.gz)
    hi, lo = cat == R.SAT_HI, cat == R.SAT_LO
    sat = hi | lo
    assert np.isfinite(prob).all() and np.isfinite(gz).all() and np.isfinite(loss)
    # the clipped examples: p == 1.0f / p < 1e-7, d loss / d z exactly zero whatever the label
    assert np.array_equal(prob[hi], np.ones(hi.sum(), np.float32))
    assert (prob[lo] < 1e-7).all()
    assert np.abs(prob[sat] - p64[sat]).max() <= 1e-6
    assert np.abs(prob - p64).max() <= 1e-5                      # (live examples: the body's fp32 error in z, |z| <= 9.2)
    assert np.array_equal(gz[sat], np.zeros(sat.sum(), np.float32))
    # the head by itself: d loss / d z restated op for op in fp32 on the kernel's own p (the body's error in z is not in it)
    gz_ref = R.gz_fp32(y, prob)
    print("gz: max-abs error %.3e, scale %.3e" % (np.abs(gz - gz_ref).max(), np.abs(gz_ref).max()))
    assert np.abs(gz - gz_ref).max() <= 1e-5 * np.abs(gz_ref).max()
    assert (gz[~sat] != 0).all()
    # the loss: fp32 restatement on the kernel's own p (a clipped, mislabelled example is 15.33 in fp32, 15.42 in fp64)
    ref_loss = float(L.bce_forward(batch["label"], prob.reshape(-1, 1), np.float32))
    print("loss %.7f, fp32 restatement %.7f, fp64 oracle %.7f" % (loss, ref_loss, ref_loss64))
    assert abs(loss - ref_loss) <= 1e-5 * max(1, abs(ref_loss))
    # every gradient against the fp64 oracle (the clipped examples contribute exactly zero in both precisions)
    g = deepfm_grads(step)
    for name in DFM_DENSE:
        got = host(g[name])
        assert np.isfinite(got).all(), name
        assert close(got, ref[name].reshape(got.shape)), name
    touched = np.unique(X)
    assert np.array_equal(host(g["ids"]), touched)
    rows_e, rows_w = host(g["embed"]), host(g["w"])
    assert np.isfinite(rows_e).all() and np.isfinite(rows_w).all()
    assert close(rows_e, ref["embed.embeddings"][touched]), "embed"
    assert close(rows_w, ref["w.embeddings"][touched]), "w"
    # ids touched by clipped examples only: listed, with gradient rows of exactly zero
    spec = np.unique(X[sat, 0])
    assert spec.size == 4 and np.isin(spec, touched).all()
    pos = np.searchsorted(touched, spec)
    assert not rows_e[pos].any() and not rows_w[pos].any()
    zero = {"mixed": (), "zero1": ("MLP_layer1.kernel_0", "MLP_layer1.bias_0", "MLP_layer1.kernel_1"),
            "dead2": ("MLP_layer1.kernel_0", "MLP_layer1.bias_0", "MLP_layer1.kernel_1", "MLP_layer1.bias_1",
                      "MLP_layer2.kernel_0")}[kind]
    for name in zero:                                            # everything behind a dead ReLU: exactly zero
        assert not host(g[name]).any(), name
    for name in set(DFM_DENSE) - set(zero):
        assert host(g[name]).any(), name


@pytest.mark.parametrize("B", [200, 33])
def test_deepfm_mixed_batch_replay_is_bit_identical(B):
    from explicit_tf2_recommendation_amd import engine, data
    layer = deepfm_layer("mixed")
    dbatch = data.to_device(R.deepfm_mixed("mixed", B)[0])
    eager = engine.DeepFMFusedStep(layer, B, R.DFM_DIMS, R.DFM_OFFS, use_graph=False, want_prob=True)
    graphed = engine.DeepFMFusedStep(layer, B, R.DFM_DIMS, R.DFM_OFFS, use_graph=True, want_prob=True)
    run_step(eager, dbatch, False)
    want = deepfm_grads(eager)
    want["prob"] = eager.prob.clone()
    run_step(eager, dbatch, False)
    run_step(graphed, dbatch, True)
    for got in (dict(deepfm_grads(eager), prob=eager.prob), dict(deepfm_grads(graphed), prob=graphed.prob)):
        for k in want:
            assert torch.equal(want[k], got[k]), k


def test_deepfm_confident_batch_loss():
    """4 <= |z| <= 9.2 with the label on z's side: a loss of order 1e-3, where an absolute 1e-5 hides several percent.
    Reference: the unfused BCE kernel (logf; pinned to the oracle by test_bce*) on the fused step's own probabilities;
    agreement within 1e-5 RELATIVE to that loss."""
    from explicit_tf2_recommendation_amd import engine, data, ops
    B = 200
    layer = deepfm_layer("mixed")
    batch, X = R.deepfm_confident(B)
    step = engine.DeepFMFusedStep(layer, B, R.DFM_DIMS, R.DFM_OFFS, use_graph=False, want_prob=True)
    loss = run_step(step, data.to_device(batch), False)
    unfused = ops.bce_fwd_bwd(dev(batch["label"]), step.prob.clone(), want_dp=False)[0].item()
    ref32 = float(L.bce_forward(batch["label"], host(step.prob).reshape(-1, 1), np.float32))
    print("confident batch: fused loss %.9e, unfused kernel %.9e (relative difference %.3e), fp32 restatement %.9e"
          % (loss, unfused, abs(loss - unfused) / unfused, ref32))
    assert 1e-4 <= unfused <= 5e-3
    assert abs(loss - unfused) <= 1e-5 * unfused
    # and the gradient of such a batch
    gz, gz_ref = host(step.gz), R.gz_fp32(batch["label"], host(step.prob))
    assert np.abs(gz - gz_ref).max() <= 1e-5 * np.abs(gz_ref).max()


# ------------------------------------------------------------------------------------------------
# 2. fused DSSM step
# ------------------------------------------------------------------------------------------------
def dssm_layer(case):
    from explicit_tf2_recommendation_amd import layers
    layer = layers.DSSMTwoTowerRetrievalLayer(u_feature_names=R.UN, i_feature_names=R.IN, u_feature_dims=R.DSSM_VU,
                                              i_feature_dims=R.DSSM_VI, u_embedding_dims=R.DSSM_E,
                                              i_embedding_dims=R.DSSM_E).cuda()
    sd = dict(layer.named_parameters())
    with torch.no_grad():
        for n, v in R.dssm_state(*R.dssm_params(case)).items():
            sd[n].copy_(torch.from_numpy(v).reshape(sd[n].shape))
    return layer


@pytest.mark.parametrize("B", [200, 33])
@pytest.mark.parametrize("case", R.DSSM_CASES)
def test_dssm_degenerate_tower_outputs(case, B):
    """Dead towers (output = final bias exactly) beside live ones, with final biases that make the dead/dead examples
    identical, opposite, zero (clamp branch, ru = 1e6), tiny (clamp active on a non-zero vector) or zero on both sides."""
    from explicit_tf2_recommendation_amd import engine
    assert D.UN == R.UN and D.IN == R.IN
    layer = dssm_layer(case)
    batch, cat = R.dssm_batch(case, B)
    dbatch = D.to_dev(batch)
    step = engine.DSSMFusedStep(layer, B, use_graph=False, want_outputs=True)
    step(dbatch)
    step.check_flags()
    _, ref, u64, i64, s64 = D.oracle(layer, batch)
    score = host(step.outputs["score"])
    ue, ie = host(step.outputs["user_embedding"]), host(step.outputs["item_embedding"])
    loss = step.loss.item()
    assert np.isfinite(score).all() and np.isfinite(ue).all() and np.isfinite(ie).all() and np.isfinite(loss)
    ref_loss = float(L.bce_forward(batch["label"], score, np.float32))
    print("loss %.7f, fp32 restatement on the kernel's scores %.7f" % (loss, ref_loss))
    assert abs(loss - ref_loss) <= 1e-5 * max(1, abs(ref_loss))
    assert np.abs(score - s64).max() <= 1e-5
    for got, want in ((ue, u64), (ie, i64)):                     # (the live outputs are of size 10 here)
        assert np.abs(got - want).max() <= 1e-5 * max(1, np.abs(want).max())
    dd = cat == R.DD
    dead_u, dead_i = dd | (cat == R.DL), dd | (cat == R.LD)
    pu, pi = R.dssm_params(case)
    assert np.array_equal(ue[dead_u], np.broadcast_to(pu["final_b"][0], ue[dead_u].shape))     # h1 = h2 = 0: O = bf exactly
    assert np.array_equal(ie[dead_i], np.broadcast_to(pi["final_b"][0], ie[dead_i].shape))
    if case == "equal":
        assert np.abs(score[dd]).max() <= 1e-6
    elif case == "opposite":
        assert np.abs(score[dd] - 1).max() <= 1e-6
    elif case == "u_zero":
        assert np.array_equal(score[dead_u], np.full(dead_u.sum(), 0.5, np.float32)) and not ue[dead_u].any()
    elif case == "both_zero":
        assert np.array_equal(score[dead_u | dead_i], np.full((dead_u | dead_i).sum(), 0.5, np.float32))
    # every gradient against torch fp64 autograd
    g = step.gradients()
    for name, want in ref.items():
        if name.endswith("embed.embeddings"):
            uniq, rows = want
            ids, got, nu = g[name]
            nu = int(nu.item())
            got = host(got)
            assert nu == uniq.size and np.array_equal(host(ids)[:nu], uniq)
            assert np.isfinite(got).all(), name
            assert D.rel(got[:nu], rows) <= 2e-5, name
            assert not got[nu:].any()
            # the id of the dead/dead examples: listed, its gradient row exactly zero
            assert uniq[R.DD_ID] == R.DD_ID and not got[R.DD_ID].any() and not got[R.DX_ID].any(), name
        else:
            got = host(g[name])
            assert np.isfinite(got).all(), name
            print("%s: relative error %.2e (scale %.2e)" % (name, D.rel(got, want), np.abs(want).max()))
            assert D.rel(got, want) <= 2e-5, name
    # replayed from a graph: bit identical
    want = D._snapshot(step)
    graphed = engine.DSSMFusedStep(layer, B, use_graph=True, want_outputs=True)
    for _ in range(3):
        graphed(dbatch)
    assert len(graphed._graphs) == 1
    for a, b in zip(want, D._snapshot(graphed)):
        assert torch.equal(a, b)
    assert torch.equal(step.outputs["score"], graphed.outputs["score"])


# ------------------------------------------------------------------------------------------------
# 3. the unfused kernels that share these formulas
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [8, 5, 64])
def test_cosine_degenerate_rows(ops, d):
    u, i = R.cosine_rows(d)
    out = host(ops.cosine_fwd(dev(u), dev(i)))
    ref = L.two_tower_score(u, i, np.float64)
    assert np.isfinite(out).all() and np.abs(out - ref).max() <= 1e-6
    assert np.array_equal(out[0:24], np.full(24, 0.5, np.float32))                   # a zero vector: cos = 0 exactly
    assert np.abs(out[32:40]).max() <= 1e-6 and np.abs(out[40:48] - 1).max() <= 1e-6 # parallel, antiparallel
    g = H.rng(d).normal(size=64).astype(np.float32)
    gu, gi = (host(t) for t in ops.cosine_bwd(dev(u), dev(i), dev(g)))
    ut, it = torch.from_numpy(u).double().requires_grad_(), torch.from_numpy(i).double().requires_grad_()
    (T.two_tower_score(ut, it) * torch.from_numpy(g).double()).sum().backward()
    assert np.isfinite(gu).all() and np.isfinite(gi).all()
    for k, kind in enumerate(R.COS_GROUPS):                      # per group: the 1e6-scaled rows must not hide the others
        rows = slice(8 * k, 8 * k + 8)
        for got, want, x in ((gu[rows], ut.grad.numpy()[rows], u[rows]), (gi[rows], it.grad.numpy()[rows], i[rows])):
            scale = np.abs(want).max()
            if kind in ("parallel", "antiparallel"):
                # the exact gradient is 0: what is left is rounding of the two terms that cancel, each of size |g| / (2 |x|)
                scale = (np.abs(g[rows]) / (2 * np.linalg.norm(x.astype(np.float64), axis=1))).max()
            assert np.abs(got - want).max() <= 1e-5 * scale, (kind, np.abs(got - want).max(), scale)


def _exact_sigmoid(x):
    """where fp32 leaves no choice: 1 - sigmoid(x) < 2^-25 for x >= 20, sigmoid(x) < 2^-150 for x <= -104.  (At x = 17,
    1 - sigmoid = 4.1e-8 lies between the half-ulps on the two sides of 1.0f: 1 / (1 + e^-x) in correctly rounded steps
    gives 1.0f, the correctly rounded sigmoid 1 - 2^-24.)"""
    return np.where(x >= 20, 1.0, np.where(x <= -104, 0.0, np.nan))


def _check_sigmoid_tanh(kind, x, y):
    x64 = x.astype(np.float64)
    assert np.isfinite(y).all(), kind
    if kind == "sigmoid":
        assert np.abs(y - R.sigmoid64(x64)).max() <= 1e-6
        want = _exact_sigmoid(x64)
    else:
        assert np.abs(y - np.tanh(x64)).max() <= 1e-6
        want = np.where(np.abs(x64) >= 17, np.sign(x64), np.where(x64 == 0, 0.0, np.nan))     # 1 - tanh(17) = 3e-15
    m = ~np.isnan(want)
    assert np.array_equal(y[m], want[m].astype(np.float32)), kind


@pytest.mark.parametrize("kind", ["sigmoid", "tanh"])
def test_act_saturated(ops, kind):
    code = ops.ACT_CODE[kind]
    x = R.GRID
    _check_sigmoid_tanh(kind, x, host(ops.act_fwd(code, dev(x))))
    # x + x2 cancelling to 0 and to +-20 (one fp32 addition, as the kernel does it)
    for x2 in (-x, (20 - x.astype(np.float64)).astype(np.float32), (-20 - x.astype(np.float64)).astype(np.float32)):
        y = host(ops.act_fwd(code, dev(x), dev(x2)))
        _check_sigmoid_tanh(kind, x + x2, y)
    y0 = host(ops.act_fwd(code, dev(x), dev(-x)))
    assert np.array_equal(y0, np.full(x.size, 0.5 if kind == "sigmoid" else 0.0, np.float32))
    # backward at saturated outputs: exactly zero
    g = H.rng(3).normal(size=8).astype(np.float32) * 1e3
    post = np.array([0, 1, 1, 0, 0, 1, 0, 1] if kind == "sigmoid" else [1, -1, 1, -1, -1, 1, 1, -1], np.float32)
    assert not host(ops.act_bwd(code, dev(post), dev(g))).any()
    assert not host(ops.act_bwd(ops.ACT_RELU, dev(np.zeros(8, np.float32)), dev(g))).any()
    mid = np.array([0.5, 0.25, 0.9, 1e-3, 0.999, 0.5, 0.1, 0.7], np.float32)
    want = g * mid * (1 - mid) if kind == "sigmoid" else g * (1 - mid * mid)
    assert np.abs(host(ops.act_bwd(code, dev(mid), dev(g))) - want).max() <= 1e-6 * np.abs(want).max()


@pytest.mark.parametrize("M", [19, 266])                         # the tile kernel; the tall-skinny kernel (M >= 256, N <= 64)
@pytest.mark.parametrize("kind", ["sigmoid", "tanh"])
def test_gemm_epilogue_saturated(ops, kind, M):
    reps = M // R.GRID.size
    A = np.zeros((M, 4), np.float32)
    A[:, 0] = np.tile(R.GRID, reps)
    A[:, 1:] = H.rng(5).normal(size=(M, 3))
    Bm = np.zeros((4, 5), np.float32)
    Bm[0] = 1.0                                                  # A @ B = the grid exactly in every column
    bias = np.array([0, 0.5, -0.5, 20, -20], np.float32)
    code = ops.EPI_BIAS_SIGMOID if kind == "sigmoid" else ops.EPI_BIAS_TANH
    C = host(ops.gemm(dev(A), dev(Bm), epi=code, bias=dev(bias)))
    _check_sigmoid_tanh(kind, A[:, :1] + bias[None, :], C)


@pytest.mark.parametrize("kind", ["sigmoid", "tanh", "dice", "prelu"])
def test_feat_act_saturated(ops, kind):
    """Per-feature activations on the grid; Dice also with var = 0 (rstd = 1/sqrt(eps)): mean = x (p = 0.5 exactly) and
    |x - mean| = 10 (p = 0 or 1 exactly)."""
    x = np.stack([R.GRID, R.GRID, R.GRID, R.GRID], axis=1)
    M, N = x.shape
    alpha = np.array([0.25, -0.1, 0.5, 0.25], np.float32)          # (columns 2, 3: products below are exact)
    mean = np.array([0.1, -0.2, 0.0, 5.0], np.float32)
    var = np.array([1.0, 0.5, 0.0, 0.0], np.float32)
    if kind == "dice":                                           # two rows more: var = 0 with mean = x and |x - mean| = 10
        x = np.concatenate([x, [[1.0, 1.0, 0.0, 5.0], [1.0, 1.0, 10.0, -5.0], [1.0, 1.0, -10.0, 15.0]]]).astype(np.float32)
        M = x.shape[0]
    g = H.rng(7).normal(size=(M, N)).astype(np.float32)
    code = ops.DACT_CODE[kind]
    a = dev(alpha) if kind in ("dice", "prelu") else None
    mv = (dev(mean), dev(var)) if kind == "dice" else (None, None)
    y = host(ops.feat_act_fwd(code, dev(x), a, *mv))
    gx, ga = ops.feat_act_bwd(code, dev(x), dev(g), a, *mv, want_alpha=a is not None)
    gx = host(gx)
    assert np.isfinite(y).all() and np.isfinite(gx).all()
    if kind in ("sigmoid", "tanh"):
        _check_sigmoid_tanh(kind, x, y)
        dref = R.sigmoid64(x) * (1 - R.sigmoid64(x)) if kind == "sigmoid" else 1 - np.tanh(x.astype(np.float64)) ** 2
        assert np.abs(gx - g * dref).max() <= 1e-6 * np.abs(g).max()
        flat = np.abs(x) >= 20 if kind == "sigmoid" else np.abs(x) >= 17
        flat &= ~((kind == "sigmoid") & (x < 0) & (x > -104))     # (sigmoid(-20 .. -89) is small, not zero)
        assert not gx[flat].any()                                # derivative exactly zero where the output is 0 / 1 / +-1
        return
    act = {"kind": kind, "alpha": torch.from_numpy(alpha).double().requires_grad_(),
           "mean": torch.from_numpy(mean).double(), "var": torch.from_numpy(var).double()}
    xt = torch.from_numpy(x).double().requires_grad_()
    yt = T._din_act(act, xt)
    (yt * torch.from_numpy(g).double()).sum().backward()
    if kind == "dice":
        with np.errstate(over="ignore"):
            assert np.abs(L.dice(x.astype(np.float64), alpha, mean, var, np.float64) - yt.detach().numpy()).max() <= 1e-9
    ga = host(ga)
    assert np.isfinite(ga).all()
    # the tolerances of test_feat_act (outputs 1e-5, gradients 3e-5, relative to max(1, |ref|)), element by element:
    # the entries of size 1e4 must not hide the others
    for got, want, tol in ((y, yt.detach().numpy(), 1e-5), (gx, xt.grad.numpy(), 3e-5)):
        assert (np.abs(got - want) <= tol * np.maximum(1, np.abs(want))).all(), kind
    want_a = act["alpha"].grad.numpy()
    assert np.abs(ga.astype(np.float64).sum(0) - want_a).max() <= 3e-5 * max(1, np.abs(want_a).max())
    if kind == "dice":
        p_half = y[M - 3, 2:]                                    # var = 0, mean = x: p = 0.5 exactly
        assert np.array_equal(p_half, (alpha[2:] * np.float32(0.5) * x[M - 3, 2:] + np.float32(0.5) * x[M - 3, 2:]))
        assert np.array_equal(y[M - 2, 2], x[M - 2, 2]) and np.array_equal(y[M - 1, 3], x[M - 1, 3])          # p = 1
        assert np.array_equal(y[M - 1, 2], alpha[2] * x[M - 1, 2]) and np.array_equal(y[M - 2, 3], alpha[3] * x[M - 2, 3])


def _prob_table(F):
    """a table of 64 rows whose ids 0..3 carry w = +25 and 4..7 w = -25; 8 examples that pick only the former, 8 only
    the latter (z = -25 F: below -89 for F = 4, where expf(-z) overflows), 16 ordinary"""
    r = H.rng(9)
    V = 64
    w = r.uniform(-0.05, 0.05, size=(V, 1)).astype(np.float32)
    w[0:4], w[4:8] = 25.0, -25.0
    X = r.integers(8, V, size=(32, F)).astype(np.int64)
    X[0:8], X[8:16] = r.integers(0, 4, size=(8, F)), r.integers(4, 8, size=(8, F))
    X[16:20, 0], X[20:24, 0] = 0, 4
    return r, V, w, X


def _check_prob(z64, z, prob):
    assert np.isfinite(prob).all() and np.isfinite(z).all()
    assert np.abs(z - z64).max() <= 1e-5 * np.abs(z64).max()
    assert np.abs(prob - R.sigmoid64(z64)).max() <= 1e-6
    assert (z64[0:8] >= 90).all() and (z64[8:16] <= -90).all() and (np.abs(z64[16:24]) >= 20).all()
    assert np.array_equal(prob[z64 >= 20], np.ones((z64 >= 20).sum(), np.float32))
    assert (prob[z64 <= -20] < 1e-7).all() and (prob[z64 <= -90] < 1e-30).all()


def test_fm_and_ffm_prob_saturated(ops):
    F, E = 4, 16
    r, V, w, X = _prob_table(F)
    bias = np.array([0.1], np.float32)
    embed = r.uniform(-0.3, 0.3, size=(V, E)).astype(np.float32)
    z, prob, _, _ = ops.emb_fm_fwd(dev(embed), dev(w), dev(bias), dev(X), want_prob=True)
    with np.errstate(over="ignore"):
        z64 = L.fm_forward(embed, w, bias, X, np.float64)[1][:, 0]
    _check_prob(z64, host(z), host(prob))
    v = r.uniform(-0.3, 0.3, size=(V, F, 8)).astype(np.float32)
    z, prob = ops.ffm_fwd(dev(v), dev(w), dev(bias), dev(X), want_prob=True)
    with np.errstate(over="ignore"):
        z64 = L.ffm_forward(v, w, bias, X, np.float64)[1][:, 0]
    _check_prob(z64, host(z), host(prob))


@pytest.mark.parametrize("N", [1, 2, 80, 1000])
def test_softmax_extreme_rows(ops, N):
    x = R.softmax_rows(N)
    y = host(ops.softmax_fwd(dev(x)))
    ref = L.softmax(x.astype(np.float64))
    assert np.isfinite(y).all()
    assert np.abs(y - ref).max() <= 1e-6                         # close(.., 1e-6) of test_layernorm_and_softmax: |ref| <= 1
    assert np.abs(y.astype(np.float64).sum(1) - 1).max() <= 1e-6
    assert np.array_equal(y[3], np.full(N, y[3, 0])) and abs(float(y[3, 0]) * N - 1) <= 1e-6       # all equal
    if N > 2:
        assert (y[2] == 0).sum() >= N // 4                       # spread 200: the far entries underflow to exactly 0
        assert y[4, N // 2] == 1.0 and not np.delete(y[4], N // 2).any()
    g = H.rng(N).normal(size=x.shape).astype(np.float32)
    gx = host(ops.softmax_bwd(dev(y), dev(g)))
    gref = ref * (g - (ref * g).sum(1, keepdims=True))
    assert np.isfinite(gx).all()
    assert np.abs(gx - gref).max() <= 3e-5 * max(1.0, np.abs(gref).max())
    assert (np.abs(gx.astype(np.float64).sum(1)) <= 1e-6 * np.abs(gx).max()).all()


def _ln_ref(x, gamma, beta, g):
    xt = torch.from_numpy(x).double().requires_grad_()
    gt = torch.from_numpy(gamma).double().requires_grad_()
    yt = torch.nn.functional.layer_norm(xt, (x.shape[1],), gt, torch.from_numpy(beta).double(), eps=1e-3)
    (yt * torch.from_numpy(g).double()).sum().backward()
    x64 = x.astype(np.float64)
    rstd = 1 / np.sqrt(x64.var(axis=1) + 1e-3)
    xhat = (x64 - x64.mean(axis=1, keepdims=True)) * rstd[:, None]
    return yt.detach().numpy(), xhat, rstd, xt.grad.numpy(), g.astype(np.float64) * xhat


@pytest.mark.parametrize("N", [1, 64, 65, 1024])
def test_layernorm_constant_and_large_mean_rows(ops, N):
    """Rows: constant (2.5: its sums and their division by N are exact in fp32, so xhat = 0 exactly is well defined),
    1e4 + 1e-2 normal, ordinary.  Reference: fp64 on the fp32 inputs.  Tolerances: those of test_layernorm_and_softmax
    (outputs 1e-5, gradients 3e-5, times max(1, |ref|)), per row, times the row's conditioning max|x| / std: one fp32
    rounding of a value of size max|x| is a relative error 2^-24 max|x| / std in x - mean."""
    r = H.rng(N)
    x = np.stack([np.full(N, 2.5), 1e4 + 1e-2 * r.normal(size=N), 3 * r.normal(size=N)]).astype(np.float32)
    gamma = r.uniform(0.5, 1.5, size=N).astype(np.float32)
    beta = r.normal(size=N).astype(np.float32)
    g = r.normal(size=x.shape).astype(np.float32)
    y, xhat, rstd = ops.layernorm_fwd(dev(x), dev(gamma), dev(beta))
    gx, gg = ops.layernorm_bwd(dev(g), xhat, rstd, dev(gamma))
    y, xhat, rstd, gx, gg = (host(t) for t in (y, xhat, rstd, gx, gg))
    ry, rxhat, rrstd, rgx, rgg = _ln_ref(x, gamma, beta, g)
    cond = R.norm_conditioning(x, 1)
    for t in (y, xhat, rstd, gx, gg):
        assert np.isfinite(t).all()
    const = [0] if N > 1 else [0, 1, 2]                          # N = 1: every row is constant
    for row in const:
        assert not xhat[row].any() and np.array_equal(y[row], beta)
        assert abs(rstd[row] - 1 / np.sqrt(1e-3)) <= 1e-5 / np.sqrt(1e-3)
    for row in range(3):
        for got, want, tol in ((y, ry, 1e-5), (xhat, rxhat, 1e-5), (gx, rgx, 3e-5), (gg, rgg, 3e-5)):
            err = np.abs(got[row] - want[row]).max()
            assert err <= tol * max(1.0, np.abs(want[row]).max()) * cond[row], (row, err, cond[row])
        assert abs(rstd[row] - rrstd[row]) <= 1e-5 * rrstd[row] * cond[row]


def test_layernorm_refuses_rows_above_1024(ops):
    """The kernels hold a row in the registers of one wave (N <= 1024): a longer row is a clean error, not a wrong
    answer."""
    x = torch.zeros((2, 1025), device="cuda")
    gamma = torch.ones(1025, device="cuda")
    with pytest.raises(NotImplementedError):
        ops.layernorm_fwd(x, gamma, gamma)
    with pytest.raises(NotImplementedError):
        ops.layernorm_bwd(x, x, torch.ones(2, device="cuda"), gamma)
    with pytest.raises(NotImplementedError):
        ops.softmax_fwd(x)


@pytest.mark.parametrize("B", [1, 2, 300])
def test_batchnorm_constant_and_large_mean_columns(ops, B):
    """Training mode, N = 19: column 0 constant (2.5), column 1 = 1e4 + 1e-2 normal, the others ordinary.  fp64
    reference on the fp32 inputs; the tolerances of test_batchnorm (outputs 1e-5, moving statistics 1e-6, gradients
    2e-5, times max(1, |ref|)), per column, times the column's conditioning max|x| / std (see the layer-norm test).
    B = 1: var = 0 and xhat = 0 exactly."""
    N = 19
    r = H.rng(B)
    x = (r.normal(size=(B, N)) * 3 + 1).astype(np.float32)
    x[:, 0] = 2.5
    x[:, 1] = 1e4 + 1e-2 * r.normal(size=B)
    gamma, beta = r.uniform(0.5, 1.5, N).astype(np.float32), r.normal(size=N).astype(np.float32)
    mm, mv = r.normal(size=N).astype(np.float32), r.uniform(0.5, 2, N).astype(np.float32)
    g = r.normal(size=(B, N)).astype(np.float32)
    dm, dv = dev(mm), dev(mv)
    y, xhat, rstd = ops.batchnorm_fwd(dev(x), dev(gamma), dev(beta), dm, dv, True)
    gx, gg, gb = ops.batchnorm_bwd(dev(g), xhat, rstd, dev(gamma), True)
    y, xhat, rstd, gx, gg, gb, nm, nv = (host(t) for t in (y, xhat, rstd, gx, gg, gb, dm, dv))
    ry, rnm, rnv = L.batchnorm_forward(x, gamma, beta, mm, mv, True, dt=np.float64)
    rgx, rgg, rgb = L.batchnorm_backward(x, gamma, g, dt=np.float64)
    cond = R.norm_conditioning(x, 0)
    for t in (y, xhat, rstd, gx, gg, gb, nm, nv):
        assert np.isfinite(t).all()
    const = [0] if B > 1 else list(range(N))
    assert not xhat[:, const].any() and (B > 1 or not gx.any())
    assert np.array_equal(y[:, const], np.broadcast_to(beta[const], (B, len(const))))
    assert np.abs(rstd[const] - 1 / np.sqrt(1e-3)).max() <= 1e-5 / np.sqrt(1e-3)
    for c in range(N):
        for got, want, tol in ((y[:, c], ry[:, c], 1e-5), (nm[c], rnm[c], 1e-6), (nv[c], rnv[c], 1e-6),
                               (gx[:, c], rgx[:, c], 2e-5), (gg[c], rgg[c], 2e-5), (gb[c], rgb[c], 2e-5)):
            err = np.abs(got - want).max()
            assert err <= tol * max(1.0, np.abs(want).max()) * cond[c], (c, err, cond[c])
