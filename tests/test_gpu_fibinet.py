"""GPU tests of the FiBiNet layer (csrc/fibinet.hip): the kernels against fp64 for every bilinear type at F = 10 and 26,
an edge-shape sweep, run-to-run determinism, graph replay, layer parity against the torch-CPU restatement of
FiBiNetLayer (tests/fibinet_ref.py), out-of-range ids, and the ModelManager choice layer='FiBiNet'."""
import numpy as np
import pytest
import torch

from tests import fibinet_ref as FR

pytestmark = pytest.mark.gpu

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]
TYPES = {"all": 0, "each": 1, "interaction": 2}


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def make_inputs(B, F, E, C, mid, bilinear_type, seed, senet_off=False):
    """SENet weights keep every ReLU pre-activation clear of 0: x > 0 makes Z > 0, S0 > 0.05 makes H1 > 0, S1 > 0.05
    makes A > 0 (fp32 and fp64 then agree on the masks).  senet_off: S1 <= 0, so A == 0."""
    r = np.random.default_rng(seed)
    x = r.uniform(0.05, 1, size=(B, F, E)).astype(np.float32)
    xc = r.uniform(-1, 1, size=(B, C)).astype(np.float32)
    S0 = (r.uniform(0.05, 1, size=(F, mid)) / np.sqrt(F)).astype(np.float32)
    S1 = (r.uniform(0.05, 1, size=(mid, F)) / np.sqrt(mid)).astype(np.float32)
    if senet_off:
        S1 = -S1
    nW = {"all": 1, "each": F - 1, "interaction": F * (F - 1) // 2}[bilinear_type]
    W = (r.standard_normal((nW, E, E)) / np.sqrt(E)).astype(np.float32)
    P = F * (F - 1) // 2
    g = r.uniform(-1, 1, size=(B, 2 * P * E + C)).astype(np.float32)
    return x, xc, S0, S1, W, g


def ref(x, xc, S0, S1, W, g, bilinear_type, chunk=512):
    """fp64 reference-order reading (FR.fibinet_torch) and its autograd, in chunks of examples."""
    B = x.shape[0]
    outs, dxs = [], []
    dS0, dS1, dW = np.zeros(S0.shape), np.zeros(S1.shape), np.zeros(W.shape)
    for s in range(0, B, chunk):
        xt = torch.from_numpy(x[s:s + chunk]).double().requires_grad_()
        s0 = torch.from_numpy(S0).double().requires_grad_()
        s1 = torch.from_numpy(S1).double().requires_grad_()
        wt = [torch.from_numpy(w).double().requires_grad_() for w in W]
        out = FR.fibinet_torch(xt, torch.from_numpy(xc[s:s + chunk]).double(), s0, s1, wt, bilinear_type)
        out.backward(torch.from_numpy(g[s:s + chunk]).double())
        outs.append(out.detach().numpy())
        dxs.append(xt.grad.numpy())
        dS0 += s0.grad.numpy()
        dS1 += s1.grad.numpy()
        dW += np.stack([w.grad.numpy() for w in wt])
    return np.concatenate(outs), np.concatenate(dxs), dW, dS0, dS1


def run_gpu(x, xc, S0, S1, W, g, bilinear_type):
    from explicit_tf2_recommendation_amd import ops
    d = [torch.from_numpy(a).cuda() for a in (x, xc, S0, S1, W, g)]
    out, A, H1 = ops.fibinet_fwd(d[0], d[1], d[2], d[3], d[4], TYPES[bilinear_type])
    dx, dW, dS0, dS1 = ops.fibinet_bwd(d[0], d[5], A, H1, d[2], d[3], d[4], TYPES[bilinear_type])
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in (out, dx, dW, dS0, dS1, A)]


def check_against_ref(B, F, E, C, mid, bilinear_type, seed, tol_out=1e-5, tol_grad=3e-5, senet_off=False):
    args = make_inputs(B, F, E, C, mid, bilinear_type, seed, senet_off)
    got = run_gpu(*args, bilinear_type)
    want = ref(*args, bilinear_type)
    P = F * (F - 1) // 2
    for name, sl in (("raw", slice(0, P * E)), ("senet", slice(P * E, 2 * P * E)), ("cont", slice(2 * P * E, None))):
        if want[0][:, sl].size and np.abs(want[0][:, sl]).max() > 0:
            assert rel(got[0][:, sl], want[0][:, sl]) <= tol_out, name
        else:
            assert np.array_equal(got[0][:, sl], want[0][:, sl].astype(np.float32)), name
    for k, name in ((1, "dx"), (2, "dW"), (3, "dS0"), (4, "dS1")):
        if senet_off and name in ("dS0", "dS1"):
            assert np.array_equal(got[k], np.zeros_like(got[k])), name
        else:
            assert rel(got[k], want[k]) <= tol_grad, name
    return got


@pytest.mark.parametrize("bilinear_type", list(TYPES))
@pytest.mark.parametrize("F", [10, 26])
def test_kernels_match_fp64(F, bilinear_type):
    """F = 10 (the reference's default input set) and F = 26, E = 16, 3 continuous columns, mid = F // 3."""
    check_against_ref(2048, F, 16, 3, max(1, F // 3), bilinear_type, seed=F + TYPES[bilinear_type])


EDGES = [
    (37, 2, 16, 3, 1, "interaction"),
    (37, 2, 16, 0, 1, "all"),
    (19, 32, 16, 3, 10, "interaction"),
    (19, 32, 8, 2, 32, "each"),
    (53, 5, 1, 1, 1, "interaction"),
    (53, 5, 3, 4, 2, "each"),
    (53, 7, 64, 3, 2, "interaction"),
    (33, 6, 64, 64, 6, "all"),
    (1, 10, 16, 3, 3, "interaction"),
    (1, 3, 5, 0, 1, "each"),
    (1000, 10, 16, 0, 3, "all"),
    (33, 11, 40, 5, 1, "interaction"),
]


@pytest.mark.parametrize("B,F,E,C,mid,bilinear_type", EDGES)
def test_kernels_edge_shapes(B, F, E, C, mid, bilinear_type):
    check_against_ref(B, F, E, C, mid, bilinear_type, seed=B + F + E)


@pytest.mark.parametrize("bilinear_type", list(TYPES))
def test_senet_off_gives_an_exactly_zero_senet_half(bilinear_type):
    """S1 <= 0: A == 0, so the SENet pairs, dS0 and dS1 are exactly 0."""
    got = check_against_ref(77, 10, 16, 3, 3, bilinear_type, seed=5, senet_off=True)
    assert np.array_equal(got[5], np.zeros_like(got[5]))
    P, E = 45, 16
    assert np.array_equal(got[0][:, P * E:2 * P * E], np.zeros((77, P * E), np.float32))


def test_zero_batch_is_a_no_op():
    from explicit_tf2_recommendation_amd import ops
    x = torch.zeros((0, 4, 8), device="cuda")
    out, A, H1 = ops.fibinet_fwd(x, torch.zeros((0, 2), device="cuda"), torch.ones((4, 1), device="cuda"),
                                 torch.ones((1, 4), device="cuda"), torch.ones((6, 8, 8), device="cuda"), 2)
    assert out.shape == (0, 2 * 6 * 8 + 2)


@pytest.mark.parametrize("bilinear_type", ["interaction", "all"])
def test_gradients_are_bit_identical_run_to_run(bilinear_type):
    args = make_inputs(4099, 26, 16, 3, 8, bilinear_type, seed=3)
    a, b = run_gpu(*args, bilinear_type), run_gpu(*args, bilinear_type)
    for k in range(5):
        assert np.array_equal(a[k], b[k]), k


def test_graph_replay_equals_eager():
    """Forward and backward launches captured in one hipGraph and replayed: bit-identical to the eager launches."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    x, xc, S0, S1, W, g = [torch.from_numpy(a).cuda() for a in make_inputs(2049, 10, 16, 3, 3, "interaction", 4)]

    def step():
        out, A, H1 = ops.fibinet_fwd(x, xc, S0, S1, W, 2)
        return [out, A, H1, *ops.fibinet_bwd(x, g, A, H1, S0, S1, W, 2)]

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


def _layer(bilinear_type="interaction", V=1000, B=512, seed=7):
    from explicit_tf2_recommendation_amd import layers, data
    layers.set_init_seed(seed)
    lay = layers.FiBiNetLayer(categorical_features=CAT, continuous_features=CONT, feature_dims=V, embedding_dims=16,
                              bilinear_type=bilinear_type).cuda()
    with torch.no_grad():                                   # positive embeddings and SENet weights: ReLUs clear of 0
        lay.embedding_layer.embeddings.uniform_(0.05, 1)
        lay.SENet.excitation.kernel_0.abs_().add_(0.05)
        lay.SENet.excitation.kernel_1.abs_().add_(0.05)
    batch = data.SyntheticGenerator(CAT, V, continuous=CONT, seed=seed).batch(B)
    return lay, batch


@pytest.mark.parametrize("bilinear_type", list(TYPES))
def test_layer_parity_with_the_torch_cpu_restatement(bilinear_type):
    from explicit_tf2_recommendation_amd import data
    lay, batch = _layer(bilinear_type)
    out = lay(data.to_device(batch))["output"]
    gout = np.random.default_rng(0).uniform(-1, 1, size=tuple(out.shape)).astype(np.float32)
    out.backward(torch.from_numpy(gout).cuda())

    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in lay.named_parameters()}
    p = {"embed": sd["embedding_layer.embeddings"], "S0": sd["SENet.excitation.kernel_0"],
         "S1": sd["SENet.excitation.kernel_1"], "Ws": [sd["Bilinear." + n] for n in lay.Bilinear._w_names],
         "dnn_k": [sd["dnn_layer.kernel_%d" % i] for i in range(2)],
         "dnn_b": [sd["dnn_layer.bias_%d" % i] for i in range(2)],
         "out_k": sd["output_layer.kernel"], "out_b": sd["output_layer.bias"]}
    X = torch.from_numpy(np.stack([np.asarray(batch[n]).reshape(-1) for n in CAT], axis=1)).long()
    Xc = torch.from_numpy(np.stack([np.asarray(batch[n]).reshape(-1) for n in CONT], axis=1)).double()
    want = FR.fibinet_layer_torch(p, X, Xc, bilinear_type)
    loss_want = (torch.from_numpy(gout).double() * want).sum()
    loss_want.backward()
    assert rel(out.detach().cpu().numpy(), want.detach().numpy()) <= 1e-5
    assert abs(float((torch.from_numpy(gout).cuda() * out.detach()).sum()) - loss_want.item()) <= 1e-4 * max(
        1.0, abs(loss_want.item()))
    touched = np.unique(X.numpy())
    for name, q in lay.named_parameters():
        got = q.grad
        got = (got.to_dense() if got.is_sparse else got).cpu().numpy()
        want_g = sd[name].grad.numpy()
        if name == "embedding_layer.embeddings":
            got, want_g = got[touched], want_g[touched]
        assert rel(got, want_g) <= 3e-5, name


def test_out_of_range_ids_raise():
    from explicit_tf2_recommendation_amd import data
    lay, batch = _layer(V=100, B=64)
    bad = dict(batch)
    ids = np.array(bad["itag2"]).copy()
    ids.reshape(-1)[5] = 100
    bad["itag2"] = ids
    with pytest.raises(IndexError):
        lay(data.to_device(bad))


def _manager(engine, V=5000, B=512):
    from explicit_tf2_recommendation_amd import data
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    return ModelManager(feature_names=CAT, data_info=data.data_info(V, len(CAT)), embedding_dims=16, lr=0.01, batch=B,
                        layer="FiBiNet", model_params={"units": [64, 16], "bilinear_type": "interaction"},
                        continuous_features=CONT, engine=engine)


def test_model_manager_builds_fibinet_and_graphs_it_like_eager():
    from explicit_tf2_recommendation_amd import data, layers
    a, b = _manager("eager"), _manager("auto")
    assert isinstance(a.layer, layers.FiBiNetLayer) and a.layer.bilinear_type == "interaction"
    b.model.load_state_dict(a.model.state_dict())
    gen = data.SyntheticGenerator(CAT, 5000, continuous=CONT, dist="zipf", seed=9)
    for _ in range(3):
        batch = gen.batch(512)
        la, lb = a.train_loop(dict(batch)), b.train_loop(dict(batch))
        assert la.item() == lb.item()
    assert b._eng[0] == "graphed"
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k


def test_model_manager_training_lowers_the_loss():
    from explicit_tf2_recommendation_amd import data
    mm = _manager("auto", B=1024)
    gen = data.SyntheticGenerator(CAT, 5000, continuous=CONT, seed=11)
    batches = []
    for i in range(4):
        bt = gen.batch(1024)
        bt["label"] = (np.asarray(bt["uid"]).reshape(-1, 1) % 2 == 0).astype(np.float32).reshape(
            np.asarray(bt["label"]).shape)
        batches.append(bt)
    first = [mm.train_loop(dict(bt)).item() for bt in batches]
    for _ in range(15):
        for bt in batches:
            mm.train_loop(dict(bt))
    last = [mm.train_loop(dict(bt)).item() for bt in batches]
    assert np.mean(last) < np.mean(first) - 0.05, (first, last)
