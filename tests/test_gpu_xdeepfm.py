"""GPU tests of the xDeepFM layer (csrc/cin.hip): the CIN kernels against an fp64 restatement at the reference default and
config X26, an edge-shape sweep, run-to-run determinism, graph replay, layer parity against the torch-CPU restatement of
XDeepFMRankingLayer (tests/xdeepfm_ref.py), out-of-range ids, and the ModelManager choice layer='xDeepFM'."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import xdeepfm_ref as XR

pytestmark = pytest.mark.gpu

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def make_inputs(B, F, E, cin, seed):
    r = np.random.default_rng(seed)
    x0 = r.uniform(-1, 1, size=(B, F, E)).astype(np.float32)
    hs = [F] + list(cin)
    Ws = []
    for k in range(len(cin)):
        lim = np.sqrt(6.0 / (F * hs[k] + hs[k + 1]))
        Ws.append(r.uniform(-lim, lim, size=(1, F * hs[k], hs[k + 1])).astype(np.float32))
    g = r.uniform(-1, 1, size=(B, sum(cin))).astype(np.float32)
    return x0, Ws, g


def ref_cin(x0, Ws, g, chunk=256):
    """fp64 einsum('bme,bne,mnh->bhe') reading of CINLayer and its autograd, in chunks of examples."""
    B, F, E = x0.shape
    states, cin, dx0 = [], [], []
    dW = [np.zeros(w.shape, np.float64) for w in Ws]
    for s in range(0, B, chunk):
        x = torch.from_numpy(x0[s:s + chunk]).double().requires_grad_()
        ws = [torch.from_numpy(w).double().requires_grad_() for w in Ws]
        xk, outs = x, []
        for w in ws:
            xk = torch.einsum("bme,bne,mnh->bhe", x, xk, w.reshape(F, xk.shape[1], w.shape[-1]))
            outs.append(xk)
        st = torch.cat(outs, dim=1)
        c = st.sum(-1)
        c.backward(torch.from_numpy(g[s:s + chunk]).double())
        states.append(st.detach().numpy())
        cin.append(c.detach().numpy())
        dx0.append(x.grad.numpy())
        for k, w in enumerate(ws):
            dW[k] += w.grad.numpy()
    return np.concatenate(cin), np.concatenate(states), np.concatenate(dx0), dW


def run_gpu(x0, Ws, g):
    from explicit_tf2_recommendation_amd import ops
    xd = torch.from_numpy(x0).cuda()
    wd = [torch.from_numpy(w).cuda() for w in Ws]
    cin, states = ops.cin_fwd(xd, wd)
    dx0, dW = ops.cin_bwd(xd, states, torch.from_numpy(g).cuda(), wd)
    torch.cuda.synchronize()
    return cin.cpu().numpy(), states.cpu().numpy(), dx0.cpu().numpy(), [d.cpu().numpy() for d in dW]


def check_against_ref(B, F, E, cin_size, seed, tol_out=1e-5, tol_grad=3e-5):
    x0, Ws, g = make_inputs(B, F, E, cin_size, seed)
    got = run_gpu(x0, Ws, g)
    want = ref_cin(x0, Ws, g)
    off = 0
    for h in cin_size:                                          # every layer against its own scale
        assert rel(got[0][:, off:off + h], want[0][:, off:off + h]) <= tol_out, ("cin_part", off)
        assert rel(got[1][:, off:off + h], want[1][:, off:off + h]) <= tol_out, ("states", off)
        off += h
    assert rel(got[2], want[2]) <= tol_grad, "dx0"
    for k in range(len(cin_size)):
        assert rel(got[3][k], want[3][k]) <= tol_grad, ("dW", k)


@pytest.mark.parametrize("F", [10, 26])
def test_cin_kernels_match_fp64_at_the_reference_default_and_x26(F):
    """F = 10 (the reference's default input set) and F = 26 (config X26), E = 16, cin_size [16,32,64], B = 8192."""
    check_against_ref(8192, F, 16, [16, 32, 64], seed=F)


EDGES = [
    (1, 1, 1, [1]),
    (33, 3, 5, [7, 13]),
    (33, 26, 32, [16, 32, 64]),
    (1, 64, 64, [256]),
    (33, 64, 16, [7, 13]),
    (33, 3, 64, [256]),
    (8191, 10, 16, [16, 32, 64]),
    (8191, 3, 5, [4, 4, 4, 4, 4, 4, 4, 4]),
    (33, 26, 1, [13, 7, 5, 3, 2, 9, 11, 16]),
    (8191, 1, 32, [7, 13]),
    (33, 5, 64, [33, 17]),
]


@pytest.mark.parametrize("B,F,E,cin_size", EDGES)
def test_cin_kernels_edge_shapes(B, F, E, cin_size):
    check_against_ref(B, F, E, cin_size, seed=B + F + E)


def test_cin_gradients_are_bit_identical_run_to_run():
    x0, Ws, g = make_inputs(4099, 26, 16, [16, 32, 64], seed=3)
    a, b = run_gpu(x0, Ws, g), run_gpu(x0, Ws, g)
    assert np.array_equal(a[2], b[2])
    for k in range(3):
        assert np.array_equal(a[3][k], b[3][k])
    assert np.array_equal(a[0], b[0])


def test_cin_graph_replay_equals_eager():
    """Forward and backward launches captured in one hipGraph and replayed: bit-identical to the eager launches."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    x0, Ws, g = make_inputs(2049, 10, 16, [16, 32, 64], seed=4)
    xd = torch.from_numpy(x0).cuda()
    wd = [torch.from_numpy(w).cuda() for w in Ws]
    gd = torch.from_numpy(g).cuda()

    def step():
        cin, states = ops.cin_fwd(xd, wd)
        dx0, dW = ops.cin_bwd(xd, states, gd, wd)
        return [cin, states, dx0] + dW

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


def _layer_and_ref(V=1000, E=16, B=512, seed=7):
    from explicit_tf2_recommendation_amd import layers, data
    layers.set_init_seed(seed)
    lay = layers.XDeepFMRankingLayer(categorical_features=CAT, continuous_features=CONT, feature_dims=V,
                                     embedding_dims=E, cin_size=[16, 32, 64]).cuda()
    with torch.no_grad():                                   # embeddings of order one: every part of the output matters
        lay.embedding_layer.embeddings.uniform_(-1, 1)
        lay.w.embeddings.uniform_(-1, 1)
    batch = data.SyntheticGenerator(CAT, V, continuous=CONT, seed=seed).batch(B)
    return lay, batch


def test_layer_parity_with_the_torch_cpu_restatement():
    from explicit_tf2_recommendation_amd import data
    lay, batch = _layer_and_ref()
    out = lay(data.to_device(batch))["output"]
    r = np.random.default_rng(0)
    gout = r.uniform(-1, 1, size=tuple(out.shape)).astype(np.float32)
    out.backward(torch.from_numpy(gout).cuda())

    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in lay.named_parameters()}
    p = {"w": sd["w.embeddings"], "embed": sd["embedding_layer.embeddings"],
         "dense_k": [sd["dense_layer.hidden_layer.%d.kernel" % i] for i in range(2)],
         "dense_b": [sd["dense_layer.hidden_layer.%d.bias" % i] for i in range(2)],
         "cin_W": [sd["cin_layer.w%d" % k] for k in range(3)],
         "out_k": sd["output_layer.kernel"], "out_b": sd["output_layer.bias"]}
    X = torch.from_numpy(np.stack([np.asarray(batch[n]).reshape(-1) for n in CAT], axis=1)).long()
    Xc = torch.from_numpy(np.stack([np.asarray(batch[n]).reshape(-1) for n in CONT], axis=1)).double()
    want = XR.xdeepfm_forward(p, X, Xc)
    want.backward(torch.from_numpy(gout).double())
    assert rel(out.detach().cpu().numpy(), want.detach().numpy()) <= 1e-5
    for name, q in lay.named_parameters():
        got = q.grad
        got = (got.to_dense() if got.is_sparse else got).cpu().numpy()
        assert rel(got, sd[name].grad.numpy()) <= 3e-5, name


def test_out_of_range_ids_raise():
    from explicit_tf2_recommendation_amd import data
    lay, batch = _layer_and_ref(V=100, B=64)
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
                        layer="xDeepFM", model_params={"cin_size": [16, 32, 64]}, continuous_features=CONT,
                        engine=engine)


def test_model_manager_builds_xdeepfm_and_graphs_it_like_eager():
    from explicit_tf2_recommendation_amd import data, layers
    a, b = _manager("eager"), _manager("auto")
    assert isinstance(a.layer, layers.XDeepFMRankingLayer) and a.layer.cin_layer.cin_size == [16, 32, 64]
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
