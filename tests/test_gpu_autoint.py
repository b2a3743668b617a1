"""GPU tests of the AutoInt attention (csrc/autoint.hip): the kernels against fp64 at the AI and AI26 shapes for every
residual mode and with scaling, an edge sweep, B = 1 exactness, the batch-axis softmax told apart from a key-axis one,
run-to-run determinism, graph replay, layer parity against the torch-CPU AutoIntLayer (tests/autoint_ref.py),
out-of-range ids, and the ModelManager choice layer='AutoInt'.

Tolerance (per tensor, max |got - want| / max |want| against the fp64 transcription): 4 x the error of the same
transcription evaluated in fp32 on the CPU on the same inputs, at least 1e-5 on outputs and 3e-5 on gradients.  The
softmax sums over the batch, and the GPU sums in another order than torch-CPU; same-length sums in different orders err
by the same order of magnitude.  Inputs keep every ReLU pre-activation clear of 0: positive embeddings and continuous
fields, W_value columns of one sign with |w| >= 0.05 (all positive when a residual is added, so z > 0 everywhere)."""
import numpy as np
import pytest
import torch

from tests import autoint_ref as AR

pytestmark = pytest.mark.gpu

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def make_inputs(B, Fc, C, E, H, res, seed):
    r = np.random.default_rng(seed)
    f32 = lambda a: np.asarray(a, np.float32)
    x = f32(r.uniform(0.05, 1.0, (B, Fc, E)))
    xc = f32(r.uniform(0.1, 2.0, (B, C)))
    ce = f32(r.uniform(0.05, 1.0, (C, E)))
    Wq = f32(r.standard_normal((E, E)) / np.sqrt(E))
    Wk = f32(r.standard_normal((E, E)) / np.sqrt(E))
    sign = np.ones(E) if res else np.where(np.arange(E) % 2 == 0, 1.0, -1.0)
    Wv = f32(r.uniform(0.05, 0.5, (E, E)) * sign[None, :])
    Wr = f32(r.uniform(0.05, 0.5, (E, E)))
    dy = f32(r.uniform(-1, 1, (B, Fc + C, E)))
    return x, xc, ce, Wq, Wk, Wv, Wr, dy


def transcription(args, H, res, scaling, dtype):
    """The reference-order transcription on the CPU in ``dtype``: (y, o, [dx, dcemb, dWq, dWk, dWv, dWres])."""
    x, xc, ce, Wq, Wk, Wv, Wr, dy = args
    t = [torch.from_numpy(a).to(dtype).requires_grad_() for a in (x, ce, Wq, Wk, Wv, Wr)]
    X = AR.assemble_dense(t[0], t[1], torch.from_numpy(xc).to(dtype))
    y, o = AR.attention_torch(X, t[2], t[3], t[4], H, use_res=res > 0, res_learnable=res == 2, Wres=t[5],
                              scaling=scaling, return_o=True)
    grads = torch.autograd.grad(y, t, torch.from_numpy(dy).to(dtype), allow_unused=True)
    grads = [g.detach().numpy() if g is not None else None for g in grads]
    return y.detach().numpy(), o.detach().numpy(), grads


def run_gpu(args, H, res, scaling):
    from explicit_tf2_recommendation_amd import ops
    x, xc, ce, Wq, Wk, Wv, Wr, dy = [torch.from_numpy(a).cuda() for a in args]
    C = xc.shape[1]
    xc_, ce_ = (xc, ce) if C else (None, None)
    Wr_ = Wr if res == 2 else None
    y, stats, o = ops.autoint_fwd(x, Wq, Wk, Wv, Wr_, H, res, scaling, xc_, ce_, want_o=True)
    dx, dWq, dWk, dWv, dWr, dce = ops.autoint_bwd(x, Wq, Wk, Wv, Wr_, y, dy, stats, H, res, scaling, xc_, ce_)
    torch.cuda.synchronize()
    npy = lambda t: None if t is None else t.cpu().numpy()
    return npy(y), npy(o), [npy(dx), npy(dce), npy(dWq), npy(dWk), npy(dWv), npy(dWr)]


GNAMES = ["dx", "dcemb", "dWq", "dWk", "dWv", "dWres"]


def check(B, Fc, C, E, H, res, scaling, seed):
    args = make_inputs(B, Fc, C, E, H, res, seed)
    y64, o64, g64 = transcription(args, H, res, scaling, torch.float64)
    y32, o32, g32 = transcription(args, H, res, scaling, torch.float32)
    # the masks: fp64 pre-activations are far from 0 compared with the fp32 error on them
    z64 = o64 + (AR.assemble_np(args) if res == 1 else (AR.assemble_np(args) @ args[6] if res == 2 else 0.0))
    assert np.abs(z64).min() > 0, "an input with a pre-activation at 0"
    gy, go, gg = run_gpu(args, H, res, scaling)
    report = []
    for name, got, want, w32, floor in (("o", go, o64, o32, 1e-5), ("y", gy, y64, y32, 1e-5)):
        bound = max(floor, 4 * rel(w32, want))
        report.append((name, rel(got, want), bound))
    for k, name in enumerate(GNAMES):
        if g64[k] is None:
            continue
        if name == "dWres" and res != 2:
            continue
        bound = max(3e-5, 4 * rel(g32[k], g64[k]))
        report.append((name, rel(gg[k], g64[k]), bound))
    print("B=%d Fc=%d C=%d E=%d H=%d res=%d scaling=%d: %s" % (B, Fc, C, E, H, res, scaling, " ".join(
        "%s %.2e/%.2e" % r for r in report)))
    for name, err, bound in report:
        assert err <= bound, (name, err, bound)
    if B >= 2:                                         # the inputs tell the batch-axis softmax from a key-axis one
        Xd = torch.from_numpy(AR.assemble_np(args))
        key = AR.attention_keyaxis(Xd, *[torch.from_numpy(a).double() for a in args[3:6]], H, scaling).numpy()
        assert rel(key, o64) > 100 * report[0][2], rel(key, o64)
    return gy, go, gg, args


@pytest.mark.parametrize("res,scaling", [(1, False), (0, False), (2, False), (1, True), (0, True)])
@pytest.mark.parametrize("cfg", ["AI", "AI26"])
def test_kernels_match_fp64(cfg, res, scaling):
    """AI: 10 cat + 3 cont fields, E = 8, H = 2, B = 16384; AI26: 26 cat + 3 cont, E = 16, H = 2, B = 8192."""
    B, Fc, E = (16384, 10, 8) if cfg == "AI" else (8192, 26, 16)
    check(B, Fc, 3, E, 2, res, scaling, seed=Fc + 3 * res + scaling)


EDGES = [   # B, Fc, C, E, H
    (8191, 10, 3, 8, 2), (1000, 62, 2, 16, 2), (17, 60, 4, 64, 64), (2, 1, 0, 1, 1), (17, 4, 1, 3, 1),
    (1000, 7, 0, 12, 12), (2, 63, 1, 64, 1), (8191, 20, 9, 16, 16), (17, 3, 0, 64, 2), (1000, 1, 0, 64, 64),
    (2, 5, 2, 6, 2), (17, 12, 3, 40, 2),
]


@pytest.mark.parametrize("B,Fc,C,E,H", EDGES)
def test_kernels_edge_shapes(B, Fc, C, E, H):
    check(B, Fc, C, E, H, res=(B + E) % 3, scaling=bool(B % 2), seed=B + Fc + E)


@pytest.mark.parametrize("res", [0, 1, 2])
def test_batch_of_one_is_exact(res):
    """B = 1: P == 1, so O = sum_j V_j, and dWq and dWk are exactly 0."""
    gy, go, gg, args = check(1, 10, 3, 8, 2, res, False, seed=21 + res)
    X = AR.assemble_np(args)
    V = X @ args[5].astype(np.float64)
    assert rel(go[0], np.broadcast_to(V[0].sum(0), go[0].shape)) <= 1e-6
    assert np.array_equal(gg[2], np.zeros_like(gg[2])) and np.array_equal(gg[3], np.zeros_like(gg[3]))


def test_gradients_are_bit_identical_run_to_run():
    args = make_inputs(4099, 26, 3, 16, 2, 2, seed=3)
    a, b = run_gpu(args, 2, 2, True), run_gpu(args, 2, 2, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for k in range(6):
        assert np.array_equal(a[2][k], b[2][k]), GNAMES[k]


def test_graph_replay_equals_eager():
    """Forward and backward launches captured in one hipGraph and replayed: bit-identical to the eager launches."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    x, xc, ce, Wq, Wk, Wv, Wr, dy = [torch.from_numpy(a).cuda() for a in make_inputs(2049, 10, 3, 8, 2, 1, 4)]

    def step():
        y, stats, o = ops.autoint_fwd(x, Wq, Wk, Wv, None, 2, 1, False, xc, ce, want_o=True)
        return [y, stats, o, *[t for t in ops.autoint_bwd(x, Wq, Wk, Wv, None, y, dy, stats, 2, 1, False, xc, ce)
                               if t is not None]]

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


def _layer(V=1000, B=512, seed=7):
    from explicit_tf2_recommendation_amd import layers, data
    layers.set_init_seed(seed)
    lay = layers.AutoIntLayer(categorical_features=CAT, continuous_features=CONT, feature_dims=V).cuda()
    with torch.no_grad():                        # positive fields and W_value: every attention pre-activation > 0
        lay.embedding_layer.embeddings.uniform_(0.05, 1)
        lay.continuous_embedding.embeddings.uniform_(0.05, 1)
        for a in lay.attention_layers:
            a.value.abs_().add_(0.05)
    batch = data.SyntheticGenerator(CAT, V, continuous=CONT, seed=seed).batch(B)
    r = np.random.default_rng(seed)
    for n in CONT:
        batch[n] = r.uniform(0.1, 2.0, np.asarray(batch[n]).shape).astype(np.float32)
    return lay, batch


def test_layer_parity_with_the_torch_cpu_restatement():
    from explicit_tf2_recommendation_amd import data
    lay, batch = _layer()
    out = lay(data.to_device(batch))["output"]
    gout = np.random.default_rng(0).uniform(-1, 1, size=tuple(out.shape)).astype(np.float32)
    out.backward(torch.from_numpy(gout).cuda())
    X = torch.from_numpy(np.stack([np.asarray(batch[n]).reshape(-1) for n in CAT], axis=1)).long()
    Xc = np.stack([np.asarray(batch[n]).reshape(-1) for n in CONT], axis=1)

    def restate(dtype):
        sd = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in lay.named_parameters()}
        p = {"embed": sd["embedding_layer.embeddings"], "cemb": sd["continuous_embedding.embeddings"],
             "att": [tuple(sd["attention_layers.%d.%s" % (k, n)] for n in ("query", "key", "value"))
                     for k in range(2)],
             "dnn_k": [sd["dnn_layer.kernel_%d" % i] for i in range(2)],
             "dnn_b": [sd["dnn_layer.bias_%d" % i] for i in range(2)],
             "out_k": sd["output_layer.kernel"], "out_b": sd["output_layer.bias"]}
        want = AR.autoint_layer_torch(p, X, torch.from_numpy(Xc).to(dtype))
        (torch.from_numpy(gout).to(dtype) * want).sum().backward()
        return want.detach().numpy(), {k: v.grad.numpy() for k, v in sd.items()}

    w64, g64 = restate(torch.float64)
    w32, g32 = restate(torch.float32)
    assert rel(out.detach().cpu().numpy(), w64) <= max(1e-5, 4 * rel(w32, w64))
    touched = np.unique(X.numpy())
    for name, q in lay.named_parameters():
        got = q.grad
        got = (got.to_dense() if got.is_sparse else got).cpu().numpy()
        want, want32 = g64[name], g32[name]
        if name == "embedding_layer.embeddings":
            got, want, want32 = got[touched], want[touched], want32[touched]
        bound = max(3e-5, 4 * rel(want32, want))
        print(name, rel(got, want), bound)
        assert rel(got, want) <= bound, name


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
                        layer="AutoInt", model_params={"units": [64, 16]}, continuous_features=CONT, engine=engine)


def test_model_manager_builds_autoint_and_graphs_it_like_eager():
    from explicit_tf2_recommendation_amd import data, layers
    a, b = _manager("eager"), _manager("auto")
    assert isinstance(a.layer, layers.AutoIntLayer) and a.layer.embedding_dims == 8
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
