"""GPU tests of the fused FGCNN kernels (csrc/fgcnn.hip): against the fp64 reading (tests/fgcnn_ref.py) at the default
filters and over an edge sweep, the tie rule on identical rows, run-to-run determinism, graph replay, the optional direct
gradient, error paths, layer parity against the torch-CPU transcription, and the ModelManager choice layer='FGCNN'.

Tolerance (per tensor, max |got - want| / max |want| against fp64): 4 x the error of the reference-order transcription
evaluated in fp32 on the CPU on the same inputs, at least 1e-5 on forward tensors and 3e-5 on gradients.
The forward is continuous in its inputs, the routing of the gradient through a pooling is not: an example in which the
two largest values of a pooling window are closer than GAP_EPS = 1e-6 in fp64 (about 5 x the fp32 forward error of 2e-7)
may route differently in fp32.  The rows of every ``dp_j`` and of ``drows_direct`` of those examples are set to zero
BEFORE either side runs; every gradient is then compared in full.  Every case asserts that they are at most 10 % of its
examples; cases under 100 examples use a seed without any and assert that.  Values are drawn on the scale that reasoning
was made for (tables N(0, 0.5^2), glorot-uniform kernels, biases N(0, 0.1^2)): see ccpm_ref.make_params.
The seeds of the cases under 100 examples were chosen on the fp64 reading alone (its gap), before the kernels ran: the
first of 1, 2, 3, ... without a near tie.

Measured on the MI355X: not yet.  Every check prints ``error/bound`` per tensor (run with -s); the printout of the first
MI355X run belongs here.  Near-tie shares, counted on the fp64 reading alone: 0.66 % at (4099, 10), 1.42 % at (2049, 26),
0.84 % at (8191, 10), 2.0 % at (1000, 27, 16, [16,16], [8,3], [2,3]), 0.7 % with V = 7, none in the cases under 100
examples at the seeds below."""
import numpy as np
import pytest
import torch

from tests import ccpm_ref as CR
from tests import fgcnn_ref as FR

pytestmark = pytest.mark.gpu

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
CONT = ["itag4_origin", "itag4_square", "itag4_cube"]
GAP_EPS, MAX_NEAR, SMALL = 1e-6, 0.10, 100
DEF = ([14, 16], [7, 7], [2, 2])


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def make_inputs(B, F, E, filters, kw, pws, V, seed, X=None):
    r = np.random.default_rng(seed)
    table = CR.make_table(V, E, seed + 100)
    params = CR.make_params(filters, kw, seed + 200)
    if X is None:
        X = r.integers(0, V, (B, F))
    dps = [np.asarray(r.uniform(-1, 1, (B, h * E * c)), np.float32) for h, c in zip(FR.heights(F, pws), filters)]
    dd = np.asarray(r.uniform(-1, 1, (B, F, E)), np.float32)
    return table, np.ascontiguousarray(X, dtype=np.int64), params, list(filters), list(kw), list(pws), dps, dd


def run_gpu(args, direct=True):
    """-> [rows, p_1 .. p_L, vals, dparams] as numpy"""
    from explicit_tf2_recommendation_amd import ops
    table, X, params, filters, kw, pws, dps, dd = args
    table, X, flat, dd = [torch.from_numpy(a).cuda() for a in (table, X, CR.flat_params(params), dd)]
    dps = [torch.from_numpy(d).cuda() for d in dps]
    flag = ops.new_flag(table.device)
    rows, pooled = ops.emb_fgcnn_fwd(table, X, flat, filters, kw, pws, flag)
    vals, dflat = ops.emb_fgcnn_bwd(rows, flat, filters, kw, pws, dps, dd if direct else None)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    assert torch.equal(rows, table[X])
    return [t.cpu().numpy() for t in (rows, *pooled, vals, dflat)]


def check(B, F, E, filters, kw, pws, V, seed, X=None, exact_ties=False):
    """``exact_ties``: rows repeat inside an example, so that positions tie exactly; the gap is then taken over distinct
    values only and no example is zeroed out."""
    args = make_inputs(B, F, E, filters, kw, pws, V, seed, X)
    table, X, params, _, _, _, dps, dd = args
    L = len(filters)
    rows = table[X]
    near = FR.fgcnn_numpy(rows, params, pws, distinct_gap=exact_ties)["gap"] < GAP_EPS
    if exact_ties:
        assert not near.any()
    for d in dps + [dd]:
        d[near] = 0.0                                    # before either side runs
    ref = FR.fgcnn_numpy(rows, params, pws, dps, dd)
    p32, dr32, dp32 = FR.fgcnn_torch_grads(rows, params, pws, dps, dd, torch.float32)
    got = run_gpu(args)
    pooled, vals, dflat = got[1:1 + L], got[1 + L].reshape(B, F, E), got[2 + L]
    report = [("p%d" % (j + 1), rel(pooled[j], ref["pooled"][j]), max(1e-5, 4 * rel(p32[j], ref["pooled"][j])))
              for j in range(L)]
    report.append(("vals", rel(vals, ref["drows"]), max(3e-5, 4 * rel(dr32, ref["drows"]))))
    at = 0
    for j, kb in enumerate(ref["dparams"]):
        for name, want, w32 in zip(("dK", "db"), kb, dp32[2 * j:2 * j + 2]):
            g = dflat[at:at + want.size].reshape(want.shape)
            at += want.size
            report.append(("%s%d" % (name, j + 1), rel(g, want), max(3e-5, 4 * rel(w32, want))))
    assert at == dflat.size
    print("B=%d F=%d E=%d filters=%s kw=%s pw=%s V=%d near ties %.2f%%: %s" % (
        B, F, E, filters, kw, pws, V, 100 * near.mean(), " ".join("%s %.2e/%.2e" % r for r in report)))
    if B < SMALL:
        assert not near.any(), near.sum()
    else:
        assert near.mean() <= MAX_NEAR, near.mean()
    for name, err, bound in report:
        assert err <= bound, (name, err, bound)
    return got, ref, args


@pytest.mark.parametrize("B,F", [(4099, 10), (2049, 26), (8191, 10)])
def test_kernels_match_fp64_at_the_default_filters(B, F):
    """E = 16, filters [14,16], kernel_width [7,7], pooling_width [2,2]; V = 20000: ids repeat.  A workgroup of the
    backward holds at most 16 columns, so B = 4099 and 8191 give it more tiles than workgroups: the persistent loop
    takes a second round."""
    from explicit_tf2_recommendation_amd import ops
    if F == 10:
        assert -(-B * 16 // 16) > ops.FGCNN_BWD_GRID      # tiles = ceil(B E / 16 columns per workgroup)
    check(B, F, 16, *DEF, 20000, seed=F + B)


EDGES = [   # B, F, E, filters, kernel_width, pooling_width, seed
    (1, 3, 1, [1], [1], [3], 1), (2, 3, 6, [4, 6], [4, 2], [1, 3], 1), (17, 10, 16, *DEF, 2),
    (1000, 27, 16, [16, 16], [8, 3], [2, 3], 10), (17, 64, 64, [2, 3], [4, 2], [2, 2], 2),
    (2, 16, 16, [4, 6, 5], [4, 3, 2], [2, 2, 2], 1), (17, 20, 40, [3, 2], [5, 6], [3, 2], 1), (1, 12, 12, [4], [7], [5], 1),
]


@pytest.mark.parametrize("B,F,E,filters,kw,pws,seed", EDGES)
def test_kernels_edge_shapes(B, F, E, filters, kw, pws, seed):
    check(B, F, E, filters, kw, pws, 5000, seed=seed)


def test_repeated_ids_inside_an_example_and_across_the_batch():
    check(1000, 10, 16, *DEF, 7, seed=5)                 # 7 rows for 10 fields: every example repeats an id


def test_all_ids_equal_route_to_the_lower_field():
    """Identical rows: the interior pre-activations of layer 1 are bit-equal, so the tie rule decides where the gradient
    goes; vals must match the fp64 reading, which breaks ties to the lower field."""
    got, ref, args = check(17, 10, 16, *DEF, 50, seed=1, X=np.full((17, 10), 3), exact_ties=True)
    assert np.abs(ref["drows"] - args[7]).max() > 0      # something beyond the direct gradient arrives


def test_gradients_are_bit_identical_run_to_run():
    args = make_inputs(4099, 26, 16, *DEF, 3000, 3)
    a, b = run_gpu(args), run_gpu(args)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_no_direct_gradient_equals_zeros():
    table, X, params, filters, kw, pws, dps, dd = make_inputs(1031, 10, 16, *DEF, 3000, 4)
    a = run_gpu((table, X, params, filters, kw, pws, dps, dd), direct=False)
    b = run_gpu((table, X, params, filters, kw, pws, dps, np.zeros_like(dd)))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    c = run_gpu((table, X, params, filters, kw, pws, dps, dd))
    np.testing.assert_allclose(c[-2] - a[-2], dd.reshape(-1, 16), rtol=0, atol=1e-6)


def test_graph_replay_equals_eager():
    """Forward and backward launches captured in one hipGraph and replayed: bit-identical to the eager launches."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    table, X, params, filters, kw, pws, dps, dd = make_inputs(2049, 10, 16, *DEF, 3000, 4)
    table, X, flat, dd = [torch.from_numpy(a).cuda() for a in (table, X, CR.flat_params(params), dd)]
    dps = [torch.from_numpy(d).cuda() for d in dps]

    def step():
        rows, pooled = ops.emb_fgcnn_fwd(table, X, flat, filters, kw, pws)
        return [rows, *pooled, *ops.emb_fgcnn_bwd(rows, flat, filters, kw, pws, dps, dd)]

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


def test_cpu_tensors_and_bad_shapes_are_errors():
    from explicit_tf2_recommendation_amd import ops
    table, X, params, filters, kw, pws, dps, dd = make_inputs(8, 10, 8, *DEF, 50, 1)
    table, X, flat = torch.from_numpy(table), torch.from_numpy(X), torch.from_numpy(CR.flat_params(params))
    with pytest.raises(RuntimeError):
        ops.emb_fgcnn_fwd(table, X.cuda(), flat.cuda(), filters, kw, pws)                       # no CPU fallback
    with pytest.raises(RuntimeError):
        ops.emb_fgcnn_bwd(torch.zeros(8, 10, 8), flat.cuda(), filters, kw, pws, [torch.from_numpy(d).cuda() for d in dps])
    with pytest.raises(ValueError):
        ops.emb_fgcnn_fwd(table.cuda(), X.cuda(), flat[:-1].contiguous().cuda(), filters, kw, pws)
    with pytest.raises(ValueError):
        ops.emb_fgcnn_fwd(table.cuda(), X[:, :3].contiguous().cuda(), flat.cuda(), filters, kw, pws)   # H = 3 -> 1 -> 0
    with pytest.raises(NotImplementedError):
        ops.emb_fgcnn_fwd(table.cuda(), X.cuda(), flat.cuda(), filters, kw, [9, 1])
    rows, pooled = ops.emb_fgcnn_fwd(table.cuda(), X.cuda(), flat.cuda(), filters, kw, pws)
    with pytest.raises(ValueError):
        ops.emb_fgcnn_bwd(rows, flat.cuda(), filters, kw, pws, [torch.from_numpy(dps[0]).cuda()])
    with pytest.raises(ValueError):
        ops.emb_fgcnn_bwd(rows, flat.cuda(), filters, kw, pws, [torch.from_numpy(d).cuda() for d in dps[::-1]])
    rows, pooled = ops.emb_fgcnn_fwd(table.cuda(), X[:0].contiguous().cuda(), flat.cuda(), filters, kw, pws)
    assert tuple(rows.shape) == (0, 10, 8) and [tuple(p.shape) for p in pooled] == [(0, 5 * 8 * 14), (0, 2 * 8 * 16)]
    vals, dflat = ops.emb_fgcnn_bwd(rows, flat.cuda(), filters, kw, pws, pooled)
    assert tuple(vals.shape) == (0, 8) and tuple(dflat.shape) == tuple(flat.shape) and float(dflat.abs().max()) == 0


LAYER_B, LAYER_SEED = 64, 2


def _layer(V=1000, B=LAYER_B, seed=LAYER_SEED):
    from explicit_tf2_recommendation_amd import layers, data
    layers.set_init_seed(seed)
    lay = layers.FGCNNLayer(feature_dims=V).cuda()
    params = CR.make_params(DEF[0], DEF[1], seed)
    with torch.no_grad():                                # the scale of the kernel tests, not the U(-0.05, 0.05) initialiser
        lay.embedding_layer.embeddings.copy_(torch.from_numpy(CR.make_table(V, 16, seed)))
        for conv, (K, b) in zip(lay.fgcnn_layer.conv_layers, params):
            conv.kernel.copy_(torch.from_numpy(K))
            conv.bias.copy_(torch.from_numpy(b))
    return lay, data.SyntheticGenerator(CAT, V, continuous=CONT, seed=seed).batch(B)


def _layer_gap(lay, batch):
    X = np.stack([np.asarray(batch[n]).reshape(-1) for n in CAT], axis=1)
    sd = {k: v.detach().cpu().numpy() for k, v in lay.named_parameters()}
    params = [(sd["fgcnn_layer.conv_layers.%d.kernel" % i], sd["fgcnn_layer.conv_layers.%d.bias" % i]) for i in range(2)]
    return FR.fgcnn_numpy(sd["embedding_layer.embeddings"][X], params, DEF[2])["gap"]


def test_layer_parity_with_the_torch_cpu_restatement():
    """The whole layer in training mode: lookup, conv / pooling stack, recombinations, embeddings first and continuous
    columns last, MLP with batch-norm on batch statistics, sigmoid head; the output and every parameter gradient."""
    from explicit_tf2_recommendation_amd import data
    lay, batch = _layer()
    lay.train()
    out = lay(data.to_device(batch))["output"]
    assert tuple(out.shape) == (LAYER_B, 1)
    gout = np.random.default_rng(0).uniform(-1, 1, size=tuple(out.shape)).astype(np.float32)
    out.backward(torch.from_numpy(gout).cuda())
    X = torch.from_numpy(np.stack([np.asarray(batch[n]).reshape(-1) for n in CAT], axis=1)).long()
    Xc = np.stack([np.asarray(batch[n], np.float32).reshape(-1) for n in CONT], axis=1)
    names = dict(lay.named_parameters())

    def restate(dtype):
        sd = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in names.items()}
        p = {"embed": sd["embedding_layer.embeddings"],
             "conv": [sd["fgcnn_layer.conv_layers.%d.%s" % (i, n)] for i in range(2) for n in ("kernel", "bias")],
             "dense": [sd["fgcnn_layer.dense_layers.%d.%s" % (i, n)] for i in range(2) for n in ("kernel", "bias")],
             "k1": [sd["MLP_layer1.kernel_%d" % i] for i in range(2)],
             "b1": [sd["MLP_layer1.bias_%d" % i] for i in range(2)],
             "gamma": [sd["MLP_layer1.bn_%d.gamma" % i] for i in range(2)],
             "beta": [sd["MLP_layer1.bn_%d.beta" % i] for i in range(2)],
             "k2": sd["MLP_layer2.kernel_0"], "b2": sd["MLP_layer2.bias_0"]}
        want = FR.fgcnn_layer_torch(p, X, torch.from_numpy(Xc).to(dtype), DEF[2])
        (torch.from_numpy(gout).to(dtype) * want).sum().backward()
        return want.detach().numpy(), {k: v.grad.numpy() for k, v in sd.items()}

    w64, g64 = restate(torch.float64)
    w32, g32 = restate(torch.float32)
    assert not (_layer_gap(lay, batch) < GAP_EPS).any()  # under 100 examples: a seed without a near tie
    err, bound = rel(out.detach().cpu().numpy(), w64), max(1e-5, 4 * rel(w32, w64))
    print("output", err, bound)
    assert err <= bound
    for name, q in names.items():
        got = q.grad
        got = (got.to_dense() if got.is_sparse else got).cpu().numpy()
        if name.startswith("MLP_layer1.bias_"):          # batch statistics cancel a bias: the true value is 0, absolute
            assert np.abs(g64[name]).max() < 1e-12
            err, bound = np.abs(got - g64[name]).max(), max(3e-5, 4 * np.abs(g32[name] - g64[name]).max())
        else:
            err, bound = rel(got, g64[name]), max(3e-5, 4 * rel(g32[name], g64[name]))
        print(name, err, bound)
        assert err <= bound, name


def test_out_of_range_ids_raise():
    from explicit_tf2_recommendation_amd import data
    lay, batch = _layer(V=100, B=64)
    bad = dict(batch)
    ids = np.array(bad["itag2"]).copy()
    ids.reshape(-1)[5] = 100
    bad["itag2"] = ids
    with pytest.raises(IndexError):
        lay(data.to_device(bad))


def _manager(engine, V=5000, B=512, lr=0.01):
    from explicit_tf2_recommendation_amd import data
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    return ModelManager(feature_names=CAT, continuous_features=CONT, data_info=data.data_info(V, len(CAT)),
                        embedding_dims=16, lr=lr, batch=B, layer="FGCNN", model_params={"units": [32, 8]},
                        engine=engine)


def test_model_manager_trains_fgcnn_graphed_like_eager():
    from explicit_tf2_recommendation_amd import data, layers
    a, b = _manager("eager"), _manager("auto")
    assert isinstance(a.layer, layers.FGCNNLayer) and a.layer.units == [32, 8]
    b.model.load_state_dict(a.model.state_dict())
    gen = data.SyntheticGenerator(CAT, 5000, continuous=CONT, dist="zipf", seed=9)
    for _ in range(3):
        batch = gen.batch(512)
        la, lb = a.train_loop(dict(batch)), b.train_loop(dict(batch))
        assert np.isfinite(la.item()) and np.isfinite(lb.item())
        assert la.item() == lb.item()
    assert b._eng[0] == "graphed"
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k
