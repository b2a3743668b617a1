"""GPU tests of the fused AFM kernels (csrc/afm.hip): against the fp64 reading (tests/afm_ref.py) at the AF and AF26
shapes and over an edge sweep, F = 2 exactness, run-to-run determinism, the saved-rows backward equal to the
gather-again one, graph replay, out-of-range ids, layer parity against the torch-CPU transcription, and the
ModelManager choice layer='AFM'.

Tolerance (per tensor, max |got - want| / max |want| against fp64): 4 x the error of the reference-order transcription
evaluated in fp32 on the CPU on the same inputs (the factor covers another summation order over the pairs and over the
batch), at least 1e-5 on outputs and 3e-5 on gradients; dbh, whose true value is 0, is held to the same rule absolutely.
ReLU has a kink: an example with an attention pre-activation within rounding of 0 may take the other branch in fp32,
which moves that example's rows of ``vals`` by O(1).  The per-row comparison of ``vals`` / the table gradient leaves
out the examples whose fp64 min |pre| is below 1e-6; every case asserts that they are at most 0.5 % of its examples.
Everything else is compared in full.  Values are drawn on the scale that reasoning was made for (tables N(0, 0.5^2),
Wa glorot-scaled normal, ba N(0, 0.1^2), hv N(0, 4^2)): see afm_ref.make_params.

Measured on the MI355X (this file's own printout; kernel error / bound):
AF    (B 16384, F 10, E 16, A 3), 0.043 % left out: o 2.8e-7/1e-5, dWa 3.4e-7/3.9e-5, dba 1.2e-6/6.2e-5,
      dhv 4.7e-7/4.7e-5, dbh 3.4e-6/9.8e-5 (absolute), vals 7.6e-7/3e-5
AF26  (B 8192, F 26, E 16, A 3), 0.122 % left out: o 4.7e-7/1e-5, dWa 3.4e-7/1.2e-4, dba 1.1e-6/3e-5,
      dhv 9.7e-7/1.2e-4, dbh 3.1e-6/3.3e-5 (absolute), vals 6.6e-7/3e-5"""
import numpy as np
import pytest
import torch

from tests import afm_ref as AR

pytestmark = pytest.mark.gpu

CAT = ["uid", "iid", "utag1", "utag2", "utag3", "utag4", "itag1", "itag2", "itag3", "itag4"]
GNAMES = ["dWa", "dba", "dhv", "dbh"]
PRE_EPS, MAX_LEFT_OUT = 1e-6, 0.005
# On the scale above about 1.2e-6 of the pre-activations lie within PRE_EPS of 0 (0.12 % of the examples at AF26, which
# has P A = 975 of them per example), so an example with more than ~4000 of them is left out with a probability above
# the cap, and in a case of 17 examples a single one breaks it.  Cases with P A above 2000 (F = 64, or A = 16 at
# F = 27) therefore shift ba by +-1, three standard deviations of p Wa: the masks still differ from unit to unit, but
# the kink is approached ~100 x less often.  The cap itself is asserted for every case.
KINK_FREE_ABOVE = 2000


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(1e-30, np.abs(b).max())


def make_inputs(B, F, E, A, V, seed, X=None):
    r = np.random.default_rng(seed)
    table = AR.make_table(V, E, seed + 100)
    Wa, ba, hv, bh = AR.make_params(E, A, seed + 200)
    if F * (F - 1) // 2 * A > KINK_FREE_ABOVE:
        ba = ba + np.where(np.arange(A) % 2 == 0, 1.0, -1.0).astype(np.float32)
    if X is None:
        X = r.integers(0, V, (B, F))
    do = np.asarray(r.uniform(-1, 1, (B, E)), np.float32)
    return table, np.ascontiguousarray(X, dtype=np.int64), Wa, ba, hv, bh, do


def run_gpu(args, save_rows=False):
    from explicit_tf2_recommendation_amd import ops
    table, X, Wa, ba, hv, bh, do = [torch.from_numpy(a).cuda() for a in args]
    flag = ops.new_flag(table.device)
    o, stats, rows = ops.emb_afm_fwd(table, X, Wa, ba, hv, bh, flag, want_rows=save_rows)
    vals, dWa, dba, dhv, dbh = ops.emb_afm_bwd(table, X, Wa, ba, hv, bh, o, stats, do, rows)
    torch.cuda.synchronize()
    assert int(flag.item()) == 0
    if save_rows:
        assert torch.equal(rows, table[X])
    return [t.cpu().numpy() for t in (o, vals, dWa, dba, dhv, dbh, stats)]


def check(B, F, E, A, V, seed, X=None, want_spread=False, attn_grads_are_zero=False):
    """``attn_grads_are_zero``: every pair of an example is the same vector, so ds == 0 and dWa, dba, dhv are 0 like dbh:
    they are then compared absolutely, as dbh is."""
    args = make_inputs(B, F, E, A, V, seed, X)
    table, X, Wa, ba, hv, bh, do = args
    rows = table[X]
    ref = AR.afm_numpy(rows, Wa, ba, hv, bh, do)
    o32, g32 = AR.afm_torch_grads(rows, Wa, ba, hv, bh, do, torch.float32)
    keep = ref["pre_min"] >= PRE_EPS
    left_out = 1.0 - keep.mean()
    got = run_gpu(args)
    o, vals = got[0], got[1].reshape(B, F, E)
    report = [("o", rel(o, ref["o"]), max(1e-5, 4 * rel(o32, ref["o"])))]
    for k, name in enumerate(GNAMES[:3]):
        want, w32 = ref[name], g32[1 + k].reshape(ref[name].shape)
        if attn_grads_are_zero:
            assert np.abs(want).max() < 1e-12
            report.append((name + "(abs)", np.abs(got[2 + k].reshape(want.shape) - want).max(),
                           max(3e-5, 4 * np.abs(w32 - want).max())))
        else:
            report.append((name, rel(got[2 + k].reshape(want.shape), want), max(3e-5, 4 * rel(w32, want))))
    report.append(("dbh(abs)", abs(float(got[5].reshape(-1)[0]) - float(ref["dbh"][0])),
                   max(3e-5, 4 * abs(float(g32[4].reshape(-1)[0]) - float(ref["dbh"][0])))))
    if keep.any():
        report.append(("vals", rel(vals[keep], ref["drows"][keep]), max(3e-5, 4 * rel(g32[0][keep], ref["drows"][keep]))))
    print("B=%d F=%d E=%d A=%d V=%d left out %.3f%%: %s" % (B, F, E, A, V, 100 * left_out, " ".join(
        "%s %.2e/%.2e" % r for r in report)))
    assert left_out <= MAX_LEFT_OUT, left_out
    for name, err, bound in report:
        assert err <= bound, (name, err, bound)
    if want_spread:                                     # the softmax is exercised: max / min weight of an example > 10
        assert np.median(ref["a"].max(axis=1) / ref["a"].min(axis=1)) > 10
    saved = run_gpu(args, save_rows=True)               # the backward from the saved rows: the same bits
    for a, b in zip(got, saved):
        assert np.array_equal(a, b)
    return got, ref, args


@pytest.mark.parametrize("cfg", ["AF", "AF26"])
def test_kernels_match_fp64(cfg):
    """AF: 10 fields, B = 16384; AF26: 26 fields, B = 8192; E = 16, A = 3.  V = 20000: ids repeat across the batch."""
    B, F = (16384, 10) if cfg == "AF" else (8192, 26)
    check(B, F, 16, 3, 20000, seed=F, want_spread=True)


EDGES = [   # B, F, E, A
    (1, 2, 1, 1), (2, 3, 3, 3), (17, 27, 16, 16), (1000, 27, 3, 1), (8191, 3, 16, 3), (17, 64, 64, 16), (2, 64, 16, 1),
    (1000, 2, 64, 3), (8191, 2, 1, 16), (17, 3, 64, 1), (1, 27, 64, 3), (1000, 64, 1, 3), (2, 27, 12, 5), (17, 12, 40, 8),
]


@pytest.mark.parametrize("B,F,E,A", EDGES)
def test_kernels_edge_shapes(B, F, E, A):
    check(B, F, E, A, 5000, seed=B + F + E + A)


def test_repeated_ids_inside_an_example_and_across_the_batch():
    check(1000, 10, 16, 3, 7, seed=5)                  # 7 rows for 10 fields: every example repeats an id


def test_all_ids_equal():
    got, ref, _ = check(17, 10, 16, 3, 50, seed=6, X=np.full((17, 10), 3), attn_grads_are_zero=True)
    np.testing.assert_allclose(ref["a"], np.full_like(ref["a"], 1.0 / 45), rtol=1e-12)   # identical pairs: uniform


def test_two_fields_are_exact():
    """F = 2: P = 1, a == 1, so o = e_0 * e_1 exactly and dWa = dba = dhv = dbh = 0 exactly."""
    got, ref, args = check(1000, 2, 16, 3, 5000, seed=8)
    table, X = args[0], args[1]
    assert np.array_equal(got[0], table[X[:, 0]] * table[X[:, 1]])
    for k in range(2, 6):
        assert np.array_equal(got[k], np.zeros_like(got[k])), GNAMES[k - 2]
    vals = got[1].reshape(1000, 2, 16)
    assert np.array_equal(vals[:, 0], args[6] * table[X[:, 1]]) and np.array_equal(vals[:, 1], args[6] * table[X[:, 0]])


def test_gradients_are_bit_identical_run_to_run():
    args = make_inputs(4099, 26, 16, 3, 3000, seed=3)
    a, b = run_gpu(args), run_gpu(args)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_graph_replay_equals_eager():
    """Forward and backward launches captured in one hipGraph and replayed: bit-identical to the eager launches."""
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    table, X, Wa, ba, hv, bh, do = [torch.from_numpy(a).cuda() for a in make_inputs(2049, 10, 16, 3, 3000, 4)]

    def step():
        o, stats, _ = ops.emb_afm_fwd(table, X, Wa, ba, hv, bh)
        return [o, stats, *ops.emb_afm_bwd(table, X, Wa, ba, hv, bh, o, stats, do)]

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
    table, X, Wa, ba, hv, bh, do = [torch.from_numpy(a) for a in make_inputs(8, 4, 8, 3, 50, 1)]
    with pytest.raises(RuntimeError):
        ops.emb_afm_fwd(table, X.cuda(), Wa.cuda(), ba.cuda(), hv.cuda(), bh.cuda())       # no CPU fallback
    with pytest.raises(ValueError):
        ops.emb_afm_fwd(table.cuda(), X.cuda(), Wa[:4].contiguous().cuda(), ba.cuda(), hv.cuda(), bh.cuda())
    with pytest.raises(NotImplementedError):
        ops.emb_afm_fwd(table.cuda(), X[:, :1].contiguous().cuda(), Wa.cuda(), ba.cuda(), hv.cuda(), bh.cuda())
    o, stats, _ = ops.emb_afm_fwd(table.cuda(), X[:0].contiguous().cuda(), Wa.cuda(), ba.cuda(), hv.cuda(), bh.cuda())
    assert tuple(o.shape) == (0, 8) and tuple(stats.shape) == (0, 2)


def _layer(V=1000, B=512, seed=7, F=10):
    from explicit_tf2_recommendation_amd import layers, data
    layers.set_init_seed(seed)
    lay = layers.AttentionalFactorizationMachine(categorical_features=CAT[:F], feature_dims=V).cuda()
    Wa, ba, hv, bh = AR.make_params(16, 3, seed)
    with torch.no_grad():                                # the scale of the kernel tests, not the U(-0.05, 0.05) initialiser
        lay.embedding_layer.embeddings.copy_(torch.from_numpy(AR.make_table(V, 16, seed)))
        att = lay.attention_layer
        for p, v in ((att.attention_w.kernel, Wa), (att.attention_w.bias, ba), (att.attention_h.kernel, hv),
                     (att.attention_h.bias, bh)):
            p.copy_(torch.from_numpy(v))
    return lay, data.SyntheticGenerator(CAT[:F], V, seed=seed).batch(B)


def test_layer_parity_with_the_torch_cpu_restatement():
    from explicit_tf2_recommendation_amd import data
    lay, batch = _layer()
    out = lay(data.to_device(batch))["output"]
    assert tuple(out.shape) == (512, 1)
    gout = np.random.default_rng(0).uniform(-1, 1, size=tuple(out.shape)).astype(np.float32)
    out.backward(torch.from_numpy(gout).cuda())
    X = torch.from_numpy(np.stack([np.asarray(batch[n]).reshape(-1) for n in CAT], axis=1)).long()

    def restate(dtype):
        sd = {k: v.detach().cpu().to(dtype).requires_grad_() for k, v in lay.named_parameters()}
        p = {"embed": sd["embedding_layer.embeddings"], "Wa": sd["attention_layer.attention_w.kernel"],
             "ba": sd["attention_layer.attention_w.bias"], "hv": sd["attention_layer.attention_h.kernel"],
             "bh": sd["attention_layer.attention_h.bias"], "out_k": sd["output_layer.kernel_0"],
             "out_b": sd["output_layer.bias_0"]}
        want = AR.afm_layer_torch(p, X)
        (torch.from_numpy(gout).to(dtype) * want).sum().backward()
        return want.detach().numpy(), {k: v.grad.numpy() for k, v in sd.items()}

    w64, g64 = restate(torch.float64)
    w32, g32 = restate(torch.float32)
    sd = {k: v.detach().cpu().numpy() for k, v in lay.named_parameters()}
    pre_min = AR.afm_numpy(sd["embedding_layer.embeddings"][X.numpy()], sd["attention_layer.attention_w.kernel"],
                           sd["attention_layer.attention_w.bias"], sd["attention_layer.attention_h.kernel"],
                           sd["attention_layer.attention_h.bias"])["pre_min"]
    near = pre_min < PRE_EPS
    assert near.mean() <= MAX_LEFT_OUT
    assert rel(out.detach().cpu().numpy(), w64) <= max(1e-5, 4 * rel(w32, w64))
    touched = np.setdiff1d(np.unique(X.numpy()), np.unique(X.numpy()[near]))    # rows no left-out example touched
    for name, q in lay.named_parameters():
        got = q.grad
        got = (got.to_dense() if got.is_sparse else got).cpu().numpy()
        want, want32 = g64[name], g32[name]
        if name == "embedding_layer.embeddings":
            got, want, want32 = got[touched], want[touched], want32[touched]
            bound = max(3e-5, 4 * rel(want32, want))
            err = rel(got, want)
        elif name == "attention_layer.attention_h.bias":          # true value 0: absolute
            bound = max(3e-5, 4 * np.abs(want32 - want).max())
            err = np.abs(got - want).max()
        else:
            bound = max(3e-5, 4 * rel(want32, want))
            err = rel(got, want)
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


def test_continuous_features_are_not_accepted():
    from explicit_tf2_recommendation_amd import layers
    with pytest.raises(TypeError):
        layers.AttentionalFactorizationMachine(categorical_features=CAT, continuous_features=["x"], feature_dims=10)


def _manager(engine, V=5000, B=512, lr=0.01):
    from explicit_tf2_recommendation_amd import data
    from explicit_tf2_recommendation_amd.model_manager import ModelManager
    return ModelManager(feature_names=CAT, data_info=data.data_info(V, len(CAT)), embedding_dims=16, lr=lr, batch=B,
                        layer="AFM", model_params={"attn_size": 4}, engine=engine)


def test_model_manager_builds_afm_and_graphs_it_like_eager():
    from explicit_tf2_recommendation_amd import data, layers
    a, b = _manager("eager"), _manager("auto")
    assert isinstance(a.layer, layers.AttentionalFactorizationMachine)
    assert tuple(a.layer.attention_layer.attention_w.kernel.shape) == (16, 4)
    b.model.load_state_dict(a.model.state_dict())
    gen = data.SyntheticGenerator(CAT, 5000, dist="zipf", seed=9)
    for _ in range(3):
        batch = gen.batch(512)
        la, lb = a.train_loop(dict(batch)), b.train_loop(dict(batch))
        assert la.item() == lb.item()
    assert b._eng[0] == "graphed"
    for (k, p), (_, q) in zip(a.model.named_parameters(), b.model.named_parameters()):
        assert torch.equal(p, q), k


def test_model_manager_trains_an_epoch_graphed_like_eager_and_lowers_the_loss():
    """One epoch (train_step over a list of batches) gives the same loss graphed and eager; repeating the epoch lowers
    the loss (the label is a function of uid, which the embedding rows can learn)."""
    import random
    from explicit_tf2_recommendation_amd import data
    a, b = _manager("eager", B=1024, lr=0.02), _manager("auto", B=1024, lr=0.02)
    b.model.load_state_dict(a.model.state_dict())
    gen = data.SyntheticGenerator(CAT, 5000, seed=11)
    batches = []
    for i in range(4):
        bt = gen.batch(1024)
        bt["label"] = (np.asarray(bt["uid"]).reshape(-1, 1) % 2 == 0).astype(np.float32).reshape(
            np.asarray(bt["label"]).shape)
        batches.append(bt)
    random.seed(5)
    ra = a.train_step(batches)
    random.seed(5)
    rb = b.train_step(batches)
    assert ra["loss"] == pytest.approx(rb["loss"], rel=1e-6), (ra, rb)
    first = rb["loss"]
    for _ in range(25):
        last = b.train_step(batches)["loss"]
    assert last < first - 0.02, (first, last)
