"""PEPNet on the GPU: the EPNet lookup (csrc/epnet.hip) and the stacked POSO-MLPs (csrc/poso.hip) against the fp64 numpy
reading of tests/pepnet_ref.py, the layer in both modes against the torch-CPU transcription, inference, strided inputs,
bit identity run to run, graph capture, engine.GraphedTrainStep with three labels, the allocation seam of
tests/guarded.py, and the error paths.

Tolerance, per tensor (the project's rule, as tests/test_gpu_mmoe.py restates it): max|got - want| / max|want| against
fp64 must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors)
/ 3e-5 (gradients).  An example whose smallest |relu pre-activation| in fp64 -- over the EPNet hidden layers, every gate's
hidden layer and C d gate of every relu layer -- is below PRE_EPS = 1e-5 may take the other branch in fp32: its
output-gradient row is zeroed before either side runs, every case asserts such examples are at most 10 %
(tests/test_pepnet_host.py checks the same without a GPU), and cases under 100 examples use the first seed 1, 2, 3, ...
without any (chosen on the fp64 reading alone).  Where the fp64 value of a tensor is zero throughout, the kernels must
return exact zeros.

Measured on the MI355X (the first run, 28 of these tests passed in 4.4 s; the one that did not was a mistake of the test
about where KerasAdam leaves the gradients): a DIGEST, per case the near-kink examples and the largest error / bound
ratio over its tensors (14 per POSO-MLP case, 6 per lookup case, 101 / 59 per layer case) with the tensor it belongs to.
  poso 1x1x1x1x(1)xsigmoid, m 1               near 0 of 1       0.009 (gate)
  poso 2x15x19x3x(5,3,1), m 2                 near 0 of 2       0.012 (a)
  poso 33x72x88x3x(64,16,1), m 2              near 0 of 33      0.034 (a)
  poso 33x72x88x3x(1)xsigmoid, m 2            near 0 of 33      0.020 (h)
  poso 17x72x88x1x(64,16)xrelu relu, m 2      near 0 of 17      0.128 (dC)
  poso 17x512x512x4x(128)xlinear, m 4         near 0 of 17      0.084 (h)
  poso 2049x72x88x3x(64,16,1), m 2            near 13 of 2049   0.035 (h)
  epnet 1x3x1x1x1x1                           near 0 of 1       0.002 (dA)
  epnet 2x50x3x2x4x5                          near 0 of 2       0.010 (u)
  epnet 33x1000x9x2x8x16                      near 0 of 33      0.009 (u)
  epnet 2049x1000x9x2x8x16, zipf              near 4 of 2049    0.009 (u)
  epnet 17x100x26x4x16x16                     near 0 of 17      0.012 (u)
  epnet 33x1000x9x2x8x16, every id equal      near 0 of 33      0.006 (u)
  layer chain_layers=False, B = 32            near 0 of 32      0.160 (poso_mlp_layers.0.C_list.2)
  layer chain_layers=True, B = 32             near 0 of 32      0.044 (poso_mlp_layers.1.C_list.0)
"""
import copy
import functools

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import pepnet_ref as PR

pytestmark = pytest.mark.gpu

F32 = np.float32
CAT = ["sdk_type", "remote_host", "device_type", "dtu", "click_goods_num", "buy_click_num", "goods_show_num",
       "goods_click_num", "brand_name"]
PP = ["ppnet_cate1", "ppnet_cate2"]
EP = ["epnet_cate1", "epnet_cate2"]
POSO_DEFAULT, POSO_BIG = PR.POSO_CASES[2], PR.POSO_CASES[6]
EPNET_DEFAULT, EPNET_BIG = PR.EPNET_CASES[2], PR.EPNET_CASES[3]


def cu(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def case_id(c):
    return "x".join("-".join(map(str, v)) if isinstance(v, tuple) else str(v) for v in c)


class Worst:
    """the largest error / bound ratio of a test, for the digest"""

    def __init__(self):
        self.ratio, self.name = 0.0, "-"

    def check(self, name, got, want, t32, floor):
        err, bound = PR.rel_err(got, want), max(floor, 4 * PR.rel_err(t32, want))
        print("%-44s error/bound %.2e / %.2e = %.3f" % (name, err, bound, err / bound))
        assert np.shape(got) == np.shape(want), (name, np.shape(got), np.shape(want))
        if not np.any(want):
            assert not np.any(got), (name, "zero throughout in fp64: must be exact")
        assert err <= bound, (name, err, bound)
        if err / bound > self.ratio:
            self.ratio, self.name = err / bound, name

    def report(self, what):
        print("DIGEST %s: largest error / bound %.3f (%s)" % (what, self.ratio, self.name))


# ---- POSO-MLP -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def poso_dev(*case):
    c = PR.poso_case(*case)
    return cu(c["x"]), cu(c["g"]), [cu(p) for p in c["params"]], cu(c["dout"])


def run_poso(case, save=True, inputs=None):
    from explicit_tf2_recommendation_amd import ops
    x, g, w, dout = inputs or poso_dev(*case)
    units, acts, m = case[4], case[5], case[6]
    out, saved = ops.poso_mlp_fwd(x, g, w, units, acts, m, save=save)
    if not save:
        return out
    dx, dg, grads = ops.poso_mlp_bwd(x, g, w, saved, dout, units, acts, m)
    return [out, *saved, dx, dg, *grads]


@pytest.mark.parametrize("case", PR.POSO_CASES, ids=case_id)
def test_poso_mlp_matches_fp64(case):
    c = PR.poso_case(*case)
    near = c["near"]
    print("near-kink examples: %d of %d" % (near.sum(), len(near)))
    assert near.mean() <= 0.10 and (case[0] >= 100 or not near.any())
    ref, (tout, tdx, tdg, tgrads, tsaved) = c["ref"], PR.poso_case_t32(*case)
    res = [t.cpu().numpy() for t in run_poso(case)]
    assert len(res) == 1 + 4 + 2 + 7
    w = Worst()
    w.check("out", res[0], ref["out"], tout, 1e-5)
    for name, t in zip(PR.PO_SAVED, res[1:5]):
        w.check(name, t, ref[name], tsaved[name], 1e-5)
    w.check("dx", res[5], ref["dx"], tdx, 3e-5)
    w.check("dg", res[6], ref["dg"], tdg, 3e-5)
    for name, t, want, w32 in zip(PR.PO_NAMES, res[7:], ref["dparams"], tgrads):
        w.check("d" + name, t.reshape(np.shape(want)), want, np.reshape(w32, np.shape(want)), 3e-5)
    w.report("poso " + case_id(case))
    assert torch.equal(run_poso(case, save=False), run_poso(case)[0])    # inference writes the same out, bitwise


def test_strided_inputs_in_one_buffer_equal_contiguous_copies():
    """x and g as column blocks of one wider buffer (PEPNet's arrangement, and with an offset) against their copies."""
    case = POSO_DEFAULT
    x, g, w, dout = poso_dev(*case)
    B, Dm, Dg = case[0], case[1], case[2]
    buf = torch.full((B, 5 + Dm + 3 + Dg + 2), float("nan"), device="cuda")
    buf[:, 5:5 + Dm] = x
    buf[:, 8 + Dm:8 + Dm + Dg] = g
    xs, gs = buf[:, 5:5 + Dm], buf[:, 8 + Dm:8 + Dm + Dg]
    assert not xs.is_contiguous() and not gs.is_contiguous()
    want, got = run_poso(case), run_poso(case, inputs=(xs, gs, w, dout))
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    # x as the leading columns of g itself
    u = torch.cat([x, g[:, Dm:]], dim=1).contiguous()
    a = run_poso(case, inputs=(u[:, :Dm], u, w, dout))
    b = run_poso(case, inputs=(u[:, :Dm].contiguous(), u.clone(), w, dout))
    for s, t in zip(a, b):
        assert torch.equal(s, t)


# ---- EPNet lookup ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def epnet_dev(*case):
    c = PR.epnet_case(*case)
    return cu(c["table"]), cu(c["ids"], np.int64), [cu(p) for p in c["params"]], cu(c["du"])


def run_epnet(case, flag=None):
    from explicit_tf2_recommendation_amd import ops
    table, ids, w, du = epnet_dev(*case)
    u = ops.epnet_lookup_fwd(table, ids, case[2], *w, flag)
    drows, grads = ops.epnet_lookup_bwd(table, ids, case[2], *w, du)
    return [u, drows, *grads]


@pytest.mark.parametrize("case", PR.EPNET_CASES, ids=case_id)
def test_epnet_lookup_matches_fp64(case):
    c = PR.epnet_case(*case)
    B, V, F, P, E, Hg, kind = case
    near = c["near"]
    print("near-kink examples: %d of %d" % (near.sum(), len(near)))
    assert near.mean() <= 0.10 and (B >= 100 or not near.any())
    if kind == "equal":
        assert len(np.unique(c["ids"])) == 1
    if kind == "zipf":
        assert len(np.unique(c["ids"])) < c["ids"].size // 4               # rows repeat
    ref, (tu, tdtable, tgrads) = c["ref"], PR.epnet_case_t32(*case)
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    res = [t.cpu().numpy() for t in run_epnet(case, flag)]
    assert int(flag.item()) == 0
    w = Worst()
    w.check("u", res[0], ref["u"], tu, 1e-5)
    dtable = np.zeros((V, E))
    np.add.at(dtable, c["ids"].reshape(-1), res[1].astype(np.float64))
    w.check("dtable", dtable, ref["dtable"], tdtable, 3e-5)
    assert PR.rel_err(res[1].reshape(B, F + P, E), ref["drows"]) <= 3e-5
    for name, t, want, w32 in zip(PR.EP_NAMES, res[2:], ref["dparams"], tgrads):
        w.check("d" + name, t, want, w32, 3e-5)
    w.report("epnet " + case_id(case))


def test_sparse_gradient_of_the_lookup_is_the_dense_one():
    """functional.EmbEPNetLookup: the row gradients through the de-duplicated sparse path, every id equal included."""
    from explicit_tf2_recommendation_amd import functional as Fn
    for case in (EPNET_BIG, PR.EPNET_CASES[5]):
        c = PR.epnet_case(*case)
        table, ids, w, du = epnet_dev(*case)
        tb = table.clone().requires_grad_(True)
        ws = [t.clone().requires_grad_(True) for t in w]
        Fn.EmbEPNetLookup.apply(tb, ids, case[2], None, *ws).backward(du)
        assert tb.grad.is_sparse
        _, tdtable, _ = PR.epnet_case_t32(*case)
        Worst().check("dtable", tb.grad.to_dense().cpu().numpy(), c["ref"]["dtable"], tdtable, 3e-5)
        if case[6] == "equal":
            assert np.count_nonzero(np.abs(tb.grad.to_dense().cpu().numpy()).sum(1)) == 1     # all of it in one row


@pytest.mark.parametrize("col", [0, 10], ids=["main", "pp"])
def test_out_of_range_id_sets_the_flag(col):
    from explicit_tf2_recommendation_amd import ops
    table, ids, w, du = epnet_dev(*EPNET_DEFAULT)
    for bad in (1000, -1):
        ids2 = ids.clone()
        ids2[7, col] = bad
        flag = ops.new_flag(ids.device)
        u = ops.epnet_lookup_fwd(table, ids2, 9, *w, flag)
        assert int(flag.item()) == 1
        ids0 = ids.clone()
        ids0[7, col] = 0                                                    # reads row 0
        assert torch.equal(u, ops.epnet_lookup_fwd(table, ids0, 9, *w, None))
        drows, _ = ops.epnet_lookup_bwd(table, ids2, 9, *w, du)
        assert bool(torch.isfinite(drows).all())


# ---- both kernels: determinism, graphs, the allocation seam, errors -------------------------------------------------
def _both():
    return run_poso(POSO_BIG) + run_poso(POSO_DEFAULT) + run_epnet(EPNET_BIG) + run_epnet(EPNET_DEFAULT)


def test_every_output_is_bit_identical_run_to_run():
    a, b = _both(), _both()
    assert len(a) == 2 * 14 + 2 * 6
    for s, t in zip(a, b):
        assert torch.equal(s, t)


def test_graph_replay_equals_eager():
    """Forward + backward of both kernels captured in one hipGraph, replayed twice."""
    from explicit_tf2_recommendation_amd.engine import CAPTURE_MODE
    eager = [t.clone() for t in _both()]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        _both()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode=CAPTURE_MODE):
        static = _both()
    for _ in range(2):
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(static, eager):
            assert torch.equal(a, b)


@pytest.mark.parametrize("which", ["poso-33", "poso-2049", "epnet-33", "epnet-2049"])
def test_guards_and_poison(which):
    from explicit_tf2_recommendation_amd import ops
    case = {"poso-33": POSO_DEFAULT, "poso-2049": POSO_BIG, "epnet-33": EPNET_DEFAULT, "epnet-2049": EPNET_BIG}[which]
    run = run_poso if which.startswith("poso") else run_epnet
    want = run(case)
    with G.guarded(ops, G.POISON_NAN) as g:
        nan_run = run(case)
    assert g.allocations, "the run bypassed the seam"
    for t in nan_run:
        assert bool(torch.isfinite(t).all())
    with G.guarded(ops, G.POISON_FINITE):
        fin_run = run(case)
    for a, b, c in zip(want, nan_run, fin_run):
        assert torch.equal(a, b) and torch.equal(b, c)


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    from explicit_tf2_recommendation_amd._lib import lib
    case = PR.POSO_CASES[1]
    x, g, w, dout = poso_dev(*case)
    units, acts, m = case[4], case[5], case[6]
    with pytest.raises(RuntimeError):
        ops.poso_mlp_fwd(x.cpu(), g, w, units, acts, m)                       # no CPU fallback
    with pytest.raises(RuntimeError):
        ops.poso_mlp_fwd(x, g, [w[0].cpu()] + w[1:], units, acts, m)
    with pytest.raises(ValueError):
        ops.poso_mlp_fwd(x, g[:1], w, units, acts, m)                         # batches differ
    with pytest.raises(ValueError):
        ops.poso_mlp_fwd(x[:, :14].contiguous(), g, w, units, acts, m)        # W no longer fits
    with pytest.raises(ValueError):
        ops.poso_mlp_fwd(x, g, w[:1] + [w[1][:-1].contiguous()] + w[2:], units, acts, m)      # bg1 one short
    with pytest.raises(ValueError):
        ops.poso_mlp_fwd(x, g, w, units, acts[:2], m)
    with pytest.raises(ValueError):
        ops.poso_mlp_fwd(x.t().contiguous().t(), g, w, units, acts, m)        # inner stride is not 1
    with pytest.raises(NotImplementedError):
        ops.poso_mlp_fwd(x, g, w, units, ("relu", "PReLU", "sigmoid"), m)
    out, saved = ops.poso_mlp_fwd(x, g, w, units, acts, m)
    with pytest.raises(ValueError):
        ops.poso_mlp_bwd(x, g, w, saved, dout[:, :1].contiguous(), units, acts, m)
    with pytest.raises(ValueError):
        ops.poso_mlp_bwd(x, g, w, saved[:3] + (None,), dout, units, acts, m)
    with pytest.raises(RuntimeError):
        ops.poso_mlp_bwd(x, g, w, saved, dout.cpu(), units, acts, m)
    for bad in (dict(Dm=513), dict(Dg=513), dict(T=5), dict(units=[129]), dict(units=[128], m=5), dict(units=[1] * 5)):
        kw = dict(Dm=4, Dg=4, T=1, units=[2], m=2)
        kw.update(bad)
        with pytest.raises(NotImplementedError):
            ops.poso_mlp_check_shape(**kw)
        assert lib.rec_poso_mlp_scratch_bytes(8, kw["Dm"], kw["Dg"], kw["T"], len(kw["units"]), ops._ints(kw["units"]),
                                              kw["m"]) == 0
    with pytest.raises(ValueError):
        ops.poso_mlp_check_shape(4, 4, 1, [0])
    # the ABI itself: a workspace one byte short is -3, a NULL output -1, an unknown activation -2
    B, Dm, Dg, T = case[:4]
    need = lib.rec_poso_mlp_scratch_bytes(B, Dm, Dg, T, 3, ops._ints(units), m)
    assert need > 0
    dx, dg, grads = ops.poso_mlp_bwd(x, g, w, saved, dout, units, acts, m)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    codes = ops._ints([ops.ACT_CODE[a] for a in acts])
    P = ops._ptr
    args = (P(x), Dm, P(g), Dg, P(w[0]), P(w[2]), P(w[4]), P(w[6]), *[P(t) for t in saved], P(dout), B, Dm, Dg, T, 3,
            ops._ints(units), codes, m, P(dx), P(dg), *[P(t) for t in grads], P(ws))
    assert lib.rec_poso_mlp_bwd_f32(*args, need - 16 - 1, None) == -3         # (the query adds four floats)
    assert lib.rec_poso_mlp_fwd_f32(P(x), Dm, P(g), Dg, *[P(t) for t in w], B, Dm, Dg, T, 3, ops._ints(units), codes, m,
                                    None, None, None, None, None, None) == -1
    assert lib.rec_poso_mlp_fwd_f32(P(x), Dm, P(g), Dg, *[P(t) for t in w], B, Dm, Dg, T, 3, ops._ints(units),
                                    ops._ints([ops.ACT_TANH] * 3), m, P(out), None, None, None, None, None) == -2
    oe, se = ops.poso_mlp_fwd(x[:0], g[:0], w, units, acts, m)
    assert tuple(oe.shape) == (0, 3, 1) and [tuple(t.shape) for t in se] == [(0, 54), (0, 27), (0, 27), (0, 27)]
    dx, dg, gr = ops.poso_mlp_bwd(x[:0], g[:0], w, se, dout[:0], units, acts, m)
    assert tuple(dx.shape) == (0, 15) and tuple(dg.shape) == (0, 19)
    assert all(float(t.abs().sum()) == 0 for t in gr) and [t.shape for t in gr] == [t.shape for t in w]

    ecase = PR.EPNET_CASES[1]
    table, ids, ew, du = epnet_dev(*ecase)
    with pytest.raises(RuntimeError):
        ops.epnet_lookup_fwd(table.cpu(), ids, 3, *ew)
    with pytest.raises(RuntimeError):
        ops.epnet_lookup_fwd(table, ids.cpu(), 3, *ew)
    with pytest.raises(TypeError):
        ops.epnet_lookup_fwd(table, ids.to(torch.int32), 3, *ew)
    with pytest.raises(ValueError):
        ops.epnet_lookup_fwd(table, ids, 2, *ew)                              # the gates are three fields'
    with pytest.raises(ValueError):
        ops.epnet_lookup_fwd(table, ids, 5, *ew)                              # no personalisation column left
    with pytest.raises(ValueError):
        ops.epnet_lookup_bwd(table, ids, 3, *ew, du[:, :-1].contiguous())
    for bad in (dict(F=65), dict(E=65), dict(Hg=65), dict(P=9, E=16), dict(F=31, E=16)):
        kw = dict(F=3, P=2, E=4, Hg=5)
        kw.update(bad)
        with pytest.raises(NotImplementedError):
            ops.epnet_check_shape(**kw)
        assert lib.rec_epnet_lookup_scratch_bytes(8, kw["F"], kw["P"], kw["E"], kw["Hg"]) == 0
    with pytest.raises(NotImplementedError):
        ops.pepnet_check_shape(9, 2, 8, 16, 5)
    need = lib.rec_epnet_lookup_scratch_bytes(2, 3, 2, 4, 5)
    drows, eg = ops.epnet_lookup_bwd(table, ids, 3, *ew, du)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    assert lib.rec_epnet_lookup_bwd_f32(P(table), 50, 4, P(ids), *[P(t) for t in ew], P(du), 2, 3, 2, 4, 5, P(drows),
                                        *[P(t) for t in eg], P(ws), need - 16 - 1, None) == -3
    ue = ops.epnet_lookup_fwd(table, ids[:0], 3, *ew)
    assert tuple(ue.shape) == (0, 20)
    dr, ge = ops.epnet_lookup_bwd(table, ids[:0], 3, *ew, du[:0])
    assert tuple(dr.shape) == (0, 4) and all(float(t.abs().sum()) == 0 for t in ge)


# ---- the layer ------------------------------------------------------------------------------------------------------
def _batch(ids, with_epnet, rng=None):
    names = CAT + PP
    b = {n: ids[:, i:i + 1].copy() for i, n in enumerate(names)}
    if with_epnet:
        r = rng or np.random.default_rng(5)
        for n in EP:
            b[n] = r.integers(0, PR.LAYER_V, (ids.shape[0], 1)).astype(np.int64)
    return b


def _layer(chain, c=None, V=PR.LAYER_V):
    from explicit_tf2_recommendation_amd import layers
    lay = layers.PEPNetLayer(feature_dims=V, chain_layers=chain).cuda()
    if c is not None:
        sd = PR.state_dict_of(c["table"], c["gates"], c["towers"])
        with torch.no_grad():
            for k, p in lay.named_parameters():
                p.copy_(torch.from_numpy(np.asarray(sd[k], F32)).reshape(p.shape))
    return lay


@pytest.mark.parametrize("chain", [False, True], ids=["literal", "chained"])
def test_layer_parity_with_the_torch_cpu_transcription(chain):
    from explicit_tf2_recommendation_amd import data
    c = PR.layer_case(chain)
    assert not c["near"].any()
    lay = _layer(chain, c)
    out = lay(data.to_device(_batch(c["ids"], True)))
    assert tuple(out.shape) == (PR.LAYER_B, 3, 1)
    out.backward(cu(c["gout"]))
    args = (c["table"], c["ids"], PR.LAYER_F, c["gates"], c["towers"], chain, c["gout"])
    t64, t32 = PR.layer_torch_grads(*args, torch.float64), PR.layer_torch_grads(*args, torch.float32)
    w = Worst()
    w.check("output", out.detach().cpu().numpy(), t64[0], t32[0], 1e-5)
    want, w32 = PR.state_dict_of(*t64[1:]), PR.state_dict_of(*t32[1:])
    params = dict(lay.named_parameters())
    assert params.keys() == want.keys() and len(want) == 100
    dead = [k for k in want if want[k] is None]
    assert len(dead) == (0 if chain else 42)
    for k in want:
        if want[k] is None:
            assert params[k].grad is None, k
            continue
        g = params[k].grad
        g = (g.to_dense() if g.is_sparse else g).cpu().numpy()
        w.check(k[-44:], g.reshape(np.shape(want[k])), want[k], w32[k], 3e-5)
    assert params["embedding_layer.embeddings"].grad.is_sparse
    w.report("layer chain_layers=%s" % chain)
    # a batch without the epnet_* keys, and one with other values under them, give the same bits
    grads = {k: (p.grad.to_dense() if p.grad.is_sparse else p.grad).clone() for k, p in params.items()
             if p.grad is not None}
    for batch in (_batch(c["ids"], False), _batch(c["ids"], True, np.random.default_rng(99))):
        lay.zero_grad(set_to_none=True)
        out2 = lay(data.to_device(batch))
        assert torch.equal(out2, out)
        out2.backward(cu(c["gout"]))
        for k, p in params.items():
            if k in grads:
                assert torch.equal(p.grad.to_dense() if p.grad.is_sparse else p.grad, grads[k]), k
            else:
                assert p.grad is None
    with torch.no_grad():
        assert torch.equal(lay(data.to_device(_batch(c["ids"], False))), out)      # inference == training, bitwise
    assert torch.equal(lay.task_outputs(data.to_device(_batch(c["ids"], False))), out[:, :, 0])


def test_out_of_range_id_raises():
    from explicit_tf2_recommendation_amd import data
    lay = _layer(False, V=100)
    ids = np.random.default_rng(1).integers(0, 100, (16, 11)).astype(np.int64)
    lay(data.to_device(_batch(ids, False)))
    for col in (3, 10):
        bad = ids.copy()
        bad[5, col] = 100
        with pytest.raises(IndexError):
            lay(data.to_device(_batch(bad, False)))


def test_poso_for_mlp_layer_alone_and_gatenu_direct_call():
    """PosoForMLPLayer(main, gate) in both modes and GateNULayer's direct call against the numpy reading."""
    from explicit_tf2_recommendation_amd import layers
    case = PR.POSO_CASES[4]                                                  # one task, [64, 16], relu relu
    c = PR.poso_case(*case)
    x, g, _, _ = poso_dev(*case)
    for chain in (True, False):
        lay = layers.PosoForMLPLayer(units=[64, 16], activations=["relu", "relu"], main_dim=72, gate_dim=88,
                                     chain_layers=chain).cuda()
        tower = c["towers"][0] if chain else [None, dict(c["towers"][0][1], W=PR.f32_exact(
            np.random.default_rng(3).normal(0, 0.1, (72, 16))))]
        with torch.no_grad():
            for i, t in enumerate(tower):
                if t is None:
                    continue
                for p, k in ((lay.dense_layers[i].kernel, "W"), (lay.dense_layers[i].bias, "b"), (lay.C_list[i], "C"),
                             (lay.gates[i].gate.layers[0].kernel, "A"), (lay.gates[i].gate.layers[0].bias, "a"),
                             (lay.gates[i].gate.layers[1].kernel, "Bm"), (lay.gates[i].gate.layers[1].bias, "bm")):
                    p.copy_(cu(t[k]).reshape(p.shape))
        xg, gg = x.clone().requires_grad_(True), g.clone().requires_grad_(True)
        out = lay(xg, gg)
        assert tuple(out.shape) == (17, 16)
        out.sum().backward()
        acts = ["relu", "relu"] if chain else ["relu"]
        ref = PR.poso_numpy(c["x"], c["g"], [tower if chain else tower[1:]], acts, np.ones((17, 1, 16)))
        assert PR.rel_err(out.detach().cpu().numpy(), ref["out"][:, 0]) <= 1e-5
        assert PR.rel_err(xg.grad.cpu().numpy(), ref["dx"]) <= 3e-5          # a standalone layer uses both gradients whole
        assert PR.rel_err(gg.grad.cpu().numpy(), ref["dg"]) <= 3e-5
        assert (lay.dense_layers[0].kernel.grad is None) == (not chain)
    gate = layers.GateNULayer(8, 4, input_dim=88).cuda()
    p = {k: t.detach().cpu().numpy().astype(np.float64) for k, t in zip(PR.EP_NAMES, gate.parameters())}
    assert PR.rel_err(gate(g).detach().cpu().numpy(), PR.gatenu_numpy(c["g"], p)[2]) <= 1e-5


@pytest.mark.parametrize("chain", [False, True], ids=["literal", "chained"])
def test_graphed_train_step_equals_the_eager_loop(chain):
    """engine.GraphedTrainStep with three labels and KerasAdam, 3 steps; literal mode leaves 42 gradients None."""
    from explicit_tf2_recommendation_amd import data, engine
    from explicit_tf2_recommendation_amd import functional as Fn
    from explicit_tf2_recommendation_amd.model_manager import KerasAdam
    labels, B, V = ("l0", "l1", "l2"), 256, 500
    a = _layer(chain, V=V)
    b = copy.deepcopy(a)
    r = np.random.default_rng(7)
    batches = []
    for _ in range(3):
        bt = _batch(PR.make_ids(r, B, V, 11, "zipf"), False)
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
    assert sum(g is None for g in step.grads) == (0 if chain else 42)     # KerasAdam skipped them
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.equal(p, q), k
