"""ETA on the GPU: the fused SimHash search (csrc/eta.hip) against the numpy reading of tests/eta_ref.py, and
eta.ETALayer fused and composed against the torch-CPU transcription.

Exact inputs (table in {-8..8}/8, H in {-4..4}/4; every sum exact in fp32 in any order): scores, chosen, sel, sel_valid
and sel_ids must equal the oracle BIT FOR BIT, for every case of ER.CASES -- T on both sides of the wave and of the
workgroup, m on both sides of the 16-column kernel, K at 1, 3, 16 and T, every row-load width, D from 2 to 256 -- with
their ties, zero codes, rows without a valid step and steps padded in the first column alone.  Random inputs: an example
with an undecided projection (ER.undecided: |p64| <= 2 D 2^-24 sum |x_d H_dj|) in its item or a valid step is left out,
at most a tenth of the examples (asserted); on the others chosen, sel, sel_valid, sel_ids are compared exactly and scores
on the valid steps.

The layer: the project's rule, as tests/test_gpu_sim.py states it -- max|got - want| / max|want| against fp64 within 4 x
the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (outputs) / 3e-5 (gradients); a tensor that
is zero throughout in fp64 must be exactly zero; the key bias' gradient, zero in exact arithmetic, by the scale of the
query bias'.  Undecided examples get weight zero and are left out of the output comparison.

Measured on the MI355X: 35 passed in 4.5 s, the slowest 0.75 s.  Random inputs: 3 of 256, 0 of 256, 0 of 128 and 3 of 256
examples left out, every other one equal in every element; the five layer cases leave out 0 of 48.  The layer's 280
`error / bound` lines all sit on their floor: largest ratios output 3.9e-7 / 1e-5 (composed), gradients
`shortterm_mha._value_dense.kernel` 1.7e-6 / 3e-5 (fused) and 1.7e-6 / 3e-5 (composed).
"""
import copy

import numpy as np
import pytest
import torch

from tests import eta_ref as ER
from tests import guarded as G

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = lambda c: "x".join(map(str, c))
OUT = ("scores", "chosen", "sel", "sel_valid", "sel_ids")


def cu(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


_DEV = {}


def dev(case, kind="exact", seed=0, pad=0):
    key = (case, kind, seed, pad)
    if key not in _DEV:
        c = ER.inputs(*key)
        d = {k: cu(c[k]) for k in ("table", "H", "q", "gsel")}
        d["series"], d["items"] = cu(c["series"], np.int64), cu(c["items"], np.int64)
        _DEV[key] = d
    return _DEV[key]


def run(case, kind="exact", seed=0, pad=0, ops=None, **over):
    """-> scores, chosen, sel, sel_valid, sel_ids"""
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    d = dict(dev(case, kind, seed, pad))
    d.update(over)
    return ops.eta_search_fwd(d["table"], d["series"], d["q"], d["H"], pad, ER.dims(case)[5], d.get("oob"),
                              want_scores=d.get("want_scores", True))


def same_bits(name, got, want):
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype, want.shape, want.dtype)
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), name


def check_exact(got, ref):
    for name, t in zip(OUT, got):
        same_bits(name, host(t), ref[name])


@pytest.mark.parametrize("case", ER.CASES, ids=ids)
def test_exact_inputs_match_the_oracle_bit_for_bit(case):
    check_exact(run(case), ER.reference(case))


def test_a_padding_index_other_than_zero():
    case, pad = (6, 65, 3, 22, 32, 1), 7
    ref = ER.reference(case, "exact", 0, pad)
    assert (ER.inputs(case, "exact", 0, pad)["series"][:, :, 0] == pad).any() and not ref["valid"].all()
    check_exact(run(case, pad=pad), ref)
    case = ER.REFERENCE
    check_exact(run(case, pad=pad), ER.reference(case, "exact", 0, pad))


@pytest.mark.parametrize("case,seed", [(c, 0) for c in ER.RANDOM_CASES] + [(ER.RANDOM_CASES[0], 1)],
                         ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_random_inputs_match_where_every_sign_is_decided(case, seed):
    c, ref = ER.inputs(case, "random", seed), ER.reference(case, "random", seed)
    out = ER.undecided(c["table"], c["series"], c["q"], c["H"], 0)
    print("%s seed %d: %d of %d examples left out" % (ids(case), seed, out.sum(), len(out)))
    assert out.mean() <= ER.MAX_LEFT_OUT
    got = [host(t) for t in run(case, "random", seed)]
    keep = ~out
    for name, g in zip(OUT[1:], got[1:]):
        same_bits(name, np.ascontiguousarray(g[keep]), ref[name][keep])
    valid = ref["valid"] & keep[:, None]
    assert np.array_equal(got[0][valid], ref["scores"][valid])
    assert (got[0] >= 0).all() and (got[0] <= ER.dims(case)[4]).all()


def test_a_nan_row_equals_nothing_and_nothing_faults():
    case = (6, 63, 3, 16, 16, 16)
    c = dict(ER.inputs(case))
    table, series, items = c["table"].copy(), c["series"].copy(), c["items"].copy()
    table[ER.NAN_ROW] = np.nan
    series[4, 3], series[5, 0, 1], items[5] = ER.NAN_ROW, ER.NAN_ROW, ER.NAN_ROW     # whole steps, one column, an item
    q = ER.lookup(table, items).reshape(len(items), -1)
    ref = ER.search_numpy(table, series, q, c["H"], 0, ER.dims(case)[5])
    assert not ref["scores"][5].any() and ref["scores"][4, 3] == 0 and ref["scores"][4].any()
    got = run(case, table=cu(table), series=cu(series, np.int64), q=cu(q))
    check_exact(got, ref)


def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows():
    from explicit_tf2_recommendation_amd import ops
    case = (6, 64, 1, 48, 31, 3)
    flag = ops.new_flag("cuda")
    run(case, oob=flag)
    assert int(flag.item()) == 0
    c = ER.inputs(case)
    series = c["series"].copy()
    series[3, 2, 0], series[4, 0, 0], series[5, 5, 0] = -1, ER.V_CASE, 2 ** 40
    ref = ER.search_numpy(c["table"], series, c["q"], c["H"], 0, 3)
    got = run(case, series=cu(series, np.int64), oob=flag)
    assert int(flag.item()) == 1
    check_exact(got, ref)
    case = ER.REFERENCE                                                      # in a column that is not the first
    series = ER.inputs(case)["series"].copy()
    series[1, 4, 2] = ER.V_CASE + 5
    flag.zero_()
    c = ER.inputs(case)
    check_exact(run(case, series=cu(series, np.int64), oob=flag), ER.search_numpy(c["table"], series, c["q"], c["H"], 0, 3))
    assert int(flag.item()) == 1


def test_strided_table_strided_rows_and_no_scores():
    for case in (ER.REFERENCE, (6, 63, 3, 16, 16, 16), (6, 20, 3, 4, 8, 3)):
        table = dev(case)["table"]
        E = table.shape[1]
        for extra in (3, 4, 16):                                                 # scalar loads, 16-byte loads
            wide = torch.full((table.shape[0], E + extra), 7.0, device="cuda")
            wide[:, :E] = table
            view = wide[:, :E]
            assert view.stride(0) == E + extra
            for a, b in zip(run(case), run(case, table=view)):
                assert G.bit_equal(a, b)
        got = run(case, want_scores=False)
        assert got[0] is None
        check_exact((run(case)[0],) + got[1:], ER.reference(case))


def test_two_runs_are_bit_identical():
    for case, kind in (((5, 257, 3, 85, 32, 3), "exact"), (ER.RANDOM_CASES[0], "random"), (ER.RANDOM_CASES[2], "random")):
        for a, b in zip(run(case, kind), run(case, kind)):
            assert G.bit_equal(a, b)


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    case = ER.REFERENCE
    d = dev(case)
    B, T, Cn, E, m, K, D = ER.dims(case)
    with pytest.raises(RuntimeError):
        ops.eta_search_fwd(d["table"].cpu(), d["series"], d["q"], d["H"], 0, K)                 # no CPU fallback
    with pytest.raises(TypeError):
        ops.eta_search_fwd(d["table"], d["series"].int(), d["q"], d["H"], 0, K)
    with pytest.raises(ValueError):
        ops.eta_search_fwd(d["table"], d["series"], d["q"][:, :-1].contiguous(), d["H"], 0, K)
    with pytest.raises(ValueError):
        ops.eta_search_fwd(d["table"], d["series"], d["q"], d["H"][:-1].contiguous(), 0, K)
    with pytest.raises(ValueError):
        ops.eta_search_fwd(d["table"], d["series"], d["q"], d["H"], 0, T + 1)
    z = lambda *s: torch.zeros(*s, device="cuda")
    zi = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError, match="<= 16"):
        ops.eta_search_fwd(z(10, 4), zi(2, 20, 1), z(2, 4), z(4, 8), 0, 17)
    with pytest.raises(NotImplementedError, match="<= 32"):
        ops.eta_search_fwd(z(10, 4), zi(2, 20, 1), z(2, 4), z(4, 33), 0, 3)
    scores, chosen, sel, sel_valid, sel_ids = ops.eta_search_fwd(d["table"], d["series"][:0], d["q"][:0], d["H"], 0, K)
    assert tuple(sel.shape) == (0, K, D) and tuple(chosen.shape) == (0, K) and tuple(scores.shape) == (0, T)
    assert tuple(sel_ids.shape) == (0, K, Cn) and sel_ids.dtype == torch.int64


# ---- guards and poison under the family's allocations -------------------------------------------------------------------
def body_driver(ops, case):
    flag = ops.new_flag("cuda")
    return (flag,) + run(case, ops=ops, oob=flag) + run(case, ops=ops, want_scores=False)[1:]


@pytest.mark.parametrize("case", ((5, 1, 1, 2, 1, 1), (6, 65, 3, 22, 32, 1), (5, 257, 1, 64, 16, 16)), ids=ids)
def test_guards_and_poison(case):
    """nothing is written outside scores, chosen, sel, sel_valid and sel_ids, and every element of them is written: the
    poisoned runs equal the oracle bit for bit (0xFF reads as -1 / NaN, 0x7F as 0x7F7F7F7F)"""
    from explicit_tf2_recommendation_amd import ops
    ref = ER.reference(case)
    for poison in (G.POISON_NAN, G.POISON_FINITE):
        with G.guarded(ops, poison) as g:
            res = body_driver(ops, case)
        assert len(g.allocations) == 10                                        # the flag, 5 outputs, 4 outputs
        check_exact(res[1:6], ref)
        check_exact((res[1],) + res[6:], ref)
        assert int(res[0].item()) == 0


# ---- the backward ---------------------------------------------------------------------------------------------------------
def _dense(g):
    return host(g.coalesce().to_dense() if g.is_sparse else g)


@pytest.mark.parametrize("case", (ER.REFERENCE, (6, 63, 3, 16, 16, 16), (5, 257, 3, 85, 32, 3)), ids=ids)
def test_the_table_gradient_equals_the_composed_path_s_bit_for_bit(case):
    from explicit_tf2_recommendation_amd import functional as Fn
    d, c, ref = dev(case), ER.inputs(case), ER.reference(case)
    B, T, Cn, E, m, K, D = ER.dims(case)
    want = ER.dense_table_grad(c, ref["chosen"])
    # fused, alone
    table = d["table"].clone().requires_grad_(True)
    sel, sel_valid, chosen, scores = Fn.EtaSearch.apply(table, d["q"], d["series"], d["H"], 0, K)
    assert not sel_valid.requires_grad and not chosen.requires_grad and not scores.requires_grad
    (sel * d["gsel"]).sum().backward()
    assert table.grad.is_sparse
    same_bits("fused", _dense(table.grad), want)
    # composed: a gather of the whole series, a gather of the chosen steps; the dense [B,T,D] gradient goes back
    table2 = d["table"].clone().requires_grad_(True)
    x = Fn.Gather.apply(table2, d["series"], None).reshape(B, T, D)
    top = torch.gather(x, 1, chosen.long().unsqueeze(-1).expand(-1, -1, D))
    assert torch.equal(top, sel)
    (top * d["gsel"]).sum().backward()
    same_bits("composed", _dense(table2.grad), want)
    # through a GradSink shared with the Gather of the items: one plan, one sparse gradient
    table3 = d["table"].clone().requires_grad_(True)
    H = d["H"].clone().requires_grad_(True)
    sink = Fn.GradSink(d["items"].numel())
    q = Fn.Gather.apply(table3, d["items"], None, sink).reshape(B, D)
    sel3 = Fn.EtaSearch.apply(table3, q, d["series"], H, 0, K, None, sink)[0]
    gq = (d["gsel"][:, 0] * 2).contiguous()
    ((sel3 * d["gsel"]).sum() + (q * gq).sum()).backward()
    both = want.astype(np.float64)
    np.add.at(both, c["items"].reshape(-1), host(gq).astype(np.float64).reshape(-1, E))
    same_bits("sink", _dense(table3.grad), both.astype(F32))
    assert H.grad is None and sink.ids is None and sink.buf is None
    # no gradient through sel: nothing to do, nothing left in the sink
    table4 = d["table"].clone().requires_grad_(True)
    sink = Fn.GradSink(d["items"].numel())
    q = Fn.Gather.apply(table4, d["items"], None, sink).reshape(B, D)
    Fn.EtaSearch.apply(table4, q, d["series"], d["H"], 0, K, None, sink)
    (q * gq).sum().backward()
    only = np.zeros(want.shape, np.float64)
    np.add.at(only, c["items"].reshape(-1), host(gq).astype(np.float64).reshape(-1, E))
    same_bits("items alone", _dense(table4.grad), only.astype(F32))


# ---- the layer ----------------------------------------------------------------------------------------------------------
def check(name, got, want, t32, floor):
    err, bound = ER.rel_err(got, want), max(floor, 4 * ER.rel_err(t32, want))
    print("%-44s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


def check_dbk(name, got, want, t32, dbq):
    scale = np.abs(dbq).max() or 1.0
    err, bound = np.abs(got - want).max() / scale, max(3e-5, 4 * np.abs(t32 - want).max() / scale)
    print("%-44s error/bound %.2e / %.2e = %.2f (by max|dbq|)" % (name, err, bound, err / bound))
    assert got.shape == want.shape and err <= bound, (name, err, bound)


def _layer(seed, mask_mode, fused, k=3):
    from explicit_tf2_recommendation_amd import eta
    sd = ER.layer_state(seed)
    lay = eta.ETALayer(feature_dims=ER.LAYER_V, mask_mode=mask_mode, fused=fused, lsh_topk=k).cuda()
    lay.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    return lay, sd


def _grads(lay):
    out = {}
    for n, q in lay.named_parameters():
        out[n] = np.zeros(tuple(q.shape), F32) if q.grad is None else host(q.grad.to_dense() if q.grad.is_sparse else q.grad)
    return out


# T: the long series; S: the short one, on both sides of the attention kernel's 16 keys; k = 3 > T = 2
@pytest.mark.parametrize("mask_mode,T,S", (("reference", 20, 5), ("valid", 20, 5), ("reference", 6, 20), ("valid", 70, 16),
                                           ("valid", 2, 3)), ids=lambda v: str(v))
def test_eta_layer_fused_and_composed_against_the_transcription(mask_mode, T, S):
    from explicit_tf2_recommendation_amd import data
    seed, B = 5, ER.LAYER_B
    ins = ER.layer_inputs(seed, B, T, S)
    sd = ER.layer_state(seed)
    keep = ~ER.layer_undecided(sd, ins)
    print("%d of %d examples left out" % ((~keep).sum(), B))
    assert keep.mean() >= 1 - ER.MAX_LEFT_OUT
    w = ins.pop("weight") * keep[:, None].astype(F32)
    t64, t32 = (ER.eta_layer_torch(sd, ins, dt, mask_mode, 3, w) for dt in (torch.float64, torch.float32))
    assert np.array_equal(t64["chosen"][keep], t32["chosen"][keep])
    batch = data.to_device(ins)
    names = set(batch)
    outs = {}
    for fused in (True, False):
        lay, _ = _layer(seed, mask_mode, fused)
        res = lay(batch)
        assert res.keys() == {"output"} and set(batch) == names and tuple(res["output"].shape) == (B, 1)
        tag = "fused " if fused else "composed "
        check(tag + "output", host(res["output"])[keep], t64["output"][keep], t32["output"][keep], 1e-5)
        (res["output"] * cu(w)).sum().backward()
        grads = _grads(lay)
        assert grads.keys() == t64["grads"].keys()
        for n in grads:
            if n.endswith("_key_dense.bias"):
                check_dbk(tag + n, grads[n], t64["grads"][n], t32["grads"][n],
                          t64["grads"][n.replace("_key_dense", "_query_dense")])
            else:
                check(tag + n, grads[n], t64["grads"][n], t32["grads"][n], 3e-5)
        assert lay.H.grad is None and torch.equal(lay.H.cpu(), torch.from_numpy(sd["projection_matrix"]))
        if fused:
            assert lay.embed.embeddings.grad.is_sparse                         # one sparse gradient for all four lookups
        outs[fused] = host(res["output"])
    assert ER.rel_err(outs[True][keep], outs[False][keep]) <= 1e-5


def test_out_of_range_id_raises():
    from explicit_tf2_recommendation_amd import data
    ins = ER.layer_inputs(1, ER.LAYER_B, 6, 4)
    ins.pop("weight")
    for fused in (True, False):
        lay, _ = _layer(1, "valid", fused)
        lay(data.to_device(ins))
        for name in ("longterm_shop_ids", "shortterm_cate_ids", "label_goods_ids", "utag2"):
            bad = {k: v.copy() for k, v in ins.items()}
            bad[name].reshape(-1)[5] = ER.LAYER_V
            with pytest.raises(IndexError):
                lay(data.to_device(bad))


def test_graphed_train_step_equals_eager():
    """Forward plus backward captured once and replayed over three batches against an eager copy of the layer: the loss
    and every gradient are equal bit for bit, and the table's gradient is ONE sparse tensor."""
    from explicit_tf2_recommendation_amd import data, engine, functional as Fn
    T, S, B = 40, 8, ER.LAYER_B
    lay, _ = _layer(2, "valid", True)
    eager = copy.deepcopy(lay)

    def batch_of(seed):
        ins = ER.layer_inputs(seed, B, T, S)
        ins.pop("weight")
        ins["label"] = np.random.default_rng(seed).integers(0, 2, B)
        return data.to_device(ins)

    batches = [batch_of(s) for s in (11, 12, 13)]
    step = engine.GraphedTrainStep(lay, batches[0], label_name="label")
    for m in eager.modules():
        if hasattr(m, "check_ids"):
            m.check_ids = False
    for b in batches:
        loss = step(b)
        for q in eager.parameters():
            q.grad = None
        out = eager({k: v for k, v in b.items() if k != "label"})["output"]
        want = Fn.KerasBCE.apply(out, b["label"].to(torch.float32).contiguous())
        want.backward()
        assert torch.equal(loss.reshape(()), want.detach().reshape(()))
        for (name, a), q in zip(lay.named_parameters(), eager.parameters()):
            assert a.grad is not None and q.grad is not None and a.grad.is_sparse == q.grad.is_sparse, name
            if a.grad.is_sparse:
                assert name == "embed.embeddings"
                assert torch.equal(a.grad._indices(), q.grad._indices()), name
                assert torch.equal(a.grad._values(), q.grad._values()), name
            else:
                assert torch.equal(a.grad, q.grad), name
