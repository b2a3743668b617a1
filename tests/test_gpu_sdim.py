"""SDIM on the GPU: the fused hash-bucket interest (csrc/sdim.hip), forward and backward, against the numpy reading of
tests/sdim_ref.py, and sdim.SDIMLayer fused and composed against the torch-CPU transcription.

Exact inputs (table in {-8..8}/8, H in {-4..4}/4; every projection and bucket sum exact in fp32 in any order): out,
codes, qcodes, cnt and gkeys must equal the oracle BIT FOR BIT in both mask modes, for every case of DR.CASES -- T on
both sides of the wave and of the workgroup, G m on both sides of the 16-column kernel, S at 1 and 16, every row-load
width, D from 2 to 256 -- with their empty buckets, rows without a valid step and steps padded in the first column
alone.  Random inputs: an example with an undecided projection (DR.undecided) in a candidate or in a step that enters a
sum or a count is left out, at most a tenth of the examples (asserted); on the others codes, qcodes and cnt are compared
exactly and out and gkeys against fp64 within DR.out_bound / DR.gkeys_bound, the worst-case rounding of the kernel's own
operation count (derived in tests/sdim_ref.py, not tuned).

The layer: the project's rule, as tests/test_gpu_sim.py states it -- max|got - want| / max|want| against fp64 within 4 x
the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (outputs) / 3e-5 (gradients); a tensor that
is zero throughout in fp64 must be exactly zero; the key bias' gradient, zero in exact arithmetic, by the scale of the
query bias'.  Undecided examples get weight zero and are left out of the output comparison.

Measured on the MI355X: 56 passed in about 5 s, the slowest 0.75 s.  Random inputs: 4, 0, 2 and 2 of 256 / 256 / 128 / 256
examples left out in 'reference' mode and 4, 0, 1 and 1 in 'valid'; on the others the largest error / bound is 0.35 for
out and 0.31 for gkeys.  The six layer cases leave out 0 of 48; their 240 `error / bound` lines all sit on their floor,
the largest `shortterm_mha._value_dense.kernel` 1.6e-6 / 3e-5 (fused).
"""
import copy

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import sdim_ref as DR

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = lambda c: "x".join(map(str, c))
OUT = ("out", "codes", "qcodes", "cnt")


def cu(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


_DEV = {}


def dev(case, kind="exact", seed=0, pad=0):
    key = (case, kind, seed, pad)
    if key not in _DEV:
        c = DR.inputs(*key)
        d = {k: cu(c[k]) for k in ("table", "H", "q", "gout")}
        d["series"], d["items"] = cu(c["series"], np.int64), cu(c["items"], np.int64)
        _DEV[key] = d
    return _DEV[key]


def run(case, mode, kind="exact", seed=0, pad=0, ops=None, **over):
    """-> out, codes, qcodes, cnt, gkeys"""
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    d = dict(dev(case, kind, seed, pad))
    d.update(over)
    fwd = ops.sdim_interest_fwd(d["table"], d["series"], d["q"], d["H"], pad, mode, d.get("oob"))
    E, m = d["table"].shape[1], d["H"].shape[2]
    gkeys = ops.sdim_interest_bwd(d["series"], E, m, pad, fwd[1], fwd[2], fwd[3], d["gout"], mode)
    return fwd + (gkeys,)


def same_bits(name, got, want):
    want = np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, got.dtype, want.shape, want.dtype)
    assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(want).view(np.uint8)), name


def check_exact(got, ref, gkeys=True):
    for name, t in zip(OUT + ("gkeys",) * gkeys, got):
        same_bits(name, host(t), ref[name])


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("case", DR.CASES, ids=ids)
def test_exact_inputs_match_the_oracle_bit_for_bit(case, mode):
    check_exact(run(case, mode), DR.reference(case, mode))


def test_a_padding_index_other_than_zero():
    case, pad = (6, 65, 3, 22, 4, 8, 2), 7
    for mode in DR.MODES:
        ref = DR.reference(case, mode, "exact", 0, pad)
        assert ref["pad"].any() and not ref["pad"].all()
        check_exact(run(case, mode, pad=pad), ref)
        check_exact(run(DR.REFERENCE, mode, pad=pad), DR.reference(DR.REFERENCE, mode, "exact", 0, pad))


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("case,seed", DR.RANDOM_CASES, ids=lambda v: ids(v) if isinstance(v, tuple) else str(v))
def test_random_inputs_within_the_rounding_bound_where_every_sign_is_decided(case, seed, mode):
    c, ref = DR.inputs(case, "random", seed), DR.reference(case, mode, "random", seed)
    left = DR.undecided(c["table"], c["series"], c["q"], c["H"], 0, mode)
    print("%s seed %d %s: %d of %d examples left out" % (ids(case), seed, mode, left.sum(), len(left)))
    assert left.mean() <= DR.MAX_LEFT_OUT
    keep = ~left
    out, codes, qcodes, cnt, gkeys = [host(t) for t in run(case, mode, "random", seed)]
    same_bits("qcodes", np.ascontiguousarray(qcodes[keep]), ref["qcodes"][keep])
    same_bits("cnt", np.ascontiguousarray(cnt[keep]), ref["cnt"][keep])
    enters = keep[:, None] & (np.ones_like(ref["pad"]) if mode == "reference" else ~ref["pad"])
    assert np.array_equal(codes[enters], ref["codes"][enters])
    for name, got, bound in (("out", out, DR.out_bound(c["table"], c["series"], ref, mode, case[4])),
                             ("gkeys", gkeys, DR.gkeys_bound(c["gout"], ref, mode))):
        err = np.abs(got.astype(np.float64) - ref[name + "64"])[keep]
        worst = (err / np.maximum(bound[keep], 1e-300)).max()
        print("%-6s largest error %.3e, largest error / bound %.3f" % (name, err.max(), worst))
        assert np.isfinite(got[keep]).all() and (err <= bound[keep]).all(), name
    assert out[keep].any() and gkeys[keep].any()


@pytest.mark.parametrize("case", DR.ARITHMETIC_CASES, ids=ids)
def test_the_projection_rounds_the_product_before_the_sum_and_equal_ids_give_equal_codes(case):
    """No example is left out here.  On DR.arithmetic_inputs the sign of two projections in three is decided by their
    roundings alone, so the codes pin the arithmetic the header states -- d in order, the product rounded before the sum,
    nothing fused (a contracted build differs in two steps out of three: tests/test_sdim_host.py) -- for the steps AND
    the candidates, in the 16- and 32-column kernels and all three row-load widths; a candidate that is a copy of a step
    carries that step's code word; and csrc/eta.hip, which shares the projection, scores a query that is a copy of a step
    at m against it and every other step as the fp32 evaluation does."""
    from explicit_tf2_recommendation_amd import ops
    B, T, Cn, E, Gn, m, S, D = DR.dims(case)
    c = DR.arithmetic_inputs(case)
    x = DR.keys_of(c["table"], c["series"])
    pk, pq = DR.projections_fp32(x, c["H"]), DR.projections_fp32(c["q"], c["H"])
    table, series, H = cu(c["table"]), cu(c["series"], np.int64), cu(c["H"])
    _, codes, qcodes, _ = ops.sdim_interest_fwd(table, series, cu(c["q"]), H, 0, "valid")
    codes, qcodes = host(codes), host(qcodes)
    same_bits("codes", codes, DR.pack(pk > 0))
    same_bits("qcodes", qcodes, DR.pack(pq > 0))
    assert np.array_equal(qcodes, codes[:, (7 * np.arange(S)) % T])
    scores = host(ops.eta_search_fwd(table, series, cu(c["q"][:, 0]), H.reshape(D, Gn * m).contiguous(), 0, 1)[0])
    want = (np.sign(pk) == np.sign(pq[:, :1])).sum(-1).astype(np.int32)
    same_bits("eta scores", scores, want)
    assert (scores[:, 0] == Gn * m).all()


def test_a_nan_row_follows_the_non_finite_rule_and_nothing_faults():
    case = (6, 63, 3, 16, 4, 4, 1)
    c = dict(DR.inputs(case))
    table, series, items = c["table"].copy(), c["series"].copy(), c["items"].copy()
    table[DR.NAN_ROW] = np.nan
    series[4, 3], series[5, 0], items[5] = DR.NAN_ROW, (3, DR.NAN_ROW, 4), DR.NAN_ROW   # a whole step, one column, a candidate
    q = DR.lookup(table, items).reshape(items.shape[0], items.shape[1], -1)
    for mode in DR.MODES:
        ref = DR.interest_numpy(table, series, q, c["H"], 0, mode)
        # a NaN projection gives bit 0: example 5's candidate and its step 0 have code 0 and share every bucket, whose
        # sums are NaN in the columns of the NaN row ('reference' mode multiplies the valid step by w = 0, and 0 NaN is
        # NaN) and read as 0, element by element
        assert ref["codes"][4, 3] == 0 and ref["codes"][5, 0] == 0 and ref["qcodes"][5, 0] == 0
        assert (ref["cnt"][5] > 0).all() and not ref["out"][5, :, 16:32].any() and np.isfinite(ref["out"]).all()
        assert ref["out"][5, :, :16].any() or mode == "reference"
        got = run(case, mode, table=cu(table), series=cu(series, np.int64), q=cu(q))
        check_exact(got[:4], ref, gkeys=False)
        assert tuple(got[4].shape) == tuple(c["series"].shape[:2]) + (48,)      # the backward ran; those elements are undefined


def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows():
    from explicit_tf2_recommendation_amd import ops
    case = (6, 64, 1, 48, 31, 1, 3)
    flag = ops.new_flag("cuda")
    run(case, "valid", oob=flag)
    assert int(flag.item()) == 0
    c = DR.inputs(case)
    series = c["series"].copy()
    series[3, 2, 0], series[4, 0, 0], series[5, 5, 0] = -1, DR.V_CASE, 2 ** 40
    for mode in DR.MODES:
        flag.zero_()
        ref = DR.interest_numpy(c["table"], series, c["q"], c["H"], 0, mode, c["gout"])
        check_exact(run(case, mode, series=cu(series, np.int64), oob=flag), ref)
        assert int(flag.item()) == 1
    case = DR.REFERENCE                                                      # in a column that is not the first
    c = DR.inputs(case)
    series = c["series"].copy()
    series[1, 4, 2] = DR.V_CASE + 5
    flag.zero_()
    ref = DR.interest_numpy(c["table"], series, c["q"], c["H"], 0, "reference", c["gout"])
    check_exact(run(case, "reference", series=cu(series, np.int64), oob=flag), ref)
    assert int(flag.item()) == 1


def test_strided_table_and_strided_candidates():
    for case in (DR.REFERENCE, (6, 63, 3, 16, 4, 4, 1), (6, 65, 3, 22, 4, 8, 2), (6, 64, 1, 48, 31, 1, 3)):
        d = dev(case)
        B, T, Cn, E, Gn, m, S, D = DR.dims(case)
        want = run(case, "valid")
        for extra in (3, 4, 16):                                                 # scalar loads, 16-byte loads
            wide = torch.full((d["table"].shape[0], E + extra), 7.0, device="cuda")
            wide[:, :E] = d["table"]
            view = wide[:, :E]
            assert view.stride(0) == E + extra
            for a, b in zip(want, run(case, "valid", table=view)):
                assert G.bit_equal(a, b)
            qw = torch.full((B, S, D + extra), 7.0, device="cuda")
            qw[:, :, :D] = d["q"]
            qv = qw[:, :, :D]
            assert not qv.is_contiguous()
            for a, b in zip(want, run(case, "valid", q=qv)):
                assert G.bit_equal(a, b)
    # one candidate per example: the rows of a wider gather, read in place
    case = DR.REFERENCE
    d = dev(case)
    rows = torch.full((3, 5, 48), 7.0, device="cuda")
    rows[:, 0] = d["q"][:, 0]
    for a, b in zip(run(case, "reference"), run(case, "reference", q=rows[:, :1])):
        assert G.bit_equal(a, b)


def test_two_runs_are_bit_identical():
    for case, kind in (((5, 257, 3, 85, 32, 1, 1), "exact"), (DR.RANDOM_CASES[0][0], "random"),
                       (DR.RANDOM_CASES[2][0], "random")):
        for a, b in zip(run(case, "reference", kind), run(case, "reference", kind)):
            assert G.bit_equal(a, b)


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    case = DR.REFERENCE
    d = dev(case)
    B, T, Cn, E, Gn, m, S, D = DR.dims(case)
    with pytest.raises(RuntimeError):
        ops.sdim_interest_fwd(d["table"].cpu(), d["series"], d["q"], d["H"], 0)                 # no CPU fallback
    with pytest.raises(TypeError):
        ops.sdim_interest_fwd(d["table"], d["series"].int(), d["q"], d["H"], 0)
    with pytest.raises(ValueError):
        ops.sdim_interest_fwd(d["table"], d["series"], d["q"][:, :, :-1].contiguous(), d["H"], 0)
    with pytest.raises(ValueError):
        ops.sdim_interest_fwd(d["table"], d["series"], d["q"], d["H"][:-1].contiguous(), 0)
    with pytest.raises(ValueError, match="mask_mode"):
        ops.sdim_interest_fwd(d["table"], d["series"], d["q"], d["H"], 0, "padded")
    z = lambda *s: torch.zeros(*s, device="cuda")
    zi = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError, match="<= 16"):
        ops.sdim_interest_fwd(z(10, 4), zi(2, 20, 1), z(2, 17, 4), z(4, 2, 3), 0)
    with pytest.raises(NotImplementedError, match="<= 32"):
        ops.sdim_interest_fwd(z(10, 4), zi(2, 20, 1), z(2, 1, 4), z(4, 3, 11), 0)
    out, codes, qcodes, cnt = ops.sdim_interest_fwd(d["table"], d["series"][:0], d["q"][:0], d["H"], 0)
    assert tuple(out.shape) == (0, S, D) and tuple(codes.shape) == (0, T) and tuple(cnt.shape) == (0, S, Gn)
    gkeys = ops.sdim_interest_bwd(d["series"][:0], E, m, 0, codes, qcodes, cnt, d["gout"][:0])
    assert tuple(gkeys.shape) == (0, T, D)


# ---- guards and poison under the family's allocations -------------------------------------------------------------------
@pytest.mark.parametrize("case", ((5, 1, 1, 2, 1, 1, 1), (6, 65, 3, 22, 4, 8, 2), (5, 257, 1, 64, 2, 8, 16),
                                  (5, 257, 3, 85, 32, 1, 1)), ids=ids)
def test_guards_and_poison(case):
    """nothing is written outside out, codes, qcodes, cnt and gkeys, and every element of them is written: the poisoned
    runs equal the oracle bit for bit (0xFF reads as -1 / NaN, 0x7F as 0x7F7F7F7F)"""
    from explicit_tf2_recommendation_amd import ops
    for mode in DR.MODES:
        ref = DR.reference(case, mode)
        for poison in (G.POISON_NAN, G.POISON_FINITE):
            flag = ops.new_flag("cuda")
            with G.guarded(ops, poison) as g:
                res = run(case, mode, ops=ops, oob=flag)
            assert len(g.allocations) == 5                                     # 4 outputs forward, gkeys backward
            check_exact(res, ref)
            assert int(flag.item()) == 0


# ---- the table's gradient -------------------------------------------------------------------------------------------------
def _dense(g):
    return host(g.coalesce().to_dense() if g.is_sparse else g)


@pytest.mark.parametrize("mode", DR.MODES)
@pytest.mark.parametrize("case", (DR.REFERENCE, (6, 63, 3, 16, 4, 4, 1), (6, 65, 3, 22, 4, 8, 2)), ids=ids)
def test_the_table_gradient_against_the_oracle_and_the_composed_path(case, mode):
    """gkeys is compared bit for bit above; here the SAME values go through the de-duplication, alone and through a
    GradSink shared with the Gather of the candidates, and must equal a Gather of the whole series fed the oracle's
    gkeys -- the composed path's hand-off -- bit for bit: one plan order, one sum order."""
    from explicit_tf2_recommendation_amd import functional as Fn
    d, c, ref = dev(case), DR.inputs(case), DR.reference(case, mode)
    B, T, Cn, E, Gn, m, S, D = DR.dims(case)
    # fused, alone
    table = d["table"].clone().requires_grad_(True)
    H = d["H"].clone().requires_grad_(True)
    out, codes, qcodes, cnt = Fn.SdimInterest.apply(table, d["q"], d["series"], H, 0, mode)
    assert not codes.requires_grad and not qcodes.requires_grad and not cnt.requires_grad
    (out * d["gout"]).sum().backward()
    assert table.grad.is_sparse and H.grad is None
    # composed: a gather of the whole series; the dense [B,T,D] gradient of the oracle goes back through it
    table2 = d["table"].clone().requires_grad_(True)
    x = Fn.Gather.apply(table2, d["series"], None).reshape(B, T, D)
    (x * cu(ref["gkeys"])).sum().backward()
    same_bits("fused against composed", _dense(table.grad), _dense(table2.grad))
    want = DR.dense_table_grad(c, ref["gkeys"])
    assert np.abs(_dense(table.grad) - want).max() <= 4 * T * B * DR.U * max(np.abs(want).max(), 1e-30)
    # through a GradSink shared with the Gather of the candidates: one plan, one sparse gradient
    table3 = d["table"].clone().requires_grad_(True)
    sink = Fn.GradSink(d["items"].numel())
    q = Fn.Gather.apply(table3, d["items"].reshape(B, S * Cn), None, sink).reshape(B, S, D)
    out3 = Fn.SdimInterest.apply(table3, q, d["series"], d["H"], 0, mode, None, sink)[0]
    gq = (d["gout"] * 2).contiguous()
    ((out3 * d["gout"]).sum() + (q * gq).sum()).backward()
    table4 = d["table"].clone().requires_grad_(True)
    both = Fn.Gather.apply(table4, torch.cat([d["items"].reshape(-1), d["series"].reshape(-1)]), None)
    (both * torch.cat([gq.reshape(-1, E), cu(ref["gkeys"]).reshape(-1, E)])).sum().backward()
    same_bits("sink", _dense(table3.grad), _dense(table4.grad))
    assert sink.ids is None and sink.buf is None
    # no gradient through out: nothing to do, nothing left in the sink
    table5 = d["table"].clone().requires_grad_(True)
    sink = Fn.GradSink(d["items"].numel())
    q = Fn.Gather.apply(table5, d["items"].reshape(B, S * Cn), None, sink).reshape(B, S, D)
    Fn.SdimInterest.apply(table5, q, d["series"], d["H"], 0, mode, None, sink)
    (q * gq).sum().backward()
    table6 = d["table"].clone().requires_grad_(True)
    (Fn.Gather.apply(table6, d["items"].reshape(-1), None) * gq.reshape(-1, E)).sum().backward()
    same_bits("items alone", _dense(table5.grad), _dense(table6.grad))


# ---- the layer ----------------------------------------------------------------------------------------------------------
def check(name, got, want, t32, floor):
    err, bound = DR.rel_err(got, want), max(floor, 4 * DR.rel_err(t32, want))
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


def _layer(seed, mask_mode, fused):
    from explicit_tf2_recommendation_amd import sdim
    sd = DR.layer_state(seed)
    lay = sdim.SDIMLayer(feature_dims=DR.LAYER_V, mask_mode=mask_mode, fused=fused).cuda()
    lay.load_state_dict({n: torch.from_numpy(v) for n, v in sd.items()})
    return lay, sd


def _grads(lay):
    out = {}
    for n, q in lay.named_parameters():
        out[n] = np.zeros(tuple(q.shape), F32) if q.grad is None else host(q.grad.to_dense() if q.grad.is_sparse else q.grad)
    return out


# T: the long series; Ns: the short one, on both sides of the attention kernel's 16 keys; S candidates; the item
# features' rank for S = 1
@pytest.mark.parametrize("mask_mode,T,Ns,S,rank", (("reference", 20, 5, 1, 1), ("valid", 20, 5, 1, 2),
                                                   ("reference", 6, 20, 3, None), ("valid", 70, 16, 1, 1),
                                                   ("valid", 9, 17, 1, 1), ("valid", 12, 3, 3, None)),
                         ids=lambda v: str(v))
def test_sdim_layer_fused_and_composed_against_the_transcription(mask_mode, T, Ns, S, rank):
    from explicit_tf2_recommendation_amd import data
    seed, B = 5, DR.LAYER_B
    ins = DR.layer_inputs(seed, B, T, Ns, S, item_rank=rank)
    sd = DR.layer_state(seed)
    keep = ~DR.layer_undecided(sd, ins, mask_mode)
    print("%d of %d examples left out" % ((~keep).sum(), B))
    assert keep.mean() >= 1 - DR.MAX_LEFT_OUT
    w = ins.pop("weight") * keep[:, None, None].astype(F32)
    t64, t32 = (DR.sdim_layer_torch(sd, ins, dt, mask_mode, w) for dt in (torch.float64, torch.float32))
    assert np.array_equal(t64["cnt"][keep], t32["cnt"][keep]) and t64["interest"][keep].any()
    batch = data.to_device(ins)
    names = set(batch)
    outs = {}
    for fused in (True, False):
        lay, _ = _layer(seed, mask_mode, fused)
        res = lay(batch)
        assert res.keys() == {"output"} and set(batch) == names and tuple(res["output"].shape) == (B, S, 1)
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
    assert DR.rel_err(outs[True][keep], outs[False][keep]) <= 1e-5


def test_out_of_range_id_raises():
    from explicit_tf2_recommendation_amd import data
    ins = DR.layer_inputs(1, DR.LAYER_B, 6, 4)
    ins.pop("weight")
    for fused in (True, False):
        lay, _ = _layer(1, "valid", fused)
        lay(data.to_device(ins))
        for name in ("longterm_shop_ids", "shortterm_cate_ids", "label_goods_ids", "utag2"):
            bad = {k: v.copy() for k, v in ins.items()}
            bad[name].reshape(-1)[5] = DR.LAYER_V
            with pytest.raises(IndexError):
                lay(data.to_device(bad))


def test_graphed_train_step_equals_eager():
    """Forward plus backward captured once and replayed over three batches against an eager copy of the layer: the loss
    and every gradient are equal bit for bit, and the table's gradient is ONE sparse tensor."""
    from explicit_tf2_recommendation_amd import data, engine, functional as Fn
    T, Ns, B = 40, 8, DR.LAYER_B
    lay, _ = _layer(2, "valid", True)
    eager = copy.deepcopy(lay)

    def batch_of(seed):
        ins = DR.layer_inputs(seed, B, T, Ns, 1, item_rank=1)
        ins.pop("weight")
        ins["label"] = np.random.default_rng(seed).integers(0, 2, B)
        return data.to_device(ins)

    batches = [batch_of(s) for s in (11, 12, 13)]
    step = engine.GraphedTrainStep(lay, batches[0], label_name="label",
                                   output_fn=lambda layer, ins: layer(ins)["output"].reshape(B, 1))
    for m in eager.modules():
        if hasattr(m, "check_ids"):
            m.check_ids = False
    for b in batches:
        loss = step(b)
        for q in eager.parameters():
            q.grad = None
        out = eager({k: v for k, v in b.items() if k != "label"})["output"]
        want = Fn.KerasBCE.apply(out.reshape(B, 1), b["label"].to(torch.float32).contiguous())
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
