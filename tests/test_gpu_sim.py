"""SIM on the GPU: the fused search and ESU attention kernels (csrc/sim.hip) against the fp64 numpy reading of
tests/sim_ref.py -- the search with and without a gradient through the selected rows, the attention under masks that are
all zero, all one and mixed -- bit identity run to run, a strided table, out-of-range ids, guards and poison under the
family's allocations, the error paths, the layers (SIMLayer fused and composed in both mask modes, ESULayer alone)
against the torch-CPU transcription, and one graphed train step with functional.sim_loss.

Tolerance, per tensor (the project's rule, as tests/test_gpu_dien.py states it): max|got - want| / max|want| against fp64
must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors) /
3e-5 (gradients); a tensor that is zero throughout in fp64 must be exactly zero.  Every test prints `name error / bound`.
chosen and sel_valid must equal the fp64 reading exactly, for every case and every row.  dbk -- zero in exact arithmetic,
rounding residue in every implementation -- is normalised by max|dbq| instead of its own maximum, against 4 x the
transcription's same ratio with the 3e-5 floor.

Measured on the MI355X, the printout as a DIGEST (651 `error / bound` lines in all).  49 passed in 4.3 s.  641 of the 651
bounds sit on their floor: the fp32 CPU transcription is that close to fp64 itself on these inputs.
  search (6 cases, with and without gsel): chosen and sel_valid equal in every row; largest ratio pooled 4.12e-07 /
      1.00e-05, gq 8.48e-07 / 3.00e-05; sel is a bit-exact copy of the rows
  attention (6 cases x 4 masks): largest ratio dbq 5.42e-07 / 3.00e-05; the all-masked rows give p = 1/K exactly
  layers, T = 6 in both mask modes and T = 20: largest ratio fused gsu_layer.mlp.layers.6.dense.bias 2.50e-06 / 3.00e-05,
      composed the same tensor 4.75e-06 / 3.00e-05
  guards and poison: 43 allocations per case, 2.7 KB (1x1x1x4x3x1) to 2.6 MB (65x9x1x64x4x2) through the seam
"""
import copy

import numpy as np
import pytest
import torch

from tests import dien_ref as DR
from tests import guarded as G
from tests import sim_ref as SR

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = lambda c: "x".join(map(str, c))
CASES = list(SR.CASES)


def cu(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(name, got, want, t32, floor):
    err, bound = SR.rel_err(got, want), max(floor, 4 * SR.rel_err(t32, want))
    print("%-22s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


def check_dbk(name, got, want, t32, dbq):
    """dbk by the scale of dbq: its own maximum is rounding residue"""
    scale = np.abs(dbq).max() or 1.0                          # K = 1: no logit gets a gradient, dbq = 0 and dbk = 0 exactly
    err, bound = np.abs(got - want).max() / scale, max(3e-5, 4 * np.abs(t32 - want).max() / scale)
    print("%-22s error/bound %.2e / %.2e = %.2f (by max|dbq|)" % (name, err, bound, err / bound))
    assert got.shape == want.shape and err <= bound, (name, err, bound)


# ---- bodies -------------------------------------------------------------------------------------------------------------
_DEV = {}


def dev(case):
    if case not in _DEV:
        c = SR.inputs(case)
        d = {k: cu(c[k]) for k in ("table", "q", "gpooled", "gsel", "gout", "sel")}
        d["series"] = cu(c["series"], np.int64)
        d["w"] = tuple(cu(c["w"][n]) for n in SR.WEIGHTS)
        d["masks"] = {m: cu(v, np.int32) for m, v in c["masks"].items()}
        _DEV[case] = d
    return _DEV[case]


def run_search(case, with_gsel=True, table=None, series=None, oob=None, ops=None):
    """-> scores, pooled, sel, gkeys, gq (SR.SEARCH_OUT + SR.SEARCH_GRADS), then chosen, sel_valid"""
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    d = dev(case)
    tab = d["table"] if table is None else table
    ser = d["series"] if series is None else series
    K = SR.dims(case)[4]
    scores, pooled, chosen, sel, sel_valid = ops.sim_search_fwd(tab, ser, d["q"], 0, K, oob)
    gkeys, gq = ops.sim_search_bwd(tab, ser, d["q"], 0, scores, d["gpooled"], chosen, d["gsel"] if with_gsel else None)
    return scores, pooled, sel, gkeys, gq, chosen, sel_valid


def run_attn(case, mask, ops=None):
    """-> out, probs, then the ten gradients (SR.ATTN_OUT + SR.ATTN_GRADS)"""
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    d = dev(case)
    out, probs = ops.esu_attn_fwd(d["q"], d["sel"], d["masks"][mask], d["w"], want_probs=True)
    return (out, probs) + ops.esu_attn_bwd(d["q"], d["sel"], d["masks"][mask], d["w"], d["gout"])


@pytest.mark.parametrize("with_gsel", (True, False), ids=("gsel", "nogsel"))
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_search_matches_fp64(case, with_gsel):
    got = run_search(case, with_gsel)
    ref, t32 = SR.cached(SR.search_numpy, case, with_gsel), SR.cached(SR.search_torch, case, with_gsel)
    assert np.array_equal(host(got[5]), ref["chosen"])                         # every row, exactly
    assert np.array_equal(host(got[6]) != 0, ref["sel_valid"])
    assert got[5].dtype == torch.int32 and got[6].dtype == torch.int32
    for name, t in zip(SR.SEARCH_OUT + SR.SEARCH_GRADS, got):
        check(name, host(t), ref[name], t32[name], 1e-5 if name in SR.SEARCH_OUT else 3e-5)
    c = SR.inputs(case)
    assert not host(got[0])[~c["valid"]].any()                               # a padded step scores exactly zero
    sel = host(got[2])
    rows = np.arange(len(sel))[:, None]
    assert np.array_equal(sel, c["x"].astype(F32)[rows, ref["chosen"]])      # the selected rows are copies, padded ones too
    if not with_gsel:                                                        # nothing reaches a padded step then
        assert not host(got[3])[~c["valid"]].any()


@pytest.mark.parametrize("mask", ("zeros", "ones", "mixed", "search"))
@pytest.mark.parametrize("case", CASES, ids=ids)
def test_attention_matches_fp64(case, mask):
    got = run_attn(case, mask)
    ref, t32 = SR.cached(SR.attention_numpy, case, mask), SR.cached(SR.attention_torch, case, mask)
    for name, t in zip(SR.ATTN_OUT + SR.ATTN_GRADS, got):
        if name == "dbk":
            check_dbk(name, host(t), ref[name], t32[name], ref["dbq"])
        else:
            check(name, host(t), ref[name], t32[name], 1e-5 if name in SR.ATTN_OUT else 3e-5)
    assert all(bool(torch.isfinite(t).all()) for t in got)
    if mask == "zeros":                                                      # -1e9 exactly: the uniform attention
        K = SR.dims(case)[4]
        assert torch.equal(got[1], torch.full_like(got[1], 1.0) / K)


def test_every_output_is_bit_identical_run_to_run():
    for case in (SR.RAGGED, SR.LONG):
        for a, b in zip(run_search(case), run_search(case)):
            assert torch.equal(a, b)
        for a, b in zip(run_attn(case, "mixed"), run_attn(case, "mixed")):
            assert torch.equal(a, b)


def test_strided_table_is_bit_identical_to_the_packed_one():
    case = SR.DEFAULTS
    table = dev(case)["table"]
    wide = torch.full((table.shape[0], table.shape[1] + 3), 7.0, device="cuda")
    wide[:, :table.shape[1]] = table
    view = wide[:, :table.shape[1]]
    assert view.stride(0) == table.shape[1] + 3
    for a, b in zip(run_search(case), run_search(case, table=view)):
        assert torch.equal(a, b)


def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows():
    from explicit_tf2_recommendation_amd import ops
    case = SR.DEFAULTS
    c = SR.inputs(case)
    flag = ops.new_flag("cuda")
    run_search(case, oob=flag)
    assert int(flag.item()) == 0
    series = c["series"].copy()
    series[3, 2, 1], series[8, 0, 0], series[4, 5, 2] = -1, SR.V_CASE, 2 ** 40    # (a first-feature id too: not padding)
    bad = dict(c)
    bad.update(series=series, valid=series[:, :, 0] != 0, x=SR.lookup(c["table"], series))
    ref = SR.search_numpy(bad, c["gpooled"], c["gsel"])
    t32 = SR.search_torch(bad, torch.float32, c["gpooled"], c["gsel"])
    got = run_search(case, series=cu(series, np.int64), oob=flag)
    assert int(flag.item()) == 1
    assert np.array_equal(host(got[5]), ref["chosen"]) and np.array_equal(host(got[6]) != 0, ref["sel_valid"])
    for name, t in zip(SR.SEARCH_OUT + SR.SEARCH_GRADS, got):
        check(name, host(t), ref[name], t32[name], 1e-5 if name in SR.SEARCH_OUT else 3e-5)


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    case = SR.DEFAULTS
    d = dev(case)
    B, T, Cn, E, K, H, D = SR.dims(case)
    with pytest.raises(RuntimeError):
        ops.sim_search_fwd(d["table"].cpu(), d["series"], d["q"], 0, K)       # no CPU fallback
    with pytest.raises(TypeError):
        ops.sim_search_fwd(d["table"], d["series"].int(), d["q"], 0, K)
    with pytest.raises(ValueError):
        ops.sim_search_fwd(d["table"], d["series"], d["q"][:, :-1].contiguous(), 0, K)
    with pytest.raises(ValueError):
        ops.sim_search_fwd(d["table"], d["series"], d["q"], 0, T + 1)
    with pytest.raises(ValueError):
        ops.esu_attn_fwd(d["q"], d["sel"], d["masks"]["ones"][:, :-1].contiguous(), d["w"])
    with pytest.raises(TypeError):
        ops.esu_attn_fwd(d["q"], d["sel"], d["masks"]["ones"].long(), d["w"])
    z = lambda *s: torch.zeros(*s, device="cuda")
    zi = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError, match="<= 16"):
        ops.sim_search_fwd(z(10, 4), zi(2, 20, 1), z(2, 4), 0, 17)
    with pytest.raises(NotImplementedError, match="<= 64"):
        ops.esu_attn_fwd(z(2, 66), z(2, 3, 66), torch.ones(2, 3, dtype=torch.int32, device="cuda"),
                         (z(66, 2, 66), z(2, 66), z(66, 2, 66), z(2, 66), z(66, 2, 66), z(2, 66), z(2, 66, 66), z(66)))
    scores, pooled, chosen, sel, sel_valid = ops.sim_search_fwd(d["table"], d["series"][:0], d["q"][:0], 0, K)
    assert tuple(sel.shape) == (0, K, D) and tuple(chosen.shape) == (0, K) and tuple(scores.shape) == (0, T)
    gkeys, gq = ops.sim_search_bwd(d["table"], d["series"][:0], d["q"][:0], 0, scores, d["gpooled"][:0], chosen)
    assert tuple(gkeys.shape) == (0, T, D) and tuple(gq.shape) == (0, D)
    out, _ = ops.esu_attn_fwd(d["q"][:0], d["sel"][:0], d["masks"]["ones"][:0], d["w"])
    res = ops.esu_attn_bwd(d["q"][:0], d["sel"][:0], d["masks"]["ones"][:0], d["w"], d["gout"][:0])
    assert tuple(out.shape) == (0, D) and [tuple(t.shape) for t in res[2:]] == [tuple(t.shape) for t in d["w"]]
    assert all(not t.any() for t in res)


# ---- guards and poison under the family's allocations -------------------------------------------------------------------
def body_driver(ops, case):
    flag = ops.new_flag("cuda")
    return (flag,) + run_search(case, oob=flag, ops=ops) + run_search(case, False, ops=ops) \
        + run_attn(case, "mixed", ops=ops) + run_attn(case, "zeros", ops=ops)


@pytest.mark.parametrize("case", (SR.SMALLEST, SR.RAGGED), ids=ids)
def test_guards_and_poison(case):
    from explicit_tf2_recommendation_amd import ops
    want = G.flatten(body_driver(ops, case))
    with G.guarded(ops, G.POISON_NAN) as g:
        nan_run = G.flatten(body_driver(ops, case))
    print("%s: %d allocations, %d bytes through the seam" % (ids(case), len(g.allocations), g.total_bytes()))
    assert len(g.allocations) >= 40
    for i, t in enumerate(nan_run):
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), "returned tensor %d %s holds poison or a non-finite value" % (i, tuple(t.shape))
    for what, a, b in (("0xFF poison against the plain run", nan_run, want),):
        assert len(a) == len(b)
        for i, (p, q) in enumerate(zip(a, b)):
            assert G.bit_equal(p, q), "%s: returned tensor %d %s differs" % (what, i, tuple(p.shape))
    with G.guarded(ops, G.POISON_FINITE):
        fin_run = G.flatten(body_driver(ops, case))
    for i, (p, q) in enumerate(zip(fin_run, nan_run)):
        assert G.bit_equal(p, q), "0x7F poison against 0xFF poison: returned tensor %d %s differs" % (i, tuple(p.shape))


# ---- the layers ----------------------------------------------------------------------------------------------------------
def _tensors(sd):
    return {k: torch.from_numpy(np.asarray(v, F32)) for k, v in sd.items()}


def _dien():
    from explicit_tf2_recommendation_amd import layers
    return layers.DIENLayer(feature_dims=DR.LAYER_V, activation="PReLU", mask_mode="valid", stage="inference")


def _sim_layer(seed, mask_mode, fused=True):
    from explicit_tf2_recommendation_amd import layers
    sd = SR.layer_state(seed, SR.sim_state_shapes())
    lay = layers.SIMLayer(feature_dims=DR.LAYER_V, activation="PReLU", mask_mode=mask_mode, fused=fused,
                          dien_layer=_dien()).cuda()
    lay.load_state_dict(_tensors(sd))
    return lay, sd


def _grads(lay):
    out = {}
    for k, q in lay.named_parameters():
        if q.requires_grad:
            out[k] = np.zeros(tuple(q.shape), F32) if q.grad is None else host(q.grad.to_dense() if q.grad.is_sparse else q.grad)
    return out


def check_grads(tag, grads, g64, g32):
    """every parameter by the rule; the key bias by the scale of the query bias' gradient, as dbk"""
    for k in grads:
        if k.endswith("_key_dense.bias"):
            check_dbk(tag + k, grads[k], g64[k], g32[k], g64[k.replace("_key_dense", "_query_dense")])
        else:
            check(tag + k, grads[k], g64[k], g32[k], 3e-5)


@pytest.mark.parametrize("mask_mode,T", (("reference", 6), ("valid", 6), ("valid", 20)), ids=lambda v: str(v))
def test_sim_layer_fused_and_composed_against_the_transcription(mask_mode, T):
    from explicit_tf2_recommendation_amd import data
    seed = 5
    ins = SR.layer_inputs(seed, DR.LAYER_B, T)
    sd = SR.layer_state(seed, SR.sim_state_shapes())
    t64, t32 = (SR.sim_layer_torch(sd, ins, dt, mask_mode) for dt in (torch.float64, torch.float32))
    assert np.array_equal(t64["chosen"], t32["chosen"])
    batch = data.to_device(ins)
    weight = batch.pop("weight")
    keys = set(batch)
    results = {}
    for fused in (True, False):
        lay, _ = _sim_layer(seed, mask_mode, fused)
        res = lay(batch)
        assert res.keys() == {"gsu_logits", "esu_logits"} and set(batch) == keys          # the caller's dict is untouched
        tag = "fused " if fused else "composed "
        for k in ("gsu_logits", "esu_logits"):
            assert tuple(res[k].shape) == (DR.LAYER_B, 2)
            check(tag + k, host(res[k]), t64[k], t32[k], 1e-5)
        (torch.cat([res["gsu_logits"], res["esu_logits"]], 1) * weight).sum().backward()
        grads = _grads(lay)
        assert grads.keys() == t64["grads"].keys()
        check_grads(tag, grads, t64["grads"], t32["grads"])
        assert all(q.grad is None for q in lay.esu_layer.dien_layer.parameters())
        results[fused] = (res, grads)
    for k in ("gsu_logits", "esu_logits"):                                   # fused against composed, directly
        assert SR.rel_err(host(results[True][0][k]), host(results[False][0][k])) <= 1e-5


@pytest.mark.parametrize("mask_mode", ("reference", "valid"))
def test_esu_layer_alone_with_given_extracted_series(mask_mode):
    from explicit_tf2_recommendation_amd import data, layers
    seed, T, K = 6, 6, 3
    ins = SR.layer_inputs(seed, DR.LAYER_B, T)
    rng = np.random.default_rng(seed)
    extracted = (rng.standard_normal((DR.LAYER_B, K, DR.LAYER_H)) * 0.3).astype(F32)
    series_mask = rng.random((DR.LAYER_B, K)) < 0.4
    series_mask[0], series_mask[1] = True, False                             # everything / nothing padded
    sd = SR.layer_state(seed, SR.esu_state_shapes())
    t64, t32 = (SR.esu_layer_torch(sd, ins, extracted, series_mask, dt, mask_mode) for dt in (torch.float64, torch.float32))
    batch = data.to_device(ins)
    weight = batch.pop("weight")[:, :2]
    batch["extracted_series"], batch["series_mask"] = cu(extracted), torch.from_numpy(series_mask).cuda()
    for fused in (True, False):
        lay = layers.ESULayer(feature_dims=DR.LAYER_V, activation="PReLU", dien_layer=_dien(), mask_mode=mask_mode,
                              fused=fused).cuda()
        lay.load_state_dict(_tensors(sd))
        res = lay(batch)
        assert res.keys() == {"output"}
        tag = "fused " if fused else "composed "
        check(tag + "output", host(res["output"]), t64["output"], t32["output"], 1e-5)
        (res["output"] * weight).sum().backward()
        grads = _grads(lay)
        assert grads.keys() == t64["grads"].keys()
        check_grads(tag, grads, t64["grads"], t32["grads"])


def test_out_of_range_id_raises():
    from explicit_tf2_recommendation_amd import data
    lay, _ = _sim_layer(1, "valid")
    ins = SR.layer_inputs(1, DR.LAYER_B, 6)
    ins.pop("weight")
    lay(data.to_device(ins))
    for name in ("visited_shop_ids", "i_shop_id"):
        bad = {k: v.copy() for k, v in ins.items()}
        bad[name].reshape(-1)[5] = DR.LAYER_V
        with pytest.raises(IndexError):
            lay(data.to_device(bad))


def test_graphed_train_step_with_sim_loss_equals_eager():
    """Forward plus backward captured once and replayed over three batches against an eager copy of the layer, with the
    usage INTEGRATION.md shows: the loss and every gradient are equal bit for bit, the frozen DIEN gets no gradient and
    the table's gradient is ONE sparse tensor (item and series lookups de-duplicated together)."""
    from explicit_tf2_recommendation_amd import data, engine, functional as Fn
    T, B = 6, DR.LAYER_B
    lay, _ = _sim_layer(2, "valid")
    eager = copy.deepcopy(lay)
    output_fn = lambda l, x: torch.cat(list(l(x).values()), 1)
    loss_fn = lambda out, y: Fn.sim_loss(out[:, :2], out[:, 2:], y[:, 0])

    def batch_of(seed):
        ins = SR.layer_inputs(seed, B, T)
        ins.pop("weight")
        ins["label"] = np.random.default_rng(seed).integers(0, 2, B)
        return data.to_device(ins)

    batches = [batch_of(s) for s in (11, 12, 13)]
    step = engine.GraphedTrainStep(lay, batches[0], label_name="label", output_fn=output_fn, loss_fn=loss_fn)
    for m in eager.modules():
        if hasattr(m, "check_ids"):
            m.check_ids = False
    frozen = {id(q) for q in lay.esu_layer.dien_layer.parameters()}
    for b in batches:
        loss = step(b)
        for q in eager.parameters():
            q.grad = None
        res = eager({k: v for k, v in b.items() if k != "label"})
        want = Fn.sim_loss(res["gsu_logits"], res["esu_logits"], b["label"].to(torch.float32))
        want.backward()
        assert torch.equal(loss.reshape(()), want.detach().reshape(()))
        for (name, a), q in zip(lay.named_parameters(), eager.parameters()):
            if id(a) in frozen:
                assert a.grad is None and q.grad is None, name
                continue
            assert a.grad is not None and q.grad is not None and a.grad.is_sparse == q.grad.is_sparse, name
            if a.grad.is_sparse:
                assert name == "embed.embeddings"
                assert torch.equal(a.grad._indices(), q.grad._indices()), name
                assert torch.equal(a.grad._values(), q.grad._values()), name
            else:
                assert torch.equal(a.grad, q.grad), name
