"""DIEN on the GPU: the fused GRU / AUGRU sequence kernels (csrc/dien.hip) against the fp64 numpy reading of
tests/dien_ref.py -- the extractor with the series and negative lookups and the auxiliary loss, the evolution with both
values of mask_valid in AGRU and AUGRU, the dense-input mode -- bit identity run to run, a strided table, out-of-range
ids, guards and poison under the family's allocations, the error codes, the layer (fused and composed, three modes, both
mask modes) against the torch-CPU transcription, and one graphed train step with the auxiliary loss.

Tolerance, per tensor (the project's rule, as tests/test_gpu_dmr.py states it): max|got - want| / max|want| against fp64
must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors) /
3e-5 (gradients); a tensor that is zero throughout in fp64 must be exactly zero.  Every test prints `name error / bound`.
The bound compounds over T through the transcription's own error, which is measured, not chosen.

Measured on the MI355X, the printout as a DIGEST (685 `error / bound` lines in all).  68 passed in 6.7 s.  Every bound sits
on its floor, the T = 100 cases included: the fp32 CPU transcription is that close to fp64 itself on these inputs.
  bodies (extractor, auxiliary loss alone, AGRU / AUGRU x mask_valid, dense mode; 7 cases each): largest ratio
      gru_output 4.64e-07 / 1.00e-05; every gradient below 1.3e-06 / 3.00e-05
  layer, fused and composed, 3 modes x 2 mask modes at T = 6 and AUGRU 'valid' at T = 20: largest ratio
      composed mlp.layers.6.dense.bias 6.20e-06 / 3.00e-05, fused 6.01e-06 / 3.00e-05; output 4.52e-07 / 1.00e-05
  guards and poison: 35 allocations per case, 1.4 KB (1x1x1x1) to 79.7 MB (2049x6x3x16) through the seam
"""
import copy
import ctypes as C

import numpy as np
import pytest
import torch

from tests import dien_ref as DR
from tests import guarded as G

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = lambda c: "x".join(map(str, c))
EVO_KINDS = ("AUGRU", "AGRU")


def cu(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(name, got, want, t32, floor):
    err, bound = DR.rel_err(got, want), max(floor, 4 * DR.rel_err(t32, want))
    print("%-22s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


# ---- bodies -------------------------------------------------------------------------------------------------------------
_DEV = {}
FLOATS = ("table", "kernel", "recurrent_kernel", "bias", "q", "dgru_output", "dh_final", "gaux", "g")


def dev(case):
    if case not in _DEV:
        c = DR.inputs(case)
        d = {k: cu(c[k]) for k in FLOATS}
        d.update(series=cu(c["series"], np.int64), negatives=cu(c["negatives"], np.int64))
        for kind in EVO_KINDS:
            d[kind] = [cu(v) for v in DR.evo_weights(c, kind)]
        _DEV[case] = d
    return _DEV[case]


def run_gru(case, table=None, series=None, negatives=None, oob=None, ops=None, main=True, aux=True):
    """-> gru_output, aux, dx, dneg, dkernel, drecurrent_kernel, dbias in the order of DR.GRU_OUT + DR.GRU_GRADS"""
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    d = dev(case)
    tab = d["table"] if table is None else table
    ser = d["series"] if series is None else series
    neg = d["negatives"] if negatives is None else negatives
    w = (d["kernel"], d["recurrent_kernel"], d["bias"])
    out, _, loss = ops.dien_gru_fwd(*w, embed=tab, series=ser, negatives=neg, oob=oob)
    grads = ops.dien_gru_bwd(*w, out, d["dgru_output"] if main else None, None, d["gaux"] if aux else None, embed=tab,
                             series=ser, negatives=neg)
    return (out, loss) + tuple(grads)


def run_evo(case, kind, mask_valid, ops=None):
    """-> scores, h_final, dgru_output, dq, dWx, dUh, dbx (DR.EVO_OUT + DR.EVO_GRADS), then the saved states"""
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    d = dev(case)
    args = (d["g"], d["q"], d["series"], ops.DIEN_MODE[kind], *d[kind])
    scores, states, fin = ops.dien_augru_fwd(*args, 0, mask_valid)
    grads = ops.dien_augru_bwd(*args, scores, states, d["dh_final"], 0, mask_valid)
    return (scores, fin) + tuple(grads) + (states,)


def run_dense(case, ops=None):
    """-> h_final, dx, dkernel, drecurrent_kernel, dbias (DR.DENSE_OUT + DR.DENSE_GRADS), then the saved states"""
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    d = dev(case)
    w = (d["kernel"], d["recurrent_kernel"], d["bias"])
    mask = d["series"][:, :, 0].contiguous()
    states, fin, _ = ops.dien_gru_fwd(*w, x=d["g"], mask_ids=mask, want_final=True)
    dx, _, dK, dU, db = ops.dien_gru_bwd(*w, states, None, d["dh_final"], None, x=d["g"], mask_ids=mask)
    return fin, dx, dK, dU, db, states


def check_named(names, outs, got, ref, t32, tag=""):
    for name, t in zip(names, got):
        check(tag + name, host(t), ref[name], t32[name], 1e-5 if name in outs else 3e-5)


@pytest.mark.parametrize("case", DR.CASES, ids=ids)
def test_extractor_matches_fp64(case):
    got = run_gru(case)
    check_named(DR.GRU_OUT + DR.GRU_GRADS, DR.GRU_OUT, got, DR.cached(DR.extractor_numpy, case),
                DR.cached(DR.extractor_torch, case))
    valid = DR.inputs(case)["valid"]
    out = host(got[0])
    allpad = ~valid.any(1)
    assert not out[allpad].any()                                             # an all-padded row outputs zeros throughout
    assert not host(got[3])[:, 0].any()                                      # no negative is scored at position 0


@pytest.mark.parametrize("case", [(1, 1, 1, 1), DR.MASKED, (5, 100, 3, 32)], ids=ids)
def test_auxiliary_loss_and_its_gradients_alone(case):
    c = DR.inputs(case)
    got = run_gru(case, main=False)
    ref, t32 = DR.extractor_numpy(c, None, c["gaux"]), DR.extractor_torch(c, torch.float32, None, c["gaux"])
    check_named(DR.GRU_OUT + DR.GRU_GRADS, DR.GRU_OUT, got, ref, t32)
    if case[1] == 1:
        assert float(got[1]) == 0.0 and all(not g.any() for g in got[2:])     # T = 1: no pair to score


def test_an_absent_upstream_equals_zeros_bit_for_bit():
    from explicit_tf2_recommendation_amd import ops
    case = DR.MASKED
    d = dev(case)
    w = (d["kernel"], d["recurrent_kernel"], d["bias"])
    kw = dict(embed=d["table"], series=d["series"], negatives=d["negatives"])
    out = ops.dien_gru_fwd(*w, **kw)[0]
    z = torch.zeros_like
    for a, b in ((ops.dien_gru_bwd(*w, out, None, None, d["gaux"], **kw),
                  ops.dien_gru_bwd(*w, out, z(d["dgru_output"]), z(d["dh_final"]), d["gaux"], **kw)),
                 (ops.dien_gru_bwd(*w, out, d["dgru_output"], None, None, **kw),
                  ops.dien_gru_bwd(*w, out, d["dgru_output"], None, z(d["gaux"]), **kw))):
        for p, q in zip(a, b):
            assert torch.equal(p, q)


@pytest.mark.parametrize("mask_valid", (0, 1))
@pytest.mark.parametrize("kind", EVO_KINDS)
@pytest.mark.parametrize("case", DR.CASES, ids=ids)
def test_evolution_matches_fp64(case, kind, mask_valid):
    got = run_evo(case, kind, mask_valid)
    ref = DR.cached(DR.evolution_numpy, case, kind, mask_valid)
    check_named(DR.EVO_OUT + DR.EVO_GRADS, DR.EVO_OUT, got[:-1], ref, DR.cached(DR.evolution_torch, case, kind, mask_valid))
    assert torch.equal(got[-1][:, -1], got[1])                               # the saved states end in the final state
    if mask_valid == 0:                                                      # the reference's convention
        assert not got[1].any() and all(not g.any() for g in got[2:7])
    valid = DR.inputs(case)["valid"]
    nothing = valid.all(1) if mask_valid == 0 else ~valid.any(1)
    assert not host(got[0])[nothing].any() and not host(got[3])[nothing].any()
    assert all(bool(torch.isfinite(g).all()) for g in got)


@pytest.mark.parametrize("case", DR.CASES, ids=ids)
def test_dense_input_mode_matches_fp64(case):
    c = DR.inputs(case)
    got = run_dense(case)
    ref, t32 = DR.dense_numpy(c, c["dh_final"]), DR.dense_torch(c, torch.float32, c["dh_final"])
    check_named(DR.DENSE_OUT + DR.DENSE_GRADS, DR.DENSE_OUT, got[:-1], ref, t32)
    check("states", host(got[-1]), ref["states"], t32["states"], 1e-5)
    from explicit_tf2_recommendation_amd import ops
    d = dev(case)
    only = ops.dien_gru_fwd(d["kernel"], d["recurrent_kernel"], d["bias"], x=d["g"],
                            mask_ids=d["series"][:, :, 0].contiguous(), want_output=False, want_final=True)
    assert only[0] is None and torch.equal(only[1], got[0])                   # the final state alone


def test_every_output_is_bit_identical_run_to_run():
    for a, b in zip(run_gru(DR.LARGEST), run_gru(DR.LARGEST)):
        assert torch.equal(a, b)
    for kind in EVO_KINDS:
        for a, b in zip(run_evo(DR.LARGEST, kind, 1), run_evo(DR.LARGEST, kind, 1)):
            assert torch.equal(a, b)
    for a, b in zip(run_dense(DR.LARGEST), run_dense(DR.LARGEST)):
        assert torch.equal(a, b)


def _strided(table, pad=3):
    wide = torch.full((table.shape[0], table.shape[1] + pad), 7.0, device="cuda")
    wide[:, :table.shape[1]] = table
    view = wide[:, :table.shape[1]]
    assert view.stride(0) == table.shape[1] + pad
    return view


def test_strided_table_is_bit_identical_to_the_packed_one():
    case = (33, 7, 3, 5)
    for a, b in zip(run_gru(case), run_gru(case, table=_strided(dev(case)["table"]))):
        assert torch.equal(a, b)


def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows():
    from explicit_tf2_recommendation_amd import ops
    case = DR.MASKED
    c = DR.inputs(case)
    flag = ops.new_flag("cuda")
    run_gru(case, oob=flag)
    assert int(flag.item()) == 0
    series, negatives = c["series"].copy(), c["negatives"].copy()
    series[5, 2, 1], series[7, 0, 0], series[4, 5, 2] = -1, DR.V_CASE, 2 ** 40    # (a first-feature id too: not padding)
    negatives[4, 3, 0], negatives[6, 1, 2] = DR.V_CASE + 5, -7
    for ser, neg in ((series, None), (None, negatives)):                      # either lookup alone sets it
        flag = ops.new_flag("cuda")
        run_gru(case, series=cu(ser, np.int64), negatives=cu(neg, np.int64), oob=flag)
        assert int(flag.item()) == 1
    bad = dict(c)
    bad.update(series=series, negatives=negatives, valid=series[:, :, 0] != 0, x=DR.lookup(c["table"], series),
               xn=DR.lookup(c["table"], negatives))
    ref = DR.extractor_numpy(bad, c["dgru_output"], c["gaux"])
    t32 = DR.extractor_torch(bad, torch.float32, c["dgru_output"], c["gaux"])
    got = run_gru(case, series=cu(series, np.int64), negatives=cu(negatives, np.int64), oob=flag)
    check_named(DR.GRU_OUT + DR.GRU_GRADS, DR.GRU_OUT, got, ref, t32)


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    case = (3, 5, 1, 8)
    d = dev(case)
    w = (d["kernel"], d["recurrent_kernel"], d["bias"])
    tab, ser, neg = d["table"], d["series"], d["negatives"]
    with pytest.raises(RuntimeError):
        ops.dien_gru_fwd(*w, embed=tab.cpu(), series=ser)                    # no CPU fallback
    with pytest.raises(TypeError):
        ops.dien_gru_fwd(*w, embed=tab, series=ser.int())
    with pytest.raises(ValueError):
        ops.dien_gru_fwd(*w, embed=tab, series=ser, negatives=neg[:, :4].contiguous())
    with pytest.raises(ValueError):
        ops.dien_gru_fwd(w[0][:, :-1].contiguous(), w[1], w[2], embed=tab, series=ser)
    with pytest.raises(ValueError):
        ops.dien_gru_fwd(*w, embed=tab, series=ser, x=d["g"])
    with pytest.raises(ValueError):
        ops.dien_augru_fwd(d["g"], d["q"][:, :-1].contiguous(), ser, ops.DIEN_AUGRU, *d["AUGRU"])
    with pytest.raises(ValueError):
        ops.dien_augru_fwd(d["g"], d["q"], ser, ops.DIEN_AGRU, *d["AUGRU"])    # the AUGRU's packed weights
    z = lambda *s: torch.zeros(*s, device="cuda")
    zi = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
    with pytest.raises(NotImplementedError, match="<= 128"):
        ops.dien_gru_fwd(z(129, 387), z(129, 387), z(2, 387), embed=z(10, 43), series=zi(2, 4, 3))
    with pytest.raises(NotImplementedError, match="tile of 32 examples"):
        ops.dien_augru_fwd(z(1, 132, 128), z(1, 128), zi(1, 132), ops.DIEN_AUGRU, z(128, 384), z(128, 384), z(384))
    out, fin, aux = ops.dien_gru_fwd(*w, embed=tab, series=ser[:0], negatives=neg[:0])
    assert tuple(out.shape) == (0, 5, 8) and fin is None and float(aux) == 0.0
    res = ops.dien_gru_bwd(*w, out, None, None, d["gaux"], embed=tab, series=ser[:0], negatives=neg[:0])
    assert [tuple(t.shape) for t in res] == [(0, 5, 8), (0, 5, 8), (8, 24), (8, 24), (2, 24)]
    assert all(not t.any() for t in res)
    scores, states, fin = ops.dien_augru_fwd(d["g"][:0], d["q"][:0], ser[:0], ops.DIEN_AUGRU, *d["AUGRU"])
    assert tuple(scores.shape) == (0, 5) and tuple(fin.shape) == (0, 8)


def test_error_codes_on_the_device():
    """H = 129: -2; a negative size: -1; a NULL pointer: -1 -- with real device pointers everywhere else."""
    from explicit_tf2_recommendation_amd._lib import lib
    d = dev((3, 5, 1, 8))
    p = lambda t: C.c_void_p(t.data_ptr())
    out, fin = torch.empty(3, 5, 8, device="cuda"), torch.empty(3, 8, device="cuda")

    def gru(B=3, T=5, H=8, E=8, kernel=p(d["kernel"]), out=p(out)):
        return lib.rec_dien_gru_fwd_f32(p(d["table"]), 8, DR.V_CASE, E, 1, p(d["series"]), None, None, None, B, T, H, kernel,
                                        p(d["recurrent_kernel"]), p(d["bias"]), 0, out, None, None, None, None, 0, None)

    def evo(B=3, T=5, H=8, q=p(d["q"])):
        return lib.rec_dien_augru_fwd_f32(p(d["g"]), q, p(d["series"]), 1, B, T, H, 1, *[p(t) for t in d["AUGRU"]], 0, 1,
                                          p(torch.empty(3, 5, device="cuda")), None, p(fin), None)

    assert gru() == 0 and evo() == 0
    torch.cuda.synchronize()
    assert gru(H=129, E=129) == -2 and evo(H=129) == -2
    assert gru(B=-1) == -1 and gru(T=-3) == -1 and evo(B=-1) == -1 and evo(T=0) == -1
    assert gru(kernel=None) == -1 and gru(out=None) == -1 and evo(q=None) == -1


# ---- guards and poison under the family's allocations -------------------------------------------------------------------
def body_driver(ops, case):
    flag = ops.new_flag("cuda")
    return (flag,) + run_gru(case, oob=flag, ops=ops) + run_evo(case, "AUGRU", 1, ops=ops) + run_evo(case, "AGRU", 0, ops=ops) \
        + run_dense(case, ops=ops)


def _compare(what, got, want):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert G.bit_equal(a, b), "%s: returned tensor %d %s %s differs" % (what, i, tuple(a.shape), a.dtype)


@pytest.mark.parametrize("case", DR.CASES, ids=ids)
def test_guards_and_poison(case):
    from explicit_tf2_recommendation_amd import ops
    want = G.flatten(body_driver(ops, case))
    with G.guarded(ops, G.POISON_NAN) as g:
        nan_run = G.flatten(body_driver(ops, case))
    print("%s: %d allocations, %d bytes through the seam" % (ids(case), len(g.allocations), g.total_bytes()))
    assert len(g.allocations) >= 25
    for i, t in enumerate(nan_run):
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), "returned tensor %d %s holds poison or a non-finite value" % (i, tuple(t.shape))
    _compare("0xFF poison against the plain run", nan_run, want)
    with G.guarded(ops, G.POISON_FINITE):
        fin_run = G.flatten(body_driver(ops, case))
    _compare("0x7F poison against 0xFF poison", fin_run, nan_run)


# ---- the layer -----------------------------------------------------------------------------------------------------------
def _layer(seed, kind, mask_mode, fused=True, stage="train"):
    from explicit_tf2_recommendation_amd import layers
    sd = DR.layer_state(seed, kind)
    lay = layers.DIENLayer(feature_dims=DR.LAYER_V, mode=kind, activation="PReLU", mask_mode=mask_mode, fused=fused,
                           stage=stage).cuda()
    lay.load_state_dict({k: torch.from_numpy(np.asarray(v, F32)) for k, v in sd.items()})
    return lay, sd


def _grads(lay):
    out = {}
    for k, q in lay.named_parameters():
        out[k] = np.zeros(tuple(q.shape), F32) if q.grad is None else host(q.grad.to_dense() if q.grad.is_sparse else q.grad)
    return out


LAYER_COMBOS = [(k, m, 6) for k in DR.KINDS for m in ("reference", "valid")] + [("AUGRU", "valid", 20)]


@pytest.mark.parametrize("kind,mask_mode,T", LAYER_COMBOS, ids=lambda v: str(v))
def test_layer_parity_with_the_torch_cpu_transcription(kind, mask_mode, T):
    from explicit_tf2_recommendation_amd import data
    seed = 7
    ins = DR.layer_inputs(seed, DR.LAYER_B, T)
    sd = DR.layer_state(seed, kind)
    mv = 1 if mask_mode == "valid" else 0
    t64, t32 = DR.layer_torch(sd, ins, torch.float64, kind, mv), DR.layer_torch(sd, ins, torch.float32, kind, mv)
    batch = data.to_device(ins)
    weight = batch.pop("weight")
    for fused in (True, False):
        lay, _ = _layer(seed, kind, mask_mode, fused)
        res = lay(batch)
        assert res.keys() == {"X_combined", "output", "auxiliary_loss"}
        assert tuple(res["output"].shape) == (DR.LAYER_B, 2) and res["auxiliary_loss"].dim() == 0
        tag = "fused " if fused else "composed "
        for k in ("X_combined", "output"):
            check(tag + k, host(res[k]), t64[k], t32[k], 1e-5)
        check(tag + "auxiliary_loss", host(res["auxiliary_loss"]).reshape(1), np.array([t64["auxiliary_loss"]]),
              np.array([t32["auxiliary_loss"]]), 1e-5)
        ((res["output"] * weight).sum() + res["auxiliary_loss"]).backward()
        grads = _grads(lay)
        assert grads.keys() == t64["grads"].keys()
        for k in grads:
            check(tag + k, grads[k], t64["grads"][k], t32["grads"][k], 3e-5)
        if kind != "AIGRU" and mask_mode == "reference":                     # the consequence of the reference's mask
            H = DR.LAYER_H
            assert not host(res["X_combined"])[:, -H:].any()
            assert all(not grads[k].any() for k in grads if k.startswith("dien_gru.") or k == "dien_activation_layer.W")


def test_stage_inference_returns_zero_and_never_reads_the_negative_features():
    from explicit_tf2_recommendation_amd import data
    ins = DR.layer_inputs(3, DR.LAYER_B, 6)
    ins.pop("weight")
    full = data.to_device(ins)
    bare = {k: v for k, v in full.items() if k not in DR.NEGATIVE}
    for fused in (True, False):
        lay, _ = _layer(3, "AUGRU", "valid", fused)
        want = lay(full)
        lay.set_stage("inference")
        with torch.no_grad():
            res = lay(bare)
        assert res["auxiliary_loss"] == 0 and isinstance(res["auxiliary_loss"], int)
        assert torch.equal(res["output"], want["output"]) and torch.equal(res["X_combined"], want["X_combined"])


def test_out_of_range_id_raises():
    from explicit_tf2_recommendation_amd import data
    lay, _ = _layer(1, "AUGRU", "valid")
    ins = DR.layer_inputs(1, DR.LAYER_B, 6)
    ins.pop("weight")
    lay(data.to_device(ins))
    for name in ("visited_shop_ids", "negative_cate_ids", "i_shop_id"):
        bad = {k: v.copy() for k, v in ins.items()}
        bad[name].reshape(-1)[5] = DR.LAYER_V
        with pytest.raises(IndexError):
            lay(data.to_device(bad))


def test_graphed_train_step_with_the_auxiliary_loss_equals_eager():
    """Forward plus backward captured once and replayed over three batches against an eager copy of the layer: an
    output_fn keeps the layer's result, an extra_loss_fn takes its auxiliary_loss out again (nothing may hold the
    autograd graph of one pass into the next); the loss and every gradient, the table's sparse rows included, are equal
    bit for bit."""
    from explicit_tf2_recommendation_amd import data, engine
    T, B = 6, DR.LAYER_B
    lay, _ = _layer(1, "AUGRU", "valid")
    eager = copy.deepcopy(lay)
    kept = {}

    def output_fn(layer, x):
        kept["res"] = layer(x)
        return kept["res"]["output"]

    loss_fn = lambda out, y: (out * y).sum()
    extra = lambda ins: kept.pop("res")["auxiliary_loss"]
    batches = [data.to_device(DR.layer_inputs(s, B, T)) for s in (11, 12, 13)]
    step = engine.GraphedTrainStep(lay, batches[0], label_name="weight", output_fn=output_fn, loss_fn=loss_fn,
                                   extra_loss_fn=extra)
    for m in eager.modules():
        if hasattr(m, "check_ids"):
            m.check_ids = False
    for b in batches:
        loss = step(b)
        for q in eager.parameters():
            q.grad = None
        res = eager({k: v for k, v in b.items() if k != "weight"})
        want = loss_fn(res["output"], b["weight"]) + res["auxiliary_loss"]
        want.backward()
        assert torch.equal(loss.reshape(()), want.detach().reshape(()))
        for (name, a), q in zip(lay.named_parameters(), eager.parameters()):
            assert a.grad is not None and q.grad is not None and a.grad.is_sparse == q.grad.is_sparse, name
            if a.grad.is_sparse:
                assert torch.equal(a.grad._indices(), q.grad._indices()), name
                assert torch.equal(a.grad._values(), q.grad._values()), name
            else:
                assert torch.equal(a.grad, q.grad), name
