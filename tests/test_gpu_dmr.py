"""DMR on the GPU: the fused attention / match-loss kernels (csrc/dmr.hip) against the fp64 numpy reading of
tests/dmr_ref.py, optional gradients, bit identity run to run, a strided table, out-of-range ids, guards and poison under
the family's allocations, the layer against the torch-CPU transcription, graph capture and the error paths.

Tolerance, per tensor (the project's rule, as tests/test_gpu_mind.py states it): max|got - want| / max|want| against fp64
must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors) /
3e-5 (gradients); a tensor that is zero throughout in fp64 must be exactly zero.  Every test prints `name error / bound`.

Measured on the MI355X, the printout as a DIGEST (179 lines in all).  25 passed in 4.5 s.  Per test: the number of
tensors checked and the one with the largest error / bound.  Every bound sits on its floor: the fp32 CPU transcription is
that close to fp64 itself on these inputs.
  body_matches_fp64[1x1x1x1x1x1]: 10 tensors, largest ratio u2i 4.51e-08 / 1.00e-05
  body_matches_fp64[3x5x1x8x4x1]: 10 tensors, largest ratio u2i 1.46e-07 / 1.00e-05
  body_matches_fp64[33x10x3x16x48x6]: 10 tensors, largest ratio u2i 5.91e-07 / 1.00e-05
  body_matches_fp64[33x7x3x5x15x33]: 10 tensors, largest ratio u2i 1.50e-07 / 1.00e-05
  body_matches_fp64[5x100x3x32x96x6]: 10 tensors, largest ratio gkeys 1.69e-06 / 3.00e-05
  body_matches_fp64[2x9x4x64x256x3]: 10 tensors, largest ratio dWe 4.14e-06 / 3.00e-05
  body_matches_fp64[2049x10x3x16x48x6]: 10 tensors, largest ratio gkeys 1.21e-06 / 3.00e-05
  auxiliary_gradient_alone_is_zero_where_one_position_is_valid: 7 tensors, largest ratio gkeys 7.54e-07 / 3.00e-05
  out_of_range_ids_set_the_flag_and_read_as_zero_rows: 10 tensors, largest ratio u2i 5.91e-07 / 1.00e-05
  layer_parity_with_the_torch_cpu_transcription[10]: 46 tensors, largest ratio composed u2i_network.Wp 1.33e-06 / 3.00e-05
  layer_parity_with_the_torch_cpu_transcription[50]: 46 tensors, largest ratio fused mlp.layers.6.kernel 1.20e-06 / 3.00e-05
"""
import copy

import numpy as np
import pytest
import torch

from tests import dmr_ref as DR
from tests import guarded as G

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = lambda c: "x".join(map(str, c))
MASKED = (33, 10, 3, 16, 48, 6)


def cu(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(name, got, want, t32, floor):
    err, bound = DR.rel_err(got, want), max(floor, 4 * DR.rel_err(t32, want))
    print("%-14s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


# ---- bodies -------------------------------------------------------------------------------------------------------------
_DEV = {}
OPERANDS = ("xi", "q", "P", "We", "z")


def dev(case):
    if case not in _DEV:
        c = DR.inputs(case)
        o = DR.operands(c)
        _DEV[case] = dict(table=cu(c["table"]), series=cu(c["series"], np.int64), negatives=cu(c["negatives"], np.int64),
                          g=[cu(c[k]) for k in DR.UPSTREAM], **{k: cu(o[k]) for k in OPERANDS})
    return _DEV[case]


def run(case, table=None, series=None, negatives=None, oob=None, ops=None, g=None):
    """-> the 3 outputs and the 7 gradients of a case, in the order of DR.OUTPUTS + DR.GRADS"""
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    d = dev(case)
    tab = d["table"] if table is None else table
    ser = d["series"] if series is None else series
    neg = d["negatives"] if negatives is None else negatives
    w = [d[k] for k in OPERANDS]
    g = d["g"] if g is None else g
    fwd = ops.dmr_fwd(tab, ser, neg, *w, 0, oob)
    return tuple(fwd) + tuple(ops.dmr_bwd(tab, ser, neg, *w, *g, 0))


def check_body(got, ref, t32):
    for name, t in zip(DR.OUTPUTS + DR.GRADS, got):
        check(name, host(t), ref[name], t32[name], 1e-5 if name in DR.OUTPUTS else 3e-5)


@pytest.mark.parametrize("case", DR.CASES, ids=ids)
def test_body_matches_fp64(case):
    got = run(case)
    check_body(got, DR.case_ref(case), DR.case_t32(case))
    if case[0] >= 5:
        valid = DR.inputs(case)["series"][:, :, 0] != 0
        named = dict(zip(DR.OUTPUTS + DR.GRADS, (host(t) for t in got)))
        assert not named["gkeys"][~valid].any()                              # rows at invalid positions
        for name in ("i2i", "u2i", "aux", "gkeys", "gneg", "gitem", "gq"):
            assert not named[name][2].any(), name                            # the example without a valid position


def test_auxiliary_gradient_alone_is_zero_where_one_position_is_valid():
    case = MASKED
    c = DR.inputs(case)
    got = dict(zip(DR.OUTPUTS + DR.GRADS, run(case, g=[None, None, dev(case)["g"][2]])))
    o = DR.operands(c)
    ref, t32 = DR.dmr_numpy(o, None, None, c["g_aux"]), DR.dmr_torch(o, torch.float32, None, None, c["g_aux"])
    for name in DR.GRADS:
        check(name, host(got[name]), ref[name], t32[name], 3e-5)
    for name in ("gkeys", "gneg", "gitem", "gq"):
        assert not got[name][1].any() and not got[name][2].any(), name
    assert not got["gitem"].any() and got["gneg"][0].any()                    # the loss never reaches xi directly


def test_an_absent_gradient_equals_zeros_bit_for_bit():
    case = MASKED
    g = dev(case)["g"]
    for i in range(3):
        absent = [None if j == i else t for j, t in enumerate(g)]
        zeros = [torch.zeros_like(t) if j == i else t for j, t in enumerate(g)]
        for a, b in zip(run(case, g=absent), run(case, g=zeros)):
            assert torch.equal(a, b), i


def test_every_output_is_bit_identical_run_to_run():
    for a, b in zip(run(DR.LARGEST), run(DR.LARGEST)):
        assert torch.equal(a, b)


def _strided(table, pad=3):
    wide = torch.full((table.shape[0], table.shape[1] + pad), 7.0, device="cuda")
    wide[:, :table.shape[1]] = table
    view = wide[:, :table.shape[1]]
    assert view.stride(0) == table.shape[1] + pad
    return view


def test_strided_table_is_bit_identical_to_the_packed_one():
    case = (33, 7, 3, 5, 15, 33)
    for a, b in zip(run(case), run(case, table=_strided(dev(case)["table"]))):
        assert torch.equal(a, b)


def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows():
    from explicit_tf2_recommendation_amd import ops
    case = MASKED
    c = DR.inputs(case)
    flag = ops.new_flag("cuda")
    run(case, oob=flag)
    assert int(flag.item()) == 0
    series, negatives = c["series"].copy(), c["negatives"].copy()
    series[5, 2, 1], series[7, 0, 0], series[0, 9, 2] = -1, DR.V_CASE, 2 ** 40   # (a first-feature id too: not padding)
    negatives[4, 3, 0], negatives[6, 0, 2] = DR.V_CASE + 5, -7
    o = DR.operands(c, series, negatives)
    up = [c[k] for k in DR.UPSTREAM]
    ref, t32 = DR.dmr_numpy(o, *up), DR.dmr_torch(o, torch.float32, *up)
    for ser, neg in ((series, None), (None, negatives)):                      # either lookup alone sets it
        flag = ops.new_flag("cuda")
        run(case, series=cu(ser, np.int64), negatives=cu(neg, np.int64), oob=flag)
        assert int(flag.item()) == 1
    check_body(run(case, series=cu(series, np.int64), negatives=cu(negatives, np.int64), oob=flag), ref, t32)


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    case = (3, 5, 1, 8, 4, 1)
    d = dev(case)
    tab, ser, neg, g = d["table"], d["series"], d["negatives"], d["g"]
    w = [d[k] for k in OPERANDS]
    ops.dmr_fwd(tab, ser, neg, *w)
    with pytest.raises(RuntimeError):
        ops.dmr_fwd(tab.cpu(), ser, neg, *w)                                  # no CPU fallback
    with pytest.raises(TypeError):
        ops.dmr_fwd(tab, ser.int(), neg, *w)
    with pytest.raises(TypeError):
        ops.dmr_fwd(tab, ser, neg.int(), *w)
    with pytest.raises(TypeError):
        ops.dmr_fwd(tab, ser, neg, w[0].double(), *w[1:])
    for i in range(len(w)):                                                   # every operand one row short
        bad = list(w)
        bad[i] = bad[i][:-1].contiguous()
        with pytest.raises(ValueError):
            ops.dmr_fwd(tab, ser, neg, *bad)
    with pytest.raises(ValueError):
        ops.dmr_fwd(tab, ser, neg[:2].contiguous(), *w)
    with pytest.raises(ValueError):
        ops.dmr_fwd(tab, ser[:, :, 0].contiguous(), neg, *w)
    with pytest.raises(ValueError):
        ops.dmr_bwd(tab, ser, neg, *w, g[0][:, :3].contiguous(), g[1], g[2])
    with pytest.raises(TypeError):
        ops.dmr_bwd(tab, ser, neg, *w, g[0], g[1], g[2].double())
    with pytest.raises(NotImplementedError, match="DMR holds one example"):  # T beyond the LDS fit
        z = lambda *s: torch.zeros(*s, device="cuda")
        zi = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
        ops.dmr_fwd(z(10, 16), zi(2, 245, 3), zi(2, 6, 3), z(2, 48), z(2, 48), z(245, 96), z(48, 96), z(2, 48))
    i2i, u2i, aux = ops.dmr_fwd(tab, ser[:0], neg[:0], w[0][:0], w[1][:0], *w[2:])
    assert tuple(i2i.shape) == (0, 9) and tuple(u2i.shape) == (0, 9) and tuple(aux.shape) == (0,)
    res = ops.dmr_bwd(tab, ser[:0], neg[:0], w[0][:0], w[1][:0], *w[2:], g[0][:0], g[1][:0], g[2][:0])
    assert [tuple(t.shape) for t in res] == [(0, 5, 8), (0, 1, 8), (0, 8), (0, 4), (5, 8), (8, 8), (2, 4)]
    assert all(not t.any() for t in res)


# ---- guards and poison under the family's allocations -------------------------------------------------------------------
def body_driver(ops, case):
    flag = ops.new_flag("cuda")
    return (flag,) + run(case, oob=flag, ops=ops)


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
    assert len(g.allocations) >= 11
    for i, t in enumerate(nan_run):
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), "returned tensor %d %s holds poison or a non-finite value" % (i, tuple(t.shape))
    _compare("0xFF poison against the plain run", nan_run, want)
    with G.guarded(ops, G.POISON_FINITE):
        fin_run = G.flatten(body_driver(ops, case))
    _compare("0x7F poison against 0xFF poison", fin_run, nan_run)


def test_a_short_scratch_view_trips_the_guard():
    """rec_dmr_scratch_bytes answers with 4 floats more than rec_dmr_bwd_f32 consumes, so a view 32 bytes short has its
    trailing guard on the last four floats of the last workgroup's slot, its dz, which the backward writes."""
    from explicit_tf2_recommendation_amd import ops
    with pytest.raises(G.GuardError) as e:
        with G.guarded(ops, G.POISON_NAN, short_by=32, short_if=lambda a: a.frames[0].startswith("_workspace:")):
            body_driver(ops, (3, 5, 1, 8, 4, 1))
    msg = str(e.value)
    print(msg)
    assert "after the view" in msg and "_workspace:" in msg and "before the view" not in msg


# ---- the layer -----------------------------------------------------------------------------------------------------------
def _layer(seed, T, fused=True):
    from explicit_tf2_recommendation_amd import layers
    sd = DR.layer_state(seed, T)
    lay = layers.DMRLayer(feature_dims=DR.LAYER_V, max_length=T, fused=fused).cuda()
    lay.load_state_dict({k: torch.from_numpy(np.asarray(v, F32)) for k, v in sd.items()})
    return lay, sd


def _loss(res, label):
    from explicit_tf2_recommendation_amd import functional as Fn
    return Fn.KerasBCE.apply(res["output"], label) + res["auxiliary_loss"].mean()


def _grads(lay):
    return {k: host(q.grad.to_dense() if q.grad.is_sparse else q.grad) for k, q in lay.named_parameters()
            if q.grad is not None}


@pytest.mark.parametrize("T", DR.LAYER_TS)
def test_layer_parity_with_the_torch_cpu_transcription(T):
    from explicit_tf2_recommendation_amd import data
    seed = 7
    ins = DR.layer_inputs(seed, DR.LAYER_B, T)
    sd = DR.layer_state(seed, T)
    t64, t32 = DR.layer_torch(sd, ins, torch.float64), DR.layer_torch(sd, ins, torch.float32)
    batch = data.to_device(ins)
    label = batch.pop("label")
    for fused in (True, False):
        lay, _ = _layer(seed, T, fused)
        res = lay(batch)
        assert res.keys() == {"output", "auxiliary_loss"}
        assert tuple(res["output"].shape) == (DR.LAYER_B, 1) and tuple(res["auxiliary_loss"].shape) == (DR.LAYER_B,)
        tag = "fused " if fused else "composed "
        for k in ("output", "auxiliary_loss"):
            check(tag + k, host(res[k]), t64[k], t32[k], 1e-5)
        _loss(res, label).backward()
        grads = _grads(lay)
        assert lay.i2i_network.b.grad is None and lay.u2i_network.b.grad is None
        assert grads.keys() == t64["grads"].keys()
        for k in grads:
            check(tag + k, grads[k], t64["grads"][k], t32["grads"][k], 3e-5)


def test_out_of_range_id_raises():
    from explicit_tf2_recommendation_amd import data
    lay, _ = _layer(1, 10)
    ins = DR.layer_inputs(1, DR.LAYER_B, 10)
    ins.pop("label")
    lay(data.to_device(ins))
    for name in ("visited_shop_ids", "negative_cate_ids", "i_shop_id"):
        bad = {k: v.copy() for k, v in ins.items()}
        bad[name].reshape(-1)[5] = DR.LAYER_V
        with pytest.raises(IndexError):
            lay(data.to_device(bad))


def test_graph_replay_equals_eager_bit_for_bit():
    """Forward plus backward captured once and replayed over three batches against an eager copy of the layer: the loss
    and every gradient, the table's sparse rows included."""
    from explicit_tf2_recommendation_amd import data, engine
    from explicit_tf2_recommendation_amd import functional as Fn
    T, B = 10, DR.LAYER_B
    lay, _ = _layer(1, T)
    eager = copy.deepcopy(lay)

    def output_fn(layer, x):
        res = layer(x)
        return torch.cat([res["output"].reshape(-1), res["auxiliary_loss"]])

    loss_fn = lambda out, y: Fn.KerasBCE.apply(out[:B].reshape(B, 1), y) + out[B:].mean()
    batches = [data.to_device(DR.layer_inputs(s, B, T)) for s in (11, 12, 13)]
    step = engine.GraphedTrainStep(lay, batches[0], label_name="label", output_fn=output_fn, loss_fn=loss_fn)
    for m in eager.modules():
        if hasattr(m, "check_ids"):
            m.check_ids = False
    for b in batches:
        loss = step(b)
        for q in eager.parameters():
            q.grad = None
        want = loss_fn(output_fn(eager, {k: v for k, v in b.items() if k != "label"}), b["label"])
        want.backward()
        assert torch.equal(loss.reshape(()), want.detach().reshape(()))
        for (name, a), q in zip(lay.named_parameters(), eager.parameters()):
            if name.endswith(".b"):
                assert a.grad is None and q.grad is None, name
                continue
            assert a.grad is not None and a.grad.is_sparse == q.grad.is_sparse, name
            if a.grad.is_sparse:
                assert torch.equal(a.grad._indices(), q.grad._indices()), name
                assert torch.equal(a.grad._values(), q.grad._values()), name
            else:
                assert torch.equal(a.grad, q.grad), name
