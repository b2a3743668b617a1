"""SINE on the GPU: the sparse-interest kernels and the auxiliary loss (csrc/sine.hip) against the fp64 numpy reading of
tests/sine_ref.py, the order of the selection, a strided table, out-of-range ids, bit identity run to run, the layer
against the torch-CPU transcription, graph capture, guards and poison under the family's allocations and the error paths.

Tolerance, per tensor (the project's rule, as tests/test_gpu_mind.py states it): max|got - want| / max|want| against fp64
must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors) /
3e-5 (gradients); a tensor that is zero throughout in fp64 must be exactly zero.  The top-K is a kink: the near-tie
examples of a body case (sim_(K) - sim_(K+1) below 1e-4 in fp64; at most 10 % of the batch, asserted without a GPU in
tests/test_sine_host.py) are left out of out and chosen and have zero rows of gout on both sides; on every other example
sorted(chosen) equals the fp64 selection exactly.  The seed of a layer case is the first with no near-tie example at all.

Measured on the MI355X, the printout as a DIGEST (every test prints `name error / bound` for each tensor it checks; 128
lines in all).  39 passed in 4.8 s.  Per test: the number of tensors checked and the one with the largest error / bound.
Where a bound is far above its floor the fp32 CPU transcription is that far from fp64 itself: the softmax at tau = 0.1
over LayerNorm rows is badly conditioned at D = 256, and in the layer case at T = 6 the fp32 transcription's own dW4 is
37 % off (bound 1.48, the kernel's error 0.37: a gradient that nearly cancels).
  interest_matches_fp64[1x1x1x1x1x1]: 9 tensors, largest ratio out 0.00e+00 / 1.00e-05
  interest_matches_fp64[3x5x1x8x4x4]: 9 tensors, largest ratio dW1 4.00e-06 / 3.00e-05
  interest_matches_fp64[33x6x3x16x100x5]: 9 tensors, largest ratio dW4 3.67e-06 / 4.21e-05
  interest_matches_fp64[33x50x3x16x100x5]: 9 tensors, largest ratio dW2 1.55e-05 / 3.00e-05
  interest_matches_fp64[33x65x3x8x33x16]: 9 tensors, largest ratio dpool 9.46e-06 / 3.00e-05
  interest_matches_fp64[17x33x3x16x7x1]: 9 tensors, largest ratio out 1.74e-07 / 1.00e-05
  interest_matches_fp64[5x9x4x64x100x5]: 9 tensors, largest ratio dW4 1.07e-03 / 4.31e-03
  interest_matches_fp64[2049x10x3x16x100x5]: 9 tensors, largest ratio dW2 1.57e-05 / 4.61e-05
  interest_matches_fp64[40x7x3x16x100x5]: 9 tensors, largest ratio dWk2 1.77e-06 / 3.00e-05
  out_of_range_ids_set_the_flag_and_read_as_zero_rows: 9 tensors, largest ratio dW4 3.67e-06 / 4.21e-05
  aux_matches_fp64[1-1]: 2 tensors, largest ratio loss 0.00e+00 / 1.00e-05
  aux_matches_fp64[2-3]: 2 tensors, largest ratio loss 1.31e-07 / 1.00e-05
  aux_matches_fp64[7-48]: 2 tensors, largest ratio loss 3.45e-08 / 1.00e-05
  aux_matches_fp64[100-48]: 2 tensors, largest ratio loss 1.49e-07 / 1.00e-05
  aux_matches_fp64[33-256]: 2 tensors, largest ratio loss 4.03e-07 / 1.00e-05
  aux_matches_fp64[1024-5]: 2 tensors, largest ratio dpool 9.91e-07 / 3.00e-05
  layer_parity_with_the_torch_cpu_transcription[6]: 13 tensors, largest ratio W2 4.22e-05 / 1.56e-04
  layer_parity_with_the_torch_cpu_transcription[50]: 13 tensors, largest ratio user_interest 3.89e-06 / 1.00e-05
"""
import copy

import numpy as np
import pytest
import torch

from tests import guarded as G
from tests import sine_ref as SR

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = lambda c: "x".join(map(str, c))
GRADS = ("gkeys",) + tuple("d" + k for k in SR.WEIGHTS)


def cu(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(name, got, want, t32, floor):
    err, bound = SR.rel_err(got, want), max(floor, 4 * SR.rel_err(t32, want))
    print("%-12s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


# ---- bodies -------------------------------------------------------------------------------------------------------------
_DEV = {}


def dev(case):
    if case not in _DEV:
        c = SR.inputs(*case)
        _DEV[case] = (cu(c["table"]), cu(c["series"], np.int64), [cu(c["w"][k]) for k in SR.WEIGHTS], cu(c["gout"]))
    return _DEV[case]


def run(case, table=None, series=None, oob=None, ops=None):
    if ops is None:
        from explicit_tf2_recommendation_amd import ops
    tab, ser, w, gout = dev(case)
    tab = tab if table is None else table
    ser = ser if series is None else series
    out, chosen = ops.sine_interest_fwd(tab, ser, *w, case[5], SR.TAU, SR.LN_EPS, 0, oob)
    return (out, chosen) + tuple(ops.sine_interest_bwd(tab, ser, *w, chosen, gout, SR.TAU, SR.LN_EPS, 0))


def check_body(case, got, ref, t32, near):
    B, T, Cn, E, L, K = case
    out, chosen, grads = host(got[0]), host(got[1]), [host(g) for g in got[2:]]
    assert chosen.dtype == np.int32 and chosen.shape == (B, K) and out.shape == (B, Cn * E)
    assert chosen.min() >= 0 and chosen.max() < L and all(len(set(r)) == K for r in chosen.tolist())
    assert np.array_equal(np.sort(chosen[~near], 1), np.sort(ref["chosen"][~near], 1))
    assert np.array_equal(chosen[~near], ref["chosen"][~near])               # and in descending-similarity order
    check("out", out[~near], ref["out"][~near], t32["out"][~near], 1e-5)
    for name, g in zip(GRADS, grads):
        assert g.shape == ref[name].shape, name
        check(name, g, ref[name], t32[name], 3e-5)


@pytest.mark.parametrize("case", SR.CASES + [SR.SKEW_CASE], ids=ids)
def test_interest_matches_fp64(case):
    c = SR.inputs(*case)
    check_body(case, run(case), SR.ref(case), SR.case_t(case, torch.float32), c["near"])


def test_width_one_gives_exact_zeros():
    got = run(SR.CASES[0])
    assert not got[0].any() and all(not g.any() for g in got[2:]) and int(got[1][0, 0]) == 0


def test_skew_case_writes_exact_zeros_to_the_rows_nobody_chose():
    case = SR.SKEW_CASE
    got = run(case)
    chosen = host(got[1])
    live = np.zeros(case[4], bool)
    live[chosen[0]] = True
    assert (chosen == chosen[0]).all() and live.sum() == case[5]
    for name, g in zip(GRADS, got[2:]):
        if name in ("dpool", "dWk1", "dWk2"):
            rows = host(g).reshape(case[4], -1)                               # (a chosen row may underflow in fp32)
            assert not rows[~live].any() and rows[live].any(), name


def test_order_of_chosen_and_the_lower_index_on_an_exact_tie():
    """Similarities that are exactly representable: one behaviour whose row is 1 in every column, no padding, so z is that
    row whatever W1 and W2 hold, and pool rows that are multiples of basis vectors, so sim_l is the multiple.  Two pairs
    of equal values, one of them across the boundary of the selection."""
    from explicit_tf2_recommendation_amd import ops
    D, L, K = 8, 12, 4
    table = torch.ones(3, D, device="cuda")
    series = torch.ones(2, 1, 1, dtype=torch.int64, device="cuda")
    mult = [0.5, 3.0, -1.0, 2.0, 3.0, 0.25, 1.0, 2.0, -4.0, 2.0, 0.0, 1.5]    # top-4 under top_k's rule: 1, 4, 3, 7
    pool = torch.zeros(L, D, device="cuda")
    for l, m in enumerate(mult):
        pool[l, l % D] = m
    r = torch.Generator("cuda").manual_seed(5)
    w = [pool] + [torch.randn(s, device="cuda", generator=r) * 0.3 for s in ((D, D), (D,), (L, D, D), (L, D), (D, D), (D,))]
    out, chosen = ops.sine_interest_fwd(table, series, *w, K)
    assert chosen.tolist() == [[1, 4, 3, 7]] * 2
    want = SR.top_k(np.asarray([mult, mult]), K)
    assert np.array_equal(host(chosen), want)
    _, chosen = ops.sine_interest_fwd(table, series, *w, L)                   # K == L: the whole order
    assert np.array_equal(host(chosen), SR.top_k(np.asarray([mult, mult]), L))


def _strided(table, pad=3):
    wide = torch.full((table.shape[0], table.shape[1] + pad), 7.0, device="cuda")
    wide[:, :table.shape[1]] = table
    view = wide[:, :table.shape[1]]
    assert view.stride(0) == table.shape[1] + pad
    return view


def test_strided_table_is_bit_identical_to_the_packed_one():
    case = (33, 65, 3, 8, 33, 16)
    for a, b in zip(run(case), run(case, table=_strided(dev(case)[0]))):
        assert torch.equal(a, b)


def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows():
    from explicit_tf2_recommendation_amd import ops
    case = (33, 6, 3, 16, 100, 5)
    c = SR.inputs(*case)
    flag = ops.new_flag("cuda")
    run(case, oob=flag)
    assert int(flag.item()) == 0
    series = c["series"].copy()
    series[5, 2, 1], series[7, 0, 0], series[9, 3, 2] = -1, SR.V_CASE, 2 ** 40   # (a first-feature id too: not padding)
    fwd = SR.sine_numpy(c["table"], series, c["w"], case[5])
    near = SR.boundary_gap(fwd["sim"], case[5]) < SR.GAP_EPS
    assert not near[[5, 7, 9]].any() and not c["gout"][near].any()
    ref = SR.sine_numpy(c["table"], series, c["w"], case[5], gout=c["gout"])
    t32 = SR.sine_torch_grads(c["table"], series, c["w"], ref["chosen"], c["gout"], torch.float32)
    got = run(case, series=cu(series, np.int64), oob=flag)
    assert int(flag.item()) == 1
    check_body(case, got, ref, t32, near)


def test_every_output_is_bit_identical_run_to_run():
    for case in ((2049, 10, 3, 16, 100, 5), (5, 9, 4, 64, 100, 5), SR.SKEW_CASE):
        for a, b in zip(run(case), run(case)):
            assert torch.equal(a, b)


@pytest.mark.parametrize("L,D", SR.AUX_CASES, ids=lambda v: str(v))
def test_aux_matches_fp64(L, D):
    from explicit_tf2_recommendation_amd import ops
    pool = SR.aux_pool(L, D)
    ref, t32 = SR.aux_numpy(pool, 0.75), SR.aux_torch_grads(pool, 0.75, torch.float32)
    p = cu(pool)
    loss = ops.sine_aux_fwd(p)
    dpool = ops.sine_aux_bwd(p, torch.full((1,), 0.75, device="cuda"))
    assert loss.shape == () and tuple(dpool.shape) == (L, D)
    check("loss", host(loss), ref["loss"], t32["loss"], 1e-5)
    check("dpool", host(dpool), ref["dpool"], t32["dpool"], 3e-5)
    assert torch.equal(loss, ops.sine_aux_fwd(p)) and torch.equal(dpool, ops.sine_aux_bwd(p, torch.full((1,), 0.75, device="cuda")))


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    case = (3, 5, 1, 8, 4, 4)
    tab, ser, w, gout = dev(case)
    out, chosen = ops.sine_interest_fwd(tab, ser, *w, 4)
    with pytest.raises(RuntimeError):
        ops.sine_interest_fwd(tab.cpu(), ser, *w, 4)                           # no CPU fallback
    with pytest.raises(TypeError):
        ops.sine_interest_fwd(tab, ser.int(), *w, 4)
    with pytest.raises(ValueError):
        ops.sine_interest_fwd(tab, ser, w[0], w[1][:7].contiguous(), *w[2:], 4)
    with pytest.raises(ValueError):
        ops.sine_interest_fwd(tab, ser, *w[:3], w[3][:3].contiguous(), *w[4:], 4)
    with pytest.raises(ValueError):
        ops.sine_interest_fwd(tab, ser, *w, 4, tau=0.0)
    with pytest.raises(NotImplementedError):
        ops.sine_interest_fwd(tab, ser, *w, 5)                                 # K > L
    with pytest.raises(TypeError):
        ops.sine_interest_bwd(tab, ser, *w, chosen.long(), gout)
    with pytest.raises(ValueError):
        ops.sine_interest_bwd(tab, ser, *w, chosen, gout[:, :3].contiguous())
    with pytest.raises(NotImplementedError):                                    # T beyond the LDS fit
        z = lambda *s: torch.zeros(*s, device="cuda")
        ops.sine_interest_fwd(z(10, 16), torch.zeros(2, 165, 3, dtype=torch.int64, device="cuda"), z(100, 48), z(48, 48),
                              z(48), z(100, 48, 48), z(100, 48), z(48, 48), z(48), 5)
    out, chosen = ops.sine_interest_fwd(tab, ser[:0], *w, 4)
    res = ops.sine_interest_bwd(tab, ser[:0], *w, chosen, gout[:0])
    assert tuple(out.shape) == (0, 8) and tuple(chosen.shape) == (0, 4) and tuple(res[0].shape) == (0, 5, 8)
    assert all(not g.any() and g.shape == x.shape for g, x in zip(res[1:], w))


# ---- the layer -----------------------------------------------------------------------------------------------------------
def _layer(seed):
    from explicit_tf2_recommendation_amd import layers
    sd = SR.layer_state(seed)
    lay = layers.SINELayer(feature_dims=SR.LAYER_V).cuda()
    lay.load_state_dict({k: torch.from_numpy(np.asarray(v, F32)) for k, v in sd.items()})
    return lay, sd


def _grads(lay):
    return {k: host(q.grad.to_dense() if q.grad.is_sparse else q.grad) for k, q in lay.named_parameters()}


@pytest.mark.parametrize("T", SR.LAYER_TS)
def test_layer_parity_with_the_torch_cpu_transcription(T):
    from explicit_tf2_recommendation_amd import data
    seed = SR.layer_seed(T)
    lay, sd = _layer(seed)
    ins = SR.layer_inputs(seed, SR.LAYER_B, T)
    up = SR.layer_upstream(seed)
    t64, t32 = SR.layer_torch(sd, ins, torch.float64, *up), SR.layer_torch(sd, ins, torch.float32, *up)
    assert not (t64["gap"] < SR.GAP_EPS).any()                                # so no example is left out
    batch = data.to_device(ins)
    ui = lay.generate_user_interest({k: batch[k] for k in SR.SERIES})           # serving: no item features
    check("serving", host(ui), t64["user_interest"], t32["user_interest"], 1e-5)
    res = lay(batch)
    assert res.keys() == {"user_interest", "main_loss", "aux_loss"}
    assert tuple(res["user_interest"].shape) == (SR.LAYER_B, SR.LAYER_D) and tuple(res["main_loss"].shape) == (SR.LAYER_B,)
    assert res["aux_loss"].shape == () and torch.equal(res["user_interest"], ui)
    for k in ("user_interest", "main_loss", "aux_loss"):
        check(k, host(res[k]), t64[k], t32[k], 1e-5)
    check("aux alone", host(lay.compute_auxiliary_loss()), t64["aux_loss"], t32["aux_loss"], 1e-5)
    ((res["user_interest"] * cu(up[0])).sum() + (res["main_loss"] * cu(up[1])).sum() + res["aux_loss"] * up[2]).backward()
    grads = _grads(lay)
    assert grads.keys() == t64["grads"].keys() == SR.STATE_SHAPES.keys()
    for k in grads:
        check(k, grads[k], t64["grads"][k], t32["grads"][k], 3e-5)


def test_out_of_range_id_raises():
    from explicit_tf2_recommendation_amd import data
    lay, _ = _layer(1)
    ins = SR.layer_inputs(1, SR.LAYER_B, 6)
    lay(data.to_device(ins))
    for name in ("visited_shop_ids", "label_cate_ids"):
        bad = {k: v.copy() for k, v in ins.items()}
        bad[name].reshape(-1)[5] = SR.LAYER_V
        with pytest.raises(IndexError):
            lay(data.to_device(bad))
    bad = {k: v.copy() for k, v in ins.items()}
    bad["visited_cate_ids"].reshape(-1)[7] = -1
    with pytest.raises(IndexError):
        lay.generate_user_interest(data.to_device(bad))


def test_graph_replay_equals_eager_bit_for_bit():
    """Three replays over three batches against an eager copy of the layer: losses and every gradient, the table's sparse
    rows included."""
    from explicit_tf2_recommendation_amd import data, engine
    T = 50
    lay, _ = _layer(1)
    eager = copy.deepcopy(lay)
    total = lambda res: (res["main_loss"].sum() + res["aux_loss"]).reshape(1)

    def batch(seed):
        b = data.to_device(SR.layer_inputs(seed, SR.LAYER_B, T))
        b["label"] = torch.zeros(SR.LAYER_B, 1, device="cuda")                # a dummy: the layer carries its own loss
        return b

    batches = [batch(s) for s in (11, 12, 13)]
    step = engine.GraphedTrainStep(lay, batches[0], label_name="label", output_fn=lambda l, x: total(l(x)),
                                   loss_fn=lambda out, y: out.sum())
    for b in batches:
        loss = step(b)
        for q in eager.parameters():
            q.grad = None
        want = total(eager({k: v for k, v in b.items() if k != "label"})).sum()
        want.backward()
        assert torch.equal(loss.reshape(()), want.detach())
        for (name, a), q in zip(lay.named_parameters(), eager.parameters()):
            assert a.grad is not None and a.grad.is_sparse == q.grad.is_sparse, name
            if a.grad.is_sparse:
                assert torch.equal(a.grad._indices(), q.grad._indices()), name
                assert torch.equal(a.grad._values(), q.grad._values()), name
            else:
                assert torch.equal(a.grad, q.grad), name


# ---- guards and poison under the family's allocations -------------------------------------------------------------------
GUARD_CASES = [(1, 1, 1, 1, 1, 1), (3, 5, 1, 8, 4, 4), (33, 50, 3, 16, 100, 5), (33, 65, 3, 8, 33, 16), (5, 9, 4, 64, 100, 5),
               (2049, 10, 3, 16, 100, 5)]


def interest_driver(ops, case):
    flag = ops.new_flag("cuda")
    return (flag,) + run(case, oob=flag, ops=ops)


def aux_driver(ops, case):
    p = cu(SR.aux_pool(*case))
    return ops.sine_aux_fwd(p), ops.sine_aux_bwd(p, torch.full((1,), 0.75, device="cuda"))


def _compare(what, got, want):
    assert len(got) == len(want), (what, len(got), len(want))
    for i, (a, b) in enumerate(zip(got, want)):
        assert G.bit_equal(a, b), "%s: returned tensor %d %s %s differs" % (what, i, tuple(a.shape), a.dtype)


@pytest.mark.parametrize("driver,case", [(interest_driver, c) for c in GUARD_CASES] + [(aux_driver, c) for c in SR.AUX_CASES],
                         ids=lambda v: v.__name__ if callable(v) else ids(v))
def test_guards_and_poison(driver, case):
    from explicit_tf2_recommendation_amd import ops
    want = G.flatten(driver(ops, case))
    with G.guarded(ops, G.POISON_NAN) as g:
        nan_run = G.flatten(driver(ops, case))
    print("%s %s: %d allocations, %d bytes through the seam" % (driver.__name__, ids(case), len(g.allocations), g.total_bytes()))
    assert len(g.allocations) >= 2
    for i, t in enumerate(nan_run):
        if t.is_floating_point():
            assert bool(torch.isfinite(t).all()), "returned tensor %d %s holds poison or a non-finite value" % (i, tuple(t.shape))
    _compare("0xFF poison against the plain run", nan_run, want)
    with G.guarded(ops, G.POISON_FINITE):
        fin_run = G.flatten(driver(ops, case))
    _compare("0x7F poison against 0xFF poison", fin_run, nan_run)


def test_a_short_scratch_view_trips_the_guard():
    """rec_sine_scratch_bytes answers with 4 floats more than rec_sine_interest_bwd_f32 consumes, so the view is 32 bytes
    short: its trailing guard then starts on the last four floats of the last workgroup's slot, its dW4, which the
    example-major kernel writes."""
    from explicit_tf2_recommendation_amd import ops
    with pytest.raises(G.GuardError) as e:
        with G.guarded(ops, G.POISON_NAN, short_by=32, short_if=lambda a: a.frames[0].startswith("_workspace:")):
            interest_driver(ops, (3, 5, 1, 8, 4, 4))
    msg = str(e.value)
    print(msg)
    assert "after the view" in msg and "_workspace:" in msg and "before the view" not in msg
    assert msg.count("\n") == 1, "one allocation, the scratch, and no other"
