"""The CAN co-action on the GPU: the kernels of csrc/can.hip through the C ABI against the fp64 numpy reading of
tests/can_ref.py in both output modes, one shared table, strided tables, out-of-range ids, guard buffers, bit identity run
to run and under graph replay, layers.CoActionUnit against the torch-CPU transcription, and the error paths.

Tolerance, per tensor (the project's rule, as tests/test_gpu_mind.py states it): max|got - want| / max|want| against fp64
must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors) /
3e-5 (gradients); a tensor that is zero throughout in fp64 must be exactly zero.  relu cases come from the generator that
leaves no pre-activation within 1e-4 of zero (asserted without a GPU in tests/test_can_host.py): nothing is left out.

Measured on the MI355X, the first run's printout as a DIGEST (every comparison prints `name error / bound`; 287 lines
in all).  64 passed in 6.7 s.  Per tensor name, over all tests: the largest error / bound.
  all-padded               0.00e+00 / 1.00e-05
  feed grad                1.51e-07 / 3.00e-05
  feed_embedding.embeddi   2.38e-07 / 3.00e-05
  gfeed                    4.48e-07 / 3.00e-05
  gfeed[3]                 0.00e+00 / 1.00e-05
  gind                     7.02e-07 / 3.00e-05
  gind tail                0.00e+00 / 3.00e-05
  gind[:,3]                0.00e+00 / 1.00e-05
  induction_embedding.0.   1.93e-07 / 3.00e-05
  induction_embedding.1.   2.63e-07 / 3.00e-05
  induction_embedding.2.   2.80e-07 / 3.00e-05
  out                      3.52e-07 / 1.00e-05
  output                   2.61e-07 / 1.00e-05
  p feed_embedding.embed   2.94e-07 / 3.00e-05
  p induction_embedding.   2.75e-07 / 3.00e-05
  pool                     2.51e-07 / 1.00e-05
  pooled                   1.74e-07 / 1.00e-05
  shared grad              1.67e-07 / 3.00e-05
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import can_ref as CR

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = CR.case_id
CODE = {"linear": 0, "relu": 1, "sigmoid": 2, "tanh": 3}


def cu(a, dtype=F32):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(name, got, want, t32, floor):
    err, bound = CR.rel_err(got, want), max(floor, 4 * CR.rel_err(t32, want))
    print("%-12s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


# ---- the body through the C ABI ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dev_case(case, act="tanh", shared=False):
    c = CR.can_case(case, act, shared)
    return (cu(c["feed"]), tuple(cu(t) for t in c["inds"]), cu(c["iid"], np.int64), cu(c["fid"], np.int64),
            cu(c["gout"]), cu(c["gpool"]))


def run(case, act="tanh", pooled=False, shared=False, feed=None, inds=None, iid=None, fid=None, oob=None):
    from explicit_tf2_recommendation_amd import ops
    d = dev_case(case, act, shared)
    feed, inds = d[0] if feed is None else feed, d[1] if inds is None else inds
    iid, fid = d[2] if iid is None else iid, d[3] if fid is None else fid
    g = d[5] if pooled else d[4]
    res = ops.can_fwd(feed, inds, iid, fid, case[3], case[4], CODE[act], CR.PAD, pooled, oob)
    gfeed, gind = ops.can_bwd(feed, inds, iid, fid, case[3], case[4], CODE[act], g, CR.PAD, pooled)
    return res, gfeed, gind


def check_body(got, ref, t32, pooled):
    first = "pool" if pooled else "out"
    for (name, floor), g in zip(((first, 1e-5), ("gfeed", 3e-5), ("gind", 3e-5)), got):
        check(name, host(g), ref[name], t32[name], floor)


@pytest.mark.parametrize("pooled", [False, True], ids=["out", "pool"])
@pytest.mark.parametrize("case", CR.CASES + CR.EXTRA_CASES, ids=ids)
def test_body_matches_fp64(case, pooled):
    c = CR.can_case(case)
    ref, t32 = CR.can_ref(case)[pooled], CR.can_case_t(case, "tanh", torch.float32)[pooled]
    got = run(case, pooled=pooled)
    B, T, E, coefs, order = case
    assert tuple(got[0].shape) == ((B, c["Eo"]) if pooled else (order, B, max(T, 1), c["Eo"]))
    assert tuple(got[1].shape) == (B, max(T, 1), E) and tuple(got[2].shape) == (order, B, c["P"])
    check_body(got, ref, t32, pooled)
    if B >= 4:                                                         # example 3 is padded throughout
        for name, g, want in (("all-padded", got[0][3] if pooled else got[0][:, 3], None), ("gfeed[3]", got[1][3], None),
                              ("gind[:,3]", got[2][:, 3], None)):
            check(name, host(g), np.zeros(tuple(g.shape)), np.zeros(tuple(g.shape)), 1e-5)
    used = CR.layer_slices(E, coefs)[min(len(coefs), order) - 1][2]
    if used < c["P"]:                                                  # the layers the reference drops
        assert not ref["gind"][:, :, used:].any()
        check("gind tail", host(got[2][:, :, used:]), ref["gind"][:, :, used:], t32["gind"][:, :, used:], 3e-5)


@pytest.mark.parametrize("pooled", [False, True], ids=["out", "pool"])
@pytest.mark.parametrize("act", ["relu", "sigmoid", "linear"])
@pytest.mark.parametrize("case", CR.OTHER_ACT_CASES, ids=ids)
def test_other_activations_match_fp64(case, act, pooled):
    assert CR.can_case(case, act)["kink_left"] == 0
    check_body(run(case, act, pooled), CR.can_ref(case, act)[pooled], CR.can_case_t(case, act, torch.float32)[pooled],
               pooled)


def test_shared_table_gets_one_gradient_the_sum_over_the_orders():
    from explicit_tf2_recommendation_amd import functional as Fn
    case = CR.CASES[2]
    c = CR.can_case(case, "tanh", True)
    ref, t32 = CR.can_ref(case, "tanh", True)[0], CR.can_case_t(case, "tanh", torch.float32, True)[0]
    check_body(run(case, shared=True), ref, t32, False)
    feed, (table,), iid, fid, gout, _ = dev_case(case, "tanh", True)
    feed, table = torch.nn.Parameter(feed.clone()), torch.nn.Parameter(table.clone())
    out = Fn.CoAction.apply(feed, iid, fid, case[3], case[4], CODE["tanh"], CR.PAD, False, None, table)
    (out * gout).sum().backward()
    assert table.grad.is_sparse and feed.grad.is_sparse and tuple(table.grad.shape) == (CR.V_CASE, c["P"])
    tiled = np.tile(c["iid"], 3)
    check("shared grad", host(table.grad.to_dense()), CR.dense_grad(CR.V_CASE, tiled, ref["gind"].reshape(-1, c["P"])),
          CR.dense_grad(CR.V_CASE, tiled, t32["gind"].reshape(-1, c["P"])), 3e-5)
    check("feed grad", host(feed.grad.to_dense()), CR.dense_grad(CR.V_CASE, c["fid"], ref["gfeed"]),
          CR.dense_grad(CR.V_CASE, c["fid"], t32["gfeed"]), 3e-5)


def _strided(table, pad=3):
    wide = torch.full((table.shape[0], table.shape[1] + pad), 7.0, device="cuda")
    wide[:, :table.shape[1]] = table
    view = wide[:, :table.shape[1]]
    assert view.stride(0) == table.shape[1] + pad
    return view


def test_strided_tables_are_bit_identical_to_the_packed_ones():
    for case in (CR.CASES[4], CR.CASES[2]):
        d = dev_case(case)
        for pooled in (False, True):
            want = run(case, pooled=pooled)
            for got in (run(case, pooled=pooled, feed=_strided(d[0])),                            # ld_f > E
                        run(case, pooled=pooled, inds=tuple(_strided(t, 5) for t in d[1])),      # ld_i > P
                        run(case, pooled=pooled, feed=_strided(d[0], 1), inds=tuple(_strided(t, 1) for t in d[1]))):
                for a, b in zip(got, want):
                    assert torch.equal(a, b)


def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows():
    from explicit_tf2_recommendation_amd import ops
    case = CR.CASES[2]
    c = CR.can_case(case)
    flag = ops.new_flag("cuda")
    clean = run(case, oob=flag)
    assert int(flag.item()) == 0
    iid, fid = c["iid"].copy(), c["fid"].copy()
    iid[[5, 7, 9]] = -1, CR.V_CASE, 2 ** 40
    fid[6, 2], fid[8, 0], fid[10, 5] = -3, CR.V_CASE, 2 ** 40
    for which, (i, f), touched in (("iid", (iid, c["fid"]), [5, 7, 9]), ("fid", (c["iid"], fid), [6, 8, 10])):
        for pooled in (False, True):
            up = dict(gpool=c["gpool"]) if pooled else dict(gout=c["gout"])
            ref = CR.can_numpy(c["feed"], c["inds"], i, f, c["coefs"], c["order"], "tanh", CR.PAD, **up)
            t32 = CR.can_torch_grads(c["feed"], c["inds"], i, f, c["coefs"], c["order"], "tanh", torch.float32, CR.PAD,
                                     **up)
            flag = ops.new_flag("cuda")
            got = run(case, pooled=pooled, iid=cu(i, np.int64), fid=cu(f, np.int64), oob=flag)
            assert int(flag.item()) == 1, which
            check_body(got, ref, t32, pooled)
            if not pooled:                                             # the rest of the batch is unaffected, bit for bit
                rest = torch.ones(case[0], dtype=torch.bool, device="cuda")
                rest[touched] = False
                assert torch.equal(got[0][:, rest], clean[0][:, rest]) and torch.equal(got[1][rest], clean[1][rest])
                assert torch.equal(got[2][:, rest], clean[2][:, rest])


GUARD, SENTINEL = 256, -12345.0


class Guarded:
    """n elements between two runs of GUARD sentinels"""

    def __init__(self, *shape, dtype=torch.float32):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, device="cuda", dtype=dtype)
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def value(self):
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())
        return self.buf[GUARD:GUARD + self.n].reshape(self.shape)


p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)


@pytest.mark.parametrize("case", [CR.CASES[4], CR.CASES[9], CR.CASES[0], CR.CASES[6]], ids=ids)
def test_every_output_is_written_inside_its_bounds(case):
    from explicit_tf2_recommendation_amd._lib import lib
    B, T, E, coefs, order = case
    c = CR.can_case(case)
    feed, inds, iid, fid, gout, gpool = dev_case(case)
    tabs = (C.c_void_p * len(inds))(*[t.data_ptr() for t in inds])
    head = (p(feed), feed.stride(0), feed.shape[0], E, tabs, 0, inds[0].stride(0), inds[0].shape[0], len(coefs),
            (C.c_int * len(coefs))(*coefs), order, CODE["tanh"], p(iid), p(fid), B, T, CR.PAD)
    out, pool, flag = Guarded(order, B, T, c["Eo"]), Guarded(B, c["Eo"]), Guarded(1, dtype=torch.int32)
    gfeed, gind, gfeed_p, gind_p = Guarded(B, T, E), Guarded(order, B, c["P"]), Guarded(B, T, E), Guarded(order, B, c["P"])
    flag.buf[GUARD] = 0
    assert lib.rec_can_fwd_f32(*head, out.ptr, None, flag.ptr, stream()) == 0
    assert lib.rec_can_fwd_f32(*head, None, pool.ptr, flag.ptr, stream()) == 0
    assert lib.rec_can_bwd_f32(*head, p(gout), None, gfeed.ptr, gind.ptr, stream()) == 0
    assert lib.rec_can_bwd_f32(*head, None, p(gpool), gfeed_p.ptr, gind_p.ptr, stream()) == 0
    torch.cuda.synchronize()
    assert int(flag.value().item()) == 0
    for got, want in zip((out, gfeed, gind), run(case)):
        assert torch.equal(got.value(), want)
    for got, want in zip((pool, gfeed_p, gind_p), run(case, pooled=True)):
        assert torch.equal(got.value(), want)


def test_every_output_is_bit_identical_run_to_run_and_under_graph_replay():
    from explicit_tf2_recommendation_amd import engine
    for case in (CR.CASES[10], CR.CASES[9], CR.CASES[3]):
        for pooled in (False, True):
            first = run(case, pooled=pooled)
            for a, b in zip(first, run(case, pooled=pooled)):
                assert torch.equal(a, b)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with engine._capture(graph):                                # the project's capture policy
                captured = run(case, pooled=pooled)
            for t in captured:
                t.fill_(SENTINEL)
            graph.replay()
            graph.replay()
            torch.cuda.synchronize()
            for a, b in zip(first, captured):
                assert torch.equal(a, b)


def test_wide_segment_sum_adds_the_rows_of_an_id_in_one_launch():
    """rows of 816 and 8320 columns under plans with short runs, one run of the whole list and row_div"""
    from explicit_tf2_recommendation_amd import ops
    r = np.random.default_rng(4)
    for n, V, E, row_div in ((300, 7, 816, 1), (33, 97, 8320, 1), (257, 1, 816, 1), (90, 11, 260, 3)):
        ids = r.integers(0, V, n).astype(np.int64)
        vals = CR.f32_exact(r.normal(0, 1, (n // row_div, E)))
        plan = ops.DedupPlan(cu(ids, np.int64), V)
        got = plan.segment_sum(cu(vals), E, row_div, wide=True)
        sliced = plan.segment_sum(cu(vals), E, row_div)
        want = np.zeros((n, E))
        uniq = np.unique(ids)
        for k, u in enumerate(uniq):
            want[k] = vals[np.nonzero(ids == u)[0] // row_div].sum(0)
        assert tuple(got.shape) == (n, E) and int(plan.n_uniq.item()) == len(uniq)
        assert CR.rel_err(host(got), want) <= 1e-6 and CR.rel_err(host(sliced), want) <= 1e-6
        assert not got[len(uniq):].any()
        assert torch.equal(got, plan.segment_sum(cu(vals), E, row_div, wide=True))


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    z = lambda *s: torch.zeros(*s, device="cuda")
    zi = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
    case = CR.CASES[1]
    feed, inds, iid, fid, gout, gpool = dev_case(case)
    args = lambda **kw: [kw.get(k, v) for k, v in (("feed", feed), ("inds", inds), ("iid", iid), ("fid", fid))] + \
        [kw.get("coefs", case[3]), kw.get("order", 3), 3]
    with pytest.raises(RuntimeError):
        ops.can_fwd(*args(feed=feed.cpu()))                                      # no CPU fallback
    with pytest.raises(TypeError):
        ops.can_fwd(*args(fid=fid.int()))
    with pytest.raises(ValueError):
        ops.can_fwd(*args(inds=tuple(t[:, :59] for t in inds)))                  # not P columns
    with pytest.raises(ValueError):
        ops.can_fwd(*args(inds=inds[:2]))                                        # neither one table nor one per order
    with pytest.raises(ValueError):
        ops.can_fwd(*args(iid=iid[:2]))
    with pytest.raises(ValueError):
        ops.can_bwd(*args(), gout[:, :, :, :3].contiguous())
    with pytest.raises(ValueError):
        ops.can_bwd(*args(), gout, pooled=True)
    # unsupported shapes raise before anything is launched: the flag stays clear and no output exists
    flag = ops.new_flag("cuda")
    with pytest.raises(NotImplementedError):
        ops.can_fwd(z(10, 16), [z(10, 816)] * 3, zi(2), zi(2, 277), (1, 1, 1), 3, 3, oob=flag)   # T beyond the LDS fit
    with pytest.raises(NotImplementedError):
        ops.can_fwd(z(10, 16), [z(10, 16 * 80 + 80)] * 2, zi(2), zi(2, 3), (5,), 2, 3, oob=flag)  # a layer of 80 columns
    with pytest.raises(NotImplementedError):
        ops.can_fwd(z(10, 4), [z(10, 20)] * 5, zi(2), zi(2, 3), (1,), 5, 3, oob=flag)             # order 5
    with pytest.raises(NotImplementedError):
        ops.can_bwd(z(10, 64), [z(10, 8320)] * 2, zi(2), zi(2, 66), (1, 1), 2, 3, z(2, 2, 66, 64))
    assert int(flag.item()) == 0
    out = ops.can_fwd(*args(iid=iid[:0], fid=fid[:0]))
    pool = ops.can_fwd(*args(iid=iid[:0], fid=fid[:0]), pooled=True)
    gfeed, gind = ops.can_bwd(*args(iid=iid[:0], fid=fid[:0]), gout[:, :0])
    assert tuple(out.shape) == (3, 0, 5, 4) and tuple(pool.shape) == (0, 4)
    assert tuple(gfeed.shape) == (0, 5, 4) and tuple(gind.shape) == (3, 0, 60)


# ---- the layer -----------------------------------------------------------------------------------------------------------
def _layer(case, order_independent=True, activation="tanh"):
    from explicit_tf2_recommendation_amd import layers
    B, T, E, coefs, order = case
    sd = CR.layer_state(case, order_independent)
    lay = layers.CoActionUnit(CR.V_CASE, CR.V_CASE, E, list(coefs), order, order_independent, activation).cuda()
    lay.load_state_dict({k: torch.from_numpy(np.asarray(v, F32)) for k, v in sd.items()})
    return lay, sd


def _grads(lay):
    out = {}
    for k, q in lay.named_parameters():
        assert q.grad is not None and q.grad.is_sparse, k
        out[k] = host(q.grad.to_dense())
        q.grad = None
    return out


def check_layer(case, order_independent=True, same_item=False):
    lay, sd = _layer(case, order_independent)
    ins = CR.layer_inputs(case, same_item=same_item)
    gouts, gpool = CR.layer_upstream(case)
    B, T, E, coefs, order = case
    kw = dict(order_independent=order_independent)
    t64, t32 = (CR.layer_torch(sd, case, ins, dt, gouts, **kw) for dt in (torch.float64, torch.float32))
    dev_ins = [cu(a, np.int64) for a in ins]
    outs = lay(dev_ins)
    assert isinstance(outs, list) and len(outs) == order
    for i, o in enumerate(outs):
        assert tuple(o.shape) == ((B, 16) if T == 0 else (B, T, 16))
        check("output %d" % i, host(o), t64["outputs"][i], t32["outputs"][i], 1e-5)
    sum((o * cu(g)).sum() for o, g in zip(outs, gouts)).backward()
    grads = _grads(lay)
    assert grads.keys() == t64["grads"].keys() and len(grads) == 1 + (order if order_independent else 1)
    for k in grads:
        check(k[:22], grads[k], t64["grads"][k], t32["grads"][k], 3e-5)
    p64, p32 = (CR.layer_torch(sd, case, ins, dt, None, gpool, **kw) for dt in (torch.float64, torch.float32))
    pooled = lay.pooled(dev_ins)
    assert tuple(pooled.shape) == (B, 16)
    check("pooled", host(pooled), p64["pooled"], p32["pooled"], 1e-5)
    (pooled * cu(gpool)).sum().backward()
    grads = _grads(lay)
    for k in grads:
        check("p " + k[:20], grads[k], p64["grads"][k], p32["grads"][k], 3e-5)


@pytest.mark.parametrize("case", CR.LAYER_CASES, ids=ids)
def test_layer_parity_with_the_torch_cpu_transcription(case):
    check_layer(case)


def test_layer_with_one_shared_table():
    check_layer(CR.CASES[2], order_independent=False)


def test_layer_with_one_target_item_for_the_whole_batch():
    check_layer(CR.CASES[2], same_item=True)


def test_out_of_range_id_raises():
    lay, _ = _layer(CR.CASES[2])
    iid, fid = (cu(a, np.int64) for a in CR.layer_inputs(CR.CASES[2]))
    lay([iid, fid])
    for bad_i, bad_f in ((CR.V_CASE, None), (-1, None), (None, CR.V_CASE), (None, -2)):
        i, f = iid.clone(), fid.clone()
        if bad_i is not None:
            i[4, 0] = bad_i
        else:
            f[4, 1] = bad_f
        with pytest.raises(IndexError):
            lay([i, f])
        with pytest.raises(IndexError):
            lay.pooled([i, f])


def test_one_graphed_train_step_over_pooled_leaves_the_tables_of_the_eager_step():
    from explicit_tf2_recommendation_amd import engine
    case = CR.CASES[3]
    lay, _ = _layer(case)
    eager = copy.deepcopy(lay)
    iid, fid = (cu(a, np.int64) for a in CR.layer_inputs(case))
    w = cu(CR.layer_upstream(case)[1])
    batch = {"iid": iid, "fid": fid, "label": torch.zeros(case[0], 1, device="cuda")}   # a dummy: the loss is a weighting
    step = engine.GraphedTrainStep(lay, batch, label_name="label", output_fn=lambda l, x: l.pooled([x["iid"], x["fid"]]),
                                   loss_fn=lambda out, y: (out * w).sum())
    loss = step(batch)
    want = (eager.pooled([iid, fid]) * w).sum()
    want.backward()
    assert torch.equal(loss.reshape(()), want.detach())
    for model in (lay, eager):
        torch.optim.SGD(model.parameters(), lr=0.1).step()
    for (name, a), b in zip(lay.named_parameters(), eager.parameters()):
        assert torch.equal(a.grad._indices(), b.grad._indices()) and torch.equal(a.grad._values(), b.grad._values()), name
        assert torch.equal(a, b), name
    assert not torch.equal(lay.feed_embedding.embeddings, cu(CR.layer_state(case)["feed_embedding.embeddings"]))


def test_unsupported_layer_shapes_raise_before_anything_is_launched():
    from explicit_tf2_recommendation_amd import layers
    with pytest.raises(NotImplementedError):
        layers.CoActionUnit(10, 10, 16, [5])
    with pytest.raises(NotImplementedError):
        layers.CoActionUnit(10, 10, 16, order=5)
    lay = layers.CoActionUnit(10, 10, 16).cuda()
    with pytest.raises(NotImplementedError):
        lay([torch.zeros(2, dtype=torch.int64), torch.ones(2, 277, dtype=torch.int64)])
    out = lay([torch.zeros(2, dtype=torch.int64), torch.ones(2, 276, dtype=torch.int64)])
    assert len(out) == 3 and tuple(out[0].shape) == (2, 276, 16) and bool(torch.isfinite(out[2]).all())
