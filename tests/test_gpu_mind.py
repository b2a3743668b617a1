"""MIND on the GPU: the capsule-routing and label-aware-attention kernels (csrc/mind.hip) against the fp64 numpy reading
of tests/mind_ref.py, strided tables, out-of-range ids, guard buffers, bit identity run to run, the layers against the
torch-CPU transcription in training and evaluation mode, graph capture and the error paths.

Tolerance, per tensor (the project's rule, as tests/test_gpu_mmoe.py restates it): max|got - want| / max|want| against
fp64 must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors)
/ 3e-5 (gradients).  The bodies have no kink: no example is excluded from them.  The final MLP of the layer has a ReLU:
an example whose smallest |pre-activation| in fp64 is below PRE_EPS = 1e-5 would have its upstream gradient row zeroed on
both sides and such examples may be at most 10 % of the batch; the seed of a layer case is the first of 1, 2, 3, ... with
none of them, chosen on the fp64 reading alone (tests/test_mind_host.py checks that choice without a GPU), so no row is
zeroed.

Measured on the MI355X: the first run's printout, `name error / bound`; the four layer cases check 17 tensors each and are
given as a DIGEST (the capsules, the output, the loss and the three largest error / bound ratios of the gradients).
46 passed in 3.8 s.
  routing (1, 1, 1, 1, 1, 1, 1): out 1.25e-07 / 1.00e-05; gkeys 1.22e-07 / 3.00e-05; dS 1.48e-07 / 3.00e-05
  routing (3, 5, 1, 8, 8, 4, 3): out 9.09e-08 / 1.00e-05; gkeys 2.02e-07 / 3.00e-05; dS 6.15e-08 / 3.00e-05
  routing (33, 6, 3, 16, 48, 4, 3): out 4.96e-07 / 1.00e-05; gkeys 3.38e-07 / 3.00e-05; dS 5.75e-07 / 3.00e-05
  routing (33, 50, 3, 16, 48, 4, 3): out 7.62e-07 / 1.00e-05; gkeys 3.75e-07 / 3.00e-05; dS 2.88e-07 / 3.00e-05
  routing (33, 65, 3, 8, 40, 16, 3): out 3.79e-07 / 1.00e-05; gkeys 3.22e-07 / 3.00e-05; dS 2.61e-07 / 3.00e-05
  routing (17, 6, 3, 16, 48, 4, 1): out 1.94e-07 / 1.00e-05; gkeys 1.35e-07 / 3.00e-05; dS 9.01e-08 / 3.00e-05
  routing (17, 6, 3, 16, 48, 4, 5): out 6.19e-07 / 1.00e-05; gkeys 1.78e-06 / 3.76e-05; dS 9.00e-07 / 3.00e-05
  routing (17, 33, 3, 16, 48, 1, 3): out 6.77e-07 / 1.00e-05; gkeys 1.08e-06 / 3.00e-05; dS 5.05e-07 / 3.00e-05
  routing (5, 33, 4, 64, 256, 16, 3): out 9.60e-06 / 1.17e-05; gkeys 6.01e-06 / 3.00e-05; dS 4.00e-06 / 3.00e-05
  routing (2049, 50, 3, 16, 48, 4, 3): out 1.62e-06 / 1.00e-05; gkeys 7.60e-07 / 3.00e-05; dS 3.10e-07 / 3.00e-05
  attention (1, 1, 1, 1, 1), gout: out 2.81e-08 / 1.00e-05; loss 0.00e+00 / 1.00e-05; gm 3.09e-08 / 3.00e-05; gitems
    2.16e-09 / 3.00e-05
  attention (3, 2, 1, 8, 4), gout: out 7.12e-08 / 1.00e-05; loss 5.38e-08 / 1.00e-05; gm 6.15e-08 / 3.00e-05; gitems
    7.75e-08 / 3.00e-05
  attention (33, 11, 3, 16, 4), gout: out 1.72e-07 / 1.00e-05; loss 1.30e-07 / 1.00e-05; gm 1.41e-07 / 3.00e-05;
    gitems 3.19e-07 / 3.00e-05
  attention (33, 65, 3, 16, 16), gout: out 3.44e-07 / 1.00e-05; loss 1.09e-07 / 1.00e-05; gm 2.07e-07 / 3.00e-05;
    gitems 5.85e-07 / 3.00e-05
  attention (5, 33, 4, 64, 16), gout: out 3.31e-07 / 1.00e-05; loss 3.03e-07 / 1.00e-05; gm 4.33e-07 / 3.00e-05;
    gitems 8.76e-07 / 3.00e-05
  attention (2049, 11, 3, 16, 4), gout: out 3.08e-07 / 1.00e-05; loss 1.79e-07 / 1.00e-05; gm 2.89e-07 / 3.00e-05;
    gitems 4.55e-07 / 3.00e-05
  attention (1, 1, 1, 1, 1), gloss: out 2.81e-08 / 1.00e-05; loss 0.00e+00 / 1.00e-05; gm 0.00e+00 / 3.00e-05; gitems
    0.00e+00 / 3.00e-05
  attention (3, 2, 1, 8, 4), gloss: out 7.12e-08 / 1.00e-05; loss 5.38e-08 / 1.00e-05; gm 2.15e-07 / 3.00e-05; gitems
    1.31e-07 / 3.00e-05
  attention (33, 11, 3, 16, 4), gloss: out 1.72e-07 / 1.00e-05; loss 1.30e-07 / 1.00e-05; gm 2.03e-07 / 3.00e-05;
    gitems 2.94e-07 / 3.00e-05
  attention (33, 65, 3, 16, 16), gloss: out 3.44e-07 / 1.00e-05; loss 1.09e-07 / 1.00e-05; gm 3.75e-07 / 3.00e-05;
    gitems 2.91e-07 / 3.00e-05
  attention (5, 33, 4, 64, 16), gloss: out 3.31e-07 / 1.00e-05; loss 3.03e-07 / 1.00e-05; gm 1.28e-06 / 3.00e-05;
    gitems 8.69e-07 / 3.00e-05
  attention (2049, 11, 3, 16, 4), gloss: out 3.08e-07 / 1.00e-05; loss 1.79e-07 / 1.00e-05; gm 4.70e-07 / 3.00e-05;
    gitems 4.58e-07 / 3.00e-05
  attention (1, 1, 1, 1, 1), both: out 2.81e-08 / 1.00e-05; loss 0.00e+00 / 1.00e-05; gm 3.09e-08 / 3.00e-05; gitems
    2.16e-09 / 3.00e-05
  attention (3, 2, 1, 8, 4), both: out 7.12e-08 / 1.00e-05; loss 5.38e-08 / 1.00e-05; gm 9.59e-08 / 3.00e-05; gitems
    6.17e-08 / 3.00e-05
  attention (33, 11, 3, 16, 4), both: out 1.72e-07 / 1.00e-05; loss 1.30e-07 / 1.00e-05; gm 1.37e-07 / 3.00e-05;
    gitems 2.32e-07 / 3.00e-05
  attention (33, 65, 3, 16, 16), both: out 3.44e-07 / 1.00e-05; loss 1.09e-07 / 1.00e-05; gm 2.51e-07 / 3.00e-05;
    gitems 6.22e-07 / 3.00e-05
  attention (5, 33, 4, 64, 16), both: out 3.31e-07 / 1.00e-05; loss 3.03e-07 / 1.00e-05; gm 4.51e-07 / 3.00e-05;
    gitems 7.09e-07 / 3.00e-05
  attention (2049, 11, 3, 16, 4), both: out 3.08e-07 / 1.00e-05; loss 1.79e-07 / 1.00e-05; gm 3.29e-07 / 3.00e-05;
    gitems 4.74e-07 / 3.00e-05
  out-of-range ids, routing (33, 6, 3, 16, 48, 4, 3): out 4.96e-07 / 1.00e-05; gkeys 3.68e-07 / 3.00e-05; dS 3.30e-07
    / 3.00e-05
  out-of-range ids, attention (33, 11, 3, 16, 4): out 1.72e-07 / 1.00e-05; loss 1.30e-07 / 1.00e-05; gm 1.37e-07 /
    3.00e-05; gitems 2.32e-07 / 3.00e-05
  MINDLayer, B = 32, T = 6, train (digest): capsules 4.82e-07 / 1.00e-05; output 4.43e-07 / 1.00e-05; loss 1.61e-07 /
    1.00e-05; 14 gradients, the largest ratios: context_mlp.bias 2.42e-06 / 3.00e-05; embed.embeddings 5.83e-07 /
    3.00e-05; MIE_layer.S 5.54e-07 / 3.00e-05
  MINDLayer, B = 32, T = 50, train (digest): capsules 4.17e-07 / 1.00e-05; output 3.24e-07 / 1.00e-05; loss 1.86e-07 /
    1.00e-05; 14 gradients, the largest ratios: context_mlp.bias 1.94e-06 / 3.00e-05; final_mlp.layers.3.kernel
    5.57e-07 / 3.00e-05; context_bn.gamma 5.04e-07 / 3.00e-05
  MINDLayer, B = 32, T = 6, eval (digest): capsules 5.17e-07 / 1.00e-05; output 3.36e-07 / 1.00e-05; loss 2.01e-07 /
    1.00e-05; 14 gradients, the largest ratios: embed.embeddings 6.31e-07 / 3.00e-05; MIE_layer.S 4.09e-07 / 3.00e-05;
    context_mlp.kernel 3.85e-07 / 3.00e-05
  MINDLayer, B = 32, T = 50, eval (digest): capsules 4.71e-07 / 1.00e-05; output 2.01e-07 / 1.00e-05; loss 1.23e-07 /
    1.00e-05; 14 gradients, the largest ratios: final_mlp.layers.3.kernel 4.80e-07 / 3.00e-05; context_bn.gamma
    4.58e-07 / 3.00e-05; context_mlp.kernel 4.29e-07 / 3.00e-05
  MultiInterestExtractorLayer, B = 32, T = 6: out 1.04e-06 / 1.00e-05; S.grad 6.00e-07 / 3.00e-05; table.grad 7.30e-07
    / 3.00e-05
  MultiInterestExtractorLayer, B = 32, T = 50: out 3.40e-07 / 1.00e-05; S.grad 3.13e-07 / 3.00e-05; table.grad
    5.69e-07 / 3.00e-05
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import mind_ref as MR

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = lambda c: "x".join(map(str, c))


def cu(a, dtype=F32):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def host(t):
    return t.detach().cpu().numpy()


def check(name, got, want, t32, floor):
    err, bound = MR.rel_err(got, want), max(floor, 4 * MR.rel_err(t32, want))
    print("%-12s error/bound %.2e / %.2e = %.2f" % (name, err, bound, err / bound))
    if not np.any(want):
        assert not np.any(got), (name, "zero throughout in fp64: must be exact")
    assert err <= bound, (name, err, bound)


# ---- bodies -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dev_routing(*case):
    c = MR.routing_case(*case)
    return cu(c["table"]), cu(c["series"], np.int64), cu(c["S"]), cu(c["B0"]), cu(c["gout"])


def run_routing(case, table=None, series=None, oob=None):
    from explicit_tf2_recommendation_amd import ops
    tab, ser, S, B0, gout = dev_routing(*case)
    tab = tab if table is None else table
    ser = ser if series is None else series
    out = ops.mind_routing_fwd(tab, ser, S, B0, case[6], 0, oob)
    gkeys, dS = ops.mind_routing_bwd(tab, ser, S, B0, gout, case[6], 0)
    return out, gkeys, dS


@functools.lru_cache(maxsize=None)
def dev_laa(*case):
    c = MR.laa_case(*case)
    return cu(c["table"]), cu(c["items"], np.int64), cu(c["m"]), cu(c["kv"], np.int32), cu(c["gout"]), cu(c["gloss"])


def run_laa(case, way="both", table=None, items=None, oob=None):
    from explicit_tf2_recommendation_amd import ops
    tab, it, m, kv, gout, gloss = dev_laa(*case)
    tab = tab if table is None else table
    it = it if items is None else items
    use_out, use_loss = MR.LAA_WAYS[way]
    out, loss = ops.mind_laa_fwd(tab, it, m, kv, oob)
    gm, gitems = ops.mind_laa_bwd(tab, it, m, kv, gout if use_out else None, gloss if use_loss else None)
    return out, loss, gm, gitems


@pytest.mark.parametrize("case", MR.ROUTING_CASES, ids=ids)
def test_routing_matches_fp64(case):
    c, t32 = MR.routing_case(*case), MR.routing_case_t(case, torch.float32)
    out, gkeys, dS = run_routing(case)
    assert tuple(out.shape) == (case[0], case[5], case[4]) and tuple(dS.shape) == (case[2] * case[3], case[4])
    check("out", host(out), c["ref"]["out"], t32["out"], 1e-5)
    check("gkeys", host(gkeys), c["ref"]["gkeys"], t32["gkeys"], 3e-5)
    check("dS", host(dS), c["ref"]["dS"], t32["dS"], 3e-5)


@pytest.mark.parametrize("case", MR.LAA_CASES, ids=ids)
@pytest.mark.parametrize("way", list(MR.LAA_WAYS))
def test_attention_matches_fp64(case, way):
    c = MR.laa_case(*case)
    gout, gloss = MR.laa_way(c, way)
    ref = MR.laa_numpy(c["table"], c["items"], c["m"], c["kv"], gout, gloss)
    t32 = MR.laa_torch_grads(c["table"], c["items"], c["m"], c["kv"], gout, gloss, torch.float32)
    out, loss, gm, gitems = run_laa(case, way)
    for name, got, floor in (("out", out, 1e-5), ("loss", loss, 1e-5), ("gm", gm, 3e-5), ("gitems", gitems, 3e-5)):
        check(name, host(got), ref[name], t32[name], floor)


def _strided(table, pad=3):
    wide = torch.full((table.shape[0], table.shape[1] + pad), 7.0, device="cuda")
    wide[:, :table.shape[1]] = table
    view = wide[:, :table.shape[1]]
    assert view.stride(0) == table.shape[1] + pad
    return view


def test_strided_table_is_bit_identical_to_the_packed_one():
    rc, lc = (33, 65, 3, 8, 40, 16, 3), (33, 11, 3, 16, 4)
    for a, b in zip(run_routing(rc), run_routing(rc, table=_strided(dev_routing(*rc)[0]))):
        assert torch.equal(a, b)
    for a, b in zip(run_laa(lc), run_laa(lc, table=_strided(dev_laa(*lc)[0]))):
        assert torch.equal(a, b)


def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows():
    from explicit_tf2_recommendation_amd import ops
    rc, lc = (33, 6, 3, 16, 48, 4, 3), (33, 11, 3, 16, 4)
    c = MR.routing_case(*rc)
    flag = ops.new_flag("cuda")
    run_routing(rc, oob=flag)
    assert int(flag.item()) == 0
    series = c["series"].copy()
    series[5, 2, 1], series[7, 0, 0], series[9, 3, 2] = -1, MR.V_CASE, 2 ** 40        # (a first-feature id too: valid, zero row)
    ref = MR.routing_numpy(c["table"], series, c["S"], c["B0"], rc[6], 0, c["gout"])
    t32 = MR.routing_torch_grads(c["table"], series, c["S"], c["B0"], rc[6], c["gout"], torch.float32)
    out, gkeys, dS = run_routing(rc, series=cu(series, np.int64), oob=flag)
    assert int(flag.item()) == 1
    check("out", host(out), ref["out"], t32["out"], 1e-5)
    check("gkeys", host(gkeys), ref["gkeys"], t32["gkeys"], 3e-5)
    check("dS", host(dS), ref["dS"], t32["dS"], 3e-5)
    c = MR.laa_case(*lc)
    flag = ops.new_flag("cuda")
    run_laa(lc, oob=flag)
    assert int(flag.item()) == 0
    items = c["items"].copy()
    items[4, 0, 0], items[6, 10, 2], items[8, 3, 1] = -5, MR.V_CASE, 2 ** 40
    ref = MR.laa_numpy(c["table"], items, c["m"], c["kv"], c["gout"], c["gloss"])
    t32 = MR.laa_torch_grads(c["table"], items, c["m"], c["kv"], c["gout"], c["gloss"], torch.float32)
    out, loss, gm, gitems = run_laa(lc, items=cu(items, np.int64), oob=flag)
    assert int(flag.item()) == 1
    for name, got, floor in (("out", out, 1e-5), ("loss", loss, 1e-5), ("gm", gm, 3e-5), ("gitems", gitems, 3e-5)):
        check(name, host(got), ref[name], t32[name], floor)


GUARD, SENTINEL = 256, -12345.0


class Guarded:
    """n floats between two runs of GUARD sentinels"""

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * GUARD,), SENTINEL, device="cuda")
        self.ptr = C.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def value(self):
        assert bool((self.buf[:GUARD] == SENTINEL).all()) and bool((self.buf[GUARD + self.n:] == SENTINEL).all())
        return self.buf[GUARD:GUARD + self.n].reshape(self.shape)


@pytest.mark.parametrize("case", [(33, 65, 3, 8, 40, 16, 3), (5, 33, 4, 64, 256, 16, 3), (3, 5, 1, 8, 8, 4, 3)], ids=ids)
def test_routing_writes_inside_its_outputs(case):
    from explicit_tf2_recommendation_amd._lib import lib
    B, T, Cn, E, Dc, K, R = case
    tab, ser, S, B0, gout = dev_routing(*case)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, gkeys, dS = Guarded(B, K, Dc), Guarded(B, T, Cn * E), Guarded(Cn * E, Dc)
    nbytes = lib.rec_mind_routing_workspace_bytes(B, T, E, Cn, Dc, K, R)
    ws = Guarded(nbytes // 4)
    head = (p(tab), tab.stride(0), tab.shape[0], E, Cn, p(ser), B, T, p(S), p(B0), Dc, K, R, 0)
    assert lib.rec_mind_routing_fwd_f32(*head, out.ptr, None, st) == 0
    assert lib.rec_mind_routing_bwd_f32(*head, p(gout), gkeys.ptr, dS.ptr, ws.ptr, nbytes, st) == 0
    torch.cuda.synchronize()
    ws.value()
    for got, want in zip((out, gkeys, dS), run_routing(case)):
        assert torch.equal(got.value(), want)


@pytest.mark.parametrize("case", [(33, 65, 3, 16, 16), (5, 33, 4, 64, 16), (3, 2, 1, 8, 4)], ids=ids)
def test_attention_writes_inside_its_outputs(case):
    from explicit_tf2_recommendation_amd._lib import lib
    B, Ns, Cn, E, K = case
    tab, it, m, kv, gout, gloss = dev_laa(*case)
    p = lambda t: C.c_void_p(t.data_ptr())
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out, loss, gm, gitems = Guarded(B, Ns), Guarded(B), Guarded(B, K, Cn * E), Guarded(B, Ns, Cn * E)
    head = (p(tab), tab.stride(0), tab.shape[0], E, Cn, p(it), B, Ns, p(m), p(kv), K)
    assert lib.rec_mind_laa_fwd_f32(*head, out.ptr, loss.ptr, None, st) == 0
    assert lib.rec_mind_laa_bwd_f32(*head, p(gout), p(gloss), gm.ptr, gitems.ptr, st) == 0
    torch.cuda.synchronize()
    for got, want in zip((out, loss, gm, gitems), run_laa(case)):
        assert torch.equal(got.value(), want)


def test_every_output_is_bit_identical_run_to_run():
    for case in ((2049, 50, 3, 16, 48, 4, 3), (5, 33, 4, 64, 256, 16, 3)):
        for a, b in zip(run_routing(case), run_routing(case)):
            assert torch.equal(a, b)
    for a, b in zip(run_laa((2049, 11, 3, 16, 4)), run_laa((2049, 11, 3, 16, 4))):
        assert torch.equal(a, b)


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    tab, ser, S, B0, gout = dev_routing(3, 5, 1, 8, 8, 4, 3)
    with pytest.raises(RuntimeError):
        ops.mind_routing_fwd(tab.cpu(), ser, S, B0)                           # no CPU fallback
    with pytest.raises(TypeError):
        ops.mind_routing_fwd(tab, ser.int(), S, B0)
    with pytest.raises(ValueError):
        ops.mind_routing_fwd(tab, ser, S[:7].contiguous(), B0)
    with pytest.raises(ValueError):
        ops.mind_routing_fwd(tab, ser, S, B0[:, :4].contiguous())
    with pytest.raises(ValueError):
        ops.mind_routing_bwd(tab, ser, S, B0, gout[:, :3].contiguous())
    with pytest.raises(NotImplementedError):
        ops.mind_routing_fwd(tab, ser, S, B0, routing_rounds=9)
    z = lambda *s: torch.zeros(*s, device="cuda")
    with pytest.raises(NotImplementedError):                                  # T beyond the LDS fit
        ops.mind_routing_fwd(z(10, 16), torch.zeros(2, 227, 3, dtype=torch.int64, device="cuda"), z(48, 48), z(4, 227))
    out = ops.mind_routing_fwd(tab, ser[:0], S, B0)
    gk, dS = ops.mind_routing_bwd(tab, ser[:0], S, B0, gout[:0])
    assert tuple(out.shape) == (0, 4, 8) and tuple(gk.shape) == (0, 5, 8) and float(dS.abs().sum()) == 0
    tab, it, m, kv, gout, gloss = dev_laa(3, 2, 1, 8, 4)
    with pytest.raises(RuntimeError):
        ops.mind_laa_fwd(tab, it, m.cpu(), kv)
    with pytest.raises(TypeError):
        ops.mind_laa_fwd(tab, it, m, kv.long())
    with pytest.raises(ValueError):
        ops.mind_laa_fwd(tab, it, m[:, :, :7].contiguous(), kv)
    with pytest.raises(ValueError):
        ops.mind_laa_bwd(tab, it, m, kv, gout[:, :1].contiguous())
    gm, gi = ops.mind_laa_bwd(tab, it, m, kv)                                # neither gradient: zeros
    assert float(gm.abs().sum()) == 0 and float(gi.abs().sum()) == 0
    out, loss = ops.mind_laa_fwd(tab, it[:0], m[:0], kv[:0])
    gm, gi = ops.mind_laa_bwd(tab, it[:0], m[:0], kv[:0], gout[:0], gloss[:0])
    assert tuple(out.shape) == (0, 2) and tuple(loss.shape) == (0,) and tuple(gm.shape) == (0, 4, 8)


# ---- layers ---------------------------------------------------------------------------------------------------------
def _layer(seed, T, training):
    from explicit_tf2_recommendation_amd import layers
    sd = MR.layer_state(seed, T)
    lay = layers.MINDLayer(feature_dims=MR.LAYER_V, seq_length=T).cuda()
    lay.load_state_dict({k: torch.from_numpy(np.asarray(v, F32)) for k, v in sd.items()})
    lay.train(training)
    return lay, sd


def _grads(lay):
    return {k: host(p.grad.to_dense() if p.grad.is_sparse else p.grad) for k, p in lay.named_parameters()}


@pytest.mark.parametrize("T", MR.LAYER_TS)
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_layer_parity_with_the_torch_cpu_transcription(T, training):
    from explicit_tf2_recommendation_amd import data
    seed = MR.layer_seed(T, training)
    lay, sd = _layer(seed, T, training)
    ins = MR.layer_inputs(seed, MR.LAYER_B, T)
    gout, gloss = MR.layer_upstream(seed)
    t64 = MR.layer_torch(sd, ins, torch.float64, training, gout, gloss)
    t32 = MR.layer_torch(sd, ins, torch.float32, training, gout, gloss)
    near = t64["pre"] < MR.PRE_EPS
    assert near.mean() <= 0.10 and not near.any()                             # so no upstream row is zeroed
    batch = data.to_device(ins)
    mlped, mask, kv = lay.generate_interest_capsules(batch)
    check("capsules", host(mlped), t64["mlped"], t32["mlped"], 1e-5)
    assert mask.dtype == torch.bool and np.array_equal(host(mask), t64["mask"])
    assert kv.dtype == torch.int32 and np.array_equal(host(kv), t64["kv"])
    res = lay(batch)
    assert res.keys() == {"output", "loss"}
    assert tuple(res["output"].shape) == (MR.LAYER_B, MR.LAYER_NS) and tuple(res["loss"].shape) == (MR.LAYER_B,)
    check("output", host(res["output"]), t64["output"], t32["output"], 1e-5)
    check("loss", host(res["loss"]), t64["loss"], t32["loss"], 1e-5)
    ((res["output"] * cu(gout)).sum() + (res["loss"] * cu(gloss)).sum()).backward()
    grads = _grads(lay)
    assert grads.keys() == t64["grads"].keys() and len(grads) == 14
    for k in grads:
        check(k[-28:], grads[k], t64["grads"][k], t32["grads"][k], 3e-5)
    assert lay.MIE_layer.B.grad is None


@pytest.mark.parametrize("T", MR.LAYER_TS)
def test_extractor_layer_parity(T):
    from explicit_tf2_recommendation_amd import layers
    sd, ins = MR.layer_state(1, T), MR.layer_inputs(1, MR.LAYER_B, T)
    series = np.stack([ins[n] for n in MR.SERIES], axis=2)
    gout = MR.f32_exact(np.random.default_rng(5).uniform(-1, 1, (MR.LAYER_B, MR.LAYER_K, 48)))
    ext = layers.MultiInterestExtractorLayer(MR.LAYER_K, 48)                  # built by the first call
    table = torch.nn.Parameter(cu(sd["embed.embeddings"]))
    out = ext((table, cu(series, np.int64)))
    assert tuple(ext.S.shape) == (48, 48) and tuple(ext.B.shape) == (MR.LAYER_K, T) and ext.S.is_cuda
    with torch.no_grad():
        ext.S.copy_(cu(sd["MIE_layer.S"]))
        ext.B.copy_(cu(sd["MIE_layer.B"]))
    out = ext((table, cu(series, np.int64)))
    (out * cu(gout)).sum().backward()
    ref = MR.routing_numpy(sd["embed.embeddings"], series, sd["MIE_layer.S"], sd["MIE_layer.B"], 3, 0, gout)
    t32 = MR.routing_torch_grads(sd["embed.embeddings"], series, sd["MIE_layer.S"], sd["MIE_layer.B"], 3, gout,
                                 torch.float32)

    def table_grad(gkeys):                                                    # IndexedSlices values -> dense rows
        g = np.zeros_like(sd["embed.embeddings"])
        np.add.at(g, series.reshape(-1), np.asarray(gkeys, np.float64).reshape(-1, MR.LAYER_E))
        return g

    check("out", host(out), ref["out"], t32["out"], 1e-5)
    check("S.grad", host(ext.S.grad), ref["dS"], t32["dS"], 3e-5)
    check("table.grad", host(table.grad.to_dense()), table_grad(ref["gkeys"]), table_grad(t32["gkeys"]), 3e-5)


def test_out_of_range_id_raises():
    from explicit_tf2_recommendation_amd import data
    lay, _ = _layer(1, 6, False)
    ins = MR.layer_inputs(1, MR.LAYER_B, 6)
    lay(data.to_device(ins))
    for name in ("visited_shop_ids", "label_cate_ids", "utag2"):
        bad = {k: v.copy() for k, v in ins.items()}
        bad[name].reshape(-1)[5] = MR.LAYER_V
        with pytest.raises(IndexError):
            lay(data.to_device(bad))


def test_graph_replay_equals_eager_bit_for_bit():
    """Three replays over three batches against an eager copy of the layer, in training mode (the batch normalisation
    folds its moving averages on both sides): losses and every gradient, the table's sparse rows included."""
    from explicit_tf2_recommendation_amd import data, engine
    T = 50
    lay, _ = _layer(1, T, True)
    eager = copy.deepcopy(lay)

    def batch(seed):
        b = data.to_device(MR.layer_inputs(seed, MR.LAYER_B, T))
        b["label"] = torch.zeros(MR.LAYER_B, 1, device="cuda")               # a dummy: the layer carries its own loss
        return b

    batches = [batch(s) for s in (11, 12, 13)]
    step = engine.GraphedTrainStep(lay, batches[0], label_name="label",
                                   output_fn=lambda l, x: l(x)["loss"].sum().reshape(1),
                                   loss_fn=lambda out, y: out.sum())
    for b in batches:
        loss = step(b)
        for p in eager.parameters():
            p.grad = None
        want = eager({k: v for k, v in b.items() if k != "label"})["loss"].sum()
        want.backward()
        assert torch.equal(loss.reshape(()), want.detach())
        for (name, p), q in zip(lay.named_parameters(), eager.parameters()):
            assert p.grad is not None and p.grad.is_sparse == q.grad.is_sparse, name
            if p.grad.is_sparse:
                assert torch.equal(p.grad._indices(), q.grad._indices()), name
                assert torch.equal(p.grad._values(), q.grad._values()), name
            else:
                assert torch.equal(p.grad, q.grad), name
    for (name, a), b in zip(lay.named_buffers(), eager.buffers()):
        assert torch.equal(a, b), name
