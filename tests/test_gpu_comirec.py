"""ComiRec on the GPU: the dynamic-routing, self-attentive and hard-attention kernels (csrc/comirec.hip) against the fp64
numpy reading of tests/comirec_ref.py, strided tables, out-of-range ids, guard buffers, bit identity run to run, the layers
against the torch-CPU transcription in both modes and both mask senses, graph capture and the error paths.

Tolerance, per tensor (the project's rule, as tests/test_gpu_mind.py states it): max|got - want| / max|want| against fp64
must stay within 4 x the error of the fp32 CPU transcription on the same inputs, never below 1e-5 (forward tensors) /
3e-5 (gradients); a tensor that is zero throughout in fp64 must be exactly zero.  The argmax of the hard attention is a
kink: the near-tie examples of a body case (top-two gap below 1e-4 in fp64; at most 10 % of the batch, asserted without
a GPU in tests/test_comirec_host.py) are left out of chosen / inner / loss and have zero upstream gradients on both
sides; on every other example chosen equals the fp64 argmax exactly.  The seed of a layer case is the first with no
near-tie example (gap below 1e-5) at all.

Measured on the MI355X, the first run's printout as a DIGEST (every test prints `name error / bound` for each tensor it
checks; 580 lines in all).  102 passed in 5.0 s.  Per test: the number of tensors checked and the one with the largest
error / bound.
  routing_matches_fp64[1x1x1x1x1x1x1-0]: 3 tensors, largest ratio out 5.37e-08 / 1.00e-05
  routing_matches_fp64[1x1x1x1x1x1x1-1]: 3 tensors, largest ratio out 5.37e-08 / 1.00e-05
  routing_matches_fp64[3x5x1x8x8x4x3-0]: 3 tensors, largest ratio out 1.12e-07 / 1.00e-05
  routing_matches_fp64[3x5x1x8x8x4x3-1]: 3 tensors, largest ratio out 1.55e-07 / 1.00e-05
  routing_matches_fp64[33x6x3x16x48x4x3-0]: 3 tensors, largest ratio out 7.49e-07 / 1.00e-05
  routing_matches_fp64[33x6x3x16x48x4x3-1]: 3 tensors, largest ratio out 4.96e-07 / 1.00e-05
  routing_matches_fp64[33x50x3x16x48x4x3-0]: 3 tensors, largest ratio out 3.95e-07 / 1.00e-05
  routing_matches_fp64[33x50x3x16x48x4x3-1]: 3 tensors, largest ratio out 3.70e-07 / 1.00e-05
  routing_matches_fp64[33x65x3x8x40x16x3-0]: 3 tensors, largest ratio out 2.77e-07 / 1.00e-05
  routing_matches_fp64[33x65x3x8x40x16x3-1]: 3 tensors, largest ratio out 2.35e-07 / 1.00e-05
  routing_matches_fp64[17x6x3x16x48x4x1-0]: 3 tensors, largest ratio out 1.63e-07 / 1.00e-05
  routing_matches_fp64[17x6x3x16x48x4x1-1]: 3 tensors, largest ratio out 1.87e-07 / 1.00e-05
  routing_matches_fp64[17x6x3x16x48x4x5-0]: 3 tensors, largest ratio out 4.86e-06 / 1.74e-05
  routing_matches_fp64[17x6x3x16x48x4x5-1]: 3 tensors, largest ratio out 1.73e-06 / 1.00e-05
  routing_matches_fp64[17x33x3x16x48x1x3-0]: 3 tensors, largest ratio out 3.64e-07 / 1.00e-05
  routing_matches_fp64[17x33x3x16x48x1x3-1]: 3 tensors, largest ratio out 8.09e-07 / 1.00e-05
  routing_matches_fp64[5x9x4x64x256x16x3-0]: 3 tensors, largest ratio out 5.61e-06 / 1.00e-05
  routing_matches_fp64[5x9x4x64x256x16x3-1]: 3 tensors, largest ratio out 6.52e-06 / 1.00e-05
  routing_matches_fp64[2049x10x3x16x48x4x3-0]: 3 tensors, largest ratio out 1.28e-06 / 1.00e-05
  routing_matches_fp64[2049x10x3x16x48x4x3-1]: 3 tensors, largest ratio out 9.83e-07 / 1.00e-05
  self_attention_matches_fp64[1x1x1x1x1x1-0-pos]: 4 tensors, largest ratio out 1.87e-08 / 1.00e-05
  self_attention_matches_fp64[1x1x1x1x1x1-0-nopos]: 4 tensors, largest ratio out 1.87e-08 / 1.00e-05
  self_attention_matches_fp64[1x1x1x1x1x1-1-pos]: 4 tensors, largest ratio out 1.87e-08 / 1.00e-05
  self_attention_matches_fp64[1x1x1x1x1x1-1-nopos]: 4 tensors, largest ratio out 1.87e-08 / 1.00e-05
  self_attention_matches_fp64[3x5x1x8x8x4-0-pos]: 4 tensors, largest ratio out 1.17e-07 / 1.00e-05
  self_attention_matches_fp64[3x5x1x8x8x4-0-nopos]: 4 tensors, largest ratio out 1.26e-07 / 1.00e-05
  self_attention_matches_fp64[3x5x1x8x8x4-1-pos]: 4 tensors, largest ratio dW2 9.18e-07 / 3.00e-05
  self_attention_matches_fp64[3x5x1x8x8x4-1-nopos]: 4 tensors, largest ratio out 7.45e-08 / 1.00e-05
  self_attention_matches_fp64[33x6x3x16x48x4-0-pos]: 4 tensors, largest ratio out 3.09e-07 / 1.00e-05
  self_attention_matches_fp64[33x6x3x16x48x4-0-nopos]: 4 tensors, largest ratio out 2.08e-07 / 1.00e-05
  self_attention_matches_fp64[33x6x3x16x48x4-1-pos]: 4 tensors, largest ratio out 2.56e-07 / 1.00e-05
  self_attention_matches_fp64[33x6x3x16x48x4-1-nopos]: 4 tensors, largest ratio out 2.29e-07 / 1.00e-05
  self_attention_matches_fp64[33x50x3x16x48x4-0-pos]: 4 tensors, largest ratio out 2.87e-07 / 1.00e-05
  self_attention_matches_fp64[33x50x3x16x48x4-0-nopos]: 4 tensors, largest ratio out 2.80e-07 / 1.00e-05
  self_attention_matches_fp64[33x50x3x16x48x4-1-pos]: 4 tensors, largest ratio out 2.98e-07 / 1.00e-05
  self_attention_matches_fp64[33x50x3x16x48x4-1-nopos]: 4 tensors, largest ratio out 2.63e-07 / 1.00e-05
  self_attention_matches_fp64[33x65x3x8x40x16-0-pos]: 4 tensors, largest ratio out 2.97e-07 / 1.00e-05
  self_attention_matches_fp64[33x65x3x8x40x16-0-nopos]: 4 tensors, largest ratio out 1.44e-07 / 1.00e-05
  self_attention_matches_fp64[33x65x3x8x40x16-1-pos]: 4 tensors, largest ratio out 3.67e-07 / 1.00e-05
  self_attention_matches_fp64[33x65x3x8x40x16-1-nopos]: 4 tensors, largest ratio out 2.90e-07 / 1.00e-05
  self_attention_matches_fp64[17x6x3x16x48x4-0-pos]: 4 tensors, largest ratio out 2.28e-07 / 1.00e-05
  self_attention_matches_fp64[17x6x3x16x48x4-0-nopos]: 4 tensors, largest ratio out 2.19e-07 / 1.00e-05
  self_attention_matches_fp64[17x6x3x16x48x4-1-pos]: 4 tensors, largest ratio out 1.97e-07 / 1.00e-05
  self_attention_matches_fp64[17x6x3x16x48x4-1-nopos]: 4 tensors, largest ratio out 2.29e-07 / 1.00e-05
  self_attention_matches_fp64[17x33x3x16x48x1-0-pos]: 4 tensors, largest ratio out 2.31e-07 / 1.00e-05
  self_attention_matches_fp64[17x33x3x16x48x1-0-nopos]: 4 tensors, largest ratio out 1.77e-07 / 1.00e-05
  self_attention_matches_fp64[17x33x3x16x48x1-1-pos]: 4 tensors, largest ratio out 2.04e-07 / 1.00e-05
  self_attention_matches_fp64[17x33x3x16x48x1-1-nopos]: 4 tensors, largest ratio out 2.76e-07 / 1.00e-05
  self_attention_matches_fp64[5x9x4x64x256x16-0-pos]: 4 tensors, largest ratio out 4.51e-07 / 1.00e-05
  self_attention_matches_fp64[5x9x4x64x256x16-0-nopos]: 4 tensors, largest ratio out 5.05e-07 / 1.00e-05
  self_attention_matches_fp64[5x9x4x64x256x16-1-pos]: 4 tensors, largest ratio out 6.63e-07 / 1.00e-05
  self_attention_matches_fp64[5x9x4x64x256x16-1-nopos]: 4 tensors, largest ratio out 6.56e-07 / 1.00e-05
  self_attention_matches_fp64[2049x10x3x16x48x4-0-pos]: 4 tensors, largest ratio out 3.99e-07 / 1.00e-05
  self_attention_matches_fp64[2049x10x3x16x48x4-0-nopos]: 4 tensors, largest ratio out 2.74e-07 / 1.00e-05
  self_attention_matches_fp64[2049x10x3x16x48x4-1-pos]: 4 tensors, largest ratio out 4.21e-07 / 1.00e-05
  self_attention_matches_fp64[2049x10x3x16x48x4-1-nopos]: 4 tensors, largest ratio out 3.24e-07 / 1.00e-05
  select_matches_fp64[gout-1x1x1x1x1]: 4 tensors, largest ratio loss 0.00e+00 / 1.00e-05
  select_matches_fp64[gout-3x2x1x8x4]: 4 tensors, largest ratio loss 1.19e-07 / 1.00e-05
  select_matches_fp64[gout-33x11x3x16x4]: 4 tensors, largest ratio loss 1.56e-07 / 1.00e-05
  select_matches_fp64[gout-33x65x3x16x16]: 4 tensors, largest ratio loss 1.82e-07 / 1.00e-05
  select_matches_fp64[gout-5x33x4x64x16]: 4 tensors, largest ratio loss 8.72e-07 / 1.00e-05
  select_matches_fp64[gout-2049x11x3x16x4]: 4 tensors, largest ratio loss 2.58e-07 / 1.00e-05
  select_matches_fp64[gloss-1x1x1x1x1]: 4 tensors, largest ratio loss 0.00e+00 / 1.00e-05
  select_matches_fp64[gloss-3x2x1x8x4]: 4 tensors, largest ratio loss 1.19e-07 / 1.00e-05
  select_matches_fp64[gloss-33x11x3x16x4]: 4 tensors, largest ratio loss 1.56e-07 / 1.00e-05
  select_matches_fp64[gloss-33x65x3x16x16]: 4 tensors, largest ratio loss 1.82e-07 / 1.00e-05
  select_matches_fp64[gloss-5x33x4x64x16]: 4 tensors, largest ratio loss 8.72e-07 / 1.00e-05
  select_matches_fp64[gloss-2049x11x3x16x4]: 4 tensors, largest ratio loss 2.58e-07 / 1.00e-05
  select_matches_fp64[both-1x1x1x1x1]: 4 tensors, largest ratio loss 0.00e+00 / 1.00e-05
  select_matches_fp64[both-3x2x1x8x4]: 4 tensors, largest ratio loss 1.19e-07 / 1.00e-05
  select_matches_fp64[both-33x11x3x16x4]: 4 tensors, largest ratio loss 1.56e-07 / 1.00e-05
  select_matches_fp64[both-33x65x3x16x16]: 4 tensors, largest ratio loss 1.82e-07 / 1.00e-05
  select_matches_fp64[both-5x33x4x64x16]: 4 tensors, largest ratio loss 8.72e-07 / 1.00e-05
  select_matches_fp64[both-2049x11x3x16x4]: 4 tensors, largest ratio loss 2.58e-07 / 1.00e-05
  select_with_the_gradient_of_the_selected_capsules[33x11x3x16x4]: 4 tensors, largest ratio loss 1.56e-07 / 1.00e-05
  select_with_the_gradient_of_the_selected_capsules[5x33x4x64x16]: 4 tensors, largest ratio loss 8.72e-07 / 1.00e-05
  out_of_range_ids_set_the_flag_and_read_as_zero_rows: 11 tensors, largest ratio out 5.64e-07 / 1.00e-05
  layer_parity_with_the_torch_cpu_transcription[6-DR-literal]: 5 tensors, largest ratio output 4.40e-07 / 1.00e-05
  layer_parity_with_the_torch_cpu_transcription[6-DR-paper]: 5 tensors, largest ratio output 7.04e-07 / 1.00e-05
  layer_parity_with_the_torch_cpu_transcription[6-SA-literal]: 6 tensors, largest ratio output 2.63e-07 / 1.00e-05
  layer_parity_with_the_torch_cpu_transcription[6-SA-paper]: 6 tensors, largest ratio capsules 2.62e-07 / 1.00e-05
  layer_parity_with_the_torch_cpu_transcription[50-DR-literal]: 5 tensors, largest ratio output 2.68e-07 / 1.00e-05
  layer_parity_with_the_torch_cpu_transcription[50-DR-paper]: 5 tensors, largest ratio output 5.30e-07 / 1.00e-05
  layer_parity_with_the_torch_cpu_transcription[50-SA-literal]: 6 tensors, largest ratio output 2.80e-07 / 1.00e-05
  layer_parity_with_the_torch_cpu_transcription[50-SA-paper]: 6 tensors, largest ratio output 2.51e-07 / 1.00e-05
  extractor_layer_parity[6-DR]: 3 tensors, largest ratio out 7.04e-07 / 1.00e-05
  extractor_layer_parity[6-SA]: 4 tensors, largest ratio out 3.09e-07 / 1.00e-05
  extractor_layer_parity[50-DR]: 3 tensors, largest ratio out 5.30e-07 / 1.00e-05
  extractor_layer_parity[50-SA]: 4 tensors, largest ratio out 3.39e-07 / 1.00e-05
"""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import comirec_ref as CR

pytestmark = pytest.mark.gpu
F32 = np.float32
ids = lambda c: "x".join(map(str, c))
KEEPS = (0, 1)


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


# ---- bodies -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def dev_dr(*case):
    c = CR.dr_inputs(*case)
    return cu(c["table"]), cu(c["series"], np.int64), cu(c["W"]), cu(c["B0"]), cu(c["gout"])


def run_dr(case, keep, table=None, series=None, oob=None):
    from explicit_tf2_recommendation_amd import ops
    tab, ser, W, B0, gout = dev_dr(*case)
    tab = tab if table is None else table
    ser = ser if series is None else series
    out = ops.comirec_dr_fwd(tab, ser, W, B0, case[6], 0, keep, oob)
    gkeys, dW = ops.comirec_dr_bwd(tab, ser, W, B0, gout, case[6], 0, keep)
    return out, gkeys, dW


@functools.lru_cache(maxsize=None)
def dev_sa(*case):
    c = CR.sa_inputs(*case)
    return cu(c["table"]), cu(c["series"], np.int64), cu(c["W1"]), cu(c["W2"]), cu(c["pos"]), cu(c["gout"])


def run_sa(case, keep, with_pos, table=None, series=None, oob=None):
    from explicit_tf2_recommendation_amd import ops
    tab, ser, W1, W2, pos, gout = dev_sa(*case)
    tab = tab if table is None else table
    ser = ser if series is None else series
    pos = pos if with_pos else None
    out = ops.comirec_sa_fwd(tab, ser, W1, W2, pos, 0, keep, oob)
    return (out,) + ops.comirec_sa_bwd(tab, ser, W1, W2, gout, pos, 0, keep)


@functools.lru_cache(maxsize=None)
def dev_select(*case):
    c = CR.select_case(*case)
    return cu(c["table"]), cu(c["items"], np.int64), cu(c["m"]), cu(c["ginner"]), cu(c["gloss"]), cu(c["gsel"])


def run_select(case, way="both", with_gsel=False, table=None, items=None, oob=None):
    from explicit_tf2_recommendation_amd import ops
    tab, it, m, ginner, gloss, gsel = dev_select(*case)
    tab = tab if table is None else table
    it = it if items is None else items
    use_inner, use_loss = CR.SELECT_WAYS[way]
    chosen, inner, loss = ops.comirec_select_fwd(tab, it, m, oob)
    gm, gitems = ops.comirec_select_bwd(tab, it, m, chosen, ginner if use_inner else None, gloss if use_loss else None,
                                        gsel if with_gsel else None)
    return chosen, inner, loss, gm, gitems


DR_NAMES, SA_NAMES = (("out", 1e-5), ("gkeys", 3e-5), ("dW", 3e-5)), (("out", 1e-5), ("gkeys", 3e-5), ("dW1", 3e-5),
                                                                       ("dW2", 3e-5))


@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case", CR.DR_CASES, ids=ids)
def test_routing_matches_fp64(case, keep):
    ref, t32 = CR.dr_ref(case, keep), CR.dr_case_t(case, keep, torch.float32)
    got = run_dr(case, keep)
    B, T, Cn, E, Dc, K, R = case
    assert tuple(got[0].shape) == (B, K, Dc) and tuple(got[2].shape) == (K, T, Cn * E, Dc)
    for (name, floor), g in zip(DR_NAMES, got):
        check(name, host(g), ref[name], t32[name], floor)


@pytest.mark.parametrize("with_pos", [True, False], ids=["pos", "nopos"])
@pytest.mark.parametrize("keep", KEEPS)
@pytest.mark.parametrize("case", CR.SA_CASES, ids=ids)
def test_self_attention_matches_fp64(case, keep, with_pos):
    ref, t32 = CR.sa_ref(case, keep, with_pos), CR.sa_case_t(case, keep, with_pos, torch.float32)
    for (name, floor), g in zip(SA_NAMES, run_sa(case, keep, with_pos)):
        check(name, host(g), ref[name], t32[name], floor)


def check_select(c, got, up, items=None):
    items = c["items"] if items is None else items
    ref = CR.select_numpy(c["table"], items, c["m"], *up)
    t32 = CR.select_torch_grads(c["table"], items, c["m"], *up, torch.float32)
    near = ref["gap"] < CR.GAP_EPS_BODY
    assert near.mean() <= 0.10 and not any(np.any(g[near]) for g in up if g is not None)
    chosen, inner, loss, gm, gitems = (host(t) for t in got)
    assert chosen.dtype == np.int32 and np.array_equal(chosen[~near], ref["chosen"][~near])
    check("inner", inner[~near], ref["inner"][~near], t32["inner"][~near], 1e-5)
    check("loss", loss[~near], ref["loss"][~near], t32["loss"][~near], 1e-5)
    check("gm", gm, ref["gm"], t32["gm"], 3e-5)
    check("gitems", gitems, ref["gitems"], t32["gitems"], 3e-5)


@pytest.mark.parametrize("case", CR.SELECT_CASES, ids=ids)
@pytest.mark.parametrize("way", list(CR.SELECT_WAYS))
def test_select_matches_fp64(case, way):
    c = CR.select_case(*case)
    check_select(c, run_select(case, way), CR.select_way(c, way))


@pytest.mark.parametrize("case", [(33, 11, 3, 16, 4), (5, 33, 4, 64, 16)], ids=ids)
def test_select_with_the_gradient_of_the_selected_capsules(case):
    c = CR.select_case(*case)
    check_select(c, run_select(case, "both", True), CR.select_way(c, "both", True))
    from explicit_tf2_recommendation_amd import ops
    tab, it, m, ginner, gloss, gsel = dev_select(*case)
    chosen = ops.comirec_select_fwd(tab, it, m)[0]
    gm, gitems = ops.comirec_select_bwd(tab, it, m, chosen, gsel=gsel)                # gsel alone: a scatter-add by chosen
    want = torch.zeros_like(m).index_put_((torch.arange(case[0], device="cuda")[:, None].expand(-1, case[1]),
                                           chosen.long()), gsel.double().float(), accumulate=True)
    assert CR.rel_err(host(gm), host(want)) <= 1e-5 and not gitems.any()


def test_identical_capsules_tie_exactly_and_the_smallest_index_wins():
    """With fewer than two participating positions every head of the self-attentive extractor returns the same capsule,
    bit for bit, and every item of such an example chooses capsule 0; so does an m with equal rows."""
    from explicit_tf2_recommendation_amd import ops
    case = (33, 6, 3, 16, 48, 4)
    c = CR.sa_inputs(*case)
    tab, ser, W1, W2, pos, _ = dev_sa(*case)
    items = torch.randint(0, CR.V_CASE, (33, 11, 3), device="cuda", generator=torch.Generator("cuda").manual_seed(3))
    for keep in KEEPS:
        caps = ops.comirec_sa_fwd(tab, ser, W1, W2, pos, 0, keep)
        few = CR.takes_part(c["series"], keep).sum(1) <= 1
        assert few.sum() >= 2 and bool((caps[cu(few, bool)] == caps[cu(few, bool)][:, :1]).all())
        chosen, inner, _ = ops.comirec_select_fwd(tab, items, caps)
        assert not chosen[cu(few, bool)].any() and chosen[cu(~few, bool)].any()
    m = torch.randn(5, 1, 48, device="cuda").expand(-1, 4, -1).contiguous()
    chosen = ops.comirec_select_fwd(tab, items[:5], m)[0]
    gm, _ = ops.comirec_select_bwd(tab, items[:5], m, chosen, ginner=torch.ones(5, 11, device="cuda"))
    assert not chosen.any() and gm[:, 0].any() and not gm[:, 1:].any()


def _strided(table, pad=3):
    wide = torch.full((table.shape[0], table.shape[1] + pad), 7.0, device="cuda")
    wide[:, :table.shape[1]] = table
    view = wide[:, :table.shape[1]]
    assert view.stride(0) == table.shape[1] + pad
    return view


def test_strided_table_is_bit_identical_to_the_packed_one():
    dc, sc, lc = (33, 65, 3, 8, 40, 16, 3), (33, 65, 3, 8, 40, 16), (33, 11, 3, 16, 4)
    for a, b in zip(run_dr(dc, 1), run_dr(dc, 1, table=_strided(dev_dr(*dc)[0]))):
        assert torch.equal(a, b)
    for a, b in zip(run_sa(sc, 0, True), run_sa(sc, 0, True, table=_strided(dev_sa(*sc)[0]))):
        assert torch.equal(a, b)
    for a, b in zip(run_select(lc, "both", True), run_select(lc, "both", True, table=_strided(dev_select(*lc)[0]))):
        assert torch.equal(a, b)


def test_out_of_range_ids_set_the_flag_and_read_as_zero_rows():
    from explicit_tf2_recommendation_amd import ops
    dc, sc, lc = (33, 6, 3, 16, 48, 4, 3), (33, 6, 3, 16, 48, 4), (33, 11, 3, 16, 4)

    def spoil(series):
        series = series.copy()
        series[5, 2, 1], series[7, 0, 0], series[9, 3, 2] = -1, CR.V_CASE, 2 ** 40   # (a first-feature id too: not padding)
        return series

    c = CR.dr_inputs(*dc)
    flag = ops.new_flag("cuda")
    run_dr(dc, 1, oob=flag)
    assert int(flag.item()) == 0
    series = spoil(c["series"])
    ref = CR.dr_numpy(c["table"], series, c["W"], c["B0"], dc[6], 1, 0, c["gout"])
    t32 = CR.dr_torch_grads(c["table"], series, c["W"], c["B0"], dc[6], 1, c["gout"], torch.float32)
    got = run_dr(dc, 1, series=cu(series, np.int64), oob=flag)
    assert int(flag.item()) == 1
    for (name, floor), g in zip(DR_NAMES, got):
        check(name, host(g), ref[name], t32[name], floor)

    c = CR.sa_inputs(*sc)
    flag = ops.new_flag("cuda")
    run_sa(sc, 0, True, oob=flag)
    assert int(flag.item()) == 0
    series = spoil(c["series"])
    ref = CR.sa_numpy(c["table"], series, c["W1"], c["W2"], c["pos"], 0, 0, c["gout"])
    t32 = CR.sa_torch_grads(c["table"], series, c["W1"], c["W2"], c["pos"], 0, c["gout"], torch.float32)
    got = run_sa(sc, 0, True, series=cu(series, np.int64), oob=flag)
    assert int(flag.item()) == 1
    for (name, floor), g in zip(SA_NAMES, got):
        check(name, host(g), ref[name], t32[name], floor)

    c = CR.select_case(*lc)
    flag = ops.new_flag("cuda")
    run_select(lc, oob=flag)
    assert int(flag.item()) == 0
    items = c["items"].copy()
    items[4, 0, 0], items[6, 10, 2], items[8, 3, 1] = -5, CR.V_CASE, 2 ** 40
    assert not (CR.select_numpy(c["table"], items, c["m"])["gap"] < CR.GAP_EPS_BODY)[[4, 6, 8]].any()
    got = run_select(lc, "both", True, items=cu(items, np.int64), oob=flag)
    assert int(flag.item()) == 1
    check_select(c, got, CR.select_way(c, "both", True), items)


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


@pytest.mark.parametrize("case", [(33, 65, 3, 8, 40, 16, 3), (5, 9, 4, 64, 256, 16, 3), (1, 1, 1, 1, 1, 1, 1)], ids=ids)
def test_routing_and_self_attention_write_inside_their_outputs(case):
    from explicit_tf2_recommendation_amd._lib import lib
    B, T, Cn, E, Dc, K, R = case
    D = Cn * E
    tab, ser, W, B0, gout = dev_dr(*case)
    out, gkeys, dW = Guarded(B, K, Dc), Guarded(B, T, D), Guarded(K, T, D, Dc)
    nbytes = lib.rec_comirec_dr_workspace_bytes(B, T, E, Cn, Dc, K, R)
    ws = Guarded(nbytes // 4)
    head = (p(tab), tab.stride(0), tab.shape[0], E, Cn, p(ser), B, T, p(W), p(B0), Dc, K, R, 0, 1)
    assert lib.rec_comirec_dr_fwd_f32(*head, out.ptr, None, ws.ptr, nbytes, stream()) == 0
    assert lib.rec_comirec_dr_bwd_f32(*head, p(gout), gkeys.ptr, dW.ptr, ws.ptr, nbytes, stream()) == 0
    torch.cuda.synchronize()
    ws.value()
    for got, want in zip((out, gkeys, dW), run_dr(case, 1)):
        assert torch.equal(got.value(), want)

    tab, ser, W1, W2, pos, gout = dev_sa(*case[:6])
    out, gkeys, dW1, dW2 = Guarded(B, K, Dc), Guarded(B, T, D), Guarded(D, Dc), Guarded(K, Dc)
    nbytes = lib.rec_comirec_sa_workspace_bytes(B, T, E, Cn, Dc, K)
    ws = Guarded(nbytes // 4)
    head = (p(tab), tab.stride(0), tab.shape[0], E, Cn, p(ser), B, T, p(W1), p(W2), p(pos), Dc, K, 0, 1)
    assert lib.rec_comirec_sa_fwd_f32(*head, out.ptr, None, stream()) == 0
    assert lib.rec_comirec_sa_bwd_f32(*head, p(gout), gkeys.ptr, dW1.ptr, dW2.ptr, ws.ptr, nbytes, stream()) == 0
    torch.cuda.synchronize()
    ws.value()
    for got, want in zip((out, gkeys, dW1, dW2), run_sa(case[:6], 1, True)):
        assert torch.equal(got.value(), want)


@pytest.mark.parametrize("case", [(33, 65, 3, 16, 16), (5, 33, 4, 64, 16), (1, 1, 1, 1, 1)], ids=ids)
def test_select_writes_inside_its_outputs(case):
    from explicit_tf2_recommendation_amd._lib import lib
    B, Ns, Cn, E, K = case
    tab, it, m, ginner, gloss, gsel = dev_select(*case)
    chosen, inner, loss = Guarded(B, Ns, dtype=torch.int32), Guarded(B, Ns), Guarded(B)
    gm, gitems = Guarded(B, K, Cn * E), Guarded(B, Ns, Cn * E)
    head = (p(tab), tab.stride(0), tab.shape[0], E, Cn, p(it), B, Ns, p(m), K)
    assert lib.rec_comirec_select_fwd_f32(*head, chosen.ptr, inner.ptr, loss.ptr, None, stream()) == 0
    assert lib.rec_comirec_select_bwd_f32(*head, chosen.ptr, p(ginner), p(gloss), p(gsel), gm.ptr, gitems.ptr,
                                          stream()) == 0
    torch.cuda.synchronize()
    for got, want in zip((chosen, inner, loss, gm, gitems), run_select(case, "both", True)):
        assert torch.equal(got.value(), want)


def test_every_output_is_bit_identical_run_to_run():
    for case in ((2049, 10, 3, 16, 48, 4, 3), (5, 9, 4, 64, 256, 16, 3)):
        for a, b in zip(run_dr(case, 1), run_dr(case, 1)):
            assert torch.equal(a, b)
        for a, b in zip(run_sa(case[:6], 0, True), run_sa(case[:6], 0, True)):
            assert torch.equal(a, b)
    for a, b in zip(run_select((2049, 11, 3, 16, 4), "both", True), run_select((2049, 11, 3, 16, 4), "both", True)):
        assert torch.equal(a, b)


def test_cpu_tensors_bad_shapes_limits_and_empty_batches():
    from explicit_tf2_recommendation_amd import ops
    z = lambda *s: torch.zeros(*s, device="cuda")
    zi = lambda *s: torch.zeros(*s, dtype=torch.int64, device="cuda")
    tab, ser, W, B0, gout = dev_dr(3, 5, 1, 8, 8, 4, 3)
    with pytest.raises(RuntimeError):
        ops.comirec_dr_fwd(tab.cpu(), ser, W, B0)                               # no CPU fallback
    with pytest.raises(TypeError):
        ops.comirec_dr_fwd(tab, ser.int(), W, B0)
    with pytest.raises(ValueError):
        ops.comirec_dr_fwd(tab, ser, W[:, :, :7].contiguous(), B0)
    with pytest.raises(ValueError):
        ops.comirec_dr_fwd(tab, ser, W, B0[:, :4].contiguous())
    with pytest.raises(ValueError):
        ops.comirec_dr_bwd(tab, ser, W, B0, gout[:, :3].contiguous())
    with pytest.raises(NotImplementedError):
        ops.comirec_dr_fwd(tab, ser, W, B0, routing_rounds=9)
    with pytest.raises(NotImplementedError):                                    # T beyond the LDS fit
        ops.comirec_dr_fwd(z(10, 16), zi(2, 658, 1), z(1, 658, 16, 48), z(1, 658))
    out = ops.comirec_dr_fwd(tab, ser[:0], W, B0)
    gk, dW = ops.comirec_dr_bwd(tab, ser[:0], W, B0, gout[:0])
    assert tuple(out.shape) == (0, 4, 8) and tuple(gk.shape) == (0, 5, 8) and float(dW.abs().sum()) == 0

    tab, ser, W1, W2, pos, gout = dev_sa(3, 5, 1, 8, 8, 4)
    with pytest.raises(RuntimeError):
        ops.comirec_sa_fwd(tab, ser, W1.cpu(), W2)
    with pytest.raises(ValueError):
        ops.comirec_sa_fwd(tab, ser, W1, W2[:, :7].contiguous())
    with pytest.raises(ValueError):
        ops.comirec_sa_fwd(tab, ser, W1, W2, pos[:4].contiguous())
    with pytest.raises(ValueError):
        ops.comirec_sa_bwd(tab, ser, W1, W2, gout[:, :3].contiguous())
    with pytest.raises(NotImplementedError):
        ops.comirec_sa_fwd(z(10, 16), zi(2, 243, 3), z(48, 48), z(4, 48))
    out = ops.comirec_sa_fwd(tab, ser[:0], W1, W2, pos)
    gk, dW1, dW2 = ops.comirec_sa_bwd(tab, ser[:0], W1, W2, gout[:0], pos)
    assert tuple(out.shape) == (0, 4, 8) and tuple(gk.shape) == (0, 5, 8) and not dW1.any() and not dW2.any()

    tab, it, m, ginner, gloss, gsel = dev_select(3, 2, 1, 8, 4)
    chosen = ops.comirec_select_fwd(tab, it, m)[0]
    with pytest.raises(RuntimeError):
        ops.comirec_select_fwd(tab, it, m.cpu())
    with pytest.raises(ValueError):
        ops.comirec_select_fwd(tab, it, m[:, :, :7].contiguous())
    with pytest.raises(TypeError):
        ops.comirec_select_bwd(tab, it, m, chosen.long(), ginner)
    with pytest.raises(ValueError):
        ops.comirec_select_bwd(tab, it, m, chosen, ginner[:, :1].contiguous())
    gm, gi = ops.comirec_select_bwd(tab, it, m, chosen)                          # no gradient at all: zeros
    assert float(gm.abs().sum()) == 0 and float(gi.abs().sum()) == 0
    ch, inner, loss = ops.comirec_select_fwd(tab, it[:0], m[:0])
    gm, gi = ops.comirec_select_bwd(tab, it[:0], m[:0], ch, ginner[:0], gloss[:0])
    assert tuple(inner.shape) == (0, 2) and tuple(loss.shape) == (0,) and tuple(gm.shape) == (0, 4, 8)


# ---- layers ---------------------------------------------------------------------------------------------------------
def _layer(seed, T, mode, reference_mask):
    from explicit_tf2_recommendation_amd import layers
    sd = CR.layer_state(seed, T, mode)
    lay = layers.ComiRecLayer(feature_dims=CR.LAYER_V, seq_length=T, mode=mode, reference_mask=reference_mask).cuda()
    lay.load_state_dict({k: torch.from_numpy(np.asarray(v, F32)) for k, v in sd.items()})
    return lay, sd


def _grads(lay):
    return {k: host(q.grad.to_dense() if q.grad.is_sparse else q.grad) for k, q in lay.named_parameters()}


@pytest.mark.parametrize("reference_mask", [True, False], ids=["literal", "paper"])
@pytest.mark.parametrize("mode", ["DR", "SA"])
@pytest.mark.parametrize("T", CR.LAYER_TS)
def test_layer_parity_with_the_torch_cpu_transcription(T, mode, reference_mask):
    from explicit_tf2_recommendation_amd import data
    seed = CR.layer_seed(T, mode, reference_mask)
    lay, sd = _layer(seed, T, mode, reference_mask)
    ins = CR.layer_inputs(seed, CR.LAYER_B, T, mode)
    gsel, gloss = CR.layer_upstream(seed)
    t64 = CR.layer_torch(sd, ins, torch.float64, mode, reference_mask, gsel, gloss)
    t32 = CR.layer_torch(sd, ins, torch.float32, mode, reference_mask, gsel, gloss)
    assert not (t64["gap"] < CR.GAP_EPS_LAYER).any()                          # so no example is left out
    batch = data.to_device(ins)
    caps = lay.generate_interest_capsules(batch)
    check("capsules", host(caps), t64["capsules"], t32["capsules"], 1e-5)
    res = lay(batch)
    assert res.keys() == {"output", "loss"}
    assert tuple(res["output"].shape) == (CR.LAYER_B, CR.LAYER_NS, CR.LAYER_D) and tuple(res["loss"].shape) == (CR.LAYER_B,)
    check("output", host(res["output"]), t64["output"], t32["output"], 1e-5)
    check("loss", host(res["loss"]), t64["loss"], t32["loss"], 1e-5)
    ((res["output"] * cu(gsel)).sum() + (res["loss"] * cu(gloss)).sum()).backward()
    grads = _grads(lay)
    assert grads.keys() == t64["grads"].keys() and len(grads) == (2 if mode == "DR" else 3)
    for k in grads:
        check(k[-28:], grads[k], t64["grads"][k], t32["grads"][k], 3e-5)
    if mode == "DR":
        assert lay.interest_extractor.B.grad is None


@pytest.mark.parametrize("mode", ["DR", "SA"])
@pytest.mark.parametrize("T", CR.LAYER_TS)
def test_extractor_layer_parity(T, mode):
    from explicit_tf2_recommendation_amd import layers
    sd, ins = CR.layer_state(1, T, mode), CR.layer_inputs(1, CR.LAYER_B, T, "DR")
    series = np.stack([ins[n] for n in CR.SERIES], axis=2)
    D = CR.LAYER_D
    gout = CR.f32_exact(np.random.default_rng(5).uniform(-1, 1, (CR.LAYER_B, CR.LAYER_K, D)))
    table = torch.nn.Parameter(cu(sd["embed.embeddings"]))
    if mode == "DR":
        ext = layers.ComiRecDynamicRoutingLayer(CR.LAYER_K, D)                 # built by the first call
        ext((table, cu(series, np.int64)), 0, False)
        assert tuple(ext.W.shape) == (CR.LAYER_K, T, D, D) and tuple(ext.B.shape) == (CR.LAYER_K, T) and ext.W.is_cuda
        names = {"W": "interest_extractor.W", "B": "interest_extractor.B"}
    else:
        ext = layers.ComiRecSelfAttentiveLayer(CR.LAYER_K, D)
        ext((table, cu(series, np.int64)), 0, False)
        assert tuple(ext.W1.shape) == (D, D) and tuple(ext.W2.shape) == (CR.LAYER_K, D) and ext.W1.is_cuda
        names = {"W1": "interest_extractor.W1", "W2": "interest_extractor.W2"}
    with torch.no_grad():
        for k, full in names.items():
            getattr(ext, k).copy_(cu(sd[full]))
    out = ext((table, cu(series, np.int64)), 0, False)
    (out * cu(gout)).sum().backward()
    if mode == "DR":
        args = (sd["embed.embeddings"], series, sd[names["W"]], sd[names["B"]], 3, 0)
        ref, t32 = CR.dr_numpy(*args, 0, gout), CR.dr_torch_grads(*args, gout, torch.float32)
        pairs = [("W.grad", ext.W.grad, "dW")]
    else:
        pos = CR.positional_table(T, D).astype(np.float64)
        args = (sd["embed.embeddings"], series, sd[names["W1"]], sd[names["W2"]], pos, 0)
        ref, t32 = CR.sa_numpy(*args, 0, gout), CR.sa_torch_grads(*args, gout, torch.float32)
        pairs = [("W1.grad", ext.W1.grad, "dW1"), ("W2.grad", ext.W2.grad, "dW2")]

    def table_grad(gkeys):                                                    # IndexedSlices values -> dense rows
        g = np.zeros_like(sd["embed.embeddings"])
        np.add.at(g, series.reshape(-1), np.asarray(gkeys, np.float64).reshape(-1, CR.LAYER_E))
        return g

    check("out", host(out), ref["out"], t32["out"], 1e-5)
    for name, got, key in pairs:
        check(name, host(got), ref[key], t32[key], 3e-5)
    check("table.grad", host(table.grad.to_dense()), table_grad(ref["gkeys"]), table_grad(t32["gkeys"]), 3e-5)


def test_out_of_range_id_raises():
    from explicit_tf2_recommendation_amd import data
    for mode in ("DR", "SA"):
        lay, _ = _layer(1, 6, mode, True)
        ins = CR.layer_inputs(1, CR.LAYER_B, 6, mode)
        lay(data.to_device(ins))
        for name in ("visited_shop_ids", "label_cate_ids"):
            bad = {k: v.copy() for k, v in ins.items()}
            bad[name].reshape(-1)[5] = CR.LAYER_V
            with pytest.raises(IndexError):
                lay(data.to_device(bad))
        bad = {k: v.copy() for k, v in ins.items()}
        bad["visited_cate_ids"].reshape(-1)[7] = -1
        with pytest.raises(IndexError):
            lay.generate_interest_capsules(data.to_device(bad))


@pytest.mark.parametrize("mode", ["DR", "SA"])
def test_graph_replay_equals_eager_bit_for_bit(mode):
    """Three replays over three batches against an eager copy of the layer: losses and every gradient, the table's sparse
    rows included."""
    from explicit_tf2_recommendation_amd import data, engine
    T = 50
    lay, _ = _layer(1, T, mode, True)
    eager = copy.deepcopy(lay)

    def batch(seed):
        b = data.to_device(CR.layer_inputs(seed, CR.LAYER_B, T, mode))
        b["label"] = torch.zeros(CR.LAYER_B, 1, device="cuda")               # a dummy: the layer carries its own loss
        return b

    batches = [batch(s) for s in (11, 12, 13)]
    step = engine.GraphedTrainStep(lay, batches[0], label_name="label",
                                   output_fn=lambda l, x: l(x)["loss"].sum().reshape(1),
                                   loss_fn=lambda out, y: out.sum())
    for b in batches:
        loss = step(b)
        for q in eager.parameters():
            q.grad = None
        want = eager({k: v for k, v in b.items() if k != "label"})["loss"].sum()
        want.backward()
        assert torch.equal(loss.reshape(()), want.detach())
        for (name, a), q in zip(lay.named_parameters(), eager.parameters()):
            assert a.grad is not None and a.grad.is_sparse == q.grad.is_sparse, name
            if a.grad.is_sparse:
                assert torch.equal(a.grad._indices(), q.grad._indices()), name
                assert torch.equal(a.grad._values(), q.grad._values()), name
            else:
                assert torch.equal(a.grad, q.grad), name
