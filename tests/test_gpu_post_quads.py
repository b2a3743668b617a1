"""GPU tests of the four-runs-per-lane body of the direct-mode post launch (fixq_body, csrc/deepfm_fused.hip), the
body of every DeepFMFusedStep without the lazy Adam whose batch size is a multiple of 1024:

    lane L of wave w (0..3) of a column's workgroup owns runs u0 = 1024 wg + 256 w + 4 L .. u0 + 3
    ids leave as two 16-byte pieces when before + u0 is even, first-order rows as one when it is a multiple of 4
    a quadruple that straddles the column's last run, or holds a run of more than two members, goes element by element
    runs of more than two members: summed where the fast path found them (column not skewed) or under fix_spread

The batches are tests.helpers.plan_batch's: every column's run lengths are prescribed, and with the "ranked" layout
the plan slot of every run.  Each case reads back the plan and asserts the regime it was built for.  The checks are
those of tests/test_gpu_plan_edges.py (its oracle, tolerances and plan guards are imported, not restated): unique ids,
their count and the padded tail exact, row sums against the fp64 segment sums of the oracle's per-lookup gradients,
dense gradients and loss against the generic step; plus: the first-order row of a single-lookup run is gz of that
lookup, bit for bit, and two launches leave the same bytes.  B = 1000 runs the one-run-per-lane body: the dispatch.
"""
import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import test_gpu_plan_edges as PE

pytestmark = pytest.mark.gpu

QUADS_T = 1024                                               # FIX_T: the new body runs when B % 1024 == 0 (no lazy Adam)


def ranked(B, fixed):
    """run lengths in key order: fixed = {rank: length}, singles elsewhere (tests/test_gpu_plan_edges.ranked_spectrum)"""
    ranks = sorted(fixed)
    return PE.ranked_spectrum(B, ranks, [fixed[u] for u in ranks])


def pairs_at(B, ranks):
    return ranked(B, {u: 2 for u in ranks})


# pairs at each of the four positions of a quadruple (ranks 0, 5, 10, 15), in the last slot of one lane's quadruple and
# the first of the next lane's (19, 20), two in one quadruple (24, 25), across two waves (255, 256), all four of a quadruple
# (40..43) and across the two fast waves' halves of later lanes
PAIR_RANKS = (0, 5, 10, 15, 19, 20, 24, 25, 40, 41, 42, 43, 255, 256, 511, 512, 770)


def case_distinct_f1():
    """(a) F = 1, every id distinct: before = 0, nu = B, no tail"""
    B = 1024
    return B, [5000], [[1] * B], "ranked", lambda plan: PE.expect(plan, B, 0, skew=False, nu=B, longest=1)


def case_pairs_f1():
    """(c) F = 1 (before = 0: every full quadruple takes the 16-byte stores): pairs at every position"""
    B = 1024
    spec = pairs_at(B, PAIR_RANKS)

    def guard(plan):
        r = PE.expect(plan, B, 0, skew=False, nu=B - len(PAIR_RANKS), longest=2)
        assert np.array_equal(np.nonzero(r["runs"] == 2)[0], np.array(sorted(PAIR_RANKS)))
    return B, [5000], [spec], "ranked", guard


def case_straddle_f3(first_pairs):
    """(b) F = 3: nu % 4 = 1, 2, 3 over the columns when first_pairs = 3 (before = 0, 1021, 2043: odd, so ids and
    first-order rows of columns 1 and 2 leave element by element); first_pairs = 2 gives before = 0, 1022, 2045 (column 1:
    ids as 16-byte pieces, first-order rows element by element).  The last quadruple of every column straddles nu."""
    B = 1024
    npairs = (first_pairs, 2 if first_pairs == 3 else 1, 1)
    spectra = [pairs_at(B, [7 + 4 * i + i for i in range(n)]) for n in npairs]

    def guard(plan):
        before = 0
        for f, n in enumerate(npairs):
            r = PE.expect(plan, B, f, skew=False, nu=B - n)
            assert r["nu"] % 4 != 0
            if f:
                assert before % 4 != 0
            before += r["nu"]
    return B, [4000, 4000, 4000], spectra, "ranked", guard


def case_wide_f26():
    """F = 26 at B = 1024: (d) runs of 3, 17, 18, 128, 129 members in a skewed column and -- split so that no column
    has more than 256 repeats -- in columns that are not; (e) a column that is one id beside a distinct one; (c) the
    pair positions; uniform columns in between"""
    B, F = 1024, 26
    dims = [3000] * F
    spectra = ["uniform"] * F
    spectra[0] = [1] * B                                     # distinct
    spectra[1] = [B]                                         # one id
    spectra[2] = [1] * B
    spectra[3] = pairs_at(B, PAIR_RANKS)
    spectra[5] = ranked(B, {2: 3, 9: 17, 300: 18, 301: 128, 600: 129, 3: 2, 601: 2})       # skewed: 290 + 2 repeats
    spectra[6] = ranked(B, {1: 3, 6: 17, 11: 18, 260: 129, 500: 2})                        # not skewed: 164 repeats
    spectra[7] = ranked(B, {0: 128, 5: 3, 6: 3, 7: 3, 700: 18})                            # not skewed: 150 repeats
    spectra[25] = ranked(B, {4: 3, 5: 2, 6: 17, 7: 2})                                      # the last column

    def guard(plan):
        PE.expect(plan, B, 0, skew=False, nu=B)
        PE.expect(plan, B, 1, skew=True, nu=1, longest=B)
        PE.expect(plan, B, 2, skew=False, nu=B)
        PE.expect(plan, B, 5, skew=True, has=(1, 2, 3, 17, 18, 128, 129))
        PE.expect(plan, B, 6, skew=False, has=(1, 2, 3, 17, 18, 129))
        PE.expect(plan, B, 7, skew=False, has=(1, 3, 18, 128))
        PE.expect(plan, B, 25, skew=False, has=(2, 3, 17))
    return B, dims, spectra, "ranked", guard


def case_two_wgs():
    """B = 2048, F = 2: two workgroups per column.  Column 0 skewed with every run-length class and pairs on both sides
    of the workgroup boundary; column 1 not skewed, pairs and a run of three around slot 1024"""
    B = 2048
    c0 = ranked(B, {0: 200, 1: 129, 2: 128, 3: 18, 4: 17, 5: 3, 6: 2, 1022: 2, 1023: 2, 1024: 2, 1025: 3, 1030: 40})
    c1 = ranked(B, {1021: 2, 1023: 2, 1024: 2, 1027: 3, 1500: 19, 2000: 2})

    def guard(plan):
        r = PE.expect(plan, B, 0, skew=True, has=(1, 2, 3, 17, 18, 40, 128, 129, 200))
        assert r["nu"] > QUADS_T                             # live runs in the second workgroup
        r = PE.expect(plan, B, 1, skew=False, has=(1, 2, 3, 19))
        assert r["nu"] > QUADS_T
    return B, [6000, 6000], [c0, c1], "ranked", guard


def case_many_huge():
    """(f) 17 runs of more than 128 members in workgroup 0 of a column (two rounds of the ordered list), B = 3072:
    three workgroups per column; a uniform column beside it"""
    B = 3072
    c0 = PE.ranked_spectrum(B, PE.wg0_ranks(B, 17), PE.huge_lens(17, 5), extra=((60, 17), (61, 3), (62, 2)))

    def guard(plan):
        PE.expect(plan, B, 0, skew=True, wg0_huge=17, has=(17, 3, 2))
        PE.expect(plan, B, 1, skew=False)
    return B, [5000, 40000], [c0, "uniform"], "ranked", guard


def case_old_body():
    """B = 1000: not a multiple of 1024, the one-run-per-lane body (tests/test_gpu_plan_edges.case_sweep's batch)"""
    return PE.case_sweep(1000)


CASES = [("distinct-F1", case_distinct_f1), ("pairs-F1", case_pairs_f1),
         ("straddle-F3-odd", lambda: case_straddle_f3(3)), ("straddle-F3-even", lambda: case_straddle_f3(2)),
         ("wide-F26", case_wide_f26), ("two-wgs-B2048", case_two_wgs), ("many-huge-B3072", case_many_huge),
         ("old-body-B1000", case_old_body)]
GRAPHED = ("wide-F26",)                                      # also replayed from a hipGraph, bytes compared with eager


def single_lookup_rows_exact(step, host, names, tag):
    """g_w of a run of one lookup == gz of that lookup, bit for bit"""
    g = step.gradients()
    ids, wrows, nu = g["w.embeddings"]
    nu = int(nu.item())
    ids, wrows = ids.cpu().numpy()[:nu], wrows.cpu().numpy()[:nu, 0]
    gz = step.gz.cpu().numpy()
    n = 0
    for nm in names:
        col = host[nm].reshape(-1)
        uid, first, cnt = np.unique(col, return_index=True, return_counts=True)
        one = cnt == 1
        slot = np.searchsorted(ids, uid[one])
        assert np.array_equal(ids[slot], uid[one]), (tag, nm)
        assert np.array_equal(wrows[slot].view(np.uint32), gz[first[one]].view(np.uint32)), (tag, nm)
        n += int(one.sum())
    return n


@pytest.mark.parametrize("name,fn", CASES, ids=[c[0] for c in CASES])
def test_post_quads_case(name, fn):
    from explicit_tf2_recommendation_amd import engine, data
    seed = 40 + [c[0] for c in CASES].index(name)
    B, dims, spectra, layout, guard = fn()
    offsets = H.field_offsets(dims)
    host = H.plan_batch(B, dims, offsets, spectra, layout, seed)
    F, V = len(dims), int(sum(dims))
    assert (B % QUADS_T == 0) == (name != "old-body-B1000")
    layer, names = PE.make_layer(F, V, seed)
    dbatch = data.to_device(host)
    ref = PE.oracle(layer, names, host)

    eager = engine.DeepFMFusedStep(layer, B, dims, offsets, use_graph=False)
    loss = eager(dbatch).item()
    eager.check_flags()
    plan = PE.read_plan(eager, PE.last_plan_buf(eager))
    PE.check_plan(plan, host, names, offsets, name)
    guard(plan)                                              # the case is in the regime it was built for
    # loss and dense gradients; unique ids, their count and the padded tail (zero rows of both tables, id col_uid[0])
    # exact; row sums of both tables against the fp64 segment sums
    PE.check_oracle(eager, loss, ref, name + "/eager")
    n_single = single_lookup_rows_exact(eager, host, names, name)
    assert n_single > 0 or name != "distinct-F1"
    want = PE.snapshot(eager)
    eager(dbatch)
    PE.same(want, PE.snapshot(eager), name + "/run-to-run")

    generic = engine.DeepFMTrainStep(layer, B, optimizer=None, use_graph=False)
    lg = generic(dbatch).item()
    assert abs(lg - want["loss"].item()) <= 1e-6, name       # (tests/test_gpu_engine.py: fused against generic)
    gg = generic.gradients()
    for k in PE.DENSE:
        assert PE.close(want[k].cpu().numpy(), gg[k].cpu().numpy(), 1e-5), (name, k)

    if name in GRAPHED:
        graphed = engine.DeepFMFusedStep(layer, B, dims, offsets, use_graph=True)
        for _ in range(3):                                   # eager, eager + capture, replay
            graphed(dbatch)
        assert len(graphed._graphs) == 1
        graphed.check_flags()
        PE.same(want, PE.snapshot(graphed), name + "/graph-vs-eager")
