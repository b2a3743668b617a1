"""GPU tests of DeepFMFusedStep on batches whose de-duplication plans are built to reach every branch of the plan sort
(colsort_onewg_kernel, csrc/colsort.hip) and of the post launch (deepfm_post_direct_kernel, csrc/deepfm_fused.hip):

    run of 1 or 2 members          fast path (one lane, fix_deal mapping)
    3 .. FIX_SHORT=17              four lanes per run (skewed columns)
    18 .. FIX_HUGE=128             one wave per run (skewed columns; in other columns every run of more than 2)
    more than 128                  the whole workgroup, through a 128-entry LDS list, 16 runs per round
    column skewed iff B - nu > 256; runs of more than two members of a skewed column are looked at through fix_spread
    (the identity when B % 64 != 0); the lazy Adam of a row runs in the workgroup that finished its sum

and, in the sort, kpt = 8 / 16 (B <= 8192 / above), 16-byte perm stores (B % 8 == 0, kpt 8), ceil(key_bits / 7) radix
passes and sort words of up to 32 bits.  The batches come from tests.helpers.plan_batch, which prescribes every
column's run lengths; every case reads back the plan it produced and asserts the regime it was built for, so that a
change of the builder or of a threshold cannot turn a case into a trivial one.  Gradients are checked against the fp64
oracle (oracle/torch_ref.py), eagerly and from a replayed hipGraph.
"""
import os
import socket

import numpy as np
import pytest
import torch

from oracle import layers_np as L
from oracle import torch_ref as T
from tests import helpers as H

pytestmark = pytest.mark.gpu

# thresholds of the post launch (csrc/deepfm_fused.hip: FIX_T, FIX_HUGE, FIX_SHORT, FIX_SKEW)
FIX_T, FIX_HUGE, FIX_SHORT, FIX_SKEW = 1024, 128, 17, 256
DENSE = ("MLP_layer1.kernel_0", "MLP_layer1.bias_0", "MLP_layer1.kernel_1", "MLP_layer1.bias_1",
         "MLP_layer2.kernel_0", "MLP_layer2.bias_0", "bias")
TABLES = ("embed.embeddings", "w.embeddings")


def make_layer(F, V, seed):
    """make16 of tests/test_gpu_engine.py with a table of V rows"""
    from explicit_tf2_recommendation_amd import layers
    names = ["f%d" % i for i in range(F)]
    layers.set_init_seed(seed)
    layer = layers.DeepFMRankingLayer(feature_names=names, feature_dims=V, embedding_dims=16, mlp_dims=[32, 8]).cuda()
    torch.manual_seed(2000 + seed)
    with torch.no_grad():
        for n, p in layer.named_parameters():
            if "bias_" in n:
                p.uniform_(-0.1, 0.1)
        layer.embed.embeddings.mul_(6.0 if F <= 8 else 2.0)
    return layer, names


def close(a, b, tol=2e-5, floor=1e-3):
    """max-abs error <= tol * max|reference| (tests/test_gpu_engine.py)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return True
    err, scale = np.abs(a - b).max(), max(floor, np.abs(b).max())
    if err > tol * scale:
        print("close(): max-abs error %.3e vs scale %.3e (ratio %.2e > tol %.1e)" % (err, scale, err / scale, tol))
    return err <= tol * scale


def oracle(layer, names, batch):
    """fp64 loss and gradients of one train_loop iteration (the oracle's deepfm_forward + keras_bce), with the
    gradient of every LOOKUP kept: the table is replaced by the B*F gathered rows, so d loss / d row[b, f] is one row of
    the gradient.  Row sums per unique id, sums of |member rows| and run lengths follow in fp64."""
    pr = {k: v.detach().cpu().double() for k, v in layer.named_parameters()}
    X = L.index_assemble(batch, names)
    B, F = X.shape
    flat = torch.from_numpy(X.reshape(-1))
    leaf = {k: pr[k].clone().requires_grad_() for k in DENSE}
    le = pr["embed.embeddings"][flat].clone().requires_grad_()
    lw = pr["w.embeddings"][flat].clone().requires_grad_()
    b0 = pr["MLP_layer1.bias_0"].expand(B, -1).clone().requires_grad_()   # one bias row per example: its gradient is
    p = {"embed": le, "w": lw, "bias": leaf["bias"],                       # delta_b of layer 1, per example
         "k1": [leaf["MLP_layer1.kernel_0"], leaf["MLP_layer1.kernel_1"]],
         "b1": [b0, leaf["MLP_layer1.bias_1"]],
         "k2": [leaf["MLP_layer2.kernel_0"]], "b2": [leaf["MLP_layer2.bias_0"]]}
    Xl = torch.arange(B * F, dtype=torch.int64).reshape(B, F)
    loss = T.keras_bce(torch.from_numpy(batch["label"]).double(), T.deepfm_forward(p, Xl))
    loss.backward()
    touched, inv = np.unique(X.reshape(-1), return_inverse=True)
    out = {"loss": loss.item(), "touched": touched, "count": np.bincount(inv, minlength=touched.size)}
    for k in DENSE:
        out[k] = leaf[k].grad.numpy() if k != "MLP_layer1.bias_0" else b0.grad.numpy().sum(0)
    # a column that is ONE id: its 16 rows of dK0 are x (x) sum_b delta_b, a sum of B terms that cancel (see rows_ok)
    one = [f for f in range(F) if np.all(X[:, f] == X[0, f])] if B >= LONG_RUN else []
    out["one_id_rows"] = np.array([f * 16 + d for f in one for d in range(16)], np.int64)
    out["one_id_abs"] = np.concatenate([np.abs(pr["embed.embeddings"][X[0, f]].numpy())[:, None] *
                                        np.abs(b0.grad.numpy()).sum(0)[None, :] for f in one]) if one else None
    out["B"] = B
    # how close the batch sits to a ReLU kink: |pre-activation| / sum|terms| of layers 1 and 2, smallest over examples and
    # units.  Below fp32 rounding (~6e-8) the fp32 kernel and the fp64 oracle may put an example on opposite sides of the
    # kink, and that example's whole delta of the unit shows up as a gradient error: a property of the data, not of a
    # kernel (it hits the generic step as well)
    with torch.no_grad():
        Dx = le.detach().reshape(B, F * 16)
        K0, K1 = pr["MLP_layer1.kernel_0"], pr["MLP_layer1.kernel_1"]
        bb0, bb1 = pr["MLP_layer1.bias_0"], pr["MLP_layer1.bias_1"]
        h1 = Dx @ K0 + bb0
        r1 = (h1.abs() / (Dx.abs() @ K0.abs() + bb0.abs())).numpy()
        a1 = torch.relu(h1)
        r2 = ((a1 @ K1 + bb1).abs() / (a1 @ K1.abs() + bb1.abs())).numpy()
    b_, u_ = np.unravel_index(r1.argmin(), r1.shape)
    out["margin"] = min(r1.min(), r2.min())
    out["margin_where"] = "ReLU margin: layer 1 %.1e (example %d, unit %d), layer 2 %.1e" % (r1.min(), b_, u_, r2.min())
    for k, g in (("embed.embeddings", le.grad.numpy()), ("w.embeddings", lw.grad.numpy())):
        s = np.zeros((touched.size, g.shape[1]))
        a = np.zeros((touched.size, g.shape[1]))
        np.add.at(s, inv, g)
        np.add.at(a, inv, np.abs(g))
        out[k], out[k + ".abs"] = s, a
    return out


# a run of thousands of members whose terms cancel can leave a sum far below max|reference|: there the relative bound of
# close() measures the cancellation, not the kernel.  For those rows only, the bound is the fp32 error of summing n
# terms in any order, n * 2^-24 * sum|member rows|, per element (sums in fp64 from the oracle's per-lookup rows).
# The bound is loose: at n = 4096 it equals the mean |member row|, so a member of below-average size dropped or added
# twice would pass it.  Runs of up to 1023 members (one-id-B1000: a one-id column of 1000) are held to close().
LONG_RUN = 1024


def rows_ok(got, ref, key):
    want, absum, n = ref[key], ref[key + ".abs"], ref["count"]
    long_ = n >= LONG_RUN
    ok = close(got[~long_], want[~long_])
    if long_.any():
        bound = (n[long_, None] * 2.0 ** -24) * absum[long_]
        err = np.abs(got[long_] - want[long_])
        if not np.all(err <= bound):
            print("rows_ok(): long-run rows exceed n*2^-24*sum|members| by up to %.3e" % (err - bound).max())
            ok = False
    return ok


def check_oracle(step, loss, ref, tag):
    tag = "%s [%s]" % (tag, ref["margin_where"])
    assert abs(loss - ref["loss"]) <= 1e-5 * max(1, abs(ref["loss"])), (tag, loss, ref["loss"])
    g = step.gradients()
    for k in DENSE:
        got, want = g[k].cpu().numpy(), ref[k]
        if k == "MLP_layer1.kernel_0" and ref["one_id_rows"].size:
            # rows of a column that is one id: a run of B members (the bound of rows_ok), close() on all other rows
            r1 = ref["one_id_rows"]
            rest = np.setdiff1d(np.arange(want.shape[0]), r1)
            assert close(got[rest], want[rest]), (tag, k)
            err = np.abs(got[r1] - want[r1])
            assert np.all(err <= ref["B"] * 2.0 ** -24 * ref["one_id_abs"]), (tag, k, "one-id rows")
            continue
        assert close(got, want), (tag, k)
    touched = ref["touched"]
    for k in TABLES:
        ids, rows, nu = g[k]
        nu = int(nu.item())
        ids, rows = ids.cpu().numpy(), rows.cpu().numpy()
        assert nu == touched.size, (tag, nu, touched.size)
        assert np.array_equal(ids[:nu], touched), (tag, k)          # bit exact, ascending
        assert rows_ok(rows[:nu], ref, k), (tag, k)
        assert np.all(rows[nu:] == 0) and np.all(ids[nu:] == touched[0]), (tag, k)   # padded tail


def snapshot(step):
    g = step.gradients()
    out = {k: g[k].clone() for k in DENSE}
    ids, rows, nu = g["embed.embeddings"]
    out["ids"], out["rows"], out["wrows"] = ids.clone(), rows.clone(), g["w.embeddings"][1].clone()
    out["nu"] = nu.clone()
    out["loss"] = step.loss.clone()
    return out


def same(a, b, tag):
    for k in a:
        assert torch.equal(a[k], b[k]), (tag, k)


# ------------------------------------------------------------------------------------------------
# the plan on the host: read back, compared with its definition, and the regime it puts a column in
# ------------------------------------------------------------------------------------------------
def last_plan_buf(step):
    """buffer of the plan of a single call's batch when nothing was announced: the first slot of the current half"""
    return step._half * (step.NBUF // 2)


def read_plan(step, buf):
    p = step.plans[buf]
    return {k: v.cpu().numpy() for k, v in p.items()}


def check_plan(plan, batch, names, offsets, tag):
    """the plan the sort built == the host restatement of the plan (tests.helpers.host_plan), bit for bit"""
    for f, nm in enumerate(names):
        want = H.host_plan(batch[nm], offsets[f])
        nu = want["col_nu"]
        assert int(plan["col_nu"][f]) == nu, (tag, f)
        assert np.array_equal(plan["perm"][f], want["perm"]), (tag, f, "perm")
        assert np.array_equal(plan["col_uid"][f][:nu], want["col_uid"]), (tag, f, "col_uid")
        assert np.array_equal(plan["col_seg"][f], want["col_seg"]), (tag, f, "col_seg")
        assert np.array_equal(plan["dloc"][f], want["dloc"]), (tag, f, "dloc")


def col_runs(plan, f):
    nu = int(plan["col_nu"][f])
    seg = plan["col_seg"][f]
    return (seg[1:nu + 1] - seg[:nu]).astype(np.int64)


def spread_wg(u, B):
    """workgroup (of the column) that looks at run u under fix_spread: lane l of wave w takes run l * (B/64) + w"""
    u = np.asarray(u, np.int64)
    t = u if B % 64 else (u % (B // 64)) * 64 + u // (B // 64)
    return t // FIX_T


def regime(plan, f, B):
    runs = col_runs(plan, f)
    nu = runs.size
    skew = B - nu > FIX_SKEW
    huge = np.nonzero(runs > FIX_HUGE)[0] if skew else np.zeros(0, np.int64)
    wg = spread_wg(huge, B)
    return dict(runs=runs, nu=nu, skew=skew, huge_per_wg=np.bincount(wg, minlength=1) if huge.size else np.zeros(1, int),
                lengths=set(runs.tolist()))


def expect(plan, B, f, skew=None, has=(), wg0_huge=None, longest=None, nu=None):
    r = regime(plan, f, B)
    if skew is not None:
        assert r["skew"] == skew, ("column", f, "B - nu =", B - r["nu"], "skew expected", skew)
    for x in has:
        assert x in r["lengths"], ("column", f, "has no run of", x)
    if wg0_huge is not None:
        assert r["huge_per_wg"][0] == wg0_huge, ("column", f, "huge runs in workgroup 0", r["huge_per_wg"])
    if longest is not None:
        assert r["runs"].max() == longest, ("column", f, r["runs"].max())
    if nu is not None:
        assert r["nu"] == nu, ("column", f, r["nu"])
    return r


# ------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------
def ranked_spectrum(B, huge_ranks, huge_lens, extra=()):
    """run lengths in key order: huge_lens[i] at rank huge_ranks[i], `extra` (rank, length) pairs, singles elsewhere"""
    fixed = dict(zip(huge_ranks, huge_lens))
    fixed.update(dict(extra))
    n = B - sum(fixed.values()) + len(fixed)
    assert n > max(fixed), "not enough runs for the ranks"
    spec = [1] * n
    for u, ln in fixed.items():
        spec[u] = ln
    assert sum(spec) == B
    return spec


def wg0_ranks(B, n):
    """n run ranks that fix_spread sends to workgroup 0 of the column (u mod (B/64) < 16; any u < 1024 if B % 64)"""
    if B % 64:
        return list(range(n))
    q = B // 64
    return [blk * q + i for blk in range(64) for i in range(16)][:n]


def huge_lens(n, seed):
    return [129 + (37 * i + seed) % 90 for i in range(n)]


def case_lengths(layout):
    """every run-length class in a skewed column and (split over three columns, total repeats <= 256) in columns
    that are not skewed, plus a column that is one id and a uniform one"""
    B = 4096
    dims = [6000, 4000, 6000, 6000, 50000]
    spectra = [H.fill_spectrum(B, [3, 16, 17, 18, 127, 128, 129], pairs=30), [B],
               H.fill_spectrum(B, [3, 16, 17, 18, 129], pairs=20), H.fill_spectrum(B, [127, 128]), "uniform"]

    def guard(plan):
        expect(plan, B, 0, skew=True, has=(1, 2, 3, 16, 17, 18, 127, 128, 129))
        expect(plan, B, 1, skew=True, longest=B, nu=1)
        expect(plan, B, 2, skew=False, has=(1, 2, 3, 16, 17, 18, 129))
        expect(plan, B, 3, skew=False, has=(1, 127, 128))
        expect(plan, B, 4, skew=False)
    return B, dims, spectra, layout, guard


def case_threshold():
    """B - nu = 256 (not skewed) and 257 (skewed), with long and with short runs"""
    B = 2048
    dims = [3000, 3000, 3000, 3000, 40000]
    spectra = [H.fill_spectrum(B, [129, 129]), H.fill_spectrum(B, [129, 129], pairs=1),
               H.fill_spectrum(B, pairs=256), H.fill_spectrum(B, [3], pairs=255), "uniform"]

    def guard(plan):
        for f, sk in ((0, False), (1, True), (2, False), (3, True)):
            r = expect(plan, B, f, skew=sk)
            assert B - r["nu"] == (257 if sk else 256)
        expect(plan, B, 0, longest=129)
        expect(plan, B, 1, wg0_huge=2)
        expect(plan, B, 3, has=(3,))
    return B, dims, spectra, "scattered", guard


HUGE_COUNTS = (3, 5, 7, 16, 17, 33)


def case_huge_counts(B):
    """3, 5, 7, 16, 17, 33 runs of more than 128 members in workgroup 0 of their column: 16 / nr waves per run with nr
    not dividing 16, one, two and three rounds of the list"""
    dims = [9000] * len(HUGE_COUNTS) + [30000]
    spectra = [ranked_spectrum(B, wg0_ranks(B, n), huge_lens(n, n), extra=((1100, 17), (1101, 60), (1102, 3)))
               for n in HUGE_COUNTS] + ["uniform"]

    def guard(plan):
        for f, n in enumerate(HUGE_COUNTS):
            expect(plan, B, f, skew=True, wg0_huge=n, has=(17, 60, 3))
    return B, dims, spectra, "ranked", guard


def case_capacity(B):
    """127 runs of 129 members: as many as a column of 16384 can hold; at B = 16383 (identity spread) all of them
    in workgroup 0, eight rounds"""
    runs = [129] * 127
    dims = [300, 40000]
    spectra = [H.fill_spectrum(B, runs), "uniform"]

    def guard(plan):
        r = expect(plan, B, 0, skew=True, longest=129, nu=127 + (B - 127 * 129))
        assert (r["runs"] == 129).sum() == 127
        if B % 64:
            assert r["huge_per_wg"][0] == 127
    return B, dims, spectra, "hot", guard


def case_wide(F):
    """one column entirely one id beside uniform and skewed columns"""
    B = 2048
    dims = [500] + [20000] * (F - 1)
    sk = H.fill_spectrum(B, [B // 4, 300, 129, 100, 40, 17, 3], pairs=20)
    spectra = [[B]] + [sk if f % 5 == 1 else "uniform" for f in range(1, F)]
    layouts = "hot"

    def guard(plan):
        expect(plan, B, 0, skew=True, nu=1, longest=B)
        for f in range(1, F):
            expect(plan, B, f, skew=(f % 5 == 1))
    return B, dims, spectra, layouts, guard


SWEEP_B = (1, 63, 64, 65, 1000, 1025, 8191, 8192, 8193, 12345, 16383, 16384)


def case_sweep(B):
    """batch sizes around every multiple that a kernel branches on (64, 1024, 8192, the 16-byte perm stores): a
    skewed column with runs of more than 128 members wherever B allows, a uniform column, a column of short runs"""
    m = max(B, 8)
    dims = [m + 37, 3 * m + 11, m + 5]
    if B == 1:
        return B, dims, [[1], [1], [1]], "scattered", lambda plan: expect(plan, B, 0, skew=False, nu=1)
    if B <= 1 + FIX_SKEW:
        c0 = [B]                                             # one id: a run of B that is not skewed
    else:
        runs, ln = [], 129
        while sum(runs) + ln <= B // 2 and len(runs) < 6:
            runs.append(ln)
            ln += 71
        runs += [x for x in (3, 17, 18, 100, 128) if sum(runs) + x <= B - 40]
        c0 = H.fill_spectrum(B, runs, pairs=min(40, (B - sum(runs)) // 4))
    c2 = H.fill_spectrum(B, [3, 17], pairs=min(100, (B - 20) // 4)) if B >= 64 else "uniform"
    layout = "hot" if SWEEP_B.index(B) % 2 else "scattered"

    def guard(plan):
        if B > 1 + FIX_SKEW:
            r = expect(plan, B, 0, skew=True)
            assert r["runs"].max() > FIX_HUGE
        else:
            expect(plan, B, 0, skew=False, nu=1, longest=B)
        expect(plan, B, 2, skew=False)
    return B, dims, [c0, "uniform", c2], layout, guard


# sort words (key << bits(B)) | example of every width the radix passes branch on: bits(max_key + 1) + bits(B)
# in {8, 14, 15, 21, 22, 28, 29, 32}, key widths on either side of a multiple of 7, kpt 8 and 16
WIDTHS = [(16, 16), (64, 256), (128, 256), (256, 128), (1024, 2048), (8192, 256), (16384, 256), (4096, 1 << 14),
          (8192, 1 << 15), (12345, 1 << 15), (16383, 1 << 18), (8191, 1 << 19)]


def _bits(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def case_width(B, D):
    """widest field of dim D (keys 0 and D - 1 in every column), fields of dim 1 and 2"""
    n_runs = min(D, max(2, B // 3))                          # fewer, longer runs when the field is narrow
    spec = (1 + H.rng(B + D).multinomial(B - n_runs, np.full(n_runs, 1.0 / n_runs))).tolist()
    dims = [D, 1, 2, min(D, 7)]
    spectra = [spec, [B], H.fill_spectrum(B, [B - 1]) if B >= 2 else [1], "uniform"]

    def guard(plan):
        expect(plan, B, 1, nu=1)
        expect(plan, B, 2, nu=min(2, B))
        assert plan["col_uid"][0][0] == 0 and plan["col_uid"][0][int(plan["col_nu"][0]) - 1] == D - 1
    return B, dims, spectra, "scattered", guard


def case_one_id_short():
    """a column that is one id at B = 1000: the run of 1000 members (whole-workgroup path) stays below LONG_RUN, so its
    row and its dK0 rows are held to close(), not to the n * 2^-24 * sum|members| bound"""
    B = 1000
    dims = [500, 3000, 40000]
    spectra = [[B], H.fill_spectrum(B, [300, 129, 17, 3], pairs=20), "uniform"]

    def guard(plan):
        expect(plan, B, 0, skew=True, nu=1, longest=B)
        expect(plan, B, 1, skew=True, has=(300, 129, 17, 3))
    return B, dims, spectra, "scattered", guard


CASES = ([("lengths-" + lay, (lambda lay=lay: case_lengths(lay))) for lay in ("scattered", "clustered", "hot")] +
         [("threshold", case_threshold)] +
         [("huge-counts-B%d" % b, (lambda b=b: case_huge_counts(b))) for b in (8192, 8100)] +
         [("capacity-B%d" % b, (lambda b=b: case_capacity(b))) for b in (16384, 16383)] +
         [("one-id-F%d" % F, (lambda F=F: case_wide(F))) for F in (26,)] +
         [("sweep-B%d" % b, (lambda b=b: case_sweep(b))) for b in SWEEP_B] +
         [("width-%d-B%d-D%d" % (_bits(D) + _bits(B), B, D), (lambda B=B, D=D: case_width(B, D))) for B, D in WIDTHS] +
         [("one-id-F28", (lambda: case_wide(28))), ("one-id-B1000", case_one_id_short)])

# Cases run with seed 7 + their index, except these.  one-id-F28 at its index seed (16) puts example 512 at a layer-1
# pre-activation of 2.0e-8 for unit 29 (1.6e-8 of its sum of |terms|): the fp32 kernel rounds it to the other side of
# the ReLU than the fp64 oracle, and that example's delta (8.8e-7) appeared as the whole error of db0[29] and of
# dK0[:, 29] (= x_512 * 8.8e-7).  Seed 10 keeps every pre-activation of the batch >= 5.9e-6 of its terms from the kink.
SEEDS = {"one-id-F28": 10, "one-id-B1000": 12}
KINK_FREE = 1e-6                                              # smallest ReLU margin a case with a chosen seed must keep


def case_seed(name, fn):
    return SEEDS.get(name, 7 + CASES.index((name, fn)))


def build_case(fn, seed):
    B, dims, spectra, layout, guard = fn()
    offsets = H.field_offsets(dims)
    host = H.plan_batch(B, dims, offsets, spectra, layout, seed)
    return B, dims, offsets, host, guard


# ------------------------------------------------------------------------------------------------
# section 2 / 3: every case against the oracle, eager and replayed, deterministic, equal to the generic step
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fn", CASES, ids=[c[0] for c in CASES])
def test_plan_case_matches_oracle(name, fn):
    from explicit_tf2_recommendation_amd import engine, data
    seed = case_seed(name, fn)
    B, dims, offsets, host, guard = build_case(fn, seed)
    F, V = len(dims), int(sum(dims))
    layer, names = make_layer(F, V, seed)
    dbatch = data.to_device(host)
    ref = oracle(layer, names, host)
    if name in SEEDS:
        assert ref["margin"] >= KINK_FREE, (name, ref["margin_where"])   # the seed was chosen for this

    eager = engine.DeepFMFusedStep(layer, B, dims, offsets, use_graph=False)
    loss = eager(dbatch).item()
    eager.check_flags()
    plan = read_plan(eager, last_plan_buf(eager))
    check_plan(plan, host, names, offsets, name)
    guard(plan)                                              # the case is in the regime it was built for
    check_oracle(eager, loss, ref, name + "/eager")
    want = snapshot(eager)
    eager(dbatch)
    same(want, snapshot(eager), name + "/run-to-run")

    graphed = engine.DeepFMFusedStep(layer, B, dims, offsets, use_graph=True)
    for _ in range(3):                                       # eager, eager + capture, replay
        loss = graphed(dbatch).item()
    assert len(graphed._graphs) == 1
    graphed.check_flags()
    check_oracle(graphed, loss, ref, name + "/graph")
    same(want, snapshot(graphed), name + "/graph-vs-eager")

    generic = engine.DeepFMTrainStep(layer, B, optimizer=None, use_graph=False)
    lg = generic(dbatch).item()
    assert abs(lg - want["loss"].item()) <= 1e-5 * max(1, abs(lg))
    gg, gf = generic.gradients(), eager.gradients()
    for k in DENSE:
        assert close(gf[k].cpu().numpy(), gg[k].cpu().numpy(), 1e-5), (name, k)
    nu = int(gf["embed.embeddings"][2].item())
    assert nu == int(gg["embed.embeddings"][2].item())
    assert torch.equal(gf["embed.embeddings"][0][:nu], gg["embed.embeddings"][0][:nu])
    for k in TABLES:
        assert close(gf[k][1][:nu].cpu().numpy(), gg[k][1][:nu].cpu().numpy(), 1e-5), (name, k)


@pytest.mark.parametrize("B,D", WIDTHS)
def test_sort_word_width_boundary(B, D):
    """engine.py accepts the config whose widest sort word is legal and refuses it one step past, in both clauses:
    bits(max_key + 1) + bits(B) > 32, and a word that would reach the pad word 0xFFFFFFFF"""
    from explicit_tf2_recommendation_amd import engine
    layer, names = make_layer(2, 64, 3)
    offs = [0, 1 << 24]                                      # (the constructor reads dims and offsets only)
    engine.DeepFMFusedStep(layer, B, [D, 2], offs, use_graph=False)
    bits = _bits(D) + _bits(B)
    if bits == 32:
        # first clause: one more key bit
        with pytest.raises(NotImplementedError):
            engine.DeepFMFusedStep(layer, B, [D + 1, 2], offs, use_graph=False)
        # second clause: the same 32 bits, but the widest word is the pad word
        with pytest.raises(NotImplementedError):
            engine.DeepFMFusedStep(layer, B + 1, [D, 2], offs, use_graph=False)
        with pytest.raises(NotImplementedError):
            engine.DeepFMFusedStep(layer, B, [D, 2 * D], offs, use_graph=False)


# ------------------------------------------------------------------------------------------------
# section 4: the optimizer inside the post launch on adversarial batches
# ------------------------------------------------------------------------------------------------
def adversarial_batches(B, n, seed):
    """skewed column with 17 runs of > 128 members in workgroup 0, B - nu = 257 and 256, a hot head, a uniform column"""
    dims = [5000, 5000, 5000, 5000, 8000, 600]
    offsets = H.field_offsets(dims)
    out = []
    for i in range(n):
        spectra = [ranked_spectrum(B, wg0_ranks(B, 17), huge_lens(17, i)), H.fill_spectrum(B, [3], pairs=255),
                   H.fill_spectrum(B, pairs=256), H.fill_spectrum(B, [B // 4, 300, 129, 100, 17, 3], pairs=10),
                   "uniform", [B] if i % 2 else H.fill_spectrum(B, [B - 200])]
        out.append(H.plan_batch(B, dims, offsets, spectra, "ranked" if i % 2 else "scattered", seed + i))
    return dims, offsets, out


@pytest.mark.parametrize("B", [4096, 4000])
def test_lazy_adam_in_post_launch_on_adversarial_batches(B):
    """test_fused_step_lazy_adam_in_post_launch on the batches above: a row updated by two workgroups, or by none,
    under the (ln > 2) == spread rule would leave it off the oracle's lazy Adam"""
    from explicit_tf2_recommendation_amd import engine, data
    dims, offsets, host = adversarial_batches(B, 4, 100 + B)
    F, V = len(dims), int(sum(dims))
    la, names = make_layer(F, V, 31)
    lb, _ = make_layer(F, V, 31)
    lb.load_state_dict(la.state_dict())
    a = engine.DeepFMFusedStep(la, B, dims, offsets, optimizer="lazy_adam", lr=0.01, use_graph=False)
    b = engine.DeepFMFusedStep(lb, B, dims, offsets, optimizer="lazy_adam", lr=0.01, use_graph=False, direct=False)
    assert a._fused_lazy() and not b._fused_lazy()
    emb = la.embed.embeddings.detach().cpu().numpy().copy()
    w = la.w.embeddings.detach().cpu().numpy().copy()
    st = {"e": (emb.copy(), np.zeros_like(emb), np.zeros_like(emb)), "w": (w.copy(), np.zeros_like(w), np.zeros_like(w))}
    for t in range(1, 5):
        hb = host[t - 1]
        ref = oracle(la, names, hb)
        touched = ref["touched"]
        st["e"] = L.adam_rows_step(*st["e"], touched, ref["embed.embeddings"].astype(np.float32), t, lr=0.01,
                                   dt=np.float32)
        st["w"] = L.adam_rows_step(*st["w"], touched, ref["w.embeddings"].astype(np.float32), t, lr=0.01, dt=np.float32)
        batch = data.to_device(hb)
        a(batch)
        b(batch)
        a.check_flags()
        if t == 2:                                           # (batch 1: ranked layout)
            plan = read_plan(a, last_plan_buf(a))
            expect(plan, B, 0, skew=True, wg0_huge=17)
            expect(plan, B, 1, skew=True)
            expect(plan, B, 2, skew=False)
        for (k, p), (_, q) in zip(la.named_parameters(), lb.named_parameters()):
            assert (p - q).abs().max().item() <= 1e-6, (t, k)
        assert np.abs(la.embed.embeddings.detach().cpu().numpy() - st["e"][0]).max() <= 2e-5, t
        assert np.abs(la.w.embeddings.detach().cpu().numpy() - st["w"][0]).max() <= 2e-5, t
    assert (a.state["embed.embeddings"][0] - b.state["embed.embeddings"][0]).abs().max().item() <= 1e-6
    assert (a.state["w.embeddings"][1] - b.state["w.embeddings"][1]).abs().max().item() <= 1e-6


@pytest.mark.parametrize("B,use_graph", [(4096, False), (4000, True)])
def test_keras_adam_lazy_equals_dense_sweep_on_adversarial_batches(B, use_graph):
    """test_keras_adam_evaluated_lazily_equals_the_dense_sweep_bit_for_bit on the batches above"""
    from explicit_tf2_recommendation_amd import engine, data
    dims, offsets, host = adversarial_batches(B, 4, 300 + B)
    F, V = len(dims), int(sum(dims))
    la, names = make_layer(F, V, 41)
    lb, _ = make_layer(F, V, 41)
    lb.load_state_dict(la.state_dict())
    a = engine.DeepFMFusedStep(la, B, dims, offsets, optimizer="keras_adam", lr=0.01, use_graph=False)
    b = engine.DeepFMFusedStep(lb, B, dims, offsets, optimizer="keras_adam_lazy", lr=0.01, use_graph=use_graph)
    batches = [data.to_device(h) for h in host]
    order = [0, 1, 2, 0, 3, 1, 1]
    for i in order:
        assert a(batches[i]).item() == b(batches[i]).item(), i
    last = b._last.cpu().numpy()
    assert ((last < len(order)) & (last > 0)).any() and not torch.equal(la.embed.embeddings, lb.embed.embeddings)
    b.flush()
    for (k, p), (_, q) in zip(la.named_parameters(), lb.named_parameters()):
        assert torch.equal(p, q), k
    for k in TABLES:
        assert torch.equal(a.state[k][0], b.state[k][0].contiguous()), k
        assert torch.equal(a.state[k][1], b.state[k][1].contiguous()), k


# ------------------------------------------------------------------------------------------------
# section 5: long many() cycles, the split of the next call's sorts into launches of GROUP batches
# ------------------------------------------------------------------------------------------------
THEN_LENGTHS = (1, 8, 9, 10, 17, 25, 31, 32)


def many_pool(F, n, seed):
    B = 512
    dims = [700 + 13 * f for f in range(F)]
    offsets = H.field_offsets(dims)
    pool = []
    for i in range(n):
        if i % 2:
            spectra = [H.fill_spectrum(B, [129 + i, 40, 17, 3], pairs=60) if f % 3 == 0 else "uniform" for f in range(F)]
        else:
            spectra = [H.fill_spectrum(B, [200, 129, 18], pairs=i) if f % 4 == 1 else
                       ([B] if f % 4 == 2 else "uniform") for f in range(F)]
        pool.append(H.plan_batch(B, dims, offsets, spectra, ("hot", "scattered", "clustered")[i % 3], seed + i))
    return B, dims, offsets, pool


@pytest.mark.parametrize("F", [1, 3, 26, 28])
def test_many_cycles_equal_single_calls(F):
    """state after many() (lazy Adam inside, so every step's row sums reach the parameters) bit-identical to the same
    batches one call at a time; announced plans, read back from their buffers, equal to their definition; the next
    call consumes them, also mixed with batches nobody announced; 33 batches are refused"""
    from explicit_tf2_recommendation_amd import engine, data
    B, dims, offsets, pool = many_pool(F, 40, 500 + F)
    V = int(sum(dims))
    names = ["f%d" % i for i in range(F)]
    dev = [data.to_device(h) for h in pool]
    l1, _ = make_layer(F, V, 61)
    lm, _ = make_layer(F, V, 61)
    lp, _ = make_layer(F, V, 61)
    lm.load_state_dict(l1.state_dict())
    lp.load_state_dict(l1.state_dict())
    one = engine.DeepFMFusedStep(l1, B, dims, offsets, optimizer="lazy_adam", lr=0.01, use_graph=False)
    multi = engine.DeepFMFusedStep(lm, B, dims, offsets, optimizer="lazy_adam", lr=0.01, use_graph=True)
    plain = engine.DeepFMFusedStep(lp, B, dims, offsets, optimizer="lazy_adam", lr=0.01, use_graph=False)  # many(), eager
    assert multi.GROUP == plain.GROUP == 256 // F
    steps = ((lm, multi), (lp, plain))

    def check(tag):
        for lx, sx in steps:
            for (k, p), (_, q) in zip(l1.named_parameters(), lx.named_parameters()):
                assert torch.equal(p, q), (tag, sx.use_graph, k)
            for k in one.state:
                assert torch.equal(one.state[k][0], sx.state[k][0]) and torch.equal(one.state[k][1], sx.state[k][1]), \
                    (tag, sx.use_graph, k)
            same(snapshot(one), snapshot(sx), (tag, sx.use_graph))

    def run(seq, then):
        for i in seq:
            one(dev[i])
        for _, sx in steps:
            sx.many([dev[i] for i in seq], then=[dev[i] for i in then] if then else None)
            sx.check_flags()

    for rep, m in enumerate(THEN_LENGTHS):
        seq = [(3 * rep + j) % 40 for j in range(2)]
        then = [(5 * rep + 7 + j) % 40 for j in range(m)]
        # (graphs: the two calls alternate the plan halves, so cycles 1, 3, 5 and 2, 4 repeat each other: eager,
        # captured, replayed)
        for cyc in range(5 if m in (10, 32) else 1):
            run(seq, then)
            check(("many", m, cyc))
            # the announced plans, before anything consumes them
            for _, sx in steps:
                for j, i in enumerate(then):
                    buf = sx._prefetched[sx._key([dev[i][nm] for nm in names])]
                    check_plan(read_plan(sx, buf), pool[i], names, offsets, ("announced", sx.use_graph, m, j))
            # the next call: the announced batches (the last one replaced by a batch nobody announced when m > 2)
            nxt = then[:-1] + [(then[-1] + 11) % 40] if m > 2 else then
            run(nxt, None)
            check(("consumed", m, cyc))
    with pytest.raises(ValueError):
        multi.many([dev[i % 40] for i in range(33)])
    with pytest.raises(ValueError):
        multi.many([dev[0]], then=[dev[i % 40] for i in range(33)])
    assert len(multi._graphs) >= 2 and len(plain._graphs) == 0


# ------------------------------------------------------------------------------------------------
# section 6: the sharded step at world size 1 on the same kind of batches (dedup.hip's owner path)
# ------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def test_sharded_world1_on_adversarial_batches():
    import torch.distributed as dist
    from explicit_tf2_recommendation_amd import engine, data
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_free_port())
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda", 0))
    try:
        for tag, fn in (("huge-counts", lambda: case_huge_counts(8192)), ("threshold", case_threshold),
                        ("sweep-B1000", lambda: case_sweep(1000)), ("one-id", lambda: case_lengths("hot"))):
            B, dims, offsets, host, guard = build_case(fn, 71)
            F, V = len(dims), int(sum(dims))
            layer, names = make_layer(F, V, 71)
            dbatch = data.to_device(host)
            ref = oracle(layer, names, host)
            fused = engine.DeepFMFusedStep(layer, B, dims, offsets, use_graph=False)
            sh = engine.ShardedDeepFMStep(layer, B, dims, offsets)
            lf = fused(dbatch).item()
            guard(read_plan(fused, last_plan_buf(fused)))
            ls = sh(dbatch).item()
            sh.check_flags()
            assert abs(lf - ls) <= 1e-6, tag
            gf = fused.gradients()
            for k, v in sh.g.items():
                assert torch.equal(v, gf[k]), (tag, k)        # same kernel on the same rows: bitwise
            ids, rows_e, rows_w, nu = sh.table_grad
            nu = int(nu.item())
            assert nu == ref["touched"].size and np.array_equal(ids[:nu].cpu().numpy(), ref["touched"]), tag
            assert rows_ok(rows_e[:nu].cpu().numpy(), ref, "embed.embeddings"), tag
            assert rows_ok(rows_w[:nu].cpu().numpy(), ref, "w.embeddings"), tag
    finally:
        dist.destroy_process_group()
