"""GPU tests of the per-column plan sort (csrc/colsort.hip) through rec_colsort_plan_dest_i64 itself: every field of the
plan -- perm, col_uid, col_seg (tail = B), col_nu, dloc -- bit for bit against tests.helpers.host_plan, in every branch
of the kernel: the bucket path and the radix passes (bucket_path() mirrors the kernel's choice), 1 to 4 radix passes
(rec_colsort_digits says which each case reaches), 8 or 16 words per thread (B <= 8192 or not), B around the multiples
the kernel branches on, 1 / 26 / 256 columns per launch, and uniform, Zipf, one-id, all-distinct and huge-run columns."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu


def digits(B, max_key):
    from explicit_tf2_recommendation_amd._lib import lib
    p, d = C.c_int(0), C.c_int(0)
    assert lib.rec_colsort_digits(B, max_key, C.byref(p), C.byref(d)) == 0
    return p.value, d.value


BKB, BIG, PROBE = 13, 32, 16       # csrc/colsort.hip: CS_BKB, CS_BIG, CS_PROBE


def bits(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def bucket_path(col, lo, max_key):
    """True when the kernel sorts this column on its bucket path: no bucket of the top BKB bits of the sort words
    (key << bits(B) | example) holds more than BIG words, and no round of 64 consecutive examples has more than PROBE
    in the bucket of its first one; otherwise it runs the radix passes"""
    col = np.asarray(col, np.int64).reshape(-1)
    B = col.size
    pb, kb = bits(B), max(1, int(max_key).bit_length())
    bk = (((col - lo) << pb) | np.arange(B)) >> max(0, kb + pb - BKB)
    for g in range(0, B, 64):
        if int(np.count_nonzero(bk[g:g + 64] == bk[g])) > PROBE:
            return False
    return int(np.bincount(bk).max()) <= BIG


def sort(cols, dims, offsets):
    """one launch over the columns (numpy int64 [B] each, column f inside [offsets[f], offsets[f] + dims[f]))"""
    from explicit_tf2_recommendation_amd._lib import lib, check
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    F, B = len(cols), cols[0].size
    i32, i64 = dict(dtype=torch.int32, device="cuda"), dict(dtype=torch.int64, device="cuda")
    out = dict(perm=torch.full((F, B), -7, **i32), col_uid=torch.full((F, B), -7, **i64),
               col_seg=torch.full((F, B + 1), -7, **i32), col_nu=torch.full((F,), -7, **i32),
               dloc=torch.full((F, B), -7, **i32))
    bad = torch.zeros(1, **i32)
    ws = torch.empty(lib.rec_colsort_workspace_bytes(B, F), dtype=torch.uint8, device="cuda")
    dcols = [torch.from_numpy(np.ascontiguousarray(c, dtype=np.int64)).cuda() for c in cols]
    lo = torch.tensor(offsets, **i64)
    vp = lambda t: C.c_void_p(t.data_ptr())
    arr = (C.c_void_p * F)(*[c.data_ptr() for c in dcols])
    V = int(offsets[-1]) + int(dims[-1])
    check(lib.rec_colsort_plan_dest_i64(arr, F, B, V, vp(lo), max(dims) - 1, vp(out["perm"]), vp(out["col_uid"]),
                                        vp(out["col_seg"]), vp(out["col_nu"]), vp(out["dloc"]), vp(bad), vp(ws),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rec_colsort_plan_dest_i64")
    torch.cuda.synchronize()
    assert bad.item() == 0
    return {k: v.cpu().numpy() for k, v in out.items()}


def check(got, cols, offsets):
    for f, col in enumerate(cols):
        want = H.host_plan(col, offsets[f])
        nu = int(want["col_nu"])
        assert int(got["col_nu"][f]) == nu, f
        assert np.array_equal(got["perm"][f], want["perm"]), f
        assert np.array_equal(got["col_uid"][f][:nu], want["col_uid"]), f
        assert np.all(got["col_uid"][f][nu:] == -7), f          # nothing written past the unique ids
        assert np.array_equal(got["col_seg"][f], want["col_seg"]), f
        assert np.array_equal(got["dloc"][f], want["dloc"]), f


def columns(B, dims, offsets, spectra, layout="scattered", seed=0):
    b = H.plan_batch(B, dims, offsets, spectra, layout, seed)
    return [b["f%d" % f].reshape(-1) for f in range(len(dims))]


# (B, widest field dim) -> passes x digit bits: every pass count, both words-per-thread variants, the widest legal words
WIDTHS = [(64, 2, (1, 1)), (1000, 1024, (1, 10)), (1000, 1025, (2, 6)), (8192, 384_616, (2, 10)),
          (8192, (1 << 19) - 1, (2, 10)), (8193, 5000, (2, 7)), (16384, (1 << 18) - 1, (2, 9)),
          (2048, (1 << 20) + 1, (3, 7)), (16, (1 << 28) - 1, (3, 10)), (2, (1 << 31) - 1, (4, 8))]


@pytest.mark.parametrize("B,D,want", WIDTHS)
def test_key_widths(B, D, want):
    """a uniform column of dim D (keys 0 and D - 1 present), one-id, two-id and dim-7 columns"""
    assert digits(B, D - 1) == want                       # the case reaches the pass count it targets
    dims = [D, 1, 2, min(D, 7)]
    offsets = H.field_offsets(dims)
    spectra = ["uniform", [B], H.fill_spectrum(B, [B - 1]) if B >= 2 else [1], "uniform"]
    cols = columns(B, dims, offsets, spectra, seed=B + D)
    paths = [bucket_path(c, offsets[f], D - 1) for f, c in enumerate(cols)]
    if B > BIG and max(1, (D - 1).bit_length()) >= BKB:
        assert not paths[1]                               # one id, B words in one bucket: the radix passes
    if B >= 1000 and D >= 4 * B:
        assert paths[0]                                   # a wide uniform column takes the bucket path
    check(sort(cols, dims, offsets), cols, offsets)


SWEEP_B = (1, 63, 64, 65, 1000, 1023, 1024, 1025, 8191, 8192, 8193, 12345, 16383, 16384)


@pytest.mark.parametrize("B", SWEEP_B)
def test_batch_sizes(B):
    """B around every multiple the kernel branches on (64 lanes, 1024 threads, 8 or 16 words per thread, the 16-byte
    perm stores): uniform, Zipf(1.05), one id, all distinct, runs longer than a wave and than a thread's words"""
    m = max(B, 8)
    dims = [3 * m + 11, 5 * m + 7, 17, m + 3, 2 * m]
    offsets = H.field_offsets(dims)
    r = H.rng(B)
    big = [x for x in (B // 2, B // 5, 129, 65, 9) if x >= 2]
    runs = []
    for x in big:
        if sum(runs) + x <= B:
            runs.append(x)
    spectra = ["uniform", "uniform", [B], [1] * B, H.fill_spectrum(B, runs)]
    cols = columns(B, dims, offsets, spectra, "hot" if B % 2 else "scattered", seed=B)
    z = np.minimum(r.zipf(1.05, size=B) - 1, dims[1] - 1)
    cols[1] = offsets[1] + z                              # Zipf ids: the hottest id holds ~10 % of the lookups
    check(sort(cols, dims, offsets), cols, offsets)


@pytest.mark.parametrize("F", [1, 26, 256])
@pytest.mark.parametrize("dist", ["uniform", "zipf", "one-id"])
def test_columns_per_launch(F, dist):
    """the headline shape (B = 8192, 10M ids over 26 fields: 19-bit keys, 2 passes) at 1, 26 and 256 columns"""
    B = 8192
    dims = [10_000_000 // 26] * F
    offsets = H.field_offsets(dims)
    assert digits(B, dims[0] - 1) == (2, 10)
    r = H.rng(F * 7 + len(dist))
    cols = []
    for f in range(F):
        if dist == "uniform":
            x = r.integers(0, dims[f], size=B)
        elif dist == "zipf":
            x = np.minimum(r.zipf(1.05, size=B) - 1, dims[f] - 1)
        else:
            x = np.full(B, r.integers(0, dims[f]))
        cols.append(offsets[f] + x.astype(np.int64))
    paths = {bucket_path(c, offsets[f], dims[0] - 1) for f, c in enumerate(cols)}
    assert paths == {dist == "uniform"}                   # uniform: bucket path; Zipf heads, one id: radix passes
    check(sort(cols, dims, offsets), cols, offsets)


@pytest.mark.parametrize("run", [BIG - 1, BIG, BIG + 1, 4 * BIG])
@pytest.mark.parametrize("B", [8192, 16384])
def test_bucket_threshold(B, run):
    """one bucket of exactly `run` words (equal ids), every other bucket one (B = 8192) or two (B = 16384: 2^13
    buckets) words: at most BIG words take the bucket path, more take the radix passes"""
    D = (1 << 19) - 1 if B == 8192 else (1 << 18) - 1
    pb, kb = bits(B), D.bit_length()
    step, per = 1 << (kb + pb - BKB - pb), B // 8192        # keys per bucket, other words per bucket
    r = H.rng(B + run)
    n = B - run
    keys = np.concatenate([np.arange(n, dtype=np.int64) * (step // per),
                           np.full(run, (-(-n // per) + 1) * step, np.int64)])
    assert keys.max() < D
    col = r.permutation(keys)
    dims, offsets = [D, 2], [0, D]
    other = np.full(B, D, np.int64)
    assert bucket_path(col, 0, D - 1) == (run <= BIG)
    check(sort([col, other], dims, offsets), [col, other], offsets)


def test_too_many_columns_refused():
    from explicit_tf2_recommendation_amd._lib import lib
    F, B = 257, 64
    col = torch.zeros(B, dtype=torch.int64, device="cuda")
    arr = (C.c_void_p * F)(*([col.data_ptr()] * F))
    t = torch.zeros(F * (B + 1), dtype=torch.int64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    assert lib.rec_colsort_plan_dest_i64(arr, F, B, 100, p, 10, p, p, p, p, p, p, p, None) == -2
