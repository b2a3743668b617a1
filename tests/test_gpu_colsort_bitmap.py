"""GPU tests of the bitmap path of the per-column plan sort (csrc/colsort.hip): every field of the plan -- perm, col_uid
(nothing written past col_nu), col_seg (tail = B), col_nu, dloc -- bit for bit against tests.helpers.host_plan, one sort
launch per case.  path() mirrors the kernel's choice per column (hot-bucket probe, rec_colsort_bitmap_limits, the count
of slow lookups, the bucket sizes), and every case asserts the branch it is meant for."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu

BKB, BIG, PROBE = 13, 32, 16       # csrc/colsort.hip: CS_BKB, CS_BIG, CS_PROBE
RANGE = 13 * 1024 * 32             # keys the bitmap covers (CS_BM_WORDS words of 32)
HEAD = 10_000_000 // 26            # the headline's field dim: 384,615 keys


def bits(n):
    b = 1
    while (1 << b) < n:
        b += 1
    return b


def limits(B, max_key):
    from explicit_tf2_recommendation_amd._lib import lib
    w, c = C.c_int(-1), C.c_int(-1)
    assert lib.rec_colsort_bitmap_limits(B, max_key, C.byref(w), C.byref(c)) == 0
    return w.value, c.value


def slow_lookups(keys):
    """lookups that share a 32-key word with a duplicated key"""
    wd = keys >> 5
    n = np.bincount(wd)
    d = np.bincount(np.unique(keys) >> 5, minlength=n.size)
    return int(n[n > d].sum())


def path(col, lo, max_key):
    """'bitmap', 'bucket' or 'radix': the branch of the kernel this column takes in a launch whose largest key is
    max_key"""
    col = np.asarray(col, np.int64).reshape(-1)
    B = col.size
    pb, kb = bits(B), max(1, int(max_key).bit_length())
    keys = np.clip(col - lo, 0, (1 << kb) - 1)
    words, cap = limits(B, max_key)
    if words and keys.max() > max_key:
        return "radix"                                    # a key without a bit
    bk = ((keys << pb) | np.arange(B)) >> max(0, kb + pb - BKB)
    for g in range(0, B, 64):
        if int(np.count_nonzero(bk[g:g + 64] == bk[g])) > PROBE:
            return "radix"                                # the probe found a hot bucket
    if words and slow_lookups(keys) <= cap:
        return "bitmap"
    return "bucket" if int(np.bincount(bk).max()) <= BIG else "radix"


def launch(cols, dims, offsets):
    """one launch over the columns (numpy int64 [B] each, column f inside [offsets[f], offsets[f] + dims[f])): the five
    output arrays over a -7 fill, and the bad flag"""
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
    return {k: v.cpu().numpy() for k, v in out.items()}, int(bad.item())


def exact(got, cols, offsets, only=None):
    for f, col in enumerate(cols):
        if only is not None and f not in only:
            continue
        want = H.host_plan(col, offsets[f])
        nu = int(want["col_nu"])
        assert int(got["col_nu"][f]) == nu, f
        assert np.array_equal(got["perm"][f], want["perm"]), f
        assert np.array_equal(got["col_uid"][f][:nu], want["col_uid"]), f
        assert np.all(got["col_uid"][f][nu:] == -7), f          # nothing written past the unique ids
        assert np.array_equal(got["col_seg"][f], want["col_seg"]), f
        assert np.array_equal(got["dloc"][f], want["dloc"]), f


def run(cols, dims, offsets):
    got, bad = launch(cols, dims, offsets)
    assert bad == 0
    exact(got, cols, offsets)
    return [path(c, offsets[f], max(dims) - 1) for f, c in enumerate(cols)]


EDGE_DIMS = (1, 31, 32, 33, 64, 65, 1000, 384_625, RANGE, RANGE + 1)


@pytest.mark.parametrize("B", [1, 31, 32, 33, 64, 65, 1000, 1024, 1025, 8191, 8192])
def test_word_and_size_edges(B):
    """every B with every widest field dim (one launch each: the widest dim sets the bitmap's word count -- 1, 2, 3
    words, an odd count, the full range, one key past it), uniform ids with keys 0 and dim - 1 present, next to a
    column of half the dim"""
    taken = {}
    for D in EDGE_DIMS:
        dims = [D, max(1, D // 2)]
        offsets = H.field_offsets(dims)
        b = H.plan_batch(B, dims, offsets, ["uniform", "uniform"], seed=B * 31 + D % 1009)
        cols = [b["f0"].reshape(-1), b["f1"].reshape(-1)]
        if B >= 2:
            assert cols[0].min() == 0 and cols[0].max() == D - 1
        words, cap = limits(B, D - 1)
        assert words == (0 if D > RANGE else (D + 31) // 32)
        taken[D] = run(cols, dims, offsets)
        if D > RANGE:
            assert "bitmap" not in taken[D]               # one key past the range: exact on the old paths
        elif D >= 384_625:
            assert taken[D][0] == "bitmap"                # a wide field: few words with a duplicated id
        elif B <= cap:
            # at most `cap` lookups cannot overflow the list, and the probe's buckets hold at most 16 words here (a
            # bucket of the top 13 word bits: one key and the top position bits, or a few keys)
            assert taken[D] == ["bitmap", "bitmap"], (D, taken[D])
        # (narrow fields at B >= 1000 go where path() says: the list overflows, then the bucket or the radix path)


def special_column(B, dim, groups, seed):
    """groups: (key, examples) pairs placed as given; every other example gets a key of its own in a 32-key word that no
    group and no other filler uses"""
    r = H.rng(seed)
    col = np.full(B, -1, np.int64)
    used = set()
    for key, ex in groups:
        assert 0 <= key < dim
        col[list(ex)] = key
        used.add(key >> 5)
    free = np.array([w for w in range(dim // 32) if w not in used])
    rest = np.flatnonzero(col < 0)
    col[rest] = r.choice(free, rest.size, replace=False) * 32 + r.integers(0, 32, rest.size)
    return col


def test_duplicates_inside_a_word():
    B, dim = 1100, 64 * 1100 + 8          # 2201 words, the last one partly used (keys 70400 .. 70407)
    last = dim - 8
    cases = [
        [(100 * 32 + 7, [5, 900]), (100 * 32 + 3, [40]), (100 * 32 + 20, [41])],     # a pair, singles below and above it
        [(200 * 32 + 9, [1099, 64, 512])],                                           # a triple over three waves
        [(300 * 32 + 1, [10, 20]), (300 * 32 + 30, [15, 1030]), (300 * 32 + 12, [17])],   # two duplicated keys, one word
        [(last + 5, [0, 1099]), (last + 7, [3])],                                    # the last, partly used word
        [(400 * 32, [7, 70]), (401 * 32 + 31, [8, 80]), (402 * 32, [9, 90]), (402 * 32 + 31, [91, 92])],   # bit 0, bit 31
        # a run whose members lie at descending examples relative to its word's other lookups: the head is example 2
        [(500 * 32 + 16, [1090, 700, 300, 2]), (500 * 32 + 15, [1091]), (500 * 32 + 17, [1]), (500 * 32 + 16 + 8, [0, 1095])],
    ]
    cols = [special_column(B, dim, g, 11 + i) for i, g in enumerate(cases)]
    dims = [dim] * len(cols)
    offsets = H.field_offsets(dims)
    cols = [c + offsets[f] for f, c in enumerate(cols)]
    for f, g in enumerate(cases):                         # the slow lookups are exactly the groups' members
        assert slow_lookups(cols[f] - offsets[f]) == sum(len(ex) for _, ex in g)
    assert run(cols, dims, offsets) == ["bitmap"] * len(cols)


def test_list_capacity():
    """exactly cap - 1, cap and cap + 1 slow lookups (pairs in otherwise empty words, one word of a pair and a single for
    the odd counts): the first two take the bitmap path, the third the bucket path"""
    B, dim = 8192, 384_625
    cap = limits(B, dim - 1)[1]
    cols = []
    for n in (cap - 1, cap, cap + 1):
        groups, e = [], 0
        if n % 2:
            groups += [(32 * 5 + 4, [e, e + 1]), (32 * 5 + 9, [e + 2])]
            e, n = 3, n - 3
        for i in range(n // 2):
            groups.append((32 * (10 + 3 * i) + (i % 32), [e + 2 * i, B - 1 - 2 * i]))
        cols.append(special_column(B, dim, groups, 100 + n))
    assert [slow_lookups(c) for c in cols] == [cap - 1, cap, cap + 1]
    dims = [dim] * 3
    offsets = H.field_offsets(dims)
    cols = [c + offsets[f] for f, c in enumerate(cols)]
    assert run(cols, dims, offsets) == ["bitmap", "bitmap", "bucket"]


def headline_column(r, kind, dim=HEAD):
    B = 8192
    if kind == "uniform":
        return r.integers(0, dim, size=B).astype(np.int64)
    if kind == "zipf":
        return np.minimum(r.zipf(1.05, size=B) - 1, dim - 1).astype(np.int64)
    if kind == "one-id":
        return np.full(B, r.integers(0, dim), np.int64)
    return r.integers(0, 7, size=B).astype(np.int64)      # dim-7


def test_determinism():
    """the same launch twice on 26 uniform headline columns: all five output arrays byte for byte (every count of the
    slow list is over a set that a barrier has completed, so the order of the LDS atomics cannot show)"""
    r = H.rng(26)
    dims = [HEAD] * 26
    offsets = H.field_offsets(dims)
    cols = [offsets[f] + headline_column(r, "uniform") for f in range(26)]
    cap = limits(8192, HEAD - 1)[1]
    assert all(0 < slow_lookups(c - offsets[f]) <= cap for f, c in enumerate(cols))
    assert {path(c, offsets[f], HEAD - 1) for f, c in enumerate(cols)} == {"bitmap"}
    a, bad_a = launch(cols, dims, offsets)
    b, bad_b = launch(cols, dims, offsets)
    assert bad_a == 0 and bad_b == 0
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    exact(a, cols, offsets)


@pytest.mark.parametrize("F", [26, 256])
def test_mixed_launch(F):
    kinds = ["uniform", "zipf", "one-id", "dim-7"]
    want = {"uniform": "bitmap", "zipf": "radix", "one-id": "radix", "dim-7": "radix"}
    r = H.rng(F)
    mix = [kinds[(f * 7 + f // 4) % 4] if f % 3 else "uniform" for f in range(F)]
    assert set(mix) == set(kinds)
    dims = [7 if k == "dim-7" else HEAD for k in mix]
    offsets = H.field_offsets(dims)
    cols = [offsets[f] + headline_column(r, k) for f, k in enumerate(mix)]
    assert run(cols, dims, offsets) == [want[k] for k in mix]


def test_old_paths_stay_reachable():
    B, dim = 4096, (1 << 20) - 1
    assert limits(B, dim - 1)[0] == 0                     # beyond the bitmap's range
    r = H.rng(4096)
    uni = r.integers(0, dim, size=B).astype(np.int64)
    hot = uni.copy()
    hot[r.choice(B, 100, replace=False)] = 123_456       # one id 100 times: a bucket of more than BIG words
    dims, offsets = [dim, dim], [0, dim]
    assert run([uni, hot + dim], dims, offsets) == ["bucket", "radix"]


def test_bad_ids():
    """one id below the column's range and one past it: the flag is set, the launch completes, the other columns of the
    launch are exact"""
    B, dim = 64, 100
    dims = [dim] * 4
    offsets = H.field_offsets(dims)
    b = H.plan_batch(B, dims, offsets, ["uniform"] * 4, seed=64)
    cols = [b["f%d" % f].reshape(-1) for f in range(4)]
    cols[1][10] = offsets[1] - 1
    cols[2][20] = offsets[2] + dim
    cols[2][21] = offsets[2] + dim + 60                   # past the 7 key bits as well
    got, bad = launch(cols, dims, offsets)
    assert bad == 1
    exact(got, cols, offsets, only={0, 3})
    assert [path(cols[f], offsets[f], dim - 1) for f in (0, 3)] == ["bitmap", "bitmap"]
