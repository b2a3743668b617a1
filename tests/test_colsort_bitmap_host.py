"""CPU checks of rec_colsort_bitmap_limits (csrc/colsort.hip): which launches of the plan sort rank their columns through
the LDS bitmap, with how many words, and the capacity of the list of slow lookups -- no GPU needed."""
import ctypes as C

import pytest

RANGE = 13 * 1024 * 32          # keys the bitmap covers: CS_BM_WORDS = 13 x 1024 words of 32 keys


def limits(B, max_key):
    from explicit_tf2_recommendation_amd._lib import lib
    w, c = C.c_int(-1), C.c_int(-1)
    rc = lib.rec_colsort_bitmap_limits(B, max_key, C.byref(w), C.byref(c))
    return rc, w.value, c.value


def test_headline_takes_the_bitmap():
    rc, words, cap = limits(8192, 384_624)
    assert rc == 0 and words == 12020 and cap >= 512


@pytest.mark.parametrize("B,max_key,want", [
    (1, 0, 1), (8192, 30, 1), (8192, 31, 1), (8192, 32, 2), (64, 63, 2), (64, 64, 3), (1000, 999, 32),
    (8192, RANGE - 1, RANGE // 32),               # the last key the bitmap covers
    (8192, RANGE, 0), (4096, (1 << 20) - 2, 0),   # beyond the range: the bucket path
    (8192, (1 << 19) - 2, 0),                     # the widest legal key at B = 8192 is beyond it as well
    (8193, 1000, 0), (16384, (1 << 18) - 2, 0),   # 16 words per thread: no bitmap path
])
def test_words(B, max_key, want):
    rc, words, cap = limits(B, max_key)
    assert rc == 0 and words == want and cap >= 512
    if words:
        assert words == (max_key + 32) // 32 and B <= 8192


@pytest.mark.parametrize("B,max_key,rc", [
    (0, 5, -1), (8, -1, -1), (16385, 5, -2),
    (8192, 1 << 19, -2),                          # 20 key bits + 13 position bits > 32
    (8192, (1 << 19) - 1, -2),                    # 32 bits, but the widest word is the pad word
])
def test_refused_configs(B, max_key, rc):
    from explicit_tf2_recommendation_amd._lib import lib
    p, d = C.c_int(-1), C.c_int(-1)
    assert lib.rec_colsort_digits(B, max_key, C.byref(p), C.byref(d)) == rc       # the model: same statuses
    assert limits(B, max_key)[0] == rc


def test_null_outputs_refused():
    from explicit_tf2_recommendation_amd._lib import lib
    w = C.c_int(0)
    assert lib.rec_colsort_bitmap_limits(8192, 100, None, None) == -1
    assert lib.rec_colsort_bitmap_limits(8192, 100, C.byref(w), None) == -1
    assert lib.rec_colsort_bitmap_limits(8192, 100, None, C.byref(w)) == -1
