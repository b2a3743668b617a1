"""CPU checks of the plan sort's host-side choice (csrc/colsort.hip): how many radix passes of how many bits a batch size
and key width get, and the statuses of the configurations the sort refuses -- no GPU needed."""
import ctypes as C

import pytest


def digits(B, max_key):
    from explicit_tf2_recommendation_amd._lib import lib
    p, d = C.c_int(-1), C.c_int(-1)
    rc = lib.rec_colsort_digits(B, max_key, C.byref(p), C.byref(d))
    return rc, p.value, d.value


# (B, max_key) -> (passes, digit bits): key bits = bits(max_key + 1), at most 10 per pass, spread evenly
@pytest.mark.parametrize("B,max_key,want", [
    (1, 0, (1, 1)), (64, 1, (1, 1)), (64, 2, (1, 2)), (8192, 1023, (1, 10)), (8192, 1024, (2, 6)),
    (8192, 384_615, (2, 10)),                     # the headline: 10M ids over 26 fields, 19-bit keys
    (16384, (1 << 18) - 2, (2, 9)), (4096, (1 << 20) - 2, (2, 10)), (2048, 1 << 20, (3, 7)),
    (16, (1 << 28) - 2, (3, 10)), (8, (1 << 29) - 2, (3, 10)), (2, (1 << 31) - 2, (4, 8)),
])
def test_digit_choice(B, max_key, want):
    rc, p, d = digits(B, max_key)
    assert rc == 0 and (p, d) == want
    kb = max(1, max_key.bit_length())
    assert d <= 10 and (p - 1) * d < kb <= p * d      # every pass has bits, the passes cover the key


@pytest.mark.parametrize("B,max_key,rc", [
    (0, 5, -1), (8, -1, -1), (16385, 5, -2),
    (8192, 1 << 19, -2),                          # 20 key bits + 13 position bits > 32
    (8192, (1 << 19) - 1, -2),                    # 32 bits, but the widest word is the pad word
])
def test_refused_configs(B, max_key, rc):
    assert digits(B, max_key)[0] == rc


def test_null_outputs_refused():
    from explicit_tf2_recommendation_amd._lib import lib
    assert lib.rec_colsort_digits(8192, 100, None, None) == -1
