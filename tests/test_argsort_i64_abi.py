"""The int64 argsort and record sort (dsort.h, ABI 10) as far as no GPU is needed: the library and the
binding export the new symbols, the entries reject a NULL context, and the host rule that chooses
between the narrow word and the two passes (dsort_plan_argsort_i64 -- the code the GPU path runs)
agrees with Python's integer arithmetic."""
import ctypes
import os
import re

import pytest

from conftest import PKG, REPO

LIB = os.path.join(PKG, "lib", "libdsort.so")
HEADER = os.path.join(REPO, "include", "dsort.h")
NAMES = ["dsort_argsort_dev_i64", "dsort_argsort_i64", "dsort_sort_records_dev_i64", "dsort_plan_argsort_i64"]
EINVAL = -1
I64_MIN, I64_MAX = -(2**63), 2**63 - 1


def test_library_exports_the_int64_argsort_symbols():
    lib = ctypes.CDLL(LIB)
    missing = [f for f in NAMES + ["dsort_argsort64_leg_ms"] if not hasattr(lib, f)]
    assert not missing, missing


def test_binding_lists_the_symbols_the_option_and_the_stats_field(dsort_mod):
    assert set(NAMES) <= set(dsort_mod.EXPORTS)
    for f in ("argsort_dev", "argsort", "sort_records_dev"):
        assert callable(getattr(dsort_mod.Context, f))
    assert callable(dsort_mod.plan_argsort_i64)
    assert dsort_mod.OPTIONS["argsort_wide"] == 17
    assert "argsort_passes" in [k for k, _ in dsort_mod.Stats._fields_]


def test_header_says_abi_10():
    text = open(HEADER).read()
    assert re.search(r"^#define DSORT_ABI_VERSION (\d+)$", text, flags=re.M).group(1) == "10"
    assert re.search(r"^#define DSORT_OPT_ARGSORT_WIDE 17\b", text, flags=re.M)
    assert "128-bit composite: a position" in text and "would need a 128-bit composite" not in text


def test_null_context_is_einval(dsort_mod):
    lib = dsort_mod.load()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.addressof(buf)
    assert lib.dsort_argsort_dev_i64(None, p, p, p, 4, None) == EINVAL
    assert lib.dsort_argsort_dev_i64(None, None, None, None, 0, None) == EINVAL
    assert lib.dsort_argsort_i64(None, p, p, p, 4) == EINVAL
    assert lib.dsort_sort_records_dev_i64(None, p, p, p, p, 4, 8, None) == EINVAL
    assert all(x == 0 for x in buf)


def _rule(n, kmin, kmax):
    """The rule of dsort.h in Python integers."""
    b = 1 if n <= 2 else (n - 1).bit_length()
    R = kmax - kmin  # (uint64)max - (uint64)min for min <= max
    assert 0 <= R < 2**64
    return b, 0 if n == 0 else (1 if R >> (64 - b) == 0 else 2)


PLAN_POINTS = [
    # (n, key_min, key_max, expected idx_bits, expected passes)
    (0, 5, 5, 1, 0), (0, I64_MIN, I64_MAX, 1, 0),
    (1, -7, -7, 1, 1), (2, 0, 1, 1, 1), (3, 0, 1, 2, 1),
    (4096, 0, 2**52 - 1, 12, 1), (4097, 0, 2**52 - 1, 13, 2),           # b 12 -> 13 halves the room
    (4096, -(2**51), 2**51 - 1, 12, 1), (4097, -(2**51), 2**51 - 1, 13, 2),
    (300001, -3, -3 + 2**45 - 1, 19, 1), (300001, -3, -3 + 2**45, 19, 2),
    (2, I64_MIN, -1, 1, 1), (2, I64_MIN, 0, 1, 2),                      # R = 2^63 - 1, 2^63
    (2, I64_MIN, I64_MAX, 1, 2), (300001, I64_MIN, I64_MAX, 19, 2),
    (2**32, 10, 10 + 2**32 - 1, 32, 1), (2**32, 10, 10 + 2**32, 32, 2),
    (2**32, I64_MAX - (2**32 - 1), I64_MAX, 32, 1), (2**32 - 1, 0, 2**32 - 1, 32, 1), (2**31 + 1, 0, 2**32, 32, 2),
    (2**31, 0, 2**33 - 1, 31, 1), (2**31, 0, 2**33, 31, 2),
]


@pytest.mark.parametrize("n,kmin,kmax,bits,passes", PLAN_POINTS)
def test_plan_against_python_integers(dsort_mod, n, kmin, kmax, bits, passes):
    assert _rule(n, kmin, kmax) == (bits, passes)  # the table itself
    assert dsort_mod.plan_argsort_i64(n, kmin, kmax) == (bits, passes)


def test_plan_rejects_too_many_keys_and_an_empty_range(dsort_mod):
    lib = dsort_mod.load()
    b, p = ctypes.c_int(-5), ctypes.c_int(-5)
    assert lib.dsort_plan_argsort_i64(2**32 + 1, 0, 0, ctypes.byref(b), ctypes.byref(p)) == EINVAL
    assert lib.dsort_plan_argsort_i64(10, 1, 0, ctypes.byref(b), ctypes.byref(p)) == EINVAL
    assert lib.dsort_plan_argsort_i64(10, I64_MAX, I64_MIN, ctypes.byref(b), ctypes.byref(p)) == EINVAL
    assert (b.value, p.value) == (-5, -5)  # nothing written
    with pytest.raises(dsort_mod.DsortError):
        dsort_mod.plan_argsort_i64(2**32 + 1, 0, 0)
    # either output may be NULL
    assert lib.dsort_plan_argsort_i64(2**32, 0, 0, None, ctypes.byref(p)) == 0 and p.value == 1
    assert lib.dsort_plan_argsort_i64(2**32, 0, 0, ctypes.byref(b), None) == 0 and b.value == 32


def test_plan_sweep_around_every_bit_boundary(dsort_mod):
    """For every b the largest one-pass range and the smallest two-pass one, at the smallest and the
    largest n of that b, anchored at both ends of the int64 range."""
    for b in range(1, 33):
        ns = [1, 2] if b == 1 else [2 ** (b - 1) + 1, 2**b]
        for n in ns:
            room = 2 ** (64 - b)
            for kmin in (I64_MIN, -1, 0):
                for R, want in ((room - 1, 1), (room, 2)):
                    if kmin + R > I64_MAX:
                        continue
                    assert dsort_mod.plan_argsort_i64(n, kmin, kmin + R) == (b, want), (n, kmin, R)
            assert dsort_mod.plan_argsort_i64(n, I64_MAX - (room - 1), I64_MAX) == (b, 1)
