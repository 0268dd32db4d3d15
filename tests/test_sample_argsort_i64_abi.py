"""The int64 argsort across ranks (dsort_sample_argsort_dev_i64, an ABI 10 addition) as far as no GPU is
needed: the library and the binding hold the new symbols and option 18, the entry rejects a NULL
context, and the host rule of the decision leg (dsort_plan_sample_argsort_i64 -- the code the GPU
path runs on the all-gathered table) agrees with Python's integer arithmetic."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import PKG, REPO

LIB = os.path.join(PKG, "lib", "libdsort.so")
HEADER = os.path.join(REPO, "include", "dsort.h")
NAMES = ["dsort_sample_argsort_dev_i64", "dsort_plan_sample_argsort_i64"]
EINVAL = -1
I64_MIN, I64_MAX = -(2**63), 2**63 - 1


def test_library_exports_the_new_symbols():
    lib = ctypes.CDLL(LIB)
    missing = [f for f in NAMES + ["dsort_sample_argsort64_leg_ms"] if not hasattr(lib, f)]
    assert not missing, missing


def test_binding_lists_the_symbols_and_option_18(dsort_mod):
    assert set(NAMES) <= set(dsort_mod.EXPORTS)
    assert dsort_mod.OPTIONS["test_fail_leg"] == 18
    assert callable(dsort_mod.plan_sample_argsort_i64)
    assert callable(dsort_mod.Context.sample_argsort_dev) and callable(dsort_mod.Context.sample_sort_records_dev)


def test_header_declares_them_under_abi_10():
    text = open(HEADER).read()
    assert re.search(r"^#define DSORT_ABI_VERSION 10$", text, flags=re.M)
    assert re.search(r"^#define DSORT_OPT_TEST_FAIL_LEG 18\b", text, flags=re.M)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, flags=re.M), name
    assert "int64 keys with a payload (one GPU: ABI 10)" not in text  # the gap is closed


def test_null_context_is_einval(dsort_mod):
    lib = dsort_mod.load()
    buf = (ctypes.c_int64 * 16)()
    p = ctypes.addressof(buf)
    kp, ip, n = ctypes.c_void_p(5), ctypes.c_void_p(6), ctypes.c_size_t(7)
    rc = lib.dsort_sample_argsort_dev_i64(None, p, 4, 0, ctypes.byref(kp), ctypes.byref(ip), ctypes.byref(n), None)
    assert rc == EINVAL
    assert (kp.value, ip.value, n.value) == (5, 6, 7) and all(x == 0 for x in buf)  # nothing touched


def _rule(first, count, kmin, kmax):
    """The rule of dsort.h in Python integers: None = DSORT_EINVAL."""
    live = sorted((f, f + c, lo, hi) for f, c, lo, hi in zip(first, count, kmin, kmax) if c)
    for i, (f, e, lo, hi) in enumerate(live):
        if e > 2**32 or (i and f < live[i - 1][1]) or lo > hi:
            return None
    for f, c in zip(first, count):  # (dsort_plan_gather_table checks the empty ranges' ends too)
        if f > 2**32 or c > 2**32 - f:
            return None
    if not live:
        return 1, 0
    E = max(e for _, e, _, _ in live)
    R = max(hi for *_, hi in live) - min(lo for _, _, lo, _ in live)
    b = 1 if E <= 2 else (E - 1).bit_length()
    return b, 1 if R >> (64 - b) == 0 else 2


N = 100_003
TOP = 2**32 - N  # the range [TOP, 2^32): E = 2^32, b = 32 although the keys number 100 003 (17 bits)

PLAN_CASES = {
    # ranks in any order, with holes, empty ranks carrying garbage min and max
    "any_order_holes_garbage": ([5000, 0, 77, 1000, 9999], [100, 500, 0, 1000, 0],
                                [-5, 3, I64_MAX, -9, 12], [40, 90, I64_MIN, 17, -12], (13, 1)),
    "garbage_would_widen": ([0, 10, 20], [10, 0, 10], [0, I64_MIN, 5], [100, I64_MAX, 2**40], (5, 1)),
    # min and max on different ranks, at both int64 extremes
    "extremes_split": ([0, 8], [8, 8], [I64_MIN, 0], [-1, I64_MAX], (4, 2)),
    "extremes_swapped": ([8, 0], [8, 8], [I64_MIN, 7], [I64_MIN + 1, I64_MAX], (4, 2)),
    "low_extreme_narrow": ([0, 8], [8, 8], [I64_MIN, I64_MIN + 5], [I64_MIN + 3, I64_MIN + 2**60 - 1], (4, 1)),
    "high_extreme_narrow": ([0, 8], [8, 8], [I64_MAX - 2**60 + 1, I64_MAX - 5], [I64_MAX - 9, I64_MAX], (4, 1)),
    # E's bit length exceeds the key count's: b = 32 from E
    "b_from_E_one_pass": ([TOP, TOP + N // 2], [N // 2, N - N // 2], [-7, 100], [50, -7 + 2**32 - 1], (32, 1)),
    "b_from_E_two_passes": ([TOP, TOP + N // 2], [N // 2, N - N // 2], [-7, 100], [50, -7 + 2**32], (32, 2)),
    "all_empty": ([0, 0, 17], [0, 0, 0], [3, I64_MAX, 0], [1, I64_MIN, 0], (1, 0)),
    "one_key": ([2**32 - 1], [1], [I64_MIN], [I64_MIN], (32, 1)),
    "overlap": ([0, 99], [100, 100], [0, 0], [1, 1], None),
    "overlap_unordered": ([500, 0, 400], [10, 10, 101], [0, 0, 0], [1, 1, 1], None),
    "ends_past_2_32": ([0, 2**32 - 9], [10, 10], [0, 0], [1, 1], None),
    "min_above_max": ([0, 10], [10, 10], [0, 5], [1, 4], None),
}


@pytest.mark.parametrize("case", sorted(PLAN_CASES))
def test_plan_against_python_integers(dsort_mod, case):
    first, count, kmin, kmax, want = PLAN_CASES[case]
    assert _rule(first, count, kmin, kmax) == want  # the table itself
    if want is None:
        with pytest.raises(dsort_mod.DsortError) as ei:
            dsort_mod.plan_sample_argsort_i64(first, count, kmin, kmax)
        assert ei.value.rc == EINVAL
    else:
        assert dsort_mod.plan_sample_argsort_i64(first, count, kmin, kmax) == want
        E = max(f + c for f, c in zip(first, count) if c) if any(count) else 0
        if any(count):  # ... and is dsort_plan_argsort_i64 of (E, global min, global max)
            lo = min(k for k, c in zip(kmin, count) if c)
            hi = max(k for k, c in zip(kmax, count) if c)
            assert dsort_mod.plan_argsort_i64(E, lo, hi) == want


def test_plan_random_tables_against_python_integers(dsort_mod):
    rng = np.random.default_rng(64)
    seen = set()
    for _ in range(300):
        P = int(rng.integers(1, 7))
        cuts = np.sort(rng.integers(0, 2**32 + 1, 2 * P, dtype=np.uint64)).tolist()
        order = rng.permutation(P)
        first = [int(cuts[2 * j]) for j in order]
        count = [int(cuts[2 * j + 1] - cuts[2 * j]) if rng.random() < 0.8 else 0 for j in order]
        if rng.random() < 0.1 and P > 1:
            first[0] = first[1]  # mostly an overlap
        shift = int(rng.integers(0, 62))
        base = int(rng.integers(I64_MIN >> 1, I64_MAX >> 1))
        kmin = [base + int(rng.integers(0, 2**shift)) for _ in range(P)]
        kmax = [k + int(rng.integers(0, 2**shift)) for k in kmin]
        want = _rule(first, count, kmin, kmax)
        seen.add(want if want is None else want[1])
        if want is None:
            with pytest.raises(dsort_mod.DsortError):
                dsort_mod.plan_sample_argsort_i64(first, count, kmin, kmax)
        else:
            assert dsort_mod.plan_sample_argsort_i64(first, count, kmin, kmax) == want, (first, count, kmin, kmax)
    assert {None, 1, 2} <= seen, seen  # (the sweep reaches every outcome but "no keys at all")


def test_plan_argument_errors_write_nothing(dsort_mod):
    lib = dsort_mod.load()
    f = np.array([0, 99], np.uint64)
    c = np.array([100, 100], np.uint64)
    k = np.zeros(2, np.int64)
    b, p = ctypes.c_int(-5), ctypes.c_int(-5)
    args = (f.ctypes.data, c.ctypes.data, k.ctypes.data, k.ctypes.data)
    assert lib.dsort_plan_sample_argsort_i64(2, *args, ctypes.byref(b), ctypes.byref(p)) == EINVAL  # overlap
    assert lib.dsort_plan_sample_argsort_i64(0, *args, ctypes.byref(b), ctypes.byref(p)) == EINVAL
    assert lib.dsort_plan_sample_argsort_i64(2, None, *args[1:], ctypes.byref(b), ctypes.byref(p)) == EINVAL
    assert (b.value, p.value) == (-5, -5)
    # either output may be NULL
    assert lib.dsort_plan_sample_argsort_i64(1, *args, None, ctypes.byref(p)) == 0 and p.value == 1
    assert lib.dsort_plan_sample_argsort_i64(1, *args, ctypes.byref(b), None) == 0 and b.value == 7
