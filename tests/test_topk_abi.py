"""Top-k selection (include/dsort.h, "top-k", an ABI 10 addition) as far as no GPU is needed: the
symbols, option 19, the argument checks that come before any memory is touched, and the host rule
dsort_plan_topk -- the code dsort_topk_dev_keys asks for its path."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import PKG, REPO

HEADER = os.path.join(REPO, "include", "dsort.h")
LIB = os.path.join(PKG, "lib", "libdsort.so")
NAMES = ["dsort_plan_topk", "dsort_topk_dev_keys", "dsort_topk_keys", "dsort_sample_topk_dev_keys"]
EINVAL = -1


def test_symbols_and_binding(dsort_mod):
    lib = ctypes.CDLL(LIB)
    assert not [n for n in NAMES + ["dsort_topk_leg_ms", "dsort_topk_leg_timing"] if not hasattr(lib, n)]
    assert set(NAMES) <= set(dsort_mod.EXPORTS)
    assert callable(dsort_mod.plan_topk)
    for m in ("topk_dev", "topk", "sample_topk_dev"):
        assert callable(getattr(dsort_mod.Context, m)), m


def test_option_19_is_the_last(dsort_mod):
    assert dsort_mod.OPTIONS["topk_path"] == 19 and max(dsort_mod.OPTIONS.values()) == 19
    text = open(HEADER).read()
    assert re.search(r"^#define DSORT_ABI_VERSION 10$", text, flags=re.M)
    assert re.search(r"^#define DSORT_OPT_TOPK_PATH 19\b", text, flags=re.M)
    numbers = [int(v) for v in re.findall(r"^#define DSORT_OPT_[A-Z0-9_]+ (\d+)\b", text, flags=re.M)]
    assert max(numbers) == 19 and 20 not in numbers
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, text, flags=re.M), name
    lib = dsort_mod.load()  # without a context no option can be set: both calls refuse
    v = ctypes.c_int64(5)
    assert lib.dsort_set_option(None, 19, 1) == EINVAL and lib.dsort_set_option(None, 20, 1) == EINVAL
    assert lib.dsort_get_option(None, 19, ctypes.byref(v)) == EINVAL and v.value == 5


def test_null_context_is_einval_and_touches_nothing(dsort_mod):
    lib = dsort_mod.load()
    n, k = 64, 8
    keys = np.arange(n, dtype=np.uint64)
    out = np.full(n, 7, np.uint64)
    idx = np.full(n, 9, np.uint32)
    snap = [a.copy() for a in (keys, out, idx)]
    kp, op, ip = (a.ctypes.data for a in (keys, out, idx))
    for kt in range(6):
        for fl in (0, 1):
            assert lib.dsort_topk_dev_keys(None, kp, n, k, kt, fl, op, ip, None) == EINVAL
            assert lib.dsort_topk_keys(None, kp, n, k, kt, fl, op, ip) == EINVAL
            assert lib.dsort_sample_topk_dev_keys(None, kp, n, 0, k, kt, fl, op, ip, None) == EINVAL
    for a, b in zip((keys, out, idx), snap):
        assert np.array_equal(a, b)


def test_plan_paths(dsort_mod):
    plan = dsort_mod.plan_topk
    for w, digits in ((4, 3), (8, 6)):
        assert plan(0, 0, w) == (0, digits) and plan(1 << 28, 0, w) == (0, digits)
        assert plan(1 << 28, 0, w, path=1)[0] == 0 and plan(1 << 28, 0, w, path=0)[0] == 0
        assert plan(1 << 28, 1 << 28, w)[0] == 2 and plan(1, 1, w)[0] == 2
        assert plan(1 << 28, 1, w) == (1, digits)
        assert plan(1 << 28, 1024, w)[0] == 1
        assert plan(1 << 32, 1, w)[0] == 1
        # the rule's two constants: the full argsort below 2^24 keys and above n / 2
        assert plan(1 << 24, 1 << 23, w)[0] == 1 and plan(1 << 24, (1 << 23) + 1, w)[0] == 2
        assert plan((1 << 24) - 1, 1, w)[0] == 2 and plan(1 << 24, 1, w)[0] == 1
        # the option forces either path, at any size
        for n, k in ((1, 1), (5, 5), (1 << 28, 1), (1 << 28, 1 << 28), (1 << 32, 1 << 32)):
            assert plan(n, k, w, path=1)[0] == 1 and plan(n, k, w, path=0)[0] == 2
        assert plan(1 << 28, 1, w)[1] <= (3 if w == 4 else 6)


@pytest.mark.parametrize("n", [1, 2, 1000, 16384, (1 << 24) - 1, 1 << 24, (1 << 24) + 1, (1 << 28) + 3, 1 << 32])
def test_plan_is_monotonic_in_k(dsort_mod, n):
    """At fixed n the path never goes from 2 back to 1 as k grows."""
    ks = sorted({1, 2, 3, n // 1024, n // 16, n // 8, n // 4, n // 2 - 1, n // 2, n // 2 + 1, n - 1, n} - {0})
    ks = [k for k in ks if 1 <= k <= n]
    for w in (4, 8):
        paths = [dsort_mod.plan_topk(n, k, w)[0] for k in ks]
        assert set(paths) <= {1, 2}
        assert paths == sorted(paths), (n, ks, paths)
        assert paths[-1] == 2


def test_plan_argument_errors_write_nothing(dsort_mod):
    lib = dsort_mod.load()
    p, d = ctypes.c_int(-5), ctypes.c_int(-5)
    bp, bd = ctypes.byref(p), ctypes.byref(d)
    for kb in (0, 1, 2, 3, 5, 16, -4):
        assert lib.dsort_plan_topk(100, 10, kb, -1, bp, bd) == EINVAL
    assert lib.dsort_plan_topk((1 << 32) + 1, 10, 4, -1, bp, bd) == EINVAL
    assert lib.dsort_plan_topk(10, 11, 4, -1, bp, bd) == EINVAL
    assert lib.dsort_plan_topk(10, 1, 4, 2, bp, bd) == EINVAL and lib.dsort_plan_topk(10, 1, 4, -2, bp, bd) == EINVAL
    assert (p.value, d.value) == (-5, -5)
    # either output may be NULL
    assert lib.dsort_plan_topk(1 << 28, 1, 8, -1, None, bd) == 0 and d.value == 6
    assert lib.dsort_plan_topk(1 << 28, 1, 8, -1, bp, None) == 0 and p.value == 1
    with pytest.raises(dsort_mod.DsortError) as ei:
        dsort_mod.plan_topk(10, 1, 2)
    assert ei.value.rc == EINVAL
