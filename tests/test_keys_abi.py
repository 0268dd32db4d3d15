"""Typed keys and descending order (include/dsort.h, "Key types and order"), the part that needs no
GPU: the new symbols, the constants, the argument checks that come before any memory is touched,
and the host rule of the codec -- dsort_key_encode / dsort_key_decode, the code the kernels run --
against the restatement of the header's table in keys_model.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import keys_model as km
from conftest import PKG, REPO

HEADER = os.path.join(REPO, "include", "dsort.h")
LIB = os.path.join(PKG, "lib", "libdsort.so")

NAMES = ["dsort_key_encode", "dsort_key_decode", "dsort_sort_dev_keys", "dsort_sort_dev_copy_keys",
         "dsort_sort_keys", "dsort_argsort_dev_keys", "dsort_argsort_keys", "dsort_sort_pairs_dev_keys",
         "dsort_sort_records_dev_keys", "dsort_sample_sort_dev_keys", "dsort_sample_argsort_dev_keys"]
EINVAL = -1
ORDERS = [False, True]


def test_symbols_and_binding(dsort_mod):
    lib = ctypes.CDLL(LIB)
    assert not [n for n in NAMES if not hasattr(lib, n)]
    assert set(NAMES) <= set(dsort_mod.EXPORTS)
    assert dsort_mod.KEY_TYPES == km.KEY_CODE and dsort_mod.ORDER_DESCENDING == 1


def test_header_constants():
    text = open(HEADER).read()
    assert re.search(r"#define\s+DSORT_ABI_VERSION\s+10\b", text)
    for name, code in km.KEY_CODE.items():
        assert re.search(rf"#define\s+DSORT_KEY_{name.upper()}\s+{code}\b", text), name
    assert re.search(r"#define\s+DSORT_ORDER_DESCENDING\s+1\b", text)


def test_null_context_is_einval_and_touches_nothing(dsort_mod):
    lib = dsort_mod.load()
    n = 64
    keys = np.arange(n, dtype=np.uint64)
    out = np.full(n, 7, np.uint64)
    vals = np.full(n, 5, np.uint32)
    idx = np.full(n, 9, np.uint32)
    snap = [a.copy() for a in (keys, out, vals, idx)]
    k, o, v, i = (a.ctypes.data for a in (keys, out, vals, idx))
    p1, p2, cnt = ctypes.c_void_p(0x55), ctypes.c_void_p(0x66), ctypes.c_size_t(77)
    for kt in range(6):
        for fl in (0, 1):
            assert lib.dsort_sort_dev_keys(None, k, n, kt, fl, None) == EINVAL
            assert lib.dsort_sort_dev_copy_keys(None, k, o, n, kt, fl, None) == EINVAL
            assert lib.dsort_sort_keys(None, k, n, kt, fl) == EINVAL
            assert lib.dsort_argsort_dev_keys(None, k, o, i, n, kt, fl, None) == EINVAL
            assert lib.dsort_argsort_keys(None, k, o, i, n, kt, fl) == EINVAL
            assert lib.dsort_sort_pairs_dev_keys(None, k, v, o, i, n, kt, fl, None) == EINVAL
            assert lib.dsort_sort_records_dev_keys(None, k, o, v, i, n, 4, kt, fl, None) == EINVAL
            assert lib.dsort_sample_sort_dev_keys(None, k, n, kt, fl, ctypes.byref(p1), ctypes.byref(cnt),
                                                  None) == EINVAL
            assert lib.dsort_sample_argsort_dev_keys(None, k, n, 0, kt, fl, ctypes.byref(p1), ctypes.byref(p2),
                                                     ctypes.byref(cnt), None) == EINVAL
    for a, b in zip((keys, out, vals, idx), snap):
        assert np.array_equal(a, b)
    assert (p1.value, p2.value, cnt.value) == (0x55, 0x66, 77)


@pytest.mark.parametrize("kt,fl", [(-1, 0), (6, 0), (0, 2), (2, 3), (5, -1)])
def test_encode_rejects_unknown_type_and_flags(dsort_mod, kt, fl):
    lib = dsort_mod.load()
    keys = np.arange(16, dtype=np.uint64)
    words = np.full(16, 3, np.uint64)
    for f in (lib.dsort_key_encode, lib.dsort_key_decode):
        assert f(kt, fl, keys.ctypes.data, words.ctypes.data, 16) == EINVAL
        assert (words == 3).all() and np.array_equal(keys, np.arange(16, dtype=np.uint64))
    assert lib.dsort_key_encode(0, 0, None, words.ctypes.data, 4) == EINVAL
    assert lib.dsort_key_encode(0, 0, None, None, 0) == 0


def test_binding_rejects_mismatched_override(dsort_mod):
    with pytest.raises(dsort_mod.DsortError):
        dsort_mod.key_encode(np.zeros(4, np.int32), key_type="u64")
    with pytest.raises(dsort_mod.DsortError):
        dsort_mod.key_encode(np.zeros(4, np.int32), key_type="x32")
    with pytest.raises(dsort_mod.DsortError):
        dsort_mod.key_encode(np.zeros(4, np.int16))
    # an int32 array taken as unsigned
    a = np.array([-1, 0], np.int32)
    assert dsort_mod.key_encode(a, key_type="u32").tolist() == [2**31 - 1, -2**31]


@pytest.mark.parametrize("desc", ORDERS)
@pytest.mark.parametrize("name", km.KEY_NAMES)
def test_curated_round_trip_and_order(dsort_mod, name, desc):
    x = km.curated(name)
    w = dsort_mod.key_encode(x, descending=desc)
    assert w.dtype == km.int_of(name) and w.shape == x.shape
    # the round trip is bit-exact: NaN payloads and the sign of zero survive
    back = dsort_mod.key_decode(w, name, descending=desc)
    assert back.dtype == x.dtype and np.array_equal(km.bits(back), km.bits(x))
    # listed in the type's order: strictly increasing words, strictly decreasing when descending
    d = np.diff(w.astype(object))
    assert all(v < 0 for v in d) if desc else all(v > 0 for v in d), (name, w)
    assert np.array_equal(w, km.ref_encode(x, name, desc))
    # descending is ~w of the ascending word
    assert np.array_equal(dsort_mod.key_encode(x, descending=True), ~dsort_mod.key_encode(x))


@pytest.mark.parametrize("desc", ORDERS)
@pytest.mark.parametrize("name", km.KEY_NAMES)
def test_encode_in_place(dsort_mod, name, desc):
    lib = dsort_mod.load()
    x = km.curated(name)
    buf = x.copy()
    assert lib.dsort_key_encode(km.KEY_CODE[name], int(desc), buf.ctypes.data, buf.ctypes.data, buf.size) == 0
    assert np.array_equal(buf.view(km.int_of(name)), km.ref_encode(x, name, desc))
    assert lib.dsort_key_decode(km.KEY_CODE[name], int(desc), buf.ctypes.data, buf.ctypes.data, buf.size) == 0
    assert np.array_equal(km.bits(buf), km.bits(x))


@pytest.mark.parametrize("desc", ORDERS)
@pytest.mark.parametrize("name", km.KEY_NAMES)
def test_random_bit_patterns_match_the_restatement(dsort_mod, name, desc):
    rng = np.random.default_rng(km.KEY_CODE[name] * 2 + int(desc))
    x = rng.integers(0, 1 << km.width(name), 100_000, dtype=km.uint_of(name)).view(km.NP_TYPE[name])
    w = dsort_mod.key_encode(x, descending=desc)
    assert np.array_equal(w, km.ref_encode(x, name, desc))
    assert np.array_equal(km.bits(dsort_mod.key_decode(w, name, descending=desc)), km.bits(x))


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_float_order_is_numpys_without_nan_and_negative_zero(dsort_mod, name):
    rng = np.random.default_rng(11)
    x = rng.standard_normal(100_000).astype(km.NP_TYPE[name])
    x[:1000] = x[1000:2000]  # ties
    assert not km.has_nan_or_negzero(x)
    w = dsort_mod.key_encode(x)
    assert np.array_equal(np.argsort(w, kind="stable"), np.argsort(x, kind="stable"))
    import torch
    t = torch.sort(torch.from_numpy(x), descending=True, stable=True)
    order = np.argsort(dsort_mod.key_encode(x, descending=True), kind="stable")
    assert np.array_equal(order, t.indices.numpy())
