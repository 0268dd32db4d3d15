"""The argsort / key-value sort / gather entry points (dsort.h, ABI 7) as far as no GPU is needed:
the library exports them, and each rejects a NULL context and a bad record size."""
import ctypes
import os

import pytest

from conftest import PKG

LIB = os.path.join(PKG, "lib", "libdsort.so")
NAMES = ["dsort_argsort_dev_i32", "dsort_sort_pairs_dev_i32", "dsort_gather_dev", "dsort_argsort_i32"]
EINVAL = -1


def test_library_exports_the_pairs_symbols():
    lib = ctypes.CDLL(LIB)
    missing = [f for f in NAMES if not hasattr(lib, f)]
    assert not missing, missing


def test_binding_lists_the_pairs_symbols(dsort_mod):
    assert set(NAMES) <= set(dsort_mod.EXPORTS)


def test_null_context_is_einval(dsort_mod):
    lib = dsort_mod.load()
    buf = (ctypes.c_int32 * 8)()
    p = ctypes.addressof(buf)
    assert lib.dsort_argsort_dev_i32(None, p, p, p, 4, None) == EINVAL
    assert lib.dsort_sort_pairs_dev_i32(None, p, p, p, p, 4, None) == EINVAL
    assert lib.dsort_gather_dev(None, p, p, p, 1, 4, None) == EINVAL
    assert lib.dsort_argsort_i32(None, p, p, p, 4) == EINVAL
    # ... and with nothing to do
    assert lib.dsort_argsort_dev_i32(None, None, None, None, 0, None) == EINVAL
    assert lib.dsort_gather_dev(None, None, None, None, 0, 4, None) == EINVAL


@pytest.mark.parametrize("elem_bytes", [0, 2, 12, 32])
def test_gather_rejects_record_size_without_context(dsort_mod, elem_bytes):
    lib = dsort_mod.load()
    buf = (ctypes.c_int32 * 8)()
    p = ctypes.addressof(buf)
    assert lib.dsort_gather_dev(None, p, p, p, 1, elem_bytes, None) == EINVAL
