"""The pair sample sort's entry points (dsort.h, ABI 8) as far as no GPU is needed: the library and
the binding export them, and each rejects a NULL context."""
import ctypes
import os

from conftest import PKG

LIB = os.path.join(PKG, "lib", "libdsort.so")
NAMES = ["dsort_sample_argsort_dev_i32", "dsort_sample_sort_pairs_dev_i32"]
EINVAL = -1


def test_library_exports_the_sample_pairs_symbols():
    lib = ctypes.CDLL(LIB)
    missing = [f for f in NAMES if not hasattr(lib, f)]
    assert not missing, missing


def test_binding_lists_the_sample_pairs_symbols(dsort_mod):
    assert set(NAMES) <= set(dsort_mod.EXPORTS)


def test_null_context_is_einval(dsort_mod):
    lib = dsort_mod.load()
    buf = (ctypes.c_int32 * 8)()
    p = ctypes.addressof(buf)
    ko, vo, n = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()
    outs = (ctypes.byref(ko), ctypes.byref(vo), ctypes.byref(n))
    assert lib.dsort_sample_argsort_dev_i32(None, p, 4, 0, *outs, None) == EINVAL
    assert lib.dsort_sample_sort_pairs_dev_i32(None, p, p, 4, *outs, None) == EINVAL
    # ... and with nothing to do
    assert lib.dsort_sample_argsort_dev_i32(None, None, 0, 0, None, None, None, None) == EINVAL
    assert lib.dsort_sample_sort_pairs_dev_i32(None, None, None, 0, None, None, None, None) == EINVAL
