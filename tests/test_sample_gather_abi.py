"""The distributed record gather (dsort.h, ABI 9) as far as no GPU is needed: the library and the
binding export the new symbols, the entry rejects a NULL context, and the two host planning rules
-- the code the GPU path runs -- behave: the owner table (dsort_plan_gather_table) and the routing
(dsort_plan_gather_route) against numpy."""
import ctypes
import os

import numpy as np
import pytest

from conftest import PKG

LIB = os.path.join(PKG, "lib", "libdsort.so")
NAMES = ["dsort_sample_gather_dev", "dsort_plan_gather_table", "dsort_plan_gather_route"]
EINVAL = -1


def test_library_exports_the_gather_symbols():
    lib = ctypes.CDLL(LIB)
    missing = [f for f in NAMES + ["dsort_sample_gather_leg_ms"] if not hasattr(lib, f)]
    assert not missing, missing


def test_binding_lists_the_gather_symbols(dsort_mod):
    assert set(NAMES) <= set(dsort_mod.EXPORTS)
    for f in ("sample_gather_dev", "sample_sort_records_dev"):
        assert callable(getattr(dsort_mod.Context, f))
    fields = [k for k, _ in dsort_mod.Stats._fields_]
    assert fields[-2:] == ["gather_sent", "gather_served"]


def test_null_context_is_einval(dsort_mod):
    lib = dsort_mod.load()
    buf = (ctypes.c_int32 * 16)()
    p = ctypes.addressof(buf)
    assert lib.dsort_sample_gather_dev(None, p, 4, 0, p, 4, p, 4, None) == EINVAL
    assert lib.dsort_sample_gather_dev(None, None, 0, 0, None, 0, None, 16, None) == EINVAL


def test_table_sorts_ranges_given_in_descending_rank_order(dsort_mod):
    # rank r owns chunk P-1-r: first descends with the rank
    lo, hi, owner = dsort_mod.plan_gather_table([300, 200, 100, 0], [50, 100, 100, 100])
    assert lo.tolist() == [0, 100, 200, 300]
    assert hi.tolist() == [100, 200, 300, 350]
    assert owner.tolist() == [3, 2, 1, 0]


def test_table_drops_empty_ranges(dsort_mod):
    lo, hi, owner = dsort_mod.plan_gather_table([10, 5, 0, 7], [5, 0, 10, 0])
    assert lo.tolist() == [0, 10] and hi.tolist() == [10, 15] and owner.tolist() == [2, 0]
    # (an empty range inside another one overlaps nothing)
    lo, hi, owner = dsort_mod.plan_gather_table([0, 0], [0, 0])
    assert lo.size == 0 and hi.size == 0 and owner.size == 0


def test_table_rejects_an_overlap_by_one_record(dsort_mod):
    lo, hi, _ = dsort_mod.plan_gather_table([0, 100], [100, 100])
    assert hi[0] == lo[1] == 100  # adjacent is fine
    with pytest.raises(dsort_mod.DsortError) as e:
        dsort_mod.plan_gather_table([0, 99], [100, 100])
    assert e.value.rc == EINVAL
    with pytest.raises(dsort_mod.DsortError):  # ... whichever rank comes first
        dsort_mod.plan_gather_table([99, 0], [100, 100])


def test_table_end_at_2_32(dsort_mod):
    lo, hi, owner = dsort_mod.plan_gather_table([2 ** 32 - 10, 0], [10, 5])
    assert hi.tolist() == [5, 2 ** 32] and owner.tolist() == [1, 0]
    with pytest.raises(dsort_mod.DsortError) as e:
        dsort_mod.plan_gather_table([2 ** 32 - 10, 0], [11, 5])
    assert e.value.rc == EINVAL


def test_route_matches_numpy(dsort_mod):
    """3 ranks, uneven ranges, one of them empty, one starting above 2^31; 10 007 random indices
    with repeats plus 5 that nobody owns.  The counts are the bincount of the owners, and pos on the
    owned indices is the stable owner-major position."""
    rng = np.random.default_rng(9)
    first = np.array([2 ** 31 + 1000, 777, 40], np.uint64)  # rank 0 above 2^31, rank 1 empty
    count = np.array([5000, 0, 123], np.uint64)
    lo, hi, owner = dsort_mod.plan_gather_table(first, count)
    assert owner.tolist() == [2, 0]
    owned = np.concatenate([rng.integers(40, 163, 4000), rng.integers(2 ** 31 + 1000, 2 ** 31 + 6000, 6007)])
    unowned = np.array([39, 163, 2 ** 31 + 999, 2 ** 31 + 6000, 2 ** 32 - 1])  # each just outside, and the top
    idx = np.concatenate([owned, unowned]).astype(np.uint32)
    rng.shuffle(idx)
    assert idx.size == 10_012 and np.unique(idx).size < idx.size
    want_owner = np.full(idx.size, 3)
    g = idx.astype(np.int64)
    want_owner[(g >= 40) & (g < 163)] = 2
    want_owner[(g >= 2 ** 31 + 1000) & (g < 2 ** 31 + 6000)] = 0
    counts, pos = dsort_mod.plan_gather_route(lo, hi, owner, 3, idx)
    assert counts.tolist() == np.bincount(want_owner, minlength=4).tolist()
    assert counts[3] == 5 and counts[1] == 0
    is_owned = want_owner < 3
    order = np.argsort(want_owner[is_owned], kind="stable")
    want_pos = np.empty(order.size, np.int64)
    want_pos[order] = np.arange(order.size)
    assert np.array_equal(pos[is_owned].astype(np.int64), want_pos)
    # the unowned ones come last, in input order
    assert pos[~is_owned].tolist() == list(range(10_007, 10_012))
