"""The numpy model of the slot-map decision (tests/slotmap_model.py) held to pinned values, CPU only.

tests/test_gpu_slotmaps.py asserts the sort's first_level_map against this model, so the model must not
drift along with the kernel: the maps below were worked out once for each key shape (the margins in
brackets are the model's costs at B = 1024) and the model has to reproduce them for the very inputs the GPU
cases sort, at the default oversampling of 128 samples per bucket.
"""
import time

import numpy as np
import pytest

import slotmap_model as sm

CASES = [(dt, name, B, n) for dt, table in ((np.int32, sm.KEYS32), (np.int64, sm.KEYS64)) for name in table
         for B, n in sm.SIZES + ([sm.SMALL] if dt == np.int32 and name in sm.SMALL_SHAPES else [])
         if sm.pin_of(dt, name) is not None]  # (int64 extremes_mix: a near tie, the model alone decides)


def test_slot_functions_by_hand():
    assert sm.log_m(32) == 6 and sm.log_m(64) == 5
    u = sm.flip(np.array([sm.I32_MIN, -1, 0, sm.I32_MAX], np.int32))
    assert u.tolist() == [0, 2**31 - 1, 2**31, 2**32 - 1]
    u = sm.flip(np.array([sm.I64_MIN, -1, 0, sm.I64_MAX], np.int64))
    assert u.tolist() == [0, 2**63 - 1, 2**63, 2**64 - 1]
    assert sm.bit_length(np.array([0, 1, 2, 3, 2**31, 2**63, 2**64 - 1], np.uint64)).tolist() == [0, 1, 2, 2, 32, 64, 64]
    # log, int32 (M = 6): d itself below 64; then (bit length - 6) << 6 | the 6 bits after the leading one
    d = np.array([0, 63, 64, 65, 127, 128, 130, 2**32 - 1], np.uint64)
    assert sm.slot_log(d, 0, 32).tolist() == [0, 63, 64, 65, 127, 128, 129, (26 << 6) | 63]
    # int64 (M = 5)
    d = np.array([0, 31, 32, 63, 64, 66, 2**64 - 1], np.uint64)
    assert sm.slot_log(d, 0, 64).tolist() == [0, 31, 32, 63, 64, 65, (59 << 5) | 31]
    # below ulo: slot 0
    assert sm.slot_log(np.array([5, 99, 100, 101], np.uint64), 100, 32).tolist() == [0, 0, 0, 1]
    assert sm.slot_linear(np.array([5, 100, 104, 2**32 - 1], np.uint64), 100, 2).tolist() == [0, 0, 1, 2047]
    assert sm.slot_fixed(np.array([0, 2**21 - 1, 2**21, 2**32 - 1], np.uint64), 32).tolist() == [0, 0, 1, 2047]


def test_samples_and_splitters_by_hand():
    # n = 10, B = 2, os = 2: S = 4 samples at ((2k + 1) 10) // 8 = 1, 3, 6, 8; the one splitter is the
    # second smallest sample
    a = np.array([9, 5, 9, 7, 9, 9, 5, 9, 1, 9], np.int32)
    assert sm.sample_positions(10, 2, 2).tolist() == [1, 3, 6, 8]
    keys, pos = sm.splitters(a, 2, 2)
    assert keys.tolist() == [5] and pos.tolist() == [1]  # samples (1, 8) (5, 1) (5, 6) (7, 3)
    # more samples than keys: positions repeat ((2k + 1) 3 // 16)
    assert sm.sample_positions(3, 2, 4).tolist() == [0, 0, 0, 1, 1, 2, 2, 2]


def test_decision_rules_by_hand():
    # int32: no slot of two keys anywhere -> fixed
    assert sm.decide(np.array([-5, 7], np.int32) * (1 << 22), np.int32)["map"] == 0
    # 20 splitters of 20 keys in one fixed slot, spread by the linear map -> linear
    d = sm.decide(np.arange(1, 21, dtype=np.int32), np.int32)
    assert (d["map"], d["costs"]) == (1, (20, 0, 0))
    # splitters of one key only: a one-key slot under every map costs nothing -> fixed
    assert sm.decide(np.full(50, 3, np.int32), np.int32)["costs"] == (0, 0, 0)
    # ten keys crowd one slot under every map (the linear map from INT_MIN to INT_MAX is the fixed one, the
    # log map is coarse that far above its start): that slot is refined, the rest of the fixed map is free
    spl = np.concatenate([np.full(1, sm.I32_MIN), np.arange(10, 20), np.full(1, sm.I32_MAX)]).astype(np.int32)
    assert sm.decide(spl, np.int32) == dict(map=3, slot=1024, costs=(10, 10, 10), rest=0)
    # ... but not when the fixed map's next slot is more crowded than the better adaptive map gets: 20 keys
    # in slot 1024 and 19 in slot 1025, of which the log map from key 0 keeps only ten together
    spl = np.concatenate([np.arange(0, 20), (1 << 21) + np.arange(0, 10),
                          (1 << 21) + np.arange(1, 10) * (1 << 15)]).astype(np.int32)
    assert sm.decide(spl, np.int32) == dict(map=2, slot=None, costs=(20, 20, 10), rest=None)
    # int64: a tie keeps the linear map
    assert sm.decide(np.array([1, 2, 3], np.int64), np.int64) == dict(map=1, slot=None, costs=(1, 1), rest=None)


@pytest.mark.parametrize("dt,name,B,n", CASES, ids=lambda v: v.__name__ if isinstance(v, type) else str(v))
def test_model_reproduces_the_pinned_maps(dt, name, B, n):
    pin = sm.pin_of(dt, name)
    a = sm.make_keys(dt, name, B, n)
    for order, keys in (("as generated", a), ("ascending", np.sort(a)), ("descending", np.sort(a)[::-1])):
        d = sm.predict(keys, B, sm.OS_DEFAULT)
        assert d["map"] == pin[0], (order, d)
        if pin[1] is not None:
            assert d["slot"] in pin[1], (order, d)
        else:
            assert d["slot"] is None


@pytest.mark.parametrize("B,n", sm.SIZES)
def test_refined_shapes_aim_at_the_table_edges(B, n):
    """The stats do not show the refined slot's table; the model does.  The shapes built for the edge
    branches of its construction must put their splitters there."""
    def table(name):
        a = sm.make_keys(np.int32, name, B, n)
        spl, _ = sm.splitters(a, B, sm.OS_DEFAULT)
        slot = sm.predict(a, B, sm.OS_DEFAULT)["slot"]
        first = int(sm.flip(spl)[sm.slot_fixed(sm.flip(spl), 32) == slot][0])
        return sm.flip(a), first, slot, sm.refined_table(spl, slot)

    # keys around zero: unit sub-slots from one key below the first splitter's
    u, first, slot, (lo, sh) = table("mixed100")
    assert (slot, lo, sh) == (1024, first - 1, 0)
    # a wide cluster: sub-slots of several keys
    u, first, slot, (lo, sh) = table("mixed_cluster")
    assert slot == 1024 and sh >= 20 - sm.R2_BITS - 1 and sh > 0
    # the last slot: no next slot, and the unit sub-slots run past the end of the key range
    u, first, slot, (lo, sh) = table("mixed_highedge")
    assert slot == 2047 and sh == 0 and lo + sm.R2 - 1 > 2**32 - 1 and int(u.max()) == 2**32 - 1
    assert ((u < lo) & (u >> np.uint64(21) == 2047)).any()  # (uniform keys of the slot below the table)
    # slot 0 with INT_MIN a splitter: nothing below the table, wide sub-slots
    u, first, slot, (lo, sh) = table("low3")
    assert (slot, lo, first) == (0, 0, 0) and sh > 0


def test_prediction_is_quick():
    a = sm.make_keys(np.int32, "mixed100", 1024, 500_000)
    t = time.perf_counter()
    sm.predict(a, 1024, sm.OS_DEFAULT)
    assert time.perf_counter() - t < 0.5


def test_pure_copies_tell_searched_sub_slots_from_one_key_ones():
    """mixed100: the refined slot's sub-slots are one key wide, every key of [1, 100] owns one alone and all
    its copies lie in pure buckets.  low3: the sub-slots are 2^13 keys wide; INT_MIN owns sub-slot 0, the
    hundred crowded keys share one, which searches: only the copies between a key's first and last splitter
    are sure to lie in pure buckets."""
    B, n = 1024, 500_000
    a = sm.make_keys(np.int32, "mixed100", B, n)
    owned, sure = sm.pure_copies(a, B, sm.OS_DEFAULT)
    assert owned == sure == int(((a >= 1) & (a <= 100)).sum())
    a = sm.make_keys(np.int32, "low3", B, n)
    owned, sure = sm.pure_copies(a, B, sm.OS_DEFAULT)
    low = int((a == sm.I32_MIN).sum())
    assert low < sure < owned
