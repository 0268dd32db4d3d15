"""Every slot map and every lookup instance of the first partition level (csrc/dsort_bucket.h) on the
MI355X, at the edges of the key range and at sizes where a case takes a moment.

bucket_slotmap_kernel chooses between four maps from the splitters (fixed top bits, adaptive linear,
adaptive log, fixed with one refined slot); four table formats sit on the chosen map and the host launches
one of five histogram / scatter instances after reading the choice back.  Every case here sorts a seeded
input with a forced bucket count, out of place, and asserts
  * the output against np.sort, bit for bit, and the input untouched;
  * stats()["first_level_map"] against the numpy model of the decision (tests/slotmap_model.py) for that
    very input -- and the model against the map the shape was built to reach (the pins, which
    tests/test_slotmap_model.py holds on the CPU as well).
The shapes reach what the other sorts of the suite do not: the log map for both key widths, the int64
choice between lookups and bucket ids, the refined slot at slot 0 (no slot below: c_lo = 0, no key below
the first splitter's) and at slot 2047 (no next slot, sub-slot starts beyond 2^32), keys that differ from
a splitter in bit 0 only (the packed entry's kb == sb path), and more samples than keys.  Every shape also
runs sorted and reversed: the runs hint (BkMap.hot) then selects the int32 scatter's `hot` instance and the
aggregated counts (bucket_bump) over the same splitter keys.
"""
import numpy as np
import pytest

import slotmap_model as sm

pytestmark = pytest.mark.gpu

ORDERS = ("generated", "ascending", "descending")
SEEN = {}  # (key bits, first_level_map) -> a case that reached it


def _ordered(a, order):
    if order == "generated":
        return a
    s = np.sort(a)
    return s if order == "ascending" else s[::-1].copy()


def _sort(ctx, a):
    import torch
    t = torch.from_numpy(a).cuda()
    out = torch.empty_like(t)
    ctx.sort_dev(t, out)
    torch.cuda.synchronize()
    st = ctx.stats()
    assert np.array_equal(t.cpu().numpy(), a)  # the input is left alone
    return out.cpu().numpy(), st


def _run(ctx, dt, name, B, n, order, **opts):
    a = _ordered(sm.make_keys(dt, name, B, n), order)
    with ctx.options(buckets=B, **opts):
        want = sm.predict(a, B, ctx.get_option("bucket_oversample"))
        got, st = _sort(ctx, a)
    pin = sm.pin_of(dt, name)
    print(f"{np.dtype(dt).name} {name} B={B} n={n} {order} {opts}: model {want} pin {pin} "
          f"gpu map {st['first_level_map']} tile_sort_keys {st['tile_sort_keys']}")
    assert np.array_equal(got, np.sort(a))
    assert st["first_level_map"] == want["map"], (st["first_level_map"], want)
    if pin is not None:  # the input aims where it was built to aim
        assert want["map"] == pin[0], (want, pin)
        if want["map"] == 3:
            assert want["slot"] in pin[1], (want, pin)
    SEEN.setdefault((sm.key_bits(dt), st["first_level_map"]), (name, B, n, order))
    return a, st


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B,n", sm.SIZES)
@pytest.mark.parametrize("name", list(sm.KEYS32))
def test_int32_maps(gpu_ctx, name, B, n, order):
    _run(gpu_ctx, np.int32, name, B, n, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B,n", sm.SIZES)
@pytest.mark.parametrize("name", list(sm.KEYS64))
def test_int64_maps(gpu_ctx, name, B, n, order):
    _run(gpu_ctx, np.int64, name, B, n, order)


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("name", sm.SMALL_SHAPES)
def test_more_samples_than_keys(gpu_ctx, name, order):
    """S = B os = 131072 samples of 40000 keys: every key is sampled about three times, the composites of
    one key's samples are equal, and the splitters are still the model's."""
    B, n = sm.SMALL
    assert B * gpu_ctx.get_option("bucket_oversample") > n
    _run(gpu_ctx, np.int32, name, B, n, order)


@pytest.mark.parametrize("opts", [dict(sub_gather=0), dict(sub_keys=0)], ids=["scatter", "merge"])
@pytest.mark.parametrize("dt,name", [(np.int32, "mixed100"), (np.int32, "low3"), (np.int32, "mixed_highedge"),
                                     (np.int64, "zipf")], ids=lambda v: v.__name__ if isinstance(v, type) else v)
def test_other_second_levels(gpu_ctx, dt, name, opts):
    """The sub-bucket scatter path and the merge path (no pure-bucket shortcut: the scatter writes every
    bucket) behind the refined slot at both ends of the table and the int64 bucket ids."""
    B, n = sm.SIZES[1]
    _run(gpu_ctx, dt, name, B, n, "generated", **opts)


@pytest.mark.parametrize("name", ["mixed100", "low3"])
def test_pure_buckets_skip_the_second_level(gpu_ctx, name):
    """The copies of a key that owns at least two splitters go to buckets that hold nothing else where the
    key has a one-key (sub-)slot to itself (bucket_onekey, refine_pick), and the second level skips those
    buckets: tile_sort_keys counts the keys it did sort.  At B = 1024 every small key owns about five
    splitters.

    mixed100: the refined slot's sub-slots are one key wide, so every copy of every key of [1, 100] must be
    skipped: tile_sort_keys <= n - (copies of the keys that own two or more splitters).

    low3: the refined slot is slot 0 and its sub-slots are 2^13 keys wide.  INT_MIN has sub-slot 0 to
    itself, but the hundred keys at INT_MIN + 2^20 share one sub-slot, which searches its splitters by
    (key, position): of their copies only those between the key's first and last splitter's positions land
    in pure buckets, the others in the mixed bucket on either side.  The bound for them is that count
    (slotmap_model.pure_copies), not all copies -- by the lookup's design: n - (all copies) = 244666 is
    not reached there, the sort gives 293930 = n - 206070, the count of the model.

    Both counts are what the lookups must do key for key, and no bucket is pure but by two splitters of one
    key, so the bound is met with equality (mixed100: 250010 = n - 249990)."""
    B, n = sm.SIZES[0]
    a, st = _run(gpu_ctx, np.int32, name, B, n, "generated")
    owned, sure = sm.pure_copies(a, B, gpu_ctx.get_option("bucket_oversample"))
    print(f"{name}: copies of keys with two or more splitters {owned}, surely in pure buckets {sure}, "
          f"second level sorted {st['tile_sort_keys']} of {n}")
    assert 0 < sure <= owned
    if name == "mixed100":
        assert sure == owned
    assert st["tile_sort_keys"] <= n - sure
    assert st["tile_sort_keys"] == n - sure  # (nothing else is skipped)


def test_every_map_was_reached(gpu_ctx):
    """int32 maps 0, 1, 2, 3 and int64 maps 1, 2 (which also switch the int64 scatter between lookups and
    bucket ids), as reported by the sorts of this file (selected alone, this test runs every shape at the
    smallest size first)."""
    if not SEEN:
        for dt, table in ((np.int32, sm.KEYS32), (np.int64, sm.KEYS64)):
            for name in table:
                _run(gpu_ctx, dt, name, *sm.SIZES[-1], "generated")
    want = {(32, 0), (32, 1), (32, 2), (32, 3), (64, 1), (64, 2)}
    assert want <= set(SEEN), sorted(want - set(SEEN))
