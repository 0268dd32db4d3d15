"""Stable argsort and record sort of int64 keys (dsort_pairs64.hip; dsort.h, ABI 10) on the GPU.
Every expected value is exact: numpy's stable argsort on the host, torch's stable sort at the one
size where the host would take too long.  Every test also says which path it expects -- the narrow
word (stats argsort_passes 1) or the two passes (2) -- from the rule of dsort.h in Python integers."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE64 = 8192  # the int64 sort's tile (dsort_wave.hip: TILE_OF<T> = WK * WG<T>::WAVES = 1024 * 8)
EINVAL, ESTAGE = -1, -7
I64 = np.iinfo(np.int64)
I64_MIN, I64_MAX = int(I64.min), int(I64.max)

SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025, 4096, 4097,  # groups of 256 and the tail
         TILE64 - 1, TILE64, TILE64 + 1, 2 * TILE64 - 1, 2 * TILE64, 2 * TILE64 + 1,  # int64 tile edges
         65536, 65537, 9 * TILE64 + 77, 300001]                                    # tiles and merge passes
AUTO_KINDS = ["uniform", "equal", "few", "narrow", "edge1", "edge2", "sorted", "reverse"]
WIDE_KINDS = ["low_half", "high_half", "sign_pairs", "narrow"]


def _bits(n):
    return 1 if n <= 2 else (n - 1).bit_length()


def _passes(a):
    """The rule of dsort_plan_argsort_i64 on the keys themselves."""
    if a.size == 0:
        return 0
    return 1 if (int(a.max()) - int(a.min())) >> (64 - _bits(a.size)) == 0 else 2


def _with_range(rng, n, R):
    """n >= 2 random keys whose max - min is exactly R, anywhere in the int64 range."""
    kmin = int(rng.integers(I64_MIN, I64_MAX - R, endpoint=True))
    off = rng.integers(0, R, n, dtype=np.uint64, endpoint=True)
    off[0], off[-1] = 0, R
    rng.shuffle(off)
    return (off + np.uint64(kmin % 2**64)).view(np.int64)  # (wraps modulo 2^64: two's complement)


def _keys(rng, kind, n):
    if kind == "uniform":
        return rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True)
    if kind == "equal":
        return np.full(n, -1, np.int64)
    if kind == "few":
        return rng.choice(np.array([I64_MIN, -1, 0, 1, I64_MAX], np.int64), n)
    if kind == "narrow":
        return rng.integers(-1000, 1000, n, dtype=np.int64, endpoint=True)
    if kind == "edge1":  # the widest range that still goes in one pass at this n
        return _with_range(rng, n, 2 ** (64 - _bits(n)) - 1)
    if kind == "edge2":  # one more: two passes
        return _with_range(rng, n, 2 ** (64 - _bits(n)))
    if kind == "sorted":
        return np.sort(_keys(rng, "uniform", n))
    if kind == "reverse":
        return np.sort(_keys(rng, "uniform", n))[::-1].copy()
    if kind == "low_half":  # one high word, the low words over all of uint32: their order is unsigned
        lo = rng.integers(0, 2**32, n, dtype=np.int64)
        return (np.int64(-0x1234) << 32) | lo
    if kind == "high_half":  # one low word (bit 31 set), the high words over all of int32
        hi = rng.integers(-(2**31), 2**31, n, dtype=np.int64)
        return (hi << 32) | np.int64(0x89ABCDEF)
    if kind == "sign_pairs":  # neighbours across bit 31 of the low word, under three high words
        vals = np.array([h * 2**32 + lo for h in (-1, 0, 1) for lo in (0x7FFFFFFF, 0x80000000)], np.int64)
        return rng.choice(vals, n)
    raise ValueError(kind)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _check_argsort(keys, got_keys, got_idx):
    """keys: the input (numpy); got_keys (or None): int64, got_idx: int32 from the device."""
    exp_idx = np.argsort(keys, kind="stable")
    idx = got_idx.view(np.uint32).astype(np.int64)
    assert np.array_equal(idx, exp_idx)
    if got_keys is not None:
        assert got_keys.dtype == np.int64
        assert np.array_equal(got_keys, keys[exp_idx])


def _run(ctx, a, want_keys=True):
    """Argsort of numpy keys `a` on the device: (keys_out or None, idx) as numpy; the input checked
    unchanged."""
    import torch
    d = _dev(a)
    out = torch.empty_like(d) if want_keys else None
    ko, idx = ctx.argsort_dev(d, keys_out=out)
    assert ko is out and idx.dtype == torch.int32
    assert np.array_equal(_host(d), a)
    return (None if out is None else _host(out)), _host(idx)


# ------------------------------------------------------------------------------ automatic mode
@pytest.mark.parametrize("kind,n", [(k, n) for k in AUTO_KINDS for n in SIZES
                                     if n >= 2 or not k.startswith("edge")])  # (a range needs two keys)
def test_argsort_vs_numpy(gpu_ctx, n, kind):
    rng = np.random.default_rng(n * 13 + len(kind))
    a = _keys(rng, kind, n)
    assert gpu_ctx.get_option("argsort_wide") == 0
    ko, idx = _run(gpu_ctx, a)
    _check_argsort(a, ko, idx)
    st = gpu_ctx.stats()
    assert st["argsort_passes"] == _passes(a), st
    if kind == "equal":
        assert np.array_equal(idx, np.arange(n, dtype=np.int32))
        assert st["argsort_passes"] == (1 if n else 0)
    if kind == "narrow" and n:
        assert st["argsort_passes"] == 1
    if kind == "edge1":
        assert st["argsort_passes"] == 1
    if kind == "edge2":
        assert st["argsort_passes"] == 2
    if kind == "uniform" and n > 2:
        assert st["argsort_passes"] == 2
    if kind == "few" and n >= 255:
        assert a.min() == I64_MIN and a.max() == I64_MAX and st["argsort_passes"] == 2
    assert st["keys_in"] == n and st["keys_out"] == n  # the last inner int64 sort's statistics
    if n == TILE64 + 1:  # a stale tile constant fails here instead of silently testing mid-tile sizes
        assert st["tile_keys"] == TILE64 and st["merge_passes"] == 1, st


@pytest.mark.parametrize("n", [2, 3])
def test_edge_ranges_at_the_smallest_sizes(gpu_ctx, n):
    """b = 1 and 2: the one-pass range is 2^63 - 1 and 2^62 - 1 wide, (key - min) << b uses the whole word."""
    for kind, want in (("edge1", 1), ("edge2", 2)):
        a = _keys(np.random.default_rng(n), kind, n)
        assert int(a.max()) - int(a.min()) == 2 ** (64 - _bits(n)) - (1 if want == 1 else 0)
        ko, idx = _run(gpu_ctx, a)
        _check_argsort(a, ko, idx)
        assert gpu_ctx.stats()["argsort_passes"] == want
    for hi, want in ((-1, 1), (0, 2)):  # against INT64_MIN: a range of 2^63 - 1, and of 2^63
        a = np.array([hi, I64_MIN] + [I64_MIN] * (n - 2), np.int64)
        ko, idx = _run(gpu_ctx, a)
        _check_argsort(a, ko, idx)
        assert gpu_ctx.stats()["argsort_passes"] == _passes(a)
        if n == 2:
            assert _passes(a) == want


def test_other_calls_reset_argsort_passes(gpu_ctx):
    a = _keys(np.random.default_rng(4), "uniform", 5000)
    _run(gpu_ctx, a)
    assert gpu_ctx.stats()["argsort_passes"] == 2
    gpu_ctx.sort_dev(_dev(a))
    assert gpu_ctx.stats()["argsort_passes"] == 0
    _run(gpu_ctx, _keys(np.random.default_rng(4), "narrow", 5000))
    assert gpu_ctx.stats()["argsort_passes"] == 1
    gpu_ctx.argsort_dev(_dev(a.astype(np.int32)))
    assert gpu_ctx.stats()["argsort_passes"] == 0


# ------------------------------------------------------------------------------ the two passes, forced
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", WIDE_KINDS)
def test_argsort_forced_wide_vs_numpy(gpu_ctx, n, kind):
    rng = np.random.default_rng(n * 17 + len(kind))
    a = _keys(rng, kind, n)
    if kind == "low_half" and n >= 255:
        assert ((a >> 32) == -0x1234).all() and 0.35 < ((a >> 31) & 1).mean() < 0.65
    with gpu_ctx.options(argsort_wide=1):
        ko, idx = _run(gpu_ctx, a)
        st = gpu_ctx.stats()
    _check_argsort(a, ko, idx)
    assert st["argsort_passes"] == (2 if n else 0), st
    assert st["keys_in"] == n and st["keys_out"] == n
    if kind == "narrow":  # the same keys in the automatic mode: one pass, the same bits
        ko1, idx1 = _run(gpu_ctx, a)
        assert gpu_ctx.stats()["argsort_passes"] == (1 if n else 0)
        assert np.array_equal(ko1, ko) and np.array_equal(idx1, idx)


def test_option_argsort_wide_takes_0_and_1_only(gpu_ctx, dsort_mod):
    assert gpu_ctx.get_option("argsort_wide") == 0
    for bad in (-1, 2, 17):
        with pytest.raises(dsort_mod.DsortError) as ei:
            gpu_ctx.set_option("argsort_wide", bad)
        assert ei.value.rc == EINVAL
    with gpu_ctx.options(argsort_wide=1):
        assert gpu_ctx.get_option("argsort_wide") == 1
    assert gpu_ctx.get_option("argsort_wide") == 0


# ------------------------------------------------------------------------------ views, aliasing
@pytest.mark.parametrize("ioff", [1, 3])
@pytest.mark.parametrize("n", [1025, 2 * TILE64 + 1])
@pytest.mark.parametrize("kind,passes", [("narrow", 1), ("uniform", 2)])
def test_argsort_misaligned_views(gpu_ctx, n, ioff, kind, passes):
    """Keys and sorted keys start at element 1 of a larger int64 tensor (pointers 8 mod 16), the
    indices at element 1 / 3 of a larger int32 tensor (4 / 12 mod 16); the elements around the
    output views keep their sentinel."""
    import torch
    SENT, SENT32 = 0x5A5A5A5A5A5A5A5A, 0x5A5A5A5A
    a = _keys(np.random.default_rng(n + ioff), kind, n)
    pad = 8
    kin = torch.full((n + 2 * pad,), SENT, dtype=torch.int64, device="cuda")
    kout = torch.full_like(kin, SENT)
    iout = torch.full((n + 2 * pad,), SENT32, dtype=torch.int32, device="cuda")
    kin[1:1 + n] = _dev(a)
    assert kin[1:].data_ptr() % 16 == 8 and kout[1:].data_ptr() % 16 == 8
    assert iout[ioff:].data_ptr() % 16 == 4 * ioff
    gpu_ctx.argsort_dev(kin[1:1 + n], idx_out=iout[ioff:ioff + n], keys_out=kout[1:1 + n])
    assert gpu_ctx.stats()["argsort_passes"] == passes
    _check_argsort(a, _host(kout[1:1 + n]), _host(iout[ioff:ioff + n]))
    for t, o, s in ((kin, 1, SENT), (kout, 1, SENT), (iout, ioff, SENT32)):
        h = _host(t)
        assert (h[:o] == s).all() and (h[o + n:] == s).all()
    assert np.array_equal(_host(kin[1:1 + n]), a)


@pytest.mark.parametrize("kind,passes", [("narrow", 1), ("few", 2)])
def test_argsort_keys_out_is_keys(gpu_ctx, kind, passes):
    n = 9 * TILE64 + 77
    a = _keys(np.random.default_rng(1), kind, n)
    d = _dev(a)
    ko, idx = gpu_ctx.argsort_dev(d, keys_out=d)
    assert ko is d and gpu_ctx.stats()["argsort_passes"] == passes
    _check_argsort(a, _host(d), _host(idx))


@pytest.mark.parametrize("kind,passes", [("narrow", 1), ("few", 2)])
def test_argsort_without_keys_out(gpu_ctx, kind, passes):
    n = 9 * TILE64 + 77
    a = _keys(np.random.default_rng(2), kind, n)
    ko, idx = _run(gpu_ctx, a, want_keys=False)
    assert ko is None and gpu_ctx.stats()["argsort_passes"] == passes
    _check_argsort(a, None, idx)


def test_argsort_size_limit(gpu_ctx):
    """More than 2^32 keys: DSORT_EINVAL before the (one-element) buffers are touched."""
    import torch
    k = torch.zeros(1, dtype=torch.int64, device="cuda")
    i = torch.zeros(1, dtype=torch.int32, device="cuda")
    lib = gpu_ctx.lib
    n = (1 << 32) + 1
    assert lib.dsort_argsort_dev_i64(gpu_ctx.h, k.data_ptr(), k.data_ptr(), i.data_ptr(), n, gpu_ctx._stream()) == EINVAL
    assert lib.dsort_sort_records_dev_i64(gpu_ctx.h, k.data_ptr(), k.data_ptr(), k.data_ptr(), k.data_ptr(), n, 8,
                                          gpu_ctx._stream()) == EINVAL
    host = np.zeros(1, np.int64)
    assert lib.dsort_argsort_i64(gpu_ctx.h, host.ctypes.data, host.ctypes.data, host.ctypes.data, n) == EINVAL
    torch.cuda.synchronize()
    assert _host(k)[0] == 0 and _host(i)[0] == 0 and host[0] == 0


def test_null_pointers_are_einval(gpu_ctx):
    import torch
    d = torch.zeros(16, dtype=torch.int64, device="cuda")
    p, lib, s = d.data_ptr(), gpu_ctx.lib, gpu_ctx._stream()
    assert lib.dsort_argsort_dev_i64(gpu_ctx.h, None, p, p, 4, s) == EINVAL
    assert lib.dsort_argsort_dev_i64(gpu_ctx.h, p, p, None, 4, s) == EINVAL
    assert lib.dsort_sort_records_dev_i64(gpu_ctx.h, None, p, p, p, 4, 8, s) == EINVAL
    assert lib.dsort_sort_records_dev_i64(gpu_ctx.h, p, None, None, p, 4, 8, s) == EINVAL
    assert lib.dsort_sort_records_dev_i64(gpu_ctx.h, p, None, p, None, 4, 8, s) == EINVAL
    for bad in (0, 2, 12, 32):  # the record size is checked before anything else, n = 0 included
        assert lib.dsort_sort_records_dev_i64(gpu_ctx.h, None, None, None, None, 0, bad, s) == EINVAL
    # nothing to do: fine, whatever the pointers
    assert lib.dsort_argsort_dev_i64(gpu_ctx.h, None, None, None, 0, s) == 0
    assert lib.dsort_sort_records_dev_i64(gpu_ctx.h, None, None, None, None, 0, 16, s) == 0
    assert gpu_ctx.stats()["argsort_passes"] == 0


# ------------------------------------------------------------------------------ fault injection
@pytest.mark.parametrize("kind,passes,n", [("narrow", 1, 5000), ("uniform", 2, 5000), ("uniform", 2, 20000)])
def test_argsort_stage_never_reached_still_delivers(gpu_ctx, dsort_mod, kind, passes, n):
    """DSORT_OPT_KILL_AFTER_STAGE past the stages of all inner sorts: DSORT_ESTAGE, every leg has run
    and the outputs are valid.  The stages of the two passes count on: the first stage behind both
    (2 x the stages of one sort) is already out of reach."""
    import torch
    one = gpu_ctx.sort_stages(n, 8)
    assert passes * one < 50
    a = _keys(np.random.default_rng(3), kind, n)
    d = _dev(a)
    for kill in (50, passes * one):
        out = torch.empty_like(d)
        idx = torch.empty(n, dtype=torch.int32, device="cuda")
        with gpu_ctx.options(kill_after_stage=kill):
            with pytest.raises(dsort_mod.DsortError) as ei:
                gpu_ctx.argsort_dev(d, idx_out=idx, keys_out=out)
            assert gpu_ctx.get_option("kill_after_stage") == kill  # the call put the option back
        assert ei.value.rc == ESTAGE
        assert f"has {passes * one} stages" in str(ei.value)
        assert gpu_ctx.stats()["argsort_passes"] == passes
        _check_argsort(a, _host(out), _host(idx))


def test_record_sort_stage_never_reached_still_delivers(gpu_ctx, dsort_mod):
    n = 5000
    rng = np.random.default_rng(31)
    a = _keys(rng, "few", n)
    recs = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    with gpu_ctx.options(kill_after_stage=50):
        import torch
        out = torch.zeros(n, dtype=torch.int64, device="cuda")
        with pytest.raises(dsort_mod.DsortError) as ei:
            gpu_ctx.sort_records_dev(_dev(a), _dev(recs), out=out)
    assert ei.value.rc == ESTAGE and gpu_ctx.stats()["argsort_passes"] == 2
    assert np.array_equal(_host(out), recs[np.argsort(a, kind="stable")])


# ------------------------------------------------------------------------------ shared arenas
def test_one_context_through_both_paths_and_the_int32_argsort(gpu_ctx):
    """The wide path's two arenas, the narrow word in the first of them, the int32 pair arena (the
    same one) and the wide path again, growing and shrinking sizes."""
    rng = np.random.default_rng(41)
    for kind, n, passes in (("uniform", 300001, 2), ("narrow", 1025, 1), ("i32", 70001, 0), ("uniform", 300001, 2),
                            ("narrow", 300001, 1), ("few", 9 * TILE64 + 77, 2), ("sign_pairs", 65537, 1)):
        if kind == "i32":
            a = rng.integers(-5, 5, n).astype(np.int32)
            _, idx = gpu_ctx.argsort_dev(_dev(a))
            assert np.array_equal(_host(idx).astype(np.int64), np.argsort(a, kind="stable"))
        else:
            a = _keys(rng, kind, n)
            ko, idx = _run(gpu_ctx, a)
            _check_argsort(a, ko, idx)
        assert gpu_ctx.stats()["argsort_passes"] == passes


def test_argsort_on_two_streams_shares_the_arenas(gpu_ctx):
    """Two argsorts back to back on different streams, no synchronize in between: the second must
    wait for the first before it packs into the arenas they share."""
    import torch
    n = 300001
    rng = np.random.default_rng(99)
    for ka, kb in (("uniform", "few"), ("narrow", "uniform")):
        a, b = _keys(rng, ka, n), _keys(rng, kb, n)
        da, db = _dev(a), _dev(b)
        ko = [torch.empty_like(da) for _ in range(2)]
        io = [torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2)]
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(s1):
            gpu_ctx.argsort_dev(da, idx_out=io[0], keys_out=ko[0])
        with torch.cuda.stream(s2):
            gpu_ctx.argsort_dev(db, idx_out=io[1], keys_out=ko[1])
        assert gpu_ctx.stats()["argsort_passes"] == 2
        s1.synchronize()
        s2.synchronize()
        _check_argsort(a, _host(ko[0]), _host(io[0]))
        _check_argsort(b, _host(ko[1]), _host(io[1]))


# ------------------------------------------------------------------------------ bucketed path
BIG_N = (1 << 25) + 4099


@pytest.mark.parametrize("kind,passes", [("wide", 2), ("narrow", 1)])
def test_argsort_bucketed_vs_torch(gpu_ctx, kind, passes):
    """The bucketed int64 sort's own path (>= 2^25 keys) under both words, against torch's stable sort."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(len(kind) + 23)
    n = BIG_N
    if kind == "wide":
        d = torch.empty(n, dtype=torch.int64, device="cuda")
        gpu_ctx.gen_uniform(d, 7)  # all 64 bits
    else:
        d = torch.randint(0, 1 << 20, (n,), generator=g, device="cuda", dtype=torch.int64)
    keep = d.clone()
    exp_keys, exp_idx = torch.sort(d, stable=True)
    out = torch.empty_like(d)
    _, idx = gpu_ctx.argsort_dev(d, keys_out=out)
    assert torch.equal(out, exp_keys)
    assert torch.equal(idx.to(torch.int64), exp_idx)
    assert torch.equal(d, keep)
    st = gpu_ctx.stats()
    assert st["argsort_passes"] == passes
    assert st["keys_in"] == n and st["first_level_map"] >= 0  # the bucketed sort ran


# ------------------------------------------------------------------------------ records
def _record_keys(rng, n, extremes):
    k = rng.integers(-50, 50, n, dtype=np.int64, endpoint=True)  # many ties: stability decides
    if extremes:
        k[::7] = I64_MIN
        k[3::11] = I64_MAX
    return k


@pytest.mark.parametrize("rec", [8, 16])
@pytest.mark.parametrize("extremes,passes", [(True, 2), (False, 1)])
def test_sort_records_vs_numpy(gpu_ctx, rec, extremes, passes):
    import torch
    n = 100003
    rng = np.random.default_rng(rec + 5)
    k = _record_keys(rng, n, extremes)
    if rec == 8:
        recs = rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64)
    else:
        recs = rng.integers(-(2**31), 2**31 - 1, (n, 4), dtype=np.int32)
    order = np.argsort(k, kind="stable")
    dk, dr = _dev(k), _dev(recs)
    ko = torch.empty_like(dk)
    r = gpu_ctx.sort_records_dev(dk, dr, keys_out=ko)
    assert r[0] is ko and r[1].shape == dr.shape and r[1].dtype == dr.dtype
    assert gpu_ctx.stats()["argsort_passes"] == passes
    assert np.array_equal(_host(r[1]), recs[order])
    assert np.array_equal(_host(ko), k[order])
    assert np.array_equal(_host(dk), k) and np.array_equal(_host(dr), recs)  # the inputs are not modified
    # keys in place, no sorted keys, 4-byte records
    out = torch.empty_like(dr)
    r = gpu_ctx.sort_records_dev(dk, dr, keys_out=dk, out=out)
    assert r[0] is dk and r[1] is out
    assert np.array_equal(_host(out), recs[order]) and np.array_equal(_host(dk), k[order])
    r4 = _dev(np.arange(n, dtype=np.int32))
    r = gpu_ctx.sort_records_dev(_dev(k), r4)
    assert r[0] is None and np.array_equal(_host(r[1]).astype(np.int64), order)


def test_sort_records_rejects_other_record_sizes(gpu_ctx, dsort_mod):
    import torch
    k = torch.zeros(4, dtype=torch.int64, device="cuda")
    for shape, dt in (((4, 3), torch.int32), ((4,), torch.int16), ((4, 4), torch.int64)):
        src = torch.zeros(shape, dtype=dt, device="cuda")
        with pytest.raises(dsort_mod.DsortError):
            gpu_ctx.sort_records_dev(k, src)
    assert gpu_ctx.lib.dsort_sort_records_dev_i64(gpu_ctx.h, k.data_ptr(), None, k.data_ptr(), k.data_ptr(), 2, 12,
                                                  gpu_ctx._stream()) == EINVAL
    with pytest.raises(dsort_mod.DsortError):  # one record per key
        gpu_ctx.sort_records_dev(k, torch.zeros(5, dtype=torch.int64, device="cuda"))
    with pytest.raises(dsort_mod.DsortError):  # int64 keys only
        gpu_ctx.sort_records_dev(k.to(torch.int32), torch.zeros(4, dtype=torch.int64, device="cuda"))


# ------------------------------------------------------------------------------ host form
@pytest.mark.parametrize("n", [0, 1, TILE64 + 1, 300001])
def test_host_argsort(gpu_ctx, n):
    rng = np.random.default_rng(n + 1)
    for kind in ("few", "narrow"):
        a = _keys(rng, kind, n)
        keep = a.copy()
        sk, idx = gpu_ctx.argsort(a)
        assert idx.dtype == np.uint32 and sk.dtype == np.int64
        assert np.array_equal(a, keep)
        _check_argsort(a, sk, idx.view(np.int32))
        if n:
            assert gpu_ctx.stats()["argsort_passes"] == _passes(a)
