"""Stable argsort, key-value sort and gather of int32 keys (dsort_pairs.hip; dsort.h, ABI 7) on the
GPU.  Every expected value is exact: numpy's stable argsort / lexsort on the host, torch's stable
sort at the one size where the host would take too long."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE64 = 8192  # the int64 sort's tile (dsort_wave.hip: TILE_OF<T> = WK * WG<T>::WAVES = 1024 * 8)
EINVAL, ESTAGE = -1, -7
I32 = np.iinfo(np.int32)

SIZES = [0, 1, 2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025,   # vector groups and the scalar tail
         4095, 4096, 4097,                                             # (edges of a stale TILE64 = 4096: kept)
         TILE64 - 1, TILE64, TILE64 + 1, 2 * TILE64 - 1, 2 * TILE64, 2 * TILE64 + 1,  # int64 tile edges
         9 * 4096 + 77, 9 * TILE64 + 77, 300001]                       # several tiles and merge passes
KINDS = ["uniform", "equal", "few", "extremes", "sorted", "reverse"]


def _dist(rng, kind, n, dt=np.int32):
    """The generators of tests/test_gpu_sort.py::_dist."""
    info = np.iinfo(dt)
    if kind == "uniform":
        return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    if kind == "equal":
        return np.full(n, -1, dt)
    if kind == "sorted":
        return np.sort(rng.integers(info.min, info.max, n, dtype=dt, endpoint=True))
    if kind == "reverse":
        return np.sort(rng.integers(info.min, info.max, n, dtype=dt, endpoint=True))[::-1].copy()
    if kind == "few":
        return rng.choice(np.array([info.min, -1, 0, 1, info.max], dt), n)
    if kind == "extremes":
        a = rng.integers(-3, 3, n).astype(dt)
        a[::3] = info.max
        a[1::5] = info.min
        return a
    raise ValueError(kind)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _check_argsort(keys, got_keys, got_idx):
    """keys: the input (numpy); got_keys (or None) / got_idx: numpy int32 from the device."""
    exp_idx = np.argsort(keys, kind="stable")
    idx = got_idx.view(np.uint32).astype(np.int64)
    assert np.array_equal(idx, exp_idx)
    exp_keys = np.sort(keys, kind="stable")
    assert np.array_equal(keys[idx], exp_keys)
    if got_keys is not None:
        assert np.array_equal(got_keys, exp_keys)


# ------------------------------------------------------------------------------ argsort
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", KINDS)
def test_argsort_vs_numpy(gpu_ctx, n, kind):
    import torch
    rng = np.random.default_rng(n * 11 + len(kind))
    a = _dist(rng, kind, n)
    d = _dev(a)
    out = torch.empty_like(d)
    ko, idx = gpu_ctx.argsort_dev(d, keys_out=out)
    assert ko is out
    assert np.array_equal(_host(d), a)  # the input is not modified
    _check_argsort(a, _host(out), _host(idx))
    if kind == "equal":
        assert np.array_equal(_host(idx), np.arange(n, dtype=np.int32))
    st = gpu_ctx.stats()
    assert st["keys_in"] == n and st["keys_out"] == n  # the inner int64 sort's statistics
    if n == TILE64 + 1:  # a stale tile constant fails here instead of silently testing mid-tile sizes
        assert st["tile_keys"] == TILE64 and st["merge_passes"] == 1, st


@pytest.mark.parametrize("off", [1, 3])
@pytest.mark.parametrize("n", [1025, 2 * 4096 + 1, 2 * TILE64 + 1])
def test_argsort_misaligned_views(gpu_ctx, n, off):
    """Inputs and outputs start at element 1 / 3 of a larger tensor (pointers 4 / 12 mod 16); the
    elements around the output views keep their sentinel."""
    import torch
    SENT = 0x5A5A5A5A
    rng = np.random.default_rng(n + off)
    a = _dist(rng, "uniform", n)
    pad = 8
    kin = torch.full((n + 2 * pad,), SENT, dtype=torch.int32, device="cuda")
    kout = torch.full_like(kin, SENT)
    iout = torch.full_like(kin, SENT)
    kin[off:off + n] = _dev(a)
    for t in (kin, kout, iout):
        assert t[off:].data_ptr() % 16 == 4 * off
    gpu_ctx.argsort_dev(kin[off:off + n], idx_out=iout[off:off + n], keys_out=kout[off:off + n])
    _check_argsort(a, _host(kout[off:off + n]), _host(iout[off:off + n]))
    for t in (kin, kout, iout):
        h = _host(t)
        assert (h[:off] == SENT).all() and (h[off + n:] == SENT).all()
    assert np.array_equal(_host(kin[off:off + n]), a)


@pytest.mark.parametrize("off", [1, 3])
def test_pairs_misaligned_views(gpu_ctx, off):
    """The same for the key-value sort, keys and values at different phases."""
    import torch
    SENT = 0x5A5A5A5A
    for n in (2 * 4096 + 1, 2 * TILE64 + 1):
        pad = 8
        rng = np.random.default_rng(50 + off)
        k = rng.integers(-3, 3, n, endpoint=True).astype(np.int32)
        v = rng.integers(I32.min, I32.max, n, dtype=np.int32, endpoint=True)
        voff = 4 - off  # 3 / 1: another phase than the keys
        bufs = [torch.full((n + 2 * pad,), SENT, dtype=torch.int32, device="cuda") for _ in range(4)]
        kin, vin, kout, vout = bufs
        kin[off:off + n] = _dev(k)
        vin[voff:voff + n] = _dev(v)
        gpu_ctx.sort_pairs_dev(kin[off:off + n], vin[voff:voff + n], keys_out=kout[voff:voff + n],
                               vals_out=vout[off:off + n])
        order = np.lexsort((v.view(np.uint32), k))
        assert np.array_equal(_host(kout[voff:voff + n]), k[order])
        assert np.array_equal(_host(vout[off:off + n]), v[order])
        for t, o in ((kin, off), (vin, voff), (kout, voff), (vout, off)):
            h = _host(t)
            assert (h[:o] == SENT).all() and (h[o + n:] == SENT).all()


def test_argsort_keys_out_is_keys(gpu_ctx):
    for n in (9 * 4096 + 77, 9 * TILE64 + 77):
        a = _dist(np.random.default_rng(1), "few", n)
        d = _dev(a)
        ko, idx = gpu_ctx.argsort_dev(d, keys_out=d)
        assert ko is d
        _check_argsort(a, _host(d), _host(idx))


def test_argsort_without_keys_out(gpu_ctx):
    for n in (9 * 4096 + 77, 9 * TILE64 + 77):
        a = _dist(np.random.default_rng(2), "extremes", n)
        d = _dev(a)
        ko, idx = gpu_ctx.argsort_dev(d)
        assert ko is None
        assert np.array_equal(_host(d), a)
        _check_argsort(a, None, _host(idx))


def test_argsort_stage_never_reached_still_delivers(gpu_ctx, dsort_mod):
    """DSORT_OPT_KILL_AFTER_STAGE past the inner int64 sort's stages: DSORT_ESTAGE, outputs valid."""
    import torch
    n = 5000
    assert gpu_ctx.sort_stages(n, 8) < 50
    a = _dist(np.random.default_rng(3), "uniform", n)
    d = _dev(a)
    out, idx = torch.empty_like(d), torch.empty_like(d)
    with gpu_ctx.options(kill_after_stage=50):
        with pytest.raises(dsort_mod.DsortError) as ei:
            gpu_ctx.argsort_dev(d, idx_out=idx, keys_out=out)
    assert ei.value.rc == ESTAGE
    _check_argsort(a, _host(out), _host(idx))


def test_argsort_size_limit(gpu_ctx):
    """More than 2^32 keys: DSORT_EINVAL before the (small, dummy) buffers are read."""
    import torch
    dummy = torch.zeros(16, dtype=torch.int32, device="cuda")
    lib = gpu_ctx.lib
    rc = lib.dsort_argsort_dev_i32(gpu_ctx.h, dummy.data_ptr(), dummy.data_ptr(), dummy.data_ptr(), (1 << 32) + 1,
                                   gpu_ctx._stream())
    assert rc == EINVAL
    host = np.zeros(16, np.int32)
    rc = lib.dsort_argsort_i32(gpu_ctx.h, host.ctypes.data, host.ctypes.data, host.ctypes.data, (1 << 32) + 1)
    assert rc == EINVAL
    torch.cuda.synchronize()
    assert (_host(dummy) == 0).all()


def test_null_pointers_are_einval(gpu_ctx):
    import torch
    d = torch.zeros(16, dtype=torch.int32, device="cuda")
    p, lib, s = d.data_ptr(), gpu_ctx.lib, gpu_ctx._stream()
    assert lib.dsort_argsort_dev_i32(gpu_ctx.h, None, p, p, 4, s) == EINVAL
    assert lib.dsort_argsort_dev_i32(gpu_ctx.h, p, p, None, 4, s) == EINVAL
    assert lib.dsort_sort_pairs_dev_i32(gpu_ctx.h, p, None, p, p, 4, s) == EINVAL
    assert lib.dsort_sort_pairs_dev_i32(gpu_ctx.h, p, p, p, None, 4, s) == EINVAL
    assert lib.dsort_gather_dev(gpu_ctx.h, None, p, p, 4, 4, s) == EINVAL
    for bad in (0, 2, 12, 32):
        assert lib.dsort_gather_dev(gpu_ctx.h, p, p, p, 4, bad, s) == EINVAL
    # nothing to do: fine, whatever the pointers
    assert lib.dsort_argsort_dev_i32(gpu_ctx.h, None, None, None, 0, s) == 0
    assert lib.dsort_sort_pairs_dev_i32(gpu_ctx.h, None, None, None, None, 0, s) == 0
    assert lib.dsort_gather_dev(gpu_ctx.h, None, None, None, 0, 8, s) == 0


# ------------------------------------------------------------------------------ pairs
@pytest.mark.parametrize("n", [5, 4096 + 1, TILE64 + 1, 300001])
def test_pairs_ties_order_by_unsigned_value(gpu_ctx, n):
    """Keys from [-3, 3], values over the whole uint32 range: a signed comparison of the values
    would put those >= 2^31 first."""
    import torch
    rng = np.random.default_rng(n)
    k = rng.integers(-3, 3, n, endpoint=True).astype(np.int32)
    v = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    v[:: 2] |= np.uint32(1 << 31)
    order = np.lexsort((v, k))
    dk, dv = _dev(k), _dev(v.view(np.int32))
    ko, vo = torch.empty_like(dk), torch.empty_like(dv)
    gpu_ctx.sort_pairs_dev(dk, dv, keys_out=ko, vals_out=vo)
    assert np.array_equal(_host(ko), k[order])
    assert np.array_equal(_host(vo).view(np.uint32), v[order])
    assert np.array_equal(_host(dk), k) and np.array_equal(_host(dv).view(np.uint32), v)
    # in place
    r = gpu_ctx.sort_pairs_dev(dk, dv)
    assert r[0] is dk and r[1] is dv
    assert np.array_equal(_host(dk), k[order])
    assert np.array_equal(_host(dv).view(np.uint32), v[order])


def test_pairs_unique_keys_carry_their_values(gpu_ctx):
    n = 300001
    rng = np.random.default_rng(77)
    k = (rng.permutation(n).astype(np.int64) * 14311 - 2**31).astype(np.int32)  # distinct: 14311 n < 2^32
    assert np.unique(k).size == n
    v = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    order = np.argsort(k, kind="stable")
    dk, dv = _dev(k), _dev(v.view(np.int32))
    gpu_ctx.sort_pairs_dev(dk, dv)
    assert np.array_equal(_host(dk), k[order])
    assert np.array_equal(_host(dv).view(np.uint32), v[order])


# ------------------------------------------------------------------------------ bucketed path
@pytest.mark.parametrize("kind", ["few", "equal"])
def test_argsort_forced_buckets(gpu_ctx, kind):
    """The int64 first level on packed words: all distinct, clustered where the keys repeat, no
    bucket of one key value."""
    import torch
    n = 300001
    a = _dist(np.random.default_rng(8), kind, n)
    d = _dev(a)
    out = torch.empty_like(d)
    with gpu_ctx.options(buckets=8):
        _, idx = gpu_ctx.argsort_dev(d, keys_out=out)
        torch.cuda.synchronize()
    _check_argsort(a, _host(out), _host(idx))


BIG_N = (1 << 25) + 4099


@pytest.mark.parametrize("kind", ["uniform", "equal", "few", "small", "reverse"])
def test_argsort_bucketed_vs_torch(gpu_ctx, kind):
    """The bucketed int64 sort's own path (>= 2^25 keys), against torch's stable sort."""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(len(kind) + 17)
    n = BIG_N
    if kind == "uniform":
        d = torch.randint(I32.min, I32.max + 1, (n,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
    elif kind == "equal":
        d = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    elif kind == "few":
        vals = torch.tensor([I32.min, -1, 0, 1, I32.max], dtype=torch.int32, device="cuda")
        d = vals[torch.randint(0, 5, (n,), generator=g, device="cuda")]
    elif kind == "small":
        d = torch.randint(1, 101, (n,), generator=g, device="cuda", dtype=torch.int32)
    else:
        d = torch.randint(I32.min, I32.max + 1, (n,), generator=g, device="cuda", dtype=torch.int64).to(torch.int32)
        d = torch.sort(d, descending=True).values.contiguous()
    exp_keys, exp_idx = torch.sort(d, stable=True)
    out = torch.empty_like(d)
    _, idx = gpu_ctx.argsort_dev(d, keys_out=out)
    assert torch.equal(out, exp_keys)
    assert torch.equal(idx.to(torch.int64), exp_idx)
    st = gpu_ctx.stats()
    assert st["keys_in"] == n and st["first_level_map"] >= 0  # the bucketed sort ran


# ------------------------------------------------------------------------------ two streams
def test_argsort_on_two_streams_shares_the_arena(gpu_ctx):
    """Two argsorts back to back on different streams, no synchronize in between: the second must
    wait for the first before it packs into the arena they share."""
    import torch
    n = 300001
    rng = np.random.default_rng(99)
    a, b = _dist(rng, "uniform", n), _dist(rng, "few", n)
    da, db = _dev(a), _dev(b)
    outs = [torch.empty_like(da) for _ in range(4)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s1):
        gpu_ctx.argsort_dev(da, idx_out=outs[1], keys_out=outs[0])
    with torch.cuda.stream(s2):
        gpu_ctx.argsort_dev(db, idx_out=outs[3], keys_out=outs[2])
    s1.synchronize()
    s2.synchronize()
    _check_argsort(a, _host(outs[0]), _host(outs[1]))
    _check_argsort(b, _host(outs[2]), _host(outs[3]))


# ------------------------------------------------------------------------------ gather
@pytest.mark.parametrize("n", [1, 257, 100003])
@pytest.mark.parametrize("rec", [4, 8, 16])
def test_gather_vs_numpy(gpu_ctx, n, rec):
    import torch
    rng = np.random.default_rng(n + rec)
    m = n + 5  # the source is longer than the index list
    if rec == 4:
        src = rng.integers(I32.min, I32.max, m, dtype=np.int32)
    elif rec == 8:
        src = rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, m, dtype=np.int64)
    else:
        src = rng.integers(I32.min, I32.max, (m, 4), dtype=np.int32)
    perm = rng.permutation(m)[:n].astype(np.int32)
    dsrc, didx = _dev(src), _dev(perm)
    out = torch.zeros((n,) + tuple(dsrc.shape[1:]), dtype=dsrc.dtype, device="cuda")
    assert gpu_ctx.gather_dev(dsrc, didx, out) is out
    assert np.array_equal(_host(out), src[perm])


def _gather_src(rng, m, rec):
    if rec == 4:
        return rng.integers(I32.min, I32.max, m, dtype=np.int32)
    if rec == 8:
        return rng.integers(np.iinfo(np.int64).min, np.iinfo(np.int64).max, m, dtype=np.int64)
    return rng.integers(I32.min, I32.max, (m, 4), dtype=np.int32)


def _gather_check(gpu_ctx, src, idx, view=0):
    """gather_dev against src[idx].  src, idx and out start at element `view` of their allocations;
    zero guard words of one record around out must stay zero, src and idx unchanged."""
    import torch
    n, row = idx.size, src.shape[1:]
    D = int(np.prod(row, dtype=np.int64))  # elements of one record

    def at(a):  # a device copy that starts at element `view` of its allocation
        flat = np.ascontiguousarray(a).reshape(-1)
        t = torch.zeros(view + max(flat.size, 1), dtype=torch.from_numpy(flat[:0]).dtype, device="cuda")
        t = t[view:view + flat.size]
        if flat.size:
            t.copy_(torch.from_numpy(flat))
        return t

    dsrc, didx = at(src).view(src.shape), at(idx)
    full = torch.zeros(view + (n + 2) * D, dtype=dsrc.dtype, device="cuda")
    out = full[view + D:view + D + n * D].view((n,) + row)
    assert gpu_ctx.gather_dev(dsrc, didx, out) is out
    torch.cuda.synchronize()
    assert np.array_equal(_host(out), src[idx.view(np.uint32).astype(np.int64)])
    full_h = _host(full)
    assert not full_h[:view + D].any() and not full_h[view + D + n * D:].any()
    assert np.array_equal(_host(dsrc), src) and np.array_equal(_host(didx), idx)


GATHER_TRIP = 2048 * 256  # lanes of one trip of gather_kernel's grid: a lane moves 16 / W records


@pytest.mark.parametrize("rec,sizes", [(4, [0, 2, 4, 6, 256, 258]), (8, [0, 2, 256]), (16, [0, 1, 256])])
def test_gather_tails_and_repeated_indices(gpu_ctx, rec, sizes):
    """n without a tail, with a tail of 2 records at W = 4, nothing at all; a permutation that names
    the source's last record, one index n times, indices drawn from 3 positions."""
    rng = np.random.default_rng(rec)
    for n in sizes:
        m = n + 5
        src = _gather_src(rng, m, rec)
        perm = rng.permutation(m)[:n]
        if n:
            perm[rng.integers(0, n)] = m - 1
        for idx in (perm, np.full(n, m - 1), np.full(n, 2), rng.choice(np.array([0, m // 2, m - 1]), n)):
            _gather_check(gpu_ctx, src, idx.astype(np.int32))


@pytest.mark.parametrize("rec", [4, 8, 16])
def test_gather_past_one_trip_of_the_grid(gpu_ctx, rec):
    """257 records more than 2048 workgroups of 256 lanes move in one trip: the grid-stride loop wraps,
    and a tail remains (one record at W = 4 and 8).  Indices with repeats, the last record among them."""
    n = GATHER_TRIP * (16 // rec) + 257
    rng = np.random.default_rng(40 + rec)
    m = 100_003
    src = _gather_src(rng, m, rec)
    idx = rng.integers(0, m, n)
    idx[[0, n // 2, n - 1]] = m - 1
    _gather_check(gpu_ctx, src, idx.astype(np.int32))


@pytest.mark.parametrize("rec", [4, 16])
def test_gather_views_at_element_offsets(gpu_ctx, rec):
    """src, idx and out start 1 and 3 elements into their allocations: dword alignment only."""
    rng = np.random.default_rng(60 + rec)
    for view in (1, 3):
        for n in (6, 258, 1027):
            src = _gather_src(rng, n + 5, rec)
            idx = rng.integers(0, n + 5, n)
            idx[n // 2] = n + 4
            _gather_check(gpu_ctx, src, idx.astype(np.int32), view)


def test_gather_rejects_other_record_sizes(gpu_ctx, dsort_mod):
    import torch
    idx = torch.zeros(4, dtype=torch.int32, device="cuda")
    for shape, dt in (((4, 3), torch.int32), ((4,), torch.int16), ((4, 4), torch.int64)):
        src = torch.zeros(shape, dtype=dt, device="cuda")
        with pytest.raises(dsort_mod.DsortError):
            gpu_ctx.gather_dev(src, idx, torch.zeros_like(src))


def test_sort_records_by_key_end_to_end(gpu_ctx):
    """16-byte records sorted by their first field: argsort of the keys, then the gather."""
    import torch
    n = 100003
    rng = np.random.default_rng(5)
    recs = rng.integers(I32.min, I32.max, (n, 4), dtype=np.int32)
    recs[:, 0] = rng.integers(-50, 50, n)  # many ties: stability decides
    drec = _dev(recs)
    keys = drec[:, 0].contiguous()
    _, idx = gpu_ctx.argsort_dev(keys)
    out = torch.empty_like(drec)
    gpu_ctx.gather_dev(drec, idx, out)
    assert np.array_equal(_host(out), recs[np.argsort(recs[:, 0], kind="stable")])


# ------------------------------------------------------------------------------ host form
@pytest.mark.parametrize("n", [0, 1, 100003])
def test_host_argsort(gpu_ctx, n):
    a = _dist(np.random.default_rng(n + 1), "extremes", n)
    keep = a.copy()
    sk, idx = gpu_ctx.argsort(a)
    assert idx.dtype == np.uint32 and sk.dtype == np.int32
    assert np.array_equal(a, keep)
    _check_argsort(a, sk, idx.view(np.int32))
