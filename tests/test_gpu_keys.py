"""Typed keys and descending order through the local sort entries (dsort_keys.hip and the codec
in the pack / unpack kernels of dsort_pairs.hip and dsort_pairs64.hip; dsort.h, "Key types and
order") on the GPU.

The checker is numpy on the restatement of the header's table in keys_model.py: the expected keys are
x[argsort(ref_encode(x), kind="stable")], compared as bits, and the expected indices that argsort.
On inputs without NaN and without -0.0 the second yardstick is np.sort / np.argsort(kind="stable")
/ torch.sort(stable=True, descending=...) of the typed data itself."""
import numpy as np
import pytest

import keys_model as km

pytestmark = pytest.mark.gpu

EINVAL = -1
TILE = 8192
# the pack's 256-element chunks, the unpack's groups of 4 (encode / decode: 16 bytes), one tile and
# the first merge pass
SIZES = [0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1025, TILE, TILE + 1, 2 * TILE + 1]
CASES = [(name, desc) for name in km.KEY_NAMES for desc in (False, True)]
IDS = [f"{n}-{'desc' if d else 'asc'}" for n, d in CASES]
CASES4 = [c for c in CASES if km.width(c[0]) == 32]
IDS4 = [f"{n}-{'desc' if d else 'asc'}" for n, d in CASES4]


def _kinds(name):
    return ["uniform", "special", "equal", "sorted", "reversed"] + (["narrow", "wide"] if km.width(name) == 64 else [])


def _keys(rng, name, kind, n):
    """n keys of the numpy type of `name`."""
    T, U, W = km.NP_TYPE[name], km.uint_of(name), km.width(name)
    if kind == "uniform":  # every bit pattern: NaNs and denormals for the floats
        return rng.integers(0, 1 << W, n, dtype=U).view(T)
    if kind == "special":  # the curated values, shuffled: heavy ties, both zeros, both NaN signs
        return rng.choice(km.curated(name), n)
    if kind == "equal":
        c = km.curated(name)
        return np.full(n, c[len(c) // 2 - 1], T)  # (floats: -0.0)
    if kind in ("sorted", "reversed"):
        x = _keys(rng, name, "uniform", n)
        x = x[km.ref_order(x, name)]
        return x if kind == "sorted" else x[::-1].copy()
    if kind == "narrow":  # 8-byte types: an encoded range of 2^20 at most -- one pass
        k = rng.integers(0, 1 << 20, n, dtype=np.int64)
        if name == "f64":  # one binade: 1.0 + k 2^-40
            return 1.0 + k.astype(np.float64) * 2.0 ** -40
        if name == "u64":  # ids around 2^63: the raw bits straddle the sign bit
            return (k.astype(np.uint64) + np.uint64(2 ** 63 - 2 ** 19)).astype(np.uint64)
        return k - (1 << 19)
    if kind == "wide":  # the whole encoded range: two passes from two keys on
        x = _keys(rng, name, "uniform", n)
        c = km.curated(name)
        if n >= 2:
            x[n // 3], x[n - 1] = c[-1], c[0]
        return x
    raise ValueError(kind)


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _same_bits(got, want):
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert np.array_equal(km.bits(got), km.bits(want))


def _second_yardstick(x, name, desc, exp_keys, exp_idx):
    """numpy's and torch's own order of the typed data, where the contract says they agree."""
    import torch
    if km.has_nan_or_negzero(x):
        return
    if not desc:
        assert np.array_equal(exp_idx, np.argsort(x, kind="stable"))
        _same_bits(exp_keys, np.sort(x, kind="stable"))
    if name in ("u32", "u64"):  # (torch sorts no unsigned type wider than a byte)
        return
    t = torch.sort(torch.from_numpy(x), stable=True, descending=desc)
    assert np.array_equal(exp_idx, t.indices.numpy())
    _same_bits(exp_keys, t.values.numpy())


def _expected(x, name, desc):
    order = km.ref_order(x, name, desc)
    exp = x[order]
    _second_yardstick(x, name, desc, exp, order)
    return exp, order


def _want_passes(name, kind, n):
    if km.width(name) == 32:
        return 0  # (the pair sort of 4-byte keys leaves argsort_passes 0)
    if n == 0:
        return 0
    if kind in ("narrow", "equal") or n == 1:
        return 1
    if kind == "wide":
        return 2
    return None


# ------------------------------------------------------------------------------ the four calls
@pytest.mark.parametrize("name,desc", CASES, ids=IDS)
def test_keys_only_sort(gpu_ctx, name, desc):
    import torch
    for kind in _kinds(name):
        for n in SIZES:
            rng = np.random.default_rng(n * 31 + len(kind) + km.KEY_CODE[name])
            x = _keys(rng, name, kind, n)
            exp, _ = _expected(x, name, desc)
            d = _dev(x)
            # out of place: the input stays
            out = torch.empty_like(d)
            assert gpu_ctx.sort_dev(d, out=out, descending=desc) is out
            _same_bits(_host(out), exp)
            _same_bits(_host(d), x)
            # in place
            assert gpu_ctx.sort_dev(d, descending=desc) is d
            _same_bits(_host(d), exp)
            assert gpu_ctx.stats()["keys_in"] == n


@pytest.mark.parametrize("name,desc", CASES, ids=IDS)
def test_argsort(gpu_ctx, name, desc):
    import torch
    for kind in _kinds(name):
        for n in SIZES:
            rng = np.random.default_rng(n * 37 + len(kind) + km.KEY_CODE[name])
            x = _keys(rng, name, kind, n)
            exp, order = _expected(x, name, desc)
            d = _dev(x)
            out = torch.empty_like(d)
            ko, idx = gpu_ctx.argsort_dev(d, keys_out=out, descending=desc)
            assert ko is out and idx.dtype == torch.int32
            st = gpu_ctx.stats()
            assert np.array_equal(_host(idx).view(np.uint32).astype(np.int64), order), (kind, n)
            _same_bits(_host(out), exp)
            _same_bits(_host(d), x)
            want = _want_passes(name, kind, n)
            if want is not None:
                assert st["argsort_passes"] == want, (kind, n, st["argsort_passes"])
            if kind == "equal":  # equal keys keep ascending input position in either order
                assert np.array_equal(_host(idx), np.arange(n, dtype=np.int32))


@pytest.mark.parametrize("name,desc", CASES, ids=IDS)
def test_record_sort(gpu_ctx, name, desc):
    import torch
    for kind in _kinds(name):
        for n in SIZES:
            rng = np.random.default_rng(n * 41 + len(kind) + km.KEY_CODE[name])
            x = _keys(rng, name, kind, n)
            exp, order = _expected(x, name, desc)
            rows = rng.integers(-2 ** 31, 2 ** 31, (n, 2), dtype=np.int64).astype(np.int32)  # 8-byte records
            d, r = _dev(x), _dev(rows)
            out = torch.empty_like(d)
            kw = {"key_type": "i32"} if name == "i32" else {}  # (an int32 tensor alone is refused, as before)
            ko, ro = gpu_ctx.sort_records_dev(d, r, keys_out=out, descending=desc, **kw)
            assert ko is out
            assert np.array_equal(_host(ro), rows[order]), (kind, n)
            _same_bits(_host(out), exp)
            _same_bits(_host(d), x)
            assert np.array_equal(_host(r), rows)
            want = _want_passes(name, kind, n)
            if want is not None:
                assert gpu_ctx.stats()["argsort_passes"] == want, (kind, n)


@pytest.mark.parametrize("name,desc", CASES4, ids=IDS4)
def test_pairs(gpu_ctx, name, desc):
    """Equal keys stay ordered by value as unsigned 32-bit ASCENDING, in either key order."""
    import torch
    quad = np.array([0, 1, 0x80000000, 0xFFFFFFFF], np.uint32)
    for kind in _kinds(name):
        for n in SIZES:
            rng = np.random.default_rng(n * 43 + len(kind) + km.KEY_CODE[name])
            x = _keys(rng, name, kind, n)
            v = rng.choice(quad, n) if kind in ("special", "equal") else rng.integers(0, 2 ** 32, n, dtype=np.uint32)
            order = np.lexsort((v, km.ref_encode(x, name, desc)))
            d, dv = _dev(x), _dev(v.view(np.int32))
            ko, vo = torch.empty_like(d), torch.empty_like(dv)
            gpu_ctx.sort_pairs_dev(d, dv, keys_out=ko, vals_out=vo, descending=desc)
            _same_bits(_host(ko), x[order])
            assert np.array_equal(_host(vo).view(np.uint32), v[order]), (kind, n)
            _same_bits(_host(d), x)
            # in place
            gpu_ctx.sort_pairs_dev(d, dv, descending=desc)
            _same_bits(_host(d), x[order])
            assert np.array_equal(_host(dv).view(np.uint32), v[order])


def test_pairs_u32_descending_keeps_values_ascending(gpu_ctx):
    n = TILE + 1
    rng = np.random.default_rng(5)
    x = rng.choice(np.array([0, 7, 2 ** 31, 2 ** 32 - 1], np.uint32), n)
    v = rng.integers(0, 2 ** 32, n, dtype=np.uint32)
    ko, vo = gpu_ctx.sort_pairs_dev(_dev(x), _dev(v.view(np.int32)), descending=True)
    ko, vo = _host(ko), _host(vo).view(np.uint32)
    assert (np.diff(ko.astype(np.int64)) <= 0).all() and ko[0] == 2 ** 32 - 1 and ko[-1] == 0
    for key in np.unique(x):
        assert (np.diff(vo[ko == key].astype(np.int64)) >= 0).all()
        assert np.array_equal(vo[ko == key], np.sort(v[x == key]))


# ------------------------------------------------------------------------------ views, aliasing
@pytest.mark.parametrize("name", ["f32", "f64"])
@pytest.mark.parametrize("off", [1, 3])
def test_misaligned_views(gpu_ctx, name, off):
    """Keys, keys_out, indices and values at element offsets 1 and 3 of their allocations."""
    import torch
    n, desc = 1025, True
    rng = np.random.default_rng(off)
    x = _keys(rng, name, "special", n)
    exp, order = _expected(x, name, desc)

    def view(a):
        buf = torch.zeros(n + 8, dtype=a.dtype, device="cuda")
        buf[off:off + n].copy_(a)
        return buf, buf[off:off + n]

    def guard_ok(buf):  # nothing written outside the view
        h = _host(buf)
        return not h[:off].view(np.uint8).any() and not h[off + n:].view(np.uint8).any()

    kb, k = view(_dev(x))
    ob, o = view(torch.zeros(n, dtype=k.dtype, device="cuda"))
    ib, i = view(torch.zeros(n, dtype=torch.int32, device="cuda"))
    gpu_ctx.argsort_dev(k, idx_out=i, keys_out=o, descending=desc)
    assert np.array_equal(_host(i).view(np.uint32).astype(np.int64), order)
    _same_bits(_host(o), exp)
    assert guard_ok(kb) and guard_ok(ob) and guard_ok(ib)
    # keys-only, out of place and in place, on the views
    o.zero_()
    gpu_ctx.sort_dev(k, out=o, descending=desc)
    _same_bits(_host(o), exp)
    _same_bits(_host(k), x)
    assert guard_ok(kb) and guard_ok(ob)
    rows = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype(np.int32)  # 4-byte records
    rb, r = view(_dev(rows))
    qb, q = view(torch.zeros(n, dtype=torch.int32, device="cuda"))
    gpu_ctx.sort_records_dev(k, r, out=q, descending=desc)
    assert np.array_equal(_host(q), rows[order]) and guard_ok(qb) and guard_ok(rb)
    if name == "f32":
        v = rng.integers(0, 4, n, dtype=np.int64).astype(np.int32)
        vb, vv = view(_dev(v))
        wb, w = view(torch.zeros(n, dtype=torch.int32, device="cuda"))
        gpu_ctx.sort_pairs_dev(k, vv, keys_out=o, vals_out=w, descending=desc)
        po = np.lexsort((v.view(np.uint32), km.ref_encode(x, name, desc)))
        _same_bits(_host(o), x[po])
        assert np.array_equal(_host(w), v[po]) and guard_ok(wb) and guard_ok(vb) and guard_ok(ob)
    gpu_ctx.sort_dev(k, descending=desc)
    _same_bits(_host(k), exp)
    assert guard_ok(kb)


@pytest.mark.parametrize("name,desc", [("f32", True), ("f64", False), ("u64", True), ("u32", False)])
def test_aliasing(gpu_ctx, name, desc):
    """keys_out is keys, and keys_out=None; both paths of the 8-byte types."""
    n = 2 * TILE + 1
    for kind in ("special", "uniform") + (("narrow",) if km.width(name) == 64 else ()):
        x = _keys(np.random.default_rng(n + len(kind)), name, kind, n)
        exp, order = _expected(x, name, desc)
        d = _dev(x)
        ko, idx = gpu_ctx.argsort_dev(d, descending=desc)
        assert ko is None
        assert np.array_equal(_host(idx).view(np.uint32).astype(np.int64), order)
        _same_bits(_host(d), x)
        ko, idx = gpu_ctx.argsort_dev(d, keys_out=d, descending=desc)
        assert ko is d
        assert np.array_equal(_host(idx).view(np.uint32).astype(np.int64), order)
        _same_bits(_host(d), exp)


# ------------------------------------------------------------------------------ record sort
@pytest.mark.parametrize("name", ["f32", "f64"])
@pytest.mark.parametrize("rec", [4, 8, 16])
def test_record_sizes_and_stability(gpu_ctx, name, rec):
    """Rows of 4, 8 and 16 bytes; the rows carry their input position, so rows of equal keys must
    come out in input order."""
    n = TILE + 1
    rng = np.random.default_rng(rec)
    x = rng.choice(np.array([-1.5, -0.0, 0.0, 2.0, np.inf], km.NP_TYPE[name]), n)
    rows = np.repeat(np.arange(n, dtype=np.int32)[:, None], rec // 4, axis=1)
    rows = rows[:, 0].copy() if rec == 4 else rows
    for desc in (False, True):
        exp, order = _expected(x, name, desc)
        ko, ro = gpu_ctx.sort_records_dev(_dev(x), _dev(rows), keys_out=_dev(np.zeros_like(x)), descending=desc)
        ro = _host(ro)
        _same_bits(_host(ko), exp)
        assert np.array_equal(ro, rows[order])
        pos = ro if rec == 4 else ro[:, 0]
        for b in np.unique(km.bits(x)):
            assert (np.diff(pos[km.bits(exp) == b]) > 0).all()


# ------------------------------------------------------------------------------ the bucketed path
@pytest.mark.parametrize("name", ["f32", "f64"])
def test_bucketed_path_vs_torch(gpu_ctx, name):
    """n = 2^25 + 4099: the bucketed sort.  float32 standard normal deviates crowd into a narrow
    range of the encoded space; float64 uniform in [0, 1).  NaN-free and without -0.0: element for
    element torch's stable sort, keys and indices, both orders."""
    import torch
    n = (1 << 25) + 4099
    g = torch.Generator(device="cuda").manual_seed(2026)
    dt = torch.float32 if name == "f32" else torch.float64
    x = torch.randn(n, dtype=dt, device="cuda", generator=g) if name == "f32" else \
        torch.rand(n, dtype=dt, device="cuda", generator=g)
    x[: n // 64] = x[n // 64: 2 * (n // 64)]  # ties
    assert not bool(torch.isnan(x).any()) and not bool(((x == 0) & torch.signbit(x)).any())
    for desc in (False, True):
        ref = torch.sort(x, stable=True, descending=desc)
        out = torch.empty_like(x)
        gpu_ctx.sort_dev(x, out=out, descending=desc)
        st = gpu_ctx.stats()
        print(f"{name} desc={desc} sort_dev: first_level_map={st['first_level_map']} total_ms={st['total_ms']:.2f}")
        assert torch.equal(out, ref.values)
        assert st["keys_in"] == n and st["first_level_map"] >= 0  # (the bucketed path ran)
        ko, idx = gpu_ctx.argsort_dev(x, keys_out=out, descending=desc)
        print(f"{name} desc={desc} argsort_dev: argsort_passes={gpu_ctx.stats()['argsort_passes']}")
        assert torch.equal(ko, ref.values)
        assert torch.equal(idx.to(torch.int64), ref.indices)
        del ref


# ------------------------------------------------------------------------------ integers as before
@pytest.mark.parametrize("name", ["i32", "i64"])
def test_integer_dtypes_ascending_are_the_integer_calls(gpu_ctx, name):
    """Without `descending` the integer dtypes give what they gave and report what they reported;
    the typed entry with DSORT_KEY_I32 / _I64 and flags 0 is the same call."""
    import torch
    n = 2 * TILE + 1
    x = _keys(np.random.default_rng(3), name, "uniform", n)
    exp, order = np.sort(x, kind="stable"), np.argsort(x, kind="stable")
    d = _dev(x)
    out = torch.empty_like(d)
    gpu_ctx.sort_dev(d, out=out)
    st0 = gpu_ctx.stats()
    assert np.array_equal(_host(out), exp)
    out.zero_()
    gpu_ctx.check(gpu_ctx.lib.dsort_sort_dev_copy_keys(gpu_ctx.h, d.data_ptr(), out.data_ptr(), n, km.KEY_CODE[name], 0,
                                                       gpu_ctx._stream()))
    st1 = gpu_ctx.stats()
    assert np.array_equal(_host(out), exp)
    for f in ("keys_in", "keys_out", "tile_keys", "merge_passes", "merge_kernel_launches", "first_level_map",
              "argsort_passes"):
        assert st0[f] == st1[f], f
    ko, idx = gpu_ctx.argsort_dev(d, keys_out=out)
    sa = gpu_ctx.stats()
    assert np.array_equal(_host(idx), order.astype(np.int32)) and np.array_equal(_host(ko), exp)
    idx2 = torch.empty_like(idx)
    gpu_ctx.check(gpu_ctx.lib.dsort_argsort_dev_keys(gpu_ctx.h, d.data_ptr(), None, idx2.data_ptr(), n, km.KEY_CODE[name],
                                                     0, gpu_ctx._stream()))
    assert torch.equal(idx, idx2)
    assert gpu_ctx.stats()["argsort_passes"] == sa["argsort_passes"] == (2 if name == "i64" else 0)
    # int32 keys have a record sort now, asked for by name; an int32 tensor alone is refused as before
    rows = np.arange(n, dtype=np.int32)
    _, ro = gpu_ctx.sort_records_dev(d, _dev(rows), key_type=name)
    assert np.array_equal(_host(ro), order.astype(np.int32))
    if name == "i32":
        import dsort
        with pytest.raises(dsort.DsortError):
            gpu_ctx.sort_records_dev(d, _dev(rows))


def test_unsigned_dtypes_and_override(gpu_ctx):
    """torch's uint32 / uint64 tensors dispatch by dtype; an int32 tensor sorts as unsigned with
    key_type="u32"; a width that does not match is refused."""
    import torch
    n = 1025
    for name in ("u32", "u64"):
        x = _keys(np.random.default_rng(9), name, "uniform", n)
        exp = np.sort(x)
        d = _dev(x)
        assert d.dtype == getattr(torch, "uint" + name[1:])
        _same_bits(_host(gpu_ctx.sort_dev(d.clone())), exp)
        s = _dev(x.view(km.int_of(name)))
        _same_bits(_host(gpu_ctx.sort_dev(s.clone(), key_type=name)).view(x.dtype), exp)
        _, idx = gpu_ctx.argsort_dev(s, key_type=name, descending=True)
        assert np.array_equal(_host(idx), km.ref_order(x, name, True).astype(np.int32))
    import dsort
    with pytest.raises(dsort.DsortError):
        gpu_ctx.sort_dev(_dev(np.zeros(4, np.int32)), key_type="u64")


# ------------------------------------------------------------------------------ host forms
@pytest.mark.parametrize("name", ["f32", "u64"])
@pytest.mark.parametrize("n", [0, 1, TILE + 1, 300001])
def test_host_forms(gpu_ctx, name, n):
    for desc in (False, True):
        for kind in ("uniform", "special"):
            x = _keys(np.random.default_rng(n + len(kind)), name, kind, n)
            exp, order = _expected(x, name, desc)
            keep = x.copy()
            ko, idx = gpu_ctx.argsort(x, descending=desc)
            assert idx.dtype == np.uint32 and np.array_equal(idx.astype(np.int64), order)
            _same_bits(ko, exp)
            _same_bits(x, keep)
            assert gpu_ctx.sort(x, descending=desc) is x
            _same_bits(x, exp)


# ------------------------------------------------------------------------------ errors
def test_errors_touch_nothing(gpu_ctx):
    import torch
    import dsort
    lib, h, s = gpu_ctx.lib, gpu_ctx.h, gpu_ctx._stream()
    n = 64
    k = _dev(np.arange(n, dtype=np.int64))
    v = _dev(np.arange(n, dtype=np.int32))
    o = torch.full((n,), 7, dtype=torch.int64, device="cuda")
    w = torch.full((4 * n,), 9, dtype=torch.int32, device="cuda")

    def untouched():
        torch.cuda.synchronize()
        return (bool((o == 7).all()) and bool((w == 9).all()) and np.array_equal(_host(k), np.arange(n))
                and np.array_equal(_host(v), np.arange(n)))

    for kt in (3, 4, 5):  # the pairs call takes 4-byte key types only
        for fl in (0, 1):
            assert lib.dsort_sort_pairs_dev_keys(h, k.data_ptr(), v.data_ptr(), o.data_ptr(), w.data_ptr(), n, kt, fl,
                                                 s) == EINVAL
    assert "4-byte" in lib.dsort_last_error(h).decode()
    for rec in (0, 2, 12, 32):
        for kt in (2, 5):
            assert lib.dsort_sort_records_dev_keys(h, k.data_ptr(), o.data_ptr(), v.data_ptr(), w.data_ptr(), n, rec, kt,
                                                   1, s) == EINVAL
    with pytest.raises(dsort.DsortError):
        gpu_ctx.sort_records_dev(k, torch.zeros((n, 3), dtype=torch.int32, device="cuda"), descending=True)
    big = 2 ** 32 + 1
    for kt in (2, 5):
        assert lib.dsort_argsort_dev_keys(h, k.data_ptr(), o.data_ptr(), w.data_ptr(), big, kt, 1, s) == EINVAL
        assert lib.dsort_sort_records_dev_keys(h, k.data_ptr(), o.data_ptr(), v.data_ptr(), w.data_ptr(), big, 4, kt, 0,
                                               s) == EINVAL
        assert lib.dsort_argsort_keys(h, k.data_ptr(), o.data_ptr(), w.data_ptr(), big, kt, 0) == EINVAL
    for kt, fl in ((-1, 0), (6, 0), (2, 2), (5, 3)):
        assert lib.dsort_sort_dev_keys(h, o.data_ptr(), n, kt, fl, s) == EINVAL
        assert lib.dsort_sort_dev_copy_keys(h, k.data_ptr(), o.data_ptr(), n, kt, fl, s) == EINVAL
        assert lib.dsort_argsort_dev_keys(h, k.data_ptr(), o.data_ptr(), w.data_ptr(), n, kt, fl, s) == EINVAL
        assert lib.dsort_sort_pairs_dev_keys(h, v.data_ptr(), v.data_ptr(), w.data_ptr(), w.data_ptr(), n, kt, fl,
                                             s) == EINVAL
        assert lib.dsort_sort_records_dev_keys(h, k.data_ptr(), o.data_ptr(), v.data_ptr(), w.data_ptr(), n, 4, kt, fl,
                                               s) == EINVAL
    assert untouched()
    # the context still sorts
    x = _keys(np.random.default_rng(1), "f32", "uniform", 1025)
    _same_bits(_host(gpu_ctx.sort_dev(_dev(x), descending=True)), x[km.ref_order(x, "f32", True)])
