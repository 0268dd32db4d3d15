"""Top-k selection on the GPU (dsort_topk.hip; dsort.h, "top-k"): dsort_topk_dev_keys and
dsort_topk_keys for all six key types and both orders, through the select path, the full path and
the automatic choice.

The checker is keys_model.ref_order(x, name, desc)[:k] and x[...] of it, compared as bits; on inputs
without NaN and -0.0 the VALUES of torch.topk(sorted=True) are a second yardstick (torch promises no
tie order, so its indices are not used).  The path a call took is read from the inner sort's
statistics: keys_in == k on the select path, n on the full path."""
import numpy as np
import pytest

import keys_model as km
from test_gpu_keys import _keys

pytestmark = pytest.mark.gpu

EINVAL = -1
MAXWG = 2048    # workgroups of a launch at most
MIN_TILES = 4   # tiles of a workgroup's range at least
CASES = [(name, desc) for name in km.KEY_NAMES for desc in (False, True)]
IDS = [f"{n}-{'desc' if d else 'asc'}" for n, d in CASES]
SELECT, FULL, AUTO = 1, 0, -1


def tile_of(name):
    """Keys of one tile of the select's kernels: 256 lanes x one 16-byte load."""
    return 256 * (16 // (km.width(name) // 8))


def grid_of(n, name):
    """(workgroups, keys per workgroup range) of the select's launches over n keys: the rule of
    select_grid in dsort_topk.hip, restated."""
    tile = tile_of(name)
    tiles = -(-n // tile)
    chunk = max(-(-tiles // MAXWG), MIN_TILES) * tile
    return max(-(-n // chunk), 1), chunk


def full_grid_n(name):
    """The smallest n at which the launch has its full capped grid and every workgroup loops more
    than once."""
    n = ((MAXWG - 1) * MIN_TILES + 1) * tile_of(name) + 1
    for m in (n, n - 1):
        G, chunk = grid_of(m, name)
        last = m - (G - 1) * chunk
        ok = G == MAXWG and last > tile_of(name)
        assert ok == (m == n), (m, G, chunk, last)
    return n


def range_of(name):
    """Keys of one workgroup's range below the full grid."""
    return MIN_TILES * tile_of(name)


def sizes_of(name):
    t, r = tile_of(name), range_of(name)
    return [1, 2, 3, 4, 5, 255, 256, 257, t - 1, t, t + 1, r - 1, r, r + 1, 2 * r + 1, 8193]


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _host(t):
    return t.cpu().numpy()


def _same_bits(got, want):
    assert got.dtype == want.dtype, (got.dtype, want.dtype)
    assert np.array_equal(km.bits(got), km.bits(want))


def _torch_values(x, name, desc, k, exp_keys):
    import torch
    if name in ("u32", "u64") or km.has_nan_or_negzero(x) or k == 0:
        return
    v = torch.topk(torch.from_numpy(x), k, largest=desc, sorted=True).values.numpy()
    _same_bits(exp_keys, v)


PAD = 3


def topk_checked(ctx, x, name, desc, k, path, order=None, want_keys=True):
    """One device call under the forced path, with every check of the contract; returns the stats."""
    n = x.size
    order = km.ref_order(x, name, desc) if order is None else order
    exp_idx, exp_keys = order[:k], x[order[:k]]
    d = _dev(x)
    fill = np.array([0x5A5A5A5A5A5A5A5A], np.uint64).view(km.uint_of(name))[0]
    kbuf = _dev(np.full(k + PAD, fill, km.uint_of(name)).view(km.NP_TYPE[name]))
    ibuf = _dev(np.full(k + PAD, 0x6B6B6B6B, np.uint32).view(np.int32))
    with ctx.options(topk_path=path):
        ko, io = ctx.topk_dev(d, k, descending=desc, keys_out=kbuf[:k] if want_keys else False, idx_out=ibuf[:k])
        st = ctx.stats()
    tag = (name, desc, n, k, path)
    assert np.array_equal(_host(ibuf)[:k].view(np.uint32).astype(np.int64), exp_idx), tag
    assert (_host(ibuf)[k:].view(np.uint32) == 0x6B6B6B6B).all(), tag  # nothing behind element k
    if want_keys:
        _same_bits(_host(kbuf)[:k], exp_keys)
    else:
        assert ko is None
    assert (km.bits(_host(kbuf))[k if want_keys else 0:] == fill).all(), tag
    _same_bits(_host(d), x)  # the input is unchanged
    took = path if path != AUTO else (1 if ctx_plan(ctx, n, k, name) == 1 else 0)
    assert st["keys_in"] == (k if took == SELECT else n), (tag, st["keys_in"])
    return st


def ctx_plan(ctx, n, k, name):
    import dsort
    return dsort.plan_topk(n, k, km.width(name) // 8)[0]


def ks_of(n):
    return sorted({k for k in (1, 2, n // 2, n - 1, n) if 1 <= k <= n})


# ------------------------------------------------------------------------------ sizes and paths
@pytest.mark.parametrize("name,desc", CASES, ids=IDS)
def test_sizes_kinds_and_paths(gpu_ctx, name, desc):
    kinds = ["uniform", "special"] + (["narrow", "wide"] if km.width(name) == 64 else [])
    for n in sizes_of(name):
        for kind in kinds:
            rng = np.random.default_rng(n * 53 + len(kind) + km.KEY_CODE[name])
            x = _keys(rng, name, kind, n)
            order = km.ref_order(x, name, desc)
            for k in ks_of(n):
                _torch_values(x, name, desc, k, x[order[:k]])
                st = topk_checked(gpu_ctx, x, name, desc, k, SELECT, order)
                if km.width(name) == 64:
                    if kind == "narrow" or k == 1:
                        assert st["argsort_passes"] == 1, (kind, n, k)
                    elif kind == "wide" and k == n:
                        assert st["argsort_passes"] == 2, (kind, n, k)
            for k in (1, n):  # the other two paths at both ends
                st = topk_checked(gpu_ctx, x, name, desc, k, FULL, order)
                if km.width(name) == 64 and kind == "wide" and n >= 2:
                    assert st["argsort_passes"] == 2, (kind, n, k)
                topk_checked(gpu_ctx, x, name, desc, k, AUTO, order)


def test_auto_takes_the_select_path_where_the_plan_says_so(gpu_ctx, dsort_mod):
    """The rule's own edges: n = 2^24 with k up to n / 2, and one key fewer."""
    rng = np.random.default_rng(5)
    n = 1 << 24
    x = _keys(rng, "f32", "uniform", n)
    order = km.ref_order(x, "f32", True)
    for m, k, want in ((n, 1, 1), (n, n // 2, 1), (n, n // 2 + 1, 2), (1 << 15, 1, 2)):
        assert dsort_mod.plan_topk(m, k, 4)[0] == want
        st = topk_checked(gpu_ctx, x[:m], "f32", True, k, AUTO, order if m == n else None, want_keys=k == 1)
        assert st["keys_in"] == (k if want == 1 else m)
    assert dsort_mod.plan_topk(n - 1, 1, 4)[0] == 2


# ------------------------------------------------------------------------------ inputs
def _input(rng, name, kind, n):
    T, U, W = km.NP_TYPE[name], km.uint_of(name), km.width(name)
    c = km.curated(name)
    if kind in ("equal", "sorted", "reversed"):
        return _keys(rng, name, kind, n)
    if kind == "last_digit":   # the earlier passes see one bin
        return ((U(0x3FF) << U(W - 12)) | rng.integers(0, 1 << 9, n, dtype=U)).astype(U).view(T)
    if kind == "first_digit":  # every later pass sees one bin
        return ((rng.integers(0, 1 << 11, n, dtype=U) << U(W - 11)) | U(0x155)).astype(U).view(T)
    if kind == "zeros_ones":   # the words whose digits are all 0 or all ones: the type's first and last key
        return rng.choice(np.array([c[0], c[-1]]), n)
    raise ValueError(kind)


@pytest.mark.parametrize("name,desc", CASES, ids=IDS)
def test_inputs(gpu_ctx, name, desc):
    t, r = tile_of(name), range_of(name)
    for n in (t + 1, 2 * r + t + 5):
        for kind in ("equal", "sorted", "reversed", "last_digit", "first_digit", "zeros_ones"):
            rng = np.random.default_rng(n * 59 + len(kind) + km.KEY_CODE[name])
            x = _input(rng, name, kind, n)
            order = km.ref_order(x, name, desc)
            if kind == "equal":
                assert np.array_equal(order, np.arange(n))  # expect idx == 0 .. k-1
            for k in (1, 2, n // 3, n - 1, n):
                topk_checked(gpu_ctx, x, name, desc, k, SELECT, order)
            topk_checked(gpu_ctx, x, name, desc, n // 3, FULL, order)
            topk_checked(gpu_ctx, x, name, desc, n // 3, AUTO, order)


@pytest.mark.parametrize("name,desc", CASES, ids=IDS)
def test_cut_inside_a_run_of_equal_keys(gpu_ctx, name, desc):
    """The cut on the first, a middle and the last copy of a run, and inside a run that spans more
    than three workgroup ranges: the lowest positions win."""
    t = range_of(name)
    c = km.curated(name)
    first, tie, later = (c[3], c[2], c[1]) if desc else (c[1], c[2], c[3])
    rng = np.random.default_rng(61 + km.KEY_CODE[name])
    for n, a, b in ((3 * t + 5, t // 2, t // 2 + 100), (5 * t + 7, t // 2, 4 * t + 3)):
        G, chunk = grid_of(n, name)
        assert chunk == t and (b - 1) // chunk - a // chunk >= (3 if b - a > 100 else 0)
        x = np.full(n, later, km.NP_TYPE[name])
        x[a:b] = tie
        ahead = rng.choice(np.r_[0:a, b:n], 37, replace=False)  # 37 keys that come before the run
        x[ahead] = first
        order = km.ref_order(x, name, desc)
        run = b - a
        for j in (1, 2, run // 2, run - 1, run):
            k = 37 + j
            topk_checked(gpu_ctx, x, name, desc, k, SELECT, order)
            # the winners among the copies are the first j of them
            assert np.array_equal(order[37:k], np.arange(a, a + j))
        topk_checked(gpu_ctx, x, name, desc, 37 + run // 2, FULL, order)
        # the same run in pieces: every other key of the range
        y = np.full(n, later, km.NP_TYPE[name])
        y[a:b:2] = tie
        y[ahead] = first
        topk_checked(gpu_ctx, y, name, desc, 37 + (b - a) // 4, SELECT)


@pytest.mark.parametrize("name,desc", [(n, i % 2 == 1) for i, n in enumerate(km.KEY_NAMES)],
                         ids=[f"{n}-{'desc' if i % 2 else 'asc'}" for i, n in enumerate(km.KEY_NAMES)])
def test_full_grid(gpu_ctx, name, desc):
    """The full capped grid with every workgroup looping more than once, plus 5 keys."""
    n = full_grid_n(name) + 5
    assert grid_of(n, name)[0] == MAXWG
    rng = np.random.default_rng(67 + km.KEY_CODE[name])
    x = _keys(rng, name, "uniform", n)
    c = km.curated(name)
    x[rng.integers(0, n, n // 2)] = c[0] if not desc else c[-1]  # a heavy tie on the first key of the order
    order = km.ref_order(x, name, desc)
    heavy = int((km.bits(x) == km.bits(np.array([c[0] if not desc else c[-1]]))[0]).sum())
    for k in (1, 1000, heavy - 3, heavy + 1000):
        topk_checked(gpu_ctx, x, name, desc, k, SELECT, order, want_keys=k != 1000)


# ------------------------------------------------------------------------------ the rest of the contract
def test_k_zero_touches_nothing_and_k_above_n_raises(gpu_ctx, dsort_mod):
    import torch
    lib = dsort_mod.load()
    x = np.arange(100, dtype=np.int32)
    d = _dev(x)
    idx = _dev(np.full(8, 7, np.int32))
    gpu_ctx.sort_dev(_dev(np.arange(10, dtype=np.int32)))
    before = gpu_ctx.stats()
    ko, io = gpu_ctx.topk_dev(d, 0)
    assert ko.numel() == 0 and io.numel() == 0
    # k == 0 with every pointer NULL
    assert lib.dsort_topk_dev_keys(gpu_ctx.h, None, 0, 0, 0, 0, None, None, gpu_ctx._stream()) == 0
    assert lib.dsort_topk_dev_keys(gpu_ctx.h, d.data_ptr(), 100, 0, 0, 0, None, None, gpu_ctx._stream()) == 0
    assert gpu_ctx.stats() == before
    args = (d.data_ptr(), 100)
    s = gpu_ctx._stream()
    assert lib.dsort_topk_dev_keys(gpu_ctx.h, *args, 101, 0, 0, None, idx.data_ptr(), s) == EINVAL  # k > n
    assert lib.dsort_topk_dev_keys(gpu_ctx.h, *args, 5, 6, 0, None, idx.data_ptr(), s) == EINVAL    # key type
    assert lib.dsort_topk_dev_keys(gpu_ctx.h, *args, 5, 0, 2, None, idx.data_ptr(), s) == EINVAL    # flag bit
    assert lib.dsort_topk_dev_keys(gpu_ctx.h, *args, 5, 0, 0, None, None, s) == EINVAL              # no idx_out
    assert lib.dsort_topk_dev_keys(gpu_ctx.h, None, 100, 5, 0, 0, None, idx.data_ptr(), s) == EINVAL
    assert lib.dsort_topk_dev_keys(gpu_ctx.h, *[d.data_ptr(), (1 << 32) + 1], 5, 0, 0, None, idx.data_ptr(), s) == EINVAL
    assert lib.dsort_topk_keys(gpu_ctx.h, x.ctypes.data, 100, 101, 0, 0, None, x.ctypes.data) == EINVAL
    torch.cuda.synchronize()
    assert (_host(idx) == 7).all() and np.array_equal(_host(d), x)
    with pytest.raises(dsort_mod.DsortError):
        gpu_ctx.topk_dev(d, 101)
    with pytest.raises(dsort_mod.DsortError):
        gpu_ctx.topk(x, 101)


def test_option_19_and_20(gpu_ctx, dsort_mod):
    lib = dsort_mod.load()
    assert gpu_ctx.get_option("topk_path") == -1
    for v in (-1, 0, 1):
        with gpu_ctx.options(topk_path=v):
            assert gpu_ctx.get_option("topk_path") == v
    for v in (-2, 2):
        assert lib.dsort_set_option(gpu_ctx.h, 19, v) == EINVAL
    assert lib.dsort_set_option(gpu_ctx.h, 20, 0) == EINVAL
    assert gpu_ctx.get_option("topk_path") == -1


@pytest.mark.parametrize("name,desc", CASES, ids=IDS)
def test_host_form_agrees_with_the_device_form(gpu_ctx, name, desc):
    rng = np.random.default_rng(71 + km.KEY_CODE[name])
    for n in (1, 257, 2 * range_of(name) + 5):
        x = _keys(rng, name, "special" if n == 257 else "uniform", n)
        order = km.ref_order(x, name, desc)
        for path in (SELECT, FULL):
            for k in sorted({1, n // 2 + 1, n}):
                with gpu_ctx.options(topk_path=path):
                    hk, hi = gpu_ctx.topk(x, k, descending=desc)
                    dk, di = gpu_ctx.topk_dev(_dev(x), k, descending=desc)
                assert hi.dtype == np.uint32 and np.array_equal(hi.astype(np.int64), order[:k])
                _same_bits(hk, x[order[:k]])
                _same_bits(_host(dk), hk)
                assert np.array_equal(_host(di).view(np.uint32), hi)


def test_key_type_override_and_view_at_element_one(gpu_ctx):
    """An int32 tensor taken as unsigned, and a view that starts at element 1 (4-byte aligned only)."""
    rng = np.random.default_rng(73)
    x = rng.integers(-2 ** 31, 2 ** 31, 5001, dtype=np.int64).astype(np.int32)
    d = _dev(x)
    with gpu_ctx.options(topk_path=SELECT):
        ko, io = gpu_ctx.topk_dev(d[1:], 100, descending=True, key_type="u32")
    order = km.ref_order(x[1:].view(np.uint32), "u32", True)[:100]
    assert np.array_equal(_host(io).view(np.uint32).astype(np.int64), order)
    assert np.array_equal(_host(ko), x[1:][order])
    y = rng.integers(0, 1 << 64, 3001, dtype=np.uint64).view(np.float64)
    e = _dev(y)
    with gpu_ctx.options(topk_path=SELECT):
        ko, io = gpu_ctx.topk_dev(e[1:], 64)
    order = km.ref_order(y[1:], "f64")[:64]
    assert np.array_equal(_host(io).view(np.uint32).astype(np.int64), order)
    _same_bits(_host(ko), y[1:][order])
