"""The first level's arithmetic bucket map on the GPU (csrc/dsort_bucket.h: BkMap.ar, the rule of
bucket_slotmap_kernel, the histogram's arithmetic branch and the scatter's arithmetic instance), every output
bit-exact against torch.sort.

The decision is checked against its numpy restatement (tests/bkarith_model.py) on the shapes and sizes of
tests/test_gpu_slotmaps.py, the bucket count forced with DSORT_OPT_BUCKETS: a sort on the map reports
first_level_map 0 (the map replaces the plain fixed map only).  The switch (-1 rule, 0 off, 2 whenever the
samples' key range allows it) and the flag are debug entries outside the ABI.  One sort of 2^25 + 4099 keys
takes the default path: about 7 sub-tiles per workgroup, a guarded last sub-tile, output alignments the line
scatter's phantoms depend on.
"""
import numpy as np
import pytest

import bkarith_model as bm
import slotmap_model as sm

pytestmark = pytest.mark.gpu

ORDERS = ("generated", "ascending", "descending")
N_DEFAULT = (1 << 25) + 4099
_REF = {}


def _ordered(a, order):
    if order == "generated":
        return a
    s = np.sort(a)
    return s if order == "ascending" else s[::-1].copy()


def _torch_sorted(t, descending=False):
    import torch
    return torch.sort(t, descending=descending).values


def _sort(ctx, a, B, mode=-1):
    """Sorts int32 keys `a` out of place in B buckets: (output, stats, the map's flag)."""
    import torch
    t = torch.from_numpy(a).cuda()
    out = torch.empty_like(t)
    ctx.bucket_arith_mode(mode)
    try:
        with ctx.options(buckets=B):
            ctx.sort_dev(t, out)
        torch.cuda.synchronize()
        st, flag = ctx.stats(), ctx.bucket_arith()
    finally:
        ctx.bucket_arith_mode(-1)
    assert torch.equal(out, _torch_sorted(t))
    assert np.array_equal(t.cpu().numpy(), a)  # the input is left alone
    return out.cpu().numpy(), st, flag


def _check(ctx, name, B, n, order, mode=-1):
    a = _ordered(sm.make_keys(np.int32, name, B, n), order)
    os_ = ctx.get_option("bucket_oversample")
    want = bm.decide(a, B, os_, mode)
    _, st, flag = _sort(ctx, a, B, mode)
    print(f"{name} B={B} n={n} {order} mode {mode}: model {want} flag {flag} map {st['first_level_map']}")
    assert flag == want["take"], (flag, want)
    if flag:
        assert st["first_level_map"] == 0, st
    return a, st, flag, want


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("B,n", sm.SIZES)
@pytest.mark.parametrize("name", ["uniform", "bit0"])
def test_decision_on_even_keys(gpu_ctx, name, B, n, order):
    """As generated they take the map; sorted and reversed they refuse it (the runs hint)."""
    _, _, flag, _ = _check(gpu_ctx, name, B, n, order)
    assert flag == (order == "generated")


@pytest.mark.parametrize("name,size", [("ref100", sm.SIZES[0]), ("zipf", sm.SIZES[1]), ("mixed100", sm.SIZES[2]),
                                       ("uniform", sm.SMALL)])
def test_decision_refuses(gpu_ctx, name, size):
    """One refusal of each kind: the span, the adaptive map, the refined slot, the sample count."""
    a, st, flag, want = _check(gpu_ctx, name, *size, "generated")
    assert not flag
    assert st["first_level_map"] == sm.predict(a, size[0], gpu_ctx.get_option("bucket_oversample"))["map"]


@pytest.mark.parametrize("B,n", sm.SIZES)
@pytest.mark.parametrize("name", ["uniform", "bit0"])
def test_switched_off_keeps_the_packed_lookup(gpu_ctx, name, B, n):
    """Mode 0: the sampled splitters and the packed lookup (bit0: keys that differ from a splitter in bit 0
    only), which the map otherwise takes these inputs away from."""
    a, st, flag, _ = _check(gpu_ctx, name, B, n, "generated", mode=0)
    assert not flag
    assert st["first_level_map"] == sm.predict(a, B, gpu_ctx.get_option("bucket_oversample"))["map"]


@pytest.mark.parametrize("mode", [-1, 2])
def test_edges_of_the_key_range(gpu_ctx, mode):
    """klo = INT32_MIN and klo + span = INT32_MAX are sampled or not: either way keys at and beyond the
    samples' range fall in the first and last bucket."""
    n, B = 200_003, 64
    rng = np.random.default_rng(20261)
    a = rng.integers(sm.I32_MIN, sm.I32_MAX, n, dtype=np.int32, endpoint=True)
    at = rng.choice(n, 100, replace=False)
    a[at[:50]], a[at[50:]] = sm.I32_MIN, sm.I32_MAX
    want = bm.decide(a, B, gpu_ctx.get_option("bucket_oversample"), mode)
    out, st, flag = _sort(gpu_ctx, a, B, mode)
    print(f"edges mode {mode}: model {want} flag {flag}")
    assert flag == want["take"] and (mode != 2 or flag)
    assert (out[:50] == sm.I32_MIN).all() and (out[-50:] == sm.I32_MAX).all()


def test_forced_on_clustered_keys_is_still_exact(gpu_ctx):
    """The safety net: forced onto the map, mixed_cluster puts 24 x the mean in one bucket; the second level
    sorts it whichever path that bucket takes."""
    B, n = sm.SIZES[2]
    a = sm.make_keys(np.int32, "mixed_cluster", B, n)
    _, st, flag = _sort(gpu_ctx, a, B, mode=2)
    print(f"mixed_cluster forced: flag {flag} sub_scatter_fallback {st['sub_scatter_fallback']} "
          f"sub_split_subbuckets {st['sub_split_subbuckets']}")
    assert flag and st["first_level_map"] == 0


def _default_keys():
    import torch
    if not _REF:
        a = np.random.default_rng(0xB0A).integers(sm.I32_MIN, sm.I32_MAX, N_DEFAULT, dtype=np.int32, endpoint=True)
        _REF["keys"] = torch.from_numpy(a).cuda()
        _REF["sorted"] = _torch_sorted(_REF["keys"])
    return _REF["keys"], _REF["sorted"]


@pytest.mark.parametrize("where", ["out_of_place", "in_place", "out_at_4", "out_at_12"])
def test_default_path(gpu_ctx, where):
    """Default options: 2^25 + 4099 uniform keys take the map."""
    import torch
    keys, want = _default_keys()
    if where == "in_place":
        out = gpu_ctx.sort_dev(keys.clone())
    else:
        off = {"out_of_place": 0, "out_at_4": 1, "out_at_12": 3}[where]
        buf = torch.empty(N_DEFAULT + 4, dtype=torch.int32, device="cuda")
        out = buf[off:off + N_DEFAULT]
        assert out.data_ptr() % 16 == 4 * off
        gpu_ctx.sort_dev(keys, out)
    torch.cuda.synchronize()
    assert gpu_ctx.bucket_arith()
    assert gpu_ctx.stats()["first_level_map"] == 0
    assert torch.equal(out, want)


def test_default_path_typed_keys(gpu_ctx):
    """float32 keys and descending int32 keys through the typed entries, whichever map they take."""
    import torch
    keys, want = _default_keys()
    out = torch.empty_like(keys)
    gpu_ctx.sort_dev(keys, out, descending=True)
    torch.cuda.synchronize()
    print(f"descending int32: flag {gpu_ctx.bucket_arith()}")
    assert torch.equal(out, want.flip(0))
    f = torch.from_numpy(np.random.default_rng(0xF10A7).standard_normal(N_DEFAULT).astype(np.float32)).cuda()
    fo = torch.empty_like(f)
    gpu_ctx.sort_dev(f, fo)
    torch.cuda.synchronize()
    print(f"float32: flag {gpu_ctx.bucket_arith()}")
    assert torch.equal(fo.view(torch.int32), _torch_sorted(f).view(torch.int32))
