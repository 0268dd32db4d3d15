"""The second level's arithmetic sub-bucket map on the GPU (csrc/dsort_sub.h: arith_sub, sb_splitter_kernel's
rule, sb_local_kernel's short cut), bit-exact against np.sort / torch.sort.

The smallest shapes that still have many sub-buckets and several chunks per bucket, the bucket count forced
with DSORT_OPT_BUCKETS: 2^20 + 3 keys in 8 buckets (about 85 sub-buckets, 9 chunks each), 3 * 2^20 + 1 in 4
(about 512, 52 chunks) and 2^21 in 2, whose buckets span 2^31 keys and more (the unsigned arithmetic); one
2^25-key sort on the automatic path.  Sorted and reversed input gives clumped samples (runs of 8 adjacent
keys), which the rule knows by their order and bounds by six runs per sub-bucket instead of 3 * os samples.
The switch (-1 rule, 0 off, 2 every bucket whose span allows it) and the counter (buckets of several
sub-buckets, those on the map) are debug entries outside the ABI.
"""
import numpy as np
import pytest

from subarith_model import predict_take

SHAPES = [((1 << 20) + 3, 8), (3 * (1 << 20) + 1, 4), (1 << 21, 2)]
I32 = (-(2**31), 2**31)


def uniform(n, seed):
    return np.random.default_rng(seed).integers(*I32, n, dtype=np.int64).astype(np.int32)


def smooth(n, seed):  # the sum of three uniforms over the whole key range: a bell, smooth at a bucket's scale
    r = np.random.default_rng(seed)
    return ((r.random(n) + r.random(n) + r.random(n) - 1.5) * (2**32 / 3 - 1)).astype(np.int64).astype(np.int32)


def clustered(n, seed):  # uniform keys, 30 % of them drawn from 4096 adjacent values
    r = np.random.default_rng(seed)
    k = r.integers(*I32, n, dtype=np.int64)
    hot = r.random(n) < 0.3
    k[hot] = r.integers(123_456_789, 123_456_789 + 4096, int(hot.sum()))
    return k.astype(np.int32)


def arranged(keys, order):
    return {"random": keys, "sorted": np.sort(keys), "reversed": np.sort(keys)[::-1].copy()}[order]


def run(ctx, keys, B=None, mode=-1):
    """Sorts `keys` on the GPU: (output, stats, (buckets of several sub-buckets, those on the map))."""
    import torch
    t = torch.from_numpy(keys).cuda()
    o = torch.empty_like(t)
    ctx.sub_arith_mode(mode)
    try:
        if B is None:
            ctx.sort_dev(t, o)
        else:
            with ctx.options(buckets=B):
                ctx.sort_dev(t, o)
        torch.cuda.synchronize()
        return o.cpu().numpy(), ctx.stats(), ctx.sub_arith_counts()
    finally:
        ctx.sub_arith_mode(-1)


@pytest.mark.parametrize("n,B", SHAPES)
def test_cpu_model_expects_the_uniform_inputs_to_take_the_map(n, B):
    """The rule, restated in numpy over a model of the buckets, takes every bucket of the inputs below."""
    many, take = predict_take(uniform(n, 0xA11CE + B), B)
    assert many == B and take == B


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["random", "sorted", "reversed"])
@pytest.mark.parametrize("n,B", SHAPES)
def test_uniform_takes_the_map(gpu_ctx, n, B, order):
    keys = arranged(uniform(n, 0xA11CE + B), order)
    out, st, (many, took) = run(gpu_ctx, keys, B)
    print(f"n {n} B {B} {order}: several sub-buckets {many}, on the map {took}, split {st['sub_split_subbuckets']}, "
          f"fallback {st['sub_scatter_fallback']}")
    assert np.array_equal(out, np.sort(keys))
    assert many >= 1 and took >= 0.9 * many, (many, took)
    assert st["sub_split_subbuckets"] == 0 and st["sub_scatter_fallback"] == 0, st


@pytest.mark.gpu
@pytest.mark.parametrize("n,B", SHAPES[:2])
def test_smooth_density_bit_exact(gpu_ctx, n, B):
    keys = smooth(n, 7)
    out, st, counts = run(gpu_ctx, keys, B)
    print(f"n {n} B {B} smooth: counts {counts}, split {st['sub_split_subbuckets']}")
    assert np.array_equal(out, np.sort(keys))


@pytest.mark.gpu
@pytest.mark.parametrize("n,B", SHAPES[:2])
def test_cluster_buckets_refuse_and_forcing_them_is_still_exact(gpu_ctx, n, B):
    """The buckets that hold the cluster's edges next to uniform keys refuse the map; the others take it.
    Forced onto the map (mode 2) their cluster falls into one sub-bucket far above a tile: the split-and-
    merge path sorts it, exactly."""
    keys = clustered(n, 11)
    want = np.sort(keys)
    out, st, (many, took) = run(gpu_ctx, keys, B)
    print(f"n {n} B {B} clustered: several sub-buckets {many}, on the map {took}, split {st['sub_split_subbuckets']}")
    assert np.array_equal(out, want)
    assert 1 <= took < many <= B, (many, took)
    out2, st2, (many2, took2) = run(gpu_ctx, keys, B, mode=2)
    print(f"  forced: on the map {took2} of {many2}, split {st2['sub_split_subbuckets']}, fallback {st2['sub_scatter_fallback']}")
    assert np.array_equal(out2, want)
    assert took2 > took and st2["sub_split_subbuckets"] > 0, (took2, st2)


@pytest.mark.gpu
@pytest.mark.parametrize("lo,hi", [(1, 101), (0, 1 << 16)])
def test_narrow_key_ranges(gpu_ctx, lo, hi):
    """Pure buckets and narrow spans: no bucket takes the map unless its span allows it."""
    n, B = SHAPES[0]
    keys = np.random.default_rng(3).integers(lo, hi, n).astype(np.int32)
    out, st, (many, took) = run(gpu_ctx, keys, B)
    print(f"keys in [{lo}, {hi}): several sub-buckets {many}, on the map {took}")
    assert np.array_equal(out, np.sort(keys))
    assert took <= many <= B
    if hi - lo < 2 * 85:  # (no span reaches twice a bucket's sub-buckets)
        assert took == 0


@pytest.mark.gpu
@pytest.mark.parametrize("n,B", [SHAPES[0], SHAPES[2]])
def test_extreme_keys(gpu_ctx, n, B):
    keys = uniform(n, 5)
    keys[::1001] = -(2**31)
    keys[7::1003] = 2**31 - 1
    out, st, (many, took) = run(gpu_ctx, keys, B)
    assert np.array_equal(out, np.sort(keys))
    assert out[0] == -(2**31) and out[-1] == 2**31 - 1
    assert took >= 1


@pytest.mark.gpu
def test_switch_off_gives_the_same_sort(gpu_ctx):
    n, B = SHAPES[1]
    keys = uniform(n, 21)
    on, st_on, (many, took) = run(gpu_ctx, keys, B)
    off, st_off, (many0, took0) = run(gpu_ctx, keys, B, mode=0)
    assert np.array_equal(on, off) and np.array_equal(on, np.sort(keys))
    assert st_on["tile_sort_keys"] == st_off["tile_sort_keys"]
    assert took >= 1 and took0 == 0 and many0 == many


@pytest.mark.gpu
def test_automatic_path_2p25(gpu_ctx):
    import torch
    keys = uniform(1 << 25, 99)
    out, st, (many, took) = run(gpu_ctx, keys)
    print(f"2^25 automatic: several sub-buckets {many}, on the map {took}, split {st['sub_split_subbuckets']}")
    want = torch.sort(torch.from_numpy(keys).cuda()).values.cpu().numpy()
    assert np.array_equal(out, want)
    assert many >= 1 and took >= 0.9 * many
    assert st["sub_split_subbuckets"] == 0 and st["sub_scatter_fallback"] == 0


@pytest.mark.gpu
def test_through_the_bucket_exchange(tmp_path):
    """One rank on the host transport under the wave fence: the received buckets' second level takes the map
    in both waves and changes nothing the second wave still needs."""
    from test_gpu_multirank import run_ranks
    n = (1 << 22) + 12_345
    ins, outs, meta = run_ranks(tmp_path, 1, n, opts={"all": {"test_wave_fence": 1}})
    assert meta[0]["stats"]["exchange_path"] == 1 and meta[0]["stats"]["fence_ranges"] >= 1, meta[0]["stats"]
    assert np.array_equal(np.concatenate(outs), np.sort(ins))
