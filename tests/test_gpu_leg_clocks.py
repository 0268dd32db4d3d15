"""The five leg-time readers (dsort_pairs_leg_ms, dsort_argsort64_leg_ms, dsort_sample_argsort64_leg_ms,
dsort_sample_gather_leg_ms, dsort_topk_leg_ms): not part of dsort.h, called through ctypes as
scripts/bench_pairs.py calls them.  What they document is pinned here: DSORT_EINVAL with the reader's
message while the context's last call of the feature recorded nothing (a fresh context, stage timing
off, leg timing off -- never an earlier call's times), the number of legs per path, and the slot
that is exactly zero when DSORT_OPT_ARGSORT_WIDE skipped the min/max reduction.  No time is compared
with another: each is finite and >= 0."""
import ctypes
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
EINVAL = -1
N = 8193  # one int64 tile plus one key
SAMPLE_N = 100_003
DBL, INT = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)
READERS = {  # name -> (argument types after the context, the message of "nothing recorded")
    "dsort_pairs_leg_ms": ([DBL], "no timed pair sort on this context"),
    "dsort_argsort64_leg_ms": ([DBL, INT], "no timed int64 argsort on this context"),
    "dsort_sample_argsort64_leg_ms": ([DBL, INT], "no timed int64 sample argsort on this context"),
    "dsort_sample_gather_leg_ms": ([DBL], "no timed gather on this context"),
    "dsort_topk_leg_ms": ([DBL, INT, DBL], "no timed top-k select on this context"),
}


@pytest.fixture()
def ctx(dsort_mod):
    """A fresh context per test: "before any timed call" is truly before."""
    c = dsort_mod.Context(0)
    for name, (args, _) in READERS.items():
        f = getattr(c.lib, name)
        f.restype, f.argtypes = ctypes.c_int, [ctypes.c_void_p] + args
    c.lib.dsort_topk_leg_timing.restype = ctypes.c_int
    c.lib.dsort_topk_leg_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    yield c
    c.close()


def read(ctx, name):
    """(rc, the values written, the count returned or None) of one reader."""
    ms, cnt, extra = (ctypes.c_double * 16)(), ctypes.c_int(-1), ctypes.c_double(-1.0)
    f = getattr(ctx.lib, name)
    if name == "dsort_topk_leg_ms":
        rc = f(ctx.h, ms, ctypes.byref(cnt), ctypes.byref(extra))
        return rc, list(ms[:max(cnt.value, 0)]) + [extra.value], cnt.value
    if len(READERS[name][0]) == 2:
        rc = f(ctx.h, ms, ctypes.byref(cnt))
        return rc, list(ms[:max(cnt.value, 0)]), cnt.value
    fixed = 3 if name == "dsort_pairs_leg_ms" else 5
    return f(ctx.h, ms), list(ms[:fixed]), None


def nothing_recorded(ctx, name):
    rc, _, _ = read(ctx, name)
    return rc == EINVAL and READERS[name][1] in ctx.lib.dsort_last_error(ctx.h).decode()


def sane(vals):
    return all(math.isfinite(v) and v >= 0 for v in vals)


def i32_keys(n):
    return torch.randint(-1000, 1000, (n,), dtype=torch.int32, device="cuda")


def wide_keys(ctx, n):
    k = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.gen_uniform(k, 0x5EED2026, 0)  # uniform over all 64 bits
    assert int(k.max()) - int(k.min()) > 2 ** 62
    return k


def narrow_keys(n):
    return torch.randint(0, 101, (n,), dtype=torch.int64, device="cuda")


def test_every_reader_reports_einval_on_a_fresh_context(ctx):
    for name in READERS:
        assert nothing_recorded(ctx, name), name


def test_pair_sort(ctx):
    keys, vals = i32_keys(N), torch.arange(N, dtype=torch.int32, device="cuda")
    ctx.sort_pairs_dev(keys.clone(), vals.clone())
    rc, ms, _ = read(ctx, "dsort_pairs_leg_ms")
    assert rc == 0 and len(ms) == 3 and sane(ms), (rc, ms)
    with ctx.options(stage_timing=0):  # records nothing: not the first call's times
        ctx.sort_pairs_dev(keys.clone(), vals.clone())
        assert nothing_recorded(ctx, "dsort_pairs_leg_ms")
    ctx.sort_pairs_dev(keys, vals)
    assert read(ctx, "dsort_pairs_leg_ms")[0] == 0


def test_argsort_i64(ctx):
    name = "dsort_argsort64_leg_ms"
    ctx.argsort_dev(narrow_keys(N))
    rc, ms, legs = read(ctx, name)
    assert rc == 0 and legs == 4 and sane(ms), (rc, legs, ms)
    wide = wide_keys(ctx, N)
    ctx.argsort_dev(wide)
    rc, ms, legs = read(ctx, name)
    assert rc == 0 and legs == 6 and sane(ms), (rc, legs, ms)
    with ctx.options(argsort_wide=1):  # no min/max reduction: its slot is zero
        ctx.argsort_dev(narrow_keys(N))
        rc, ms, legs = read(ctx, name)
        assert rc == 0 and legs == 6 and ms[0] == 0.0 and sane(ms), (rc, legs, ms)
    with ctx.options(stage_timing=0):
        ctx.argsort_dev(wide)
        assert nothing_recorded(ctx, name)


def test_sample_argsort_i64_on_one_rank(ctx, dsort_mod):
    name = "dsort_sample_argsort64_leg_ms"
    ctx.comm_init(1, 0, dsort_mod.Context.unique_id())
    try:
        ctx.sample_argsort_dev(narrow_keys(SAMPLE_N), 0)
        rc, ms, legs = read(ctx, name)
        assert rc == 0 and legs == 4 and sane(ms), (rc, legs, ms)
        wide = wide_keys(ctx, SAMPLE_N)
        ctx.sample_argsort_dev(wide, 0)
        rc, ms, legs = read(ctx, name)
        assert rc == 0 and legs == 10 and sane(ms), (rc, legs, ms)
        with ctx.options(stage_timing=0):
            ctx.sample_argsort_dev(wide, 0)
            assert nothing_recorded(ctx, name)
    finally:
        ctx.comm_destroy()


def test_gather_on_one_rank(ctx, dsort_mod):
    name = "dsort_sample_gather_leg_ms"
    ctx.comm_init(1, 0, dsort_mod.Context.unique_id())
    try:
        rec = torch.arange(SAMPLE_N * 4, dtype=torch.int32, device="cuda").view(SAMPLE_N, 4)  # 16-byte records
        idx = torch.randperm(SAMPLE_N, device="cuda").to(torch.int32)
        out = ctx.sample_gather_dev(rec, 0, idx)
        rc, ms, _ = read(ctx, name)
        assert rc == 0 and len(ms) == 5 and sane(ms), (rc, ms)
        assert torch.equal(out, rec[idx.to(torch.int64)])
        with ctx.options(stage_timing=0):
            ctx.sample_gather_dev(rec, 0, idx)
            assert nothing_recorded(ctx, name)
    finally:
        ctx.comm_destroy()


def test_topk_select(ctx):
    name, n, k = "dsort_topk_leg_ms", 4097, 7
    k32 = i32_keys(n)
    k64 = wide_keys(ctx, n)
    with ctx.options(topk_path=1):
        ctx.topk_dev(k32, k)  # leg timing is off by default
        assert nothing_recorded(ctx, name)
        ctx.check(ctx.lib.dsort_topk_leg_timing(ctx.h, 1))
        ctx.topk_dev(k32, k)
        rc, ms, passes = read(ctx, name)
        assert rc == 0 and passes == 3 and len(ms) == 4 and sane(ms), (rc, passes, ms)
        ctx.topk_dev(k64, k)
        rc, ms, passes = read(ctx, name)
        assert rc == 0 and passes == 6 and len(ms) == 7 and sane(ms), (rc, passes, ms)
        ctx.check(ctx.lib.dsort_topk_leg_timing(ctx.h, 0))
        ctx.topk_dev(k32, k)
        assert nothing_recorded(ctx, name)
