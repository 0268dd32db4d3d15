#!/usr/bin/env python3
"""Stable argsort of int32 keys (dsort_argsort_dev_i32) measured on one MI355X, keys resident in HBM.

For uniform keys at every --log2 size (default 2^28 and 2^30):

  argsort_ms        dsort_argsort_dev_i32 (sorted keys + indices) back to back, HIP events around
                    --steps calls on one stream;
  legs_ms           its pack, int64 sort and unpack legs, from the HIP events the library records
                    between them (dsort_pairs_leg_ms), median over --steps separate calls;
  torch_sort_ms     torch.sort(stable=True) of the same resident keys: the same (key, index) job;
  memcpy            a device-to-device hipMemcpyAsync (torch's same-device copy_ of a contiguous
                    tensor) that moves the byte total of each streaming leg -- pack reads 4n and
                    writes 8n, unpack reads 8n and writes 8n, so copies of 6n and 8n bytes -- and each
                    leg's rate as a fraction of that copy's rate in this same run.

    python scripts/bench_pairs.py [--log2 28 30] [--steps 10] [--warmup 2] [--out profiles/pairs_bench.json]

    python scripts/bench_pairs.py --sample [--log2 28] [--steps 10] [--out profiles/pairs_sample_bench.json]

--sample measures instead the global argsort (dsort_sample_argsort_dev_i32) on one RCCL rank: ms per
call of --steps back-to-back calls, its pack / sample sort / unpack legs from the same HIP events,
and dsort_argsort_dev_i32 with its legs on the same keys in the same process; it reports the ratio
and the excess leg by leg (bench_sample).

    python scripts/bench_pairs.py --gather [--log2 28] [--steps 10] [--out profiles/pairs_gather_bench.json]

--gather measures the distributed record gather (dsort_sample_gather_dev) on one RCCL rank: 2^28
records of 16 bytes, indices a random permutation, --steps back-to-back calls against
dsort_gather_dev on the same data in the same process, results compared bit for bit; its five legs
(route | request exchange | serve | reply exchange | unroute) from the library's HIP events
(dsort_sample_gather_leg_ms), and each streaming leg as a fraction of a device-to-device copy of
the same byte total in the same run (bench_gather).

    python scripts/bench_pairs.py --i64 [--log2 28 30] [--steps 10] [--out profiles/pairs_i64_bench.json]

--i64 measures the stable argsort of int64 keys (dsort_argsort_dev_i64) on three inputs -- narrow
(uniform in [-2^33, 2^33): one pass), wide (uniform over all 64 bits) and config C4's Zipf keys (both
two passes): ms per call of --steps back-to-back calls, its legs from the library's HIP events
(dsort_argsort64_leg_ms), torch.sort(stable=True) of the same keys in the same process (also the
check, bit for bit), the narrow keys again with DSORT_OPT_ARGSORT_WIDE = 1, each streaming leg as a
fraction of a device-to-device copy of the same byte total, and the two random-access legs against
dsort_gather_dev of 8-byte records over a random permutation of the same n (bench_i64).

    python scripts/bench_pairs.py --sample-i64 [--log2 28] [--steps 10] [--out profiles/pairs_sample_i64_bench.json]

--sample-i64 measures the global argsort of int64 keys (dsort_sample_argsort_dev_i64) on one RCCL rank,
on the narrow and the wide keys of --i64, against dsort_argsort_dev_i64 on the same keys in the same
process, results compared bit for bit: ms per call, the legs of both from the library's HIP events
(dsort_sample_argsort64_leg_ms: 4 legs on one pass, 10 on two), and its streaming kernels -- pack,
unpack, the two splits, regroup, final -- as fractions of a device-to-device copy of the same byte
total in the same run (bench_sample_i64).

    python scripts/bench_pairs.py --typed [--log2 28] [--steps 10] [--out profiles/pairs_typed_bench.json]

--typed measures typed keys and descending order (dsort.h, "Key types and order"; bench_typed).  Fused
paths, at every --log2 size (default 2^28): argsort_dev of float32 keys -- the uniform int32 keys of
the default mode, the same bits -- ascending and descending beside the int32 argsort_dev of those bits
in the same process; the same for float64 on the bits of --i64's wide keys and on narrow keys of one
binade (1.0 + j 2^-52, j < 2^34) beside int64 keys of the same range; every result checked against
the integer argsort of the encoded words.  Keys-only path, at 2^28 and 2^30: the encode and the
decode kernel alone for 4- and 8-byte keys (float, descending), each as a ratio to a device-to-device
copy of the same bytes in the same run, and sort_dev of 2^30 float32 keys beside the int32 sort_dev
of the same bits and torch.sort of the same tensor.

    python scripts/bench_pairs.py --topk [--log2 28] [--steps 10] [--out profiles/topk_bench.json]

--topk times top-k selection (dsort_topk_dev_keys, keys and indices) at every --log2 size (default
2^28): uniform float32 bits descending, int32 keys of [1, 100], all-equal int32 keys and uniform
float64 bits, for k in 1, 64, 2^10, 2^16, 2^20 and n / 8, with the select path and the full path
forced in turn in the same process (their results compared), torch.topk of the same tensor for
context, and the path dsort_plan_topk takes; all six key types at k = 1024; and each histogram
pass and the compaction of the select against a device-to-device copy of half the bytes it reads
(the same traffic).

Writes the JSON file and prints one summary line.  No GPU: fails (there is nothing to measure).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "distributed-sorting-with-fault-tolerance_amd"))


def timed(torch, fn, steps, warmup):
    """ms per call of fn, `steps` calls back to back between two events."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def bench_size(torch, ctx, n, steps, warmup):
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.gen_uniform(keys, 0x5EED2026, 0)
    out = torch.empty_like(keys)
    idx = torch.empty_like(keys)

    argsort_ms = timed(torch, lambda: ctx.argsort_dev(keys, idx_out=idx, keys_out=out), steps, warmup)

    leg_fn = ctx.lib.dsort_pairs_leg_ms  # not in dsort.h: the bench's view of the legs' events
    leg_fn.restype = ctypes.c_int
    leg_fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    legs = []
    for _ in range(steps):
        ctx.argsort_dev(keys, idx_out=idx, keys_out=out)
        ms = (ctypes.c_double * 3)()
        ctx.check(leg_fn(ctx.h, ms))
        legs.append(tuple(ms))
    pack_ms, sort_ms, unpack_ms = (statistics.median(x[i] for x in legs) for i in range(3))
    stats = ctx.stats()

    tvals, tidx = torch.sort(keys, stable=True)  # also the check
    exact = bool(torch.equal(out, tvals) and torch.equal(idx.to(torch.int64), tidx))
    del tvals, tidx
    torch_ms = timed(torch, lambda: torch.sort(keys, stable=True), max(3, steps // 2), 1)
    del out, idx
    torch.cuda.empty_cache()

    copies = {}
    for leg, total in (("pack", 12 * n), ("unpack", 16 * n)):
        src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        src.zero_()
        copies[leg] = timed(torch, lambda: dst.copy_(src), steps, warmup)
        del src, dst
        torch.cuda.empty_cache()
    del keys
    torch.cuda.empty_cache()

    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9  # noqa: E731
    r4 = lambda x: round(x, 4)  # noqa: E731
    return {
        "n": n,
        "argsort_ms": r4(argsort_ms),
        "argsort_gkeys_per_s": r4(n / (argsort_ms * 1e-3) / 1e9),
        "legs_ms": {"pack": r4(pack_ms), "sort_i64": r4(sort_ms), "unpack": r4(unpack_ms)},
        "inner_sort_stats": {k: stats[k] for k in ("total_ms", "merge_passes", "tile_keys", "first_level_map")},
        "torch_sort_stable_ms": r4(torch_ms),
        "torch_over_argsort": r4(torch_ms / argsort_ms),
        "exact_vs_torch_sort_stable": exact,
        "streaming": {
            "pack": {"bytes": 12 * n, "gb_per_s": r4(gbs(12 * n, pack_ms)), "memcpy_ms": r4(copies["pack"]),
                     "memcpy_gb_per_s": r4(gbs(12 * n, copies["pack"])), "frac_of_memcpy": r4(copies["pack"] / pack_ms)},
            "unpack": {"bytes": 16 * n, "gb_per_s": r4(gbs(16 * n, unpack_ms)), "memcpy_ms": r4(copies["unpack"]),
                       "memcpy_gb_per_s": r4(gbs(16 * n, copies["unpack"])),
                       "frac_of_memcpy": r4(copies["unpack"] / unpack_ms)},
        },
    }


def bench_sample(torch, dsort, ctx, n, steps, warmup):
    """--sample: dsort_sample_argsort_dev_i32 on ONE RCCL rank against dsort_argsort_dev_i32 on the
    same keys in the same process.  One rank ships nothing: what is measured is the sample sort's
    own route for the packed words (at 2^22 keys and more the bucket exchange: samples, first
    partition level, second level and tile sort wave by wave, with its host waits) against the
    local int64 sort, plus the two streaming legs."""
    ctx.comm_init(1, 0, dsort.Context.unique_id())
    keys = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.gen_uniform(keys, 0x5EED2026, 0)
    out = torch.empty_like(keys)
    idx = torch.empty_like(keys)
    leg_fn = ctx.lib.dsort_pairs_leg_ms  # not in dsort.h: the bench's view of the legs' events
    leg_fn.restype = ctypes.c_int
    leg_fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]

    def legs_of(fn):
        legs = []
        for _ in range(steps):
            fn()
            ms = (ctypes.c_double * 3)()
            ctx.check(leg_fn(ctx.h, ms))
            legs.append(tuple(ms))
        return [round(statistics.median(x[i] for x in legs), 4) for i in range(3)]

    kp, ip, nout = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()

    def sample():  # the C entry itself: the binding's copies into fresh tensors are not part of it
        ctx.check(ctx.lib.dsort_sample_argsort_dev_i32(ctx.h, keys.data_ptr(), n, 0, ctypes.byref(kp),
                                                       ctypes.byref(ip), ctypes.byref(nout), ctx._stream()))

    def local():
        ctx.argsort_dev(keys, idx_out=idx, keys_out=out)

    local_ms = timed(torch, local, steps, warmup)
    local_legs = legs_of(local)
    local_stats = ctx.stats()
    sample_ms = timed(torch, sample, steps, warmup)
    sample_legs = legs_of(sample)
    st = ctx.stats()
    sk, si = ctx.sample_argsort_dev(keys, 0)  # (the check, through the binding)
    local()
    torch.cuda.synchronize()
    exact = bool(sk.numel() == n and torch.equal(sk, out) and torch.equal(si, idx))
    ctx.comm_destroy()
    r4 = lambda x: round(x, 4)  # noqa: E731
    names = ("pack", "sort", "unpack")
    return {
        "n": n,
        "sample_argsort_ms": r4(sample_ms),
        "local_argsort_ms": r4(local_ms),
        "sample_over_local": r4(sample_ms / local_ms),
        "sample_legs_ms": dict(zip(names, sample_legs)),
        "local_legs_ms": dict(zip(names, local_legs)),
        "excess_ms_by_leg": {k: r4(a - b) for k, a, b in zip(names, sample_legs, local_legs)},
        "sample_sort_stats": {k: st[k] for k in ("exchange_path", "total_ms", "partition_ms", "bucket_hist_ms",
                                                 "bucket_scatter_ms", "sub_partition_ms", "tile_sort_kernel_ms",
                                                 "exchange_ms", "alltoall_ms", "keys_sent", "keys_out")},
        "local_sort_stats": {k: local_stats[k] for k in ("total_ms", "partition_ms", "bucket_hist_ms",
                                                         "bucket_scatter_ms", "sub_partition_ms",
                                                         "tile_sort_kernel_ms")},
        "exact_vs_local_argsort": exact,
    }


def bench_gather(torch, dsort, ctx, n, steps, warmup, W=16):
    """--gather: dsort_sample_gather_dev on ONE RCCL rank against dsort_gather_dev on the same
    records and indices.  One rank ships nothing, and there is no shortcut to the local gather:
    every kernel runs, the two exchanges are the device-to-device copies of the rank's own part, so
    the legs are what a rank pays around the links."""
    ctx.comm_init(1, 0, dsort.Context.unique_id())
    D = W // 4
    rec = torch.empty(n * D, dtype=torch.int32, device="cuda")
    ctx.gen_uniform(rec, 0xC0FFEE, 0)
    rec = rec.view(n, D)
    idx = torch.randperm(n, device="cuda").to(torch.int32)
    torch.cuda.empty_cache()
    out = torch.empty_like(rec)
    ref = torch.empty_like(rec)
    leg_fn = ctx.lib.dsort_sample_gather_leg_ms  # not in dsort.h: the bench's view of the legs' events
    leg_fn.restype = ctypes.c_int
    leg_fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double)]
    names = ("route", "request_exchange", "serve", "reply_exchange", "unroute")

    def dist():
        ctx.sample_gather_dev(rec, 0, idx, out=out)

    def local():
        ctx.gather_dev(rec, idx, ref)

    local_ms = timed(torch, local, steps, warmup)
    dist_ms = timed(torch, dist, steps, warmup)
    legs = []
    for _ in range(steps):
        dist()
        ms = (ctypes.c_double * 5)()
        ctx.check(leg_fn(ctx.h, ms))
        legs.append(tuple(ms))
    leg_ms = [statistics.median(x[i] for x in legs) for i in range(5)]
    st = ctx.stats()
    torch.cuda.synchronize()
    exact = bool(torch.equal(out, ref))
    ctx.comm_destroy()
    del out, ref
    torch.cuda.empty_cache()
    # HBM bytes of the streaming legs: route = count (4n) + place (4n + 4n); the exchanges are the
    # copies of the own part (read + write); unroute reads idx and the replies and writes the records
    leg_bytes = {"route": 12 * n, "request_exchange": 8 * n, "reply_exchange": 2 * W * n, "unroute": (4 + 2 * W) * n}
    r4 = lambda x: round(x, 4)  # noqa: E731
    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9  # noqa: E731
    streaming = {}
    for leg, total in leg_bytes.items():
        src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        src.zero_()
        copy_ms = timed(torch, lambda: dst.copy_(src), steps, warmup)
        del src, dst
        torch.cuda.empty_cache()
        ms = leg_ms[names.index(leg)]
        streaming[leg] = {"bytes": total, "gb_per_s": r4(gbs(total, ms)), "memcpy_ms": r4(copy_ms),
                          "memcpy_gb_per_s": r4(gbs(total, copy_ms)), "frac_of_memcpy": r4(copy_ms / ms)}
    top = max(range(5), key=lambda i: leg_ms[i])
    return {
        "n": n, "elem_bytes": W,
        "sample_gather_ms": r4(dist_ms),
        "local_gather_ms": r4(local_ms),
        "sample_over_local": r4(dist_ms / local_ms),
        "legs_ms": {k: r4(v) for k, v in zip(names, leg_ms)},
        "legs_sum_ms": r4(sum(leg_ms)),
        "dominant_leg": names[top],
        "serve_over_local_gather": r4(leg_ms[2] / local_ms),
        "bytes_per_record": {"sample_gather": 28 + 6 * W, "local_gather": 4 + 2 * W},
        "streaming": streaming,
        "gather_sent": st["gather_sent"], "gather_served": st["gather_served"],
        "exact_vs_local_gather": exact,
    }


# HBM bytes per element of the int64 argsort's legs with the sorted keys wanted (dsort_pairs64.hip);
# "random" = of those, the bytes read at a random address
I64_LEG_BYTES = {"minmax": 8, "pack": 16, "unpack": 20, "regroup": 24, "final": 28, "gather8": 20}
I64_LEG_NAMES = {4: ("minmax", "pack", "sort", "unpack"), 6: ("minmax", "pack", "sort_lo", "regroup", "sort_hi", "final")}


def bench_i64(torch, ctx, n, steps, warmup):
    """--i64: dsort_argsort_dev_i64 on narrow, wide and Zipf keys against torch.sort(stable=True), the
    narrow keys on both paths, and the legs against their yardsticks, all in this process."""
    leg_fn = ctx.lib.dsort_argsort64_leg_ms  # not in dsort.h: the bench's view of the legs' events
    leg_fn.restype = ctypes.c_int
    leg_fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    r4 = lambda x: round(x, 4)  # noqa: E731
    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9  # noqa: E731
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    out = torch.empty_like(keys)
    idx = torch.empty(n, dtype=torch.int32, device="cuda")

    def call():
        ctx.argsort_dev(keys, idx_out=idx, keys_out=out)

    def measure():
        ms = timed(torch, call, steps, warmup)
        legs = []
        for _ in range(steps):
            call()
            buf, cnt = (ctypes.c_double * 6)(), ctypes.c_int()
            ctx.check(leg_fn(ctx.h, buf, ctypes.byref(cnt)))
            legs.append(tuple(buf[:cnt.value]))
        names = I64_LEG_NAMES[len(legs[0])]
        st = ctx.stats()
        return {"argsort_ms": r4(ms), "argsort_gkeys_per_s": r4(n / (ms * 1e-3) / 1e9),
                "argsort_passes": st["argsort_passes"],
                "legs_ms": {k: r4(statistics.median(x[i] for x in legs)) for i, k in enumerate(names)},
                "last_inner_sort_stats": {k: st[k] for k in ("total_ms", "merge_passes", "tile_keys",
                                                             "first_level_map")}}

    # the yardsticks of this size: device-to-device copies of each streaming leg's byte total, and the
    # local gather of 8-byte records over a random permutation
    copies = {}
    for leg in ("minmax", "pack", "unpack"):
        total = I64_LEG_BYTES[leg] * n
        src = torch.empty(total // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        src.zero_()
        copies[leg] = timed(torch, lambda: dst.copy_(src), steps, warmup)
        del src, dst
        torch.cuda.empty_cache()
    perm = torch.randperm(n, device="cuda").to(torch.int32)
    torch.cuda.empty_cache()
    ctx.gen_uniform(keys, 0xC0FFEE, 0)
    gather_ms = timed(torch, lambda: ctx.gather_dev(keys, perm, out), steps, warmup)
    del perm
    torch.cuda.empty_cache()

    inputs = {}
    for name in ("narrow", "wide", "zipf_c4"):
        if name == "narrow":
            ctx.gen_uniform(keys, 0x5EED2026, 0)
            keys >>= 30  # arithmetic: uniform in [-2^33, 2^33)
        elif name == "wide":
            ctx.gen_uniform(keys, 0x5EED2026, 0)
        else:
            ctx.gen_zipf_i64(keys, 0x5EED2026, 0)
        res = measure()
        tvals, tidx = torch.sort(keys, stable=True)  # also the check
        res["exact_vs_torch_sort_stable"] = bool(torch.equal(out, tvals) and torch.equal(idx.to(torch.int64), tidx))
        del tvals, tidx
        torch.cuda.empty_cache()
        torch_ms = timed(torch, lambda: torch.sort(keys, stable=True), max(3, steps // 2), 1)
        torch.cuda.empty_cache()
        res["torch_sort_stable_ms"] = r4(torch_ms)
        res["torch_over_argsort"] = r4(torch_ms / res["argsort_ms"])
        if name == "narrow":  # the same keys through the two passes
            ko1, io1 = out.clone(), idx.clone()
            with ctx.options(argsort_wide=1):
                forced = measure()
            forced["exact_vs_automatic"] = bool(torch.equal(out, ko1) and torch.equal(idx, io1))
            forced["wide_over_narrow"] = r4(forced["argsort_ms"] / res["argsort_ms"])
            res["forced_wide"] = forced
            del ko1, io1
            torch.cuda.empty_cache()
        legs = dict(res["legs_ms"])
        if "forced_wide" in res:
            legs.update({"wide_pack": res["forced_wide"]["legs_ms"]["pack"]})
        res["streaming"] = {}
        for leg, ms in legs.items():
            ref = {"wide_pack": "pack"}.get(leg, leg)
            if ref in copies and ms > 0:
                total = I64_LEG_BYTES[ref] * n
                res["streaming"][leg] = {"bytes": total, "gb_per_s": r4(gbs(total, ms)), "memcpy_ms": r4(copies[ref]),
                                         "memcpy_gb_per_s": r4(gbs(total, copies[ref])),
                                         "frac_of_memcpy": r4(copies[ref] / ms)}
        ra = res.get("forced_wide", res)["legs_ms"]
        if "regroup" in ra:
            res["random_access"] = {
                leg: {"bytes": I64_LEG_BYTES[leg] * n, "ms": ra[leg], "over_gather8": r4(ra[leg] / gather_ms),
                      "bytes_over_gather8": r4(I64_LEG_BYTES[leg] / I64_LEG_BYTES["gather8"])}
                for leg in ("regroup", "final")}
        inputs[name] = res
    return {"n": n, "gather8_random_perm_ms": r4(gather_ms), "gather8_bytes": I64_LEG_BYTES["gather8"] * n,
            "leg_bytes_per_element": I64_LEG_BYTES, "inputs": inputs}


# HBM bytes per element of the streaming kernels of the int64 argsort across ranks (keys wanted)
S64_LEG_BYTES = {"pack": 16, "unpack": 20, "split_save": 20, "regroup": 16, "split": 12, "final": 28}
S64_LEG_NAMES = {4: ("decision", "pack", "sample_sort", "unpack"),
                 10: ("decision", "pack", "sample_sort_lo", "split_save", "key_gather", "regroup", "sample_sort_hi",
                      "split", "final_gather", "final")}


def bench_sample_i64(torch, dsort, ctx, n, steps, warmup):
    """--sample-i64: dsort_sample_argsort_dev_i64 on ONE RCCL rank, narrow and wide keys, against
    dsort_argsort_dev_i64 on the same keys in the same process, results compared bit for bit.  One
    rank ships nothing, and there is no shortcut: every leg runs, so the wide path pays two
    distributed gathers where the local call pays two random-read kernels."""
    ctx.comm_init(1, 0, dsort.Context.unique_id())
    leg_fn = ctx.lib.dsort_sample_argsort64_leg_ms  # not in dsort.h: the bench's view of the legs' events
    leg_fn.restype = ctypes.c_int
    leg_fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    loc_fn = ctx.lib.dsort_argsort64_leg_ms
    loc_fn.restype = ctypes.c_int
    loc_fn.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int)]
    r4 = lambda x: round(x, 4)  # noqa: E731
    gbs = lambda b, ms: b / (ms * 1e-3) / 1e9  # noqa: E731
    keys = torch.empty(n, dtype=torch.int64, device="cuda")
    out = torch.empty_like(keys)
    idx = torch.empty(n, dtype=torch.int32, device="cuda")
    kp, ip, nout = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_size_t()

    def sample():  # the C entry itself: the binding's copies into fresh tensors are not part of it
        ctx.check(ctx.lib.dsort_sample_argsort_dev_i64(ctx.h, keys.data_ptr(), n, 0, ctypes.byref(kp),
                                                       ctypes.byref(ip), ctypes.byref(nout), ctx._stream()))

    def local():
        ctx.argsort_dev(keys, idx_out=idx, keys_out=out)

    def legs_of(fn, hook, room, names):
        legs = []
        for _ in range(steps):
            fn()
            buf, cnt = (ctypes.c_double * room)(), ctypes.c_int()
            ctx.check(hook(ctx.h, buf, ctypes.byref(cnt)))
            legs.append(tuple(buf[:cnt.value]))
        return {k: r4(statistics.median(x[i] for x in legs)) for i, k in enumerate(names[len(legs[0])])}

    copies = {}
    for total in sorted(set(S64_LEG_BYTES.values())):
        src = torch.empty(total * n // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        src.zero_()
        copies[total] = timed(torch, lambda: dst.copy_(src), steps, warmup)
        del src, dst
        torch.cuda.empty_cache()

    inputs = {}
    for name in ("narrow", "wide"):
        ctx.gen_uniform(keys, 0x5EED2026, 0)
        if name == "narrow":
            keys >>= 30  # arithmetic: uniform in [-2^33, 2^33)
        local_ms = timed(torch, local, steps, warmup)
        local_legs = legs_of(local, loc_fn, 6, I64_LEG_NAMES)
        sample_ms = timed(torch, sample, steps, warmup)
        sample_legs = legs_of(sample, leg_fn, 10, S64_LEG_NAMES)
        st = ctx.stats()
        sk, si = ctx.sample_argsort_dev(keys, 0)  # (the check, through the binding)
        local()
        torch.cuda.synchronize()
        exact = bool(sk.numel() == n and torch.equal(sk, out) and torch.equal(si, idx))
        del sk, si
        torch.cuda.empty_cache()
        streaming = {}
        for leg, ms in sample_legs.items():
            if leg in S64_LEG_BYTES and ms > 0:
                total = S64_LEG_BYTES[leg]
                streaming[leg] = {"bytes": total * n, "gb_per_s": r4(gbs(total * n, ms)), "memcpy_ms": r4(copies[total]),
                                  "memcpy_gb_per_s": r4(gbs(total * n, copies[total])),
                                  "frac_of_memcpy": r4(copies[total] / ms)}
        inputs[name] = {"sample_argsort_ms": r4(sample_ms), "local_argsort_ms": r4(local_ms),
                        "sample_over_local": r4(sample_ms / local_ms), "argsort_passes": st["argsort_passes"],
                        "sample_legs_ms": sample_legs, "sample_legs_sum_ms": r4(sum(sample_legs.values())),
                        "local_legs_ms": local_legs, "streaming": streaming,
                        "last_sample_sort_stats": {k: st[k] for k in ("exchange_path", "total_ms", "keys_out")},
                        "exact_vs_local_argsort": exact}
    ctx.comm_destroy()
    return {"n": n, "leg_bytes_per_element": S64_LEG_BYTES, "inputs": inputs}


def bench_typed(torch, dsort, ctx, n, steps, warmup):
    """--typed, the fused paths at n keys: the typed argsort beside the integer argsort of the same
    bits (float32, float64 wide) or of the same range (float64 narrow) in one process."""
    r4 = lambda x: round(x, 4)  # noqa: E731
    res = {"n": n}

    def run(keys, **kw):
        out = torch.empty_like(keys)
        idx = torch.empty(n, dtype=torch.int32, device="cuda")
        ms = timed(torch, lambda: ctx.argsort_dev(keys, idx_out=idx, keys_out=out, **kw), steps, warmup)
        return ms, out, idx, ctx.stats()["argsort_passes"]

    def check(keys, out, idx, name, desc):
        """The typed result against the integer argsort of the encoded words, computed on the device."""
        W = keys.element_size() * 8
        it = torch.int32 if W == 32 else torch.int64
        b = keys.view(it)
        w = b ^ ((b >> (W - 1)) & ((1 << (W - 1)) - 1)) if name[0] == "f" else b
        w = ~w if desc else w
        _, ridx = ctx.argsort_dev(w.contiguous(), keys_out=None)
        ok = bool(torch.equal(idx, ridx))
        ok = ok and bool(torch.equal(out.view(it), b[ridx.to(torch.int64)]))
        del w, ridx
        torch.cuda.empty_cache()
        return ok

    def family(label, ikeys, fkeys, name):
        fam = {}
        ms, out, idx, passes = run(ikeys)
        fam["int_asc"] = {"argsort_ms": r4(ms), "argsort_passes": passes}
        del out, idx
        for desc in (False, True):
            ms, out, idx, passes = run(fkeys, descending=desc)
            fam[name + ("_desc" if desc else "_asc")] = {
                "argsort_ms": r4(ms), "argsort_passes": passes, "over_int_asc": r4(ms / fam["int_asc"]["argsort_ms"]),
                "exact_vs_int_argsort_of_encoded_words": check(fkeys, out, idx, name, desc)}
            del out, idx
            torch.cuda.empty_cache()
        ms2, out, idx, _ = run(ikeys)  # the integer call again, after the typed ones
        fam["int_asc_again"] = {"argsort_ms": r4(ms2)}
        del out, idx
        torch.cuda.empty_cache()
        res[label] = fam

    k32 = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.gen_uniform(k32, 0x5EED2026, 0)
    family("f32_uniform_bits", k32, k32.view(torch.float32), "f32")
    del k32
    torch.cuda.empty_cache()
    k64 = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.gen_uniform(k64, 0x5EED2026, 0)
    family("f64_wide_uniform_bits", k64, k64.view(torch.float64), "f64")
    k64 >>= 30  # --i64's narrow keys, uniform in [-2^33, 2^33)
    one = torch.tensor([1.0], dtype=torch.float64).view(torch.int64).item()
    f64 = (k64 + ((1 << 33) + one)).view(torch.float64)  # 1.0 + j 2^-52, j < 2^34: one binade
    family("f64_narrow_one_binade", k64, f64, "f64")
    return res


def bench_keys_only(torch, dsort, ctx, lg, steps, warmup):
    """--typed, the keys-only path at 2^lg keys: the encode and decode kernels alone against a
    device-to-device copy of the same bytes; at 2^30 also the whole float32 sort_dev."""
    n = 1 << lg
    r4 = lambda x: round(x, 4)  # noqa: E731
    hook = ctx.lib.dsort_keys_code_dev  # not in dsort.h: the bench's view of the two kernels
    hook.restype = ctypes.c_int
    hook.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_int,
                     ctypes.c_int, ctypes.c_void_p]
    res = {"n": n}
    for W, kt in ((4, dsort.KEY_TYPES["f32"]), (8, dsort.KEY_TYPES["f64"])):
        src = torch.empty(n * W, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(src)
        src.zero_()
        copy_ms = timed(torch, lambda: dst.copy_(src), steps, warmup)
        entry = {"bytes_read_plus_written": 2 * W * n, "memcpy_ms": r4(copy_ms),
                 "memcpy_gb_per_s": r4(2 * W * n / (copy_ms * 1e-3) / 1e9)}
        for what, dec in (("encode", 0), ("decode", 1)):
            oop = timed(torch, lambda: ctx.check(hook(ctx.h, src.data_ptr(), dst.data_ptr(), n, kt, 1, dec,
                                                       ctx._stream())), steps, warmup)
            inp = timed(torch, lambda: ctx.check(hook(ctx.h, dst.data_ptr(), dst.data_ptr(), n, kt, 1, dec,
                                                       ctx._stream())), steps, warmup)
            entry[what] = {"out_of_place_ms": r4(oop), "in_place_ms": r4(inp),
                           "out_of_place_over_memcpy": r4(oop / copy_ms), "in_place_over_memcpy": r4(inp / copy_ms)}
        res[f"{W}_byte_keys"] = entry
        del src, dst
        torch.cuda.empty_cache()
    if lg == 30:
        bits = torch.empty(n, dtype=torch.int32, device="cuda")
        ctx.gen_uniform(bits, 0x5EED2026, 0)
        work = torch.empty_like(bits)
        whole = {}
        whole["int32_sort_dev_ms"] = r4(timed(torch, lambda: ctx.sort_dev(bits, out=work), steps, warmup))
        fk, fw = bits.view(torch.float32), work.view(torch.float32)
        for desc in (False, True):
            ms = timed(torch, lambda: ctx.sort_dev(fk, out=fw, descending=desc), steps, warmup)
            whole["float32_sort_dev_desc_ms" if desc else "float32_sort_dev_asc_ms"] = r4(ms)
        # the check: the words of the sorted floats ascend (descending: descend) and are a permutation
        ctx.sort_dev(fk, out=fw, descending=False)
        w = work ^ ((work >> 31) & 0x7FFFFFFF)
        whole["sorted_in_total_order"] = bool((w[1:] >= w[:-1]).all()) and ctx.fingerprint(work) == ctx.fingerprint(bits)
        del w, work, fw
        torch.cuda.empty_cache()
        # torch.sort of the same tensor; the NaNs among uniform bits go last there, so NaN-free keys too
        whole["torch_sort_same_bits_ms"] = r4(timed(torch, lambda: torch.sort(fk), max(3, steps // 2), 1))
        torch.cuda.empty_cache()
        whole["float32_over_int32"] = r4(whole["float32_sort_dev_asc_ms"] / whole["int32_sort_dev_ms"])
        whole["torch_over_float32_sort_dev"] = r4(whole["torch_sort_same_bits_ms"] / whole["float32_sort_dev_asc_ms"])
        res["sort_dev_float32"] = whole
        del bits, fk
        torch.cuda.empty_cache()
    return res


def bench_topk(torch, dsort, ctx, n, steps, warmup):
    """--topk at n keys: both forced paths per shape and k, torch.topk for context, the select's legs
    against a copy of the same traffic."""
    r4 = lambda x: round(x, 4)  # noqa: E731
    lib = ctx.lib
    lib.dsort_topk_leg_timing.restype = ctypes.c_int
    lib.dsort_topk_leg_timing.argtypes = [ctypes.c_void_p, ctypes.c_int]
    lib.dsort_topk_leg_ms.restype = ctypes.c_int
    lib.dsort_topk_leg_ms.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_double)]
    res = {"n": n, "shapes": {}, "six_types_k1024": {}, "crossover": {}}

    def one(keys, k, desc, key_type=None, with_torch=True):
        W = keys.element_size()
        ko = [torch.empty(k, dtype=keys.dtype, device="cuda") for _ in range(2)]
        io = [torch.empty(k, dtype=torch.int32, device="cuda") for _ in range(2)]
        e = {"k": k, "auto_path": dsort.plan_topk(keys.numel(), k, W)[0]}
        for j, (label, path) in enumerate((("select", 1), ("full", 0))):
            with ctx.options(topk_path=path):
                runs = [timed(torch, lambda: ctx.topk_dev(keys, k, descending=desc, key_type=key_type, keys_out=ko[j],
                                                          idx_out=io[j]), steps, warmup) for _ in range(3)]
            e[label + "_ms"] = r4(statistics.median(runs))
            e[label + "_runs_ms"] = [r4(v) for v in runs]
        e["select_over_full"] = r4(e["select_ms"] / e["full_ms"])
        e["paths_agree"] = bool(torch.equal(io[0], io[1])) and bool(torch.equal(ko[0].view(torch.uint8), ko[1].view(torch.uint8)))
        if with_torch:
            try:
                e["torch_topk_ms"] = r4(timed(torch, lambda: torch.topk(keys, k, largest=desc, sorted=True),
                                              max(2, steps // 2), 1))
            except Exception as ex:  # (a dtype or size torch.topk does not take)
                e["torch_topk_ms"] = None
                e["torch_topk_error"] = str(ex)[:120]
            torch.cuda.empty_cache()
        return e

    def legs(keys, k, desc, key_type=None):
        """One select with the leg events on: each histogram pass and the compaction against a
        device-to-device copy of half the bytes it reads."""
        W = keys.element_size()
        half = torch.empty(n * W // 2, dtype=torch.uint8, device="cuda")
        dst = torch.empty_like(half)
        copy_ms = timed(torch, lambda: dst.copy_(half), steps, warmup)
        del half, dst
        torch.cuda.empty_cache()
        ctx.check(lib.dsort_topk_leg_timing(ctx.h, 1))
        hist, comp = [], []
        with ctx.options(topk_path=1):
            for _ in range(warmup + steps):
                ctx.topk_dev(keys, k, descending=desc, key_type=key_type)
                h = (ctypes.c_double * 6)()
                p, c = ctypes.c_int(), ctypes.c_double()
                ctx.check(lib.dsort_topk_leg_ms(ctx.h, h, ctypes.byref(p), ctypes.byref(c)))
                hist.append([h[i] for i in range(p.value)])
                comp.append(c.value)
        ctx.check(lib.dsort_topk_leg_timing(ctx.h, 0))
        hist, comp = hist[warmup:], comp[warmup:]
        hm = [statistics.median(col) for col in zip(*hist)]
        cm = statistics.median(comp)
        return {"k": k, "bytes_read_per_leg": n * W, "memcpy_of_half_ms": r4(copy_ms), "hist_ms": [r4(v) for v in hm],
                "hist_over_memcpy": [r4(v / copy_ms) for v in hm], "compact_ms": r4(cm),
                "compact_over_memcpy": r4(cm / copy_ms)}

    ks = [1, 64, 1 << 10, 1 << 16, 1 << 20, n // 8]
    bits32 = torch.empty(n, dtype=torch.int32, device="cuda")
    ctx.gen_uniform(bits32, 0x5EED2026, 0)
    shapes = [("f32_uniform_bits_desc", lambda: bits32.view(torch.float32), True),
              ("i32_1_to_100_asc", lambda: torch.randint(1, 101, (n,), dtype=torch.int32, device="cuda"), False),
              ("i32_all_equal_asc", lambda: torch.full((n,), 42, dtype=torch.int32, device="cuda"), False)]
    for label, make, desc in shapes:
        keys = make()
        res["shapes"][label] = {"by_k": [one(keys, k, desc) for k in ks], "legs": legs(keys, 1 << 10, desc)}
        del keys
        torch.cuda.empty_cache()
    for name in ("i32", "u32", "f32"):
        keys = bits32.view(torch.float32) if name == "f32" else bits32
        res["six_types_k1024"][name] = one(keys, 1 << 10, True, key_type=name, with_torch=False)
    del bits32
    torch.cuda.empty_cache()
    bits64 = torch.empty(n, dtype=torch.int64, device="cuda")
    ctx.gen_uniform(bits64, 0x5EED2026, 0)
    f64 = bits64.view(torch.float64)
    res["shapes"]["f64_uniform_bits_asc"] = {"by_k": [one(f64, k, False) for k in ks], "legs": legs(f64, 1 << 10, False)}
    for name in ("i64", "u64", "f64"):
        keys = f64 if name == "f64" else bits64
        res["six_types_k1024"][name] = one(keys, 1 << 10, True, key_type=name, with_torch=False)
    # where the two paths cross (dsort_plan_topk's constants): large k at n keys, and small inputs
    f32 = bits64.view(torch.float32)[:n]
    fracs = [(1, 4), (3, 8), (1, 2), (5, 8), (3, 4), (1, 1)]
    small = [1 << lg for lg in (10, 12, 14, 16, 18, 20, 22, 24, 26) if (1 << lg) < n]
    for label, keys, desc in (("f32_uniform_bits_desc", f32, True), ("f64_uniform_bits_asc", f64, False)):
        res["crossover"][label] = {
            "large_k": [{"k_over_n": f"{a}/{b}", **one(keys, n // b * a, desc, with_torch=False)} for a, b in fracs],
            "small_n": [{"n": m, "k_1": one(keys[:m], 1, desc, with_torch=False),
                         "k_n_over_64": one(keys[:m], m // 64, desc, with_torch=False),
                         "k_n_over_8": one(keys[:m], m // 8, desc, with_torch=False),
                         "k_n_over_2": one(keys[:m], m // 2, desc, with_torch=False)} for m in small]}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, nargs="+", default=None)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sample", action="store_true",
                    help="time dsort_sample_argsort_dev_i32 on one RCCL rank against the local argsort "
                         "(default 2^28 keys, profiles/pairs_sample_bench.json)")
    ap.add_argument("--gather", action="store_true",
                    help="time dsort_sample_gather_dev on one RCCL rank against dsort_gather_dev "
                         "(default 2^28 records of 16 bytes, profiles/pairs_gather_bench.json)")
    ap.add_argument("--i64", action="store_true",
                    help="time dsort_argsort_dev_i64 on narrow, wide and Zipf keys against torch.sort(stable=True) "
                         "(default 2^28 and 2^30 keys, profiles/pairs_i64_bench.json)")
    ap.add_argument("--sample-i64", action="store_true",
                    help="time dsort_sample_argsort_dev_i64 on one RCCL rank, narrow and wide keys, against "
                         "dsort_argsort_dev_i64 (default 2^28 keys, profiles/pairs_sample_i64_bench.json)")
    ap.add_argument("--typed", action="store_true",
                    help="time typed keys: argsort_dev of float32 / float64 keys, ascending and descending, beside the "
                         "integer argsort of the same bits (default 2^28 keys), and the keys-only path's encode and "
                         "decode kernels and float32 sort_dev at 2^28 and 2^30 (profiles/pairs_typed_bench.json)")
    ap.add_argument("--topk", action="store_true",
                    help="time top-k selection: the select path and the full argsort path forced in turn, torch.topk "
                         "for context, the select's passes against a copy of the same traffic (default 2^28 keys, "
                         "profiles/topk_bench.json)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    args.log2 = args.log2 or ([28] if args.sample or args.gather or args.sample_i64 or args.typed or args.topk
                              else [28, 30])
    name = "pairs_gather_bench.json" if args.gather else "pairs_sample_bench.json" if args.sample else "pairs_bench.json"
    name = "pairs_i64_bench.json" if args.i64 else name
    name = "pairs_sample_i64_bench.json" if args.sample_i64 else name
    name = "pairs_typed_bench.json" if args.typed else name
    name = "topk_bench.json" if args.topk else name
    args.out = args.out or os.path.join(REPO, "profiles", name)

    import torch

    import dsort

    if not torch.cuda.is_available():
        sys.exit("bench_pairs: no GPU visible (nothing is measured without one)")
    ctx = dsort.Context(0)
    if args.topk:
        res = {"what": "top-k selection (dsort.h, top-k), keys resident in HBM: dsort_topk_dev_keys (k keys and "
                       "indices) with the select path and the full argsort path forced in turn in one process, ms per "
                       "call of --steps back-to-back calls (median of 3 such runs, all listed), torch.topk(sorted=True) "
                       "of the same tensor for context; legs: each histogram pass and the compaction of the select "
                       "(HIP events around the kernel, median) against a device-to-device copy of half the bytes it "
                       "reads",
               "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
               "sizes": [bench_topk(torch, dsort, ctx, 1 << lg, args.steps, args.warmup) for lg in args.log2]}
        ctx.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"topk_bench": [
            {"n": s["n"],
             **{lb: {"k": [e["k"] for e in v["by_k"]], "select_ms": [e["select_ms"] for e in v["by_k"]],
                     "full_ms": [e["full_ms"] for e in v["by_k"]],
                     "torch_topk_ms": [e.get("torch_topk_ms") for e in v["by_k"]],
                     "agree": all(e["paths_agree"] for e in v["by_k"]),
                     "hist_over_memcpy": v["legs"]["hist_over_memcpy"],
                     "compact_over_memcpy": v["legs"]["compact_over_memcpy"]} for lb, v in s["shapes"].items()},
             "six_types_k1024": {t: [e["select_ms"], e["full_ms"], e["paths_agree"]]
                                 for t, e in s["six_types_k1024"].items()},
             "crossover": {lb: {"large_k": [[e["k_over_n"], e["select_ms"], e["full_ms"]] for e in v["large_k"]],
                                "small_n": [[e["n"]] + [e[c][p] for c in ("k_1", "k_n_over_64", "k_n_over_8",
                                                                          "k_n_over_2")
                                                        for p in ("select_ms", "full_ms")]
                                            for e in v["small_n"]]} for lb, v in s["crossover"].items()}}
            for s in res["sizes"]]}), flush=True)
        return
    if args.typed:
        res = {"what": "typed keys (dsort.h, Key types and order), resident in HBM.  fused: argsort_dev (sorted keys and "
                       "indices) of float keys, ascending and descending, beside the integer argsort_dev of the same "
                       "bits (f64 narrow: of the same range) in the same process, ms per call of --steps back-to-back "
                       "calls.  keys_only: the encode / decode kernel alone against a device-to-device copy of the "
                       "same bytes, and sort_dev of 2^30 float32 keys beside the int32 sort_dev of the same bits and "
                       "torch.sort of the same tensor",
               "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
               "fused": [bench_typed(torch, dsort, ctx, 1 << lg, args.steps, args.warmup) for lg in args.log2],
               "keys_only": [bench_keys_only(torch, dsort, ctx, lg, args.steps, args.warmup) for lg in (28, 30)]}
        ctx.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"pairs_typed_bench": {
            "fused": [{"n": s["n"], **{fam: {k: v["argsort_ms"] for k, v in s[fam].items()} for fam in s if fam != "n"},
                       "exact": all(v.get("exact_vs_int_argsort_of_encoded_words", True)
                                    for fam in s if fam != "n" for v in s[fam].values())} for s in res["fused"]],
            "keys_only": [{"n": s["n"],
                           **{k: {w: s[k][w]["out_of_place_over_memcpy"] for w in ("encode", "decode")}
                              for k in ("4_byte_keys", "8_byte_keys")},
                           **({"sort_dev_float32": s["sort_dev_float32"]} if "sort_dev_float32" in s else {})}
                          for s in res["keys_only"]]}}), flush=True)
        return
    if args.sample_i64:
        res = {"what": "global stable argsort of int64 keys on one RCCL rank (dsort_sample_argsort_dev_i64): narrow = "
                       "uniform in [-2^33, 2^33), one pass; wide = uniform over 64 bits, two passes with two distributed "
                       "gathers; against dsort_argsort_dev_i64 of the same resident keys, same process; ms per call of "
                       "--steps back-to-back calls, legs from the HIP events between them (median; they include the "
                       "host waits between them), streaming kernels against a device-to-device copy of the same bytes",
               "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
               "sizes": [bench_sample_i64(torch, dsort, ctx, 1 << lg, args.steps, args.warmup) for lg in args.log2]}
        ctx.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"pairs_sample_i64_bench": [
            {"n": s["n"], **{k: {"sample_argsort_ms": v["sample_argsort_ms"], "local_argsort_ms": v["local_argsort_ms"],
                                 "sample_over_local": v["sample_over_local"], "passes": v["argsort_passes"],
                                 "legs_ms": v["sample_legs_ms"],
                                 "frac_of_memcpy": {g: w["frac_of_memcpy"] for g, w in v["streaming"].items()},
                                 "exact": v["exact_vs_local_argsort"]} for k, v in s["inputs"].items()}}
            for s in res["sizes"]]}), flush=True)
        return
    if args.i64:
        res = {"what": "stable argsort of int64 keys, resident in HBM (dsort_argsort_dev_i64, sorted keys and indices): "
                       "narrow = uniform in [-2^33, 2^33), wide = uniform over 64 bits, zipf_c4 = dsort_gen_zipf_i64; ms "
                       "per call of --steps back-to-back calls, legs from the HIP events between them (median; minmax "
                       "includes its 16-byte read-back and host wait), torch.sort(stable=True) of the same keys",
               "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
               "sizes": [bench_i64(torch, ctx, 1 << lg, args.steps, args.warmup) for lg in args.log2]}
        ctx.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"pairs_i64_bench": [{"n": s["n"], **{k: {"argsort_ms": v["argsort_ms"],
                                                                 "passes": v["argsort_passes"],
                                                                 "torch_over_argsort": v["torch_over_argsort"],
                                                                 "exact": v["exact_vs_torch_sort_stable"]}
                                                             for k, v in s["inputs"].items()}}
                                              for s in res["sizes"]]}), flush=True)
        return
    if args.gather:
        res = {"what": "distributed record gather of 16-byte records on one RCCL rank (dsort_sample_gather_dev), "
                       "indices a random permutation, against dsort_gather_dev of the same resident data, same "
                       "process; ms per call of --steps back-to-back calls, legs from the HIP events between them "
                       "(median)",
               "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
               "sizes": [bench_gather(torch, dsort, ctx, 1 << lg, args.steps, args.warmup) for lg in args.log2]}
        ctx.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"pairs_gather_bench": [{k: s[k] for k in ("n", "sample_gather_ms", "local_gather_ms",
                                                                    "sample_over_local", "legs_ms", "dominant_leg",
                                                                    "exact_vs_local_gather")}
                                                 for s in res["sizes"]]}), flush=True)
        return
    if args.sample:
        res = {"what": "global stable argsort of uniform int32 keys on one RCCL rank (dsort_sample_argsort_dev_i32) "
                       "against dsort_argsort_dev_i32 of the same resident keys, same process; ms per call of "
                       "--steps back-to-back calls, legs from the HIP events between them (median)",
               "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
               "sizes": [bench_sample(torch, dsort, ctx, 1 << lg, args.steps, args.warmup) for lg in args.log2]}
        ctx.close()
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
        print(json.dumps({"pairs_sample_bench": [{k: s[k] for k in ("n", "sample_argsort_ms", "local_argsort_ms",
                                                                    "sample_over_local", "sample_legs_ms",
                                                                    "local_legs_ms", "exact_vs_local_argsort")}
                                                 for s in res["sizes"]]}), flush=True)
        return
    res = {"what": "stable argsort of uniform int32 keys, resident in HBM (dsort_argsort_dev_i32)",
           "device": torch.cuda.get_device_name(0), "steps": args.steps, "warmup": args.warmup,
           "sizes": [bench_size(torch, ctx, 1 << lg, args.steps, args.warmup) for lg in args.log2]}
    ctx.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps({"pairs_bench": [{"n": s["n"], "argsort_ms": s["argsort_ms"], "legs_ms": s["legs_ms"],
                                       "torch_sort_stable_ms": s["torch_sort_stable_ms"],
                                       "torch_over_argsort": s["torch_over_argsort"],
                                       "pack_frac_of_memcpy": s["streaming"]["pack"]["frac_of_memcpy"],
                                       "unpack_frac_of_memcpy": s["streaming"]["unpack"]["frac_of_memcpy"],
                                       "exact": s["exact_vs_torch_sort_stable"]} for s in res["sizes"]]}), flush=True)


if __name__ == "__main__":
    main()
