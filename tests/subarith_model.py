"""numpy restatement of the second level's arithmetic sub-bucket map and of the rule a bucket takes it by
(csrc/dsort_sub.h: arith_scale, arith_sub, sb_splitter_kernel), for the tests."""
import numpy as np

MAXS = 3       # SB_ARITH_MAXS: a sub-bucket may hold 3 * os of the bucket's nsub * os samples
MAXS_RUNS = 6  # SB_ARITH_MAXS_RUNS: ... 6 * os when the samples are clumped (sorted, reversed input)
RUN = 8        # SB_RUN: samples are taken in runs of 8 adjacent keys


def arith_sub(keys, klo, span, nsub):
    """The sub-bucket of every key: nsub equal key widths over [klo, klo + span], clamped outside."""
    scale = (nsub << 32) // (span + 1)
    d = np.maximum(np.asarray(keys, np.int64) - int(klo), 0)  # < 2^32, scale < 2^31: the product fits
    return np.minimum((d * scale) >> 32, nsub - 1)


def clumped(samples, run=RUN):
    """At least half of the neighbours in (key, sampling index) order come from one sample run."""
    s = np.asarray(samples)
    if run <= 1 or s.size % run:
        return False
    order = np.argsort(s, kind="stable") // run
    return 2 * int((order[1:] == order[:-1]).sum()) >= s.size


def arith_take(samples, nsub, os, run=RUN):
    """take (True) or refuse from a bucket's sample keys alone, given in sampling order."""
    s = np.asarray(samples, np.int64)
    klo, span = int(s.min()), int(s.max() - s.min())
    if nsub < 2 or span < 2 * nsub:
        return False
    maxs = MAXS_RUNS if clumped(s, run) else MAXS
    return int(np.bincount(arith_sub(s, klo, span, nsub), minlength=nsub).max()) <= maxs * os


def nsub_of(length, tile=8192, m=1536, maxs=1024):
    """sub_plan's sub-bucket count of a bucket of `length` keys (int32 defaults)."""
    return 1 if length <= tile else min(-(-length // m), maxs)


def predict_take(keys, B, os=8, seed=1):
    """The rule over a MODEL of a sort's buckets -- B equal-count ranges of the sorted keys, nsub * os
    keys drawn from each as its sample: (buckets of several sub-buckets, those that take the map)."""
    s = np.sort(np.asarray(keys))
    rng = np.random.default_rng(seed)
    many = take = 0
    for part in np.array_split(s, B):
        if part[0] == part[-1]:
            continue  # (a pure bucket)
        ns = nsub_of(part.size)
        if ns < 2:
            continue
        many += 1
        take += arith_take(rng.choice(part, ns * os), ns, os)
    return many, take
