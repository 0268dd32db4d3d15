"""numpy restatement of the first level's arithmetic bucket map (csrc/dsort_bucket.h: arith_part,
arith_splitter_key, BkMap.ar) and of the rule a sort takes it by (bucket_slotmap_kernel), from the input
keys alone -- the reference of tests/test_gpu_bkarith.py, pinned in tests/test_bkarith_host.py.

A sort of int32 keys takes the map when
  1. the sampled choice is the plain fixed map: slotmap_model.decide gives map 0 (no adaptive map, no refined
     slot), no two neighbouring splitters share a key (one-key slots) and the splitters' input positions
     do not run (nearly) monotone (the runs hint of sorted and reversed input);
  2. the samples' key range span = max - min is at least 2 B;
  3. no arithmetic bucket holds more than 3/2 os of the B os samples.
Mode 2 of the debug switch asks for rule 2 alone, mode 0 refuses.
"""
import numpy as np

import slotmap_model as sm


def arith_bucket(keys, klo, span, B):
    """The bucket of every key: B equal key widths over [klo, klo + span], clamped outside."""
    scale = (B << 32) // (span + 1)
    d = np.maximum(np.asarray(keys, np.int64) - int(klo), 0)  # < 2^32, scale < 2^31: the product fits
    return np.minimum((d * scale) >> 32, B - 1)


def sorted_samples(a, B, os):
    """(keys, positions) of the B os regular samples in (key, position) order."""
    a = np.asarray(a)
    pos = sm.sample_positions(a.size, B, os)
    smp = a[pos.astype(np.int64)]
    order = np.lexsort((pos, smp))
    return smp[order], pos[order]


def runs_hint(spl_pos):
    """bucket_runs_hint: the splitters' input positions ascend between 7/8 or more, or 1/8 or fewer, of the
    neighbours (16 splitters at least)."""
    nsp = spl_pos.size
    if nsp < 16:
        return False
    nasc = int((spl_pos[:-1] < spl_pos[1:]).sum())
    return 8 * nasc >= 7 * (nsp - 1) or 8 * nasc <= nsp - 1


def decide(a, B, os, mode=-1):
    """dict(take, why, span, fullest): whether the sort of int32 keys `a` in B buckets takes the map, the rule
    that refused it, the samples' key range and the most samples of one arithmetic bucket."""
    a = np.asarray(a, np.int32)
    keys, pos = sorted_samples(a, B, os)
    klo, span = int(keys[0]), int(keys[-1]) - int(keys[0])
    fullest = None
    if span >= 2 * B:
        fullest = int(np.bincount(arith_bucket(keys, klo, span, B), minlength=B).max())
    out = dict(take=False, why=None, span=span, fullest=fullest)
    if mode == 0:
        return dict(out, why="off")
    if span < 2 * B:
        return dict(out, why="span")
    if mode == 2:
        return dict(out, take=True)
    spl, spl_pos = keys[os - 1::os][:B - 1], pos[os - 1::os][:B - 1]
    plain = (sm.decide(spl, np.int32)["map"] == 0 and not bool((spl[1:] == spl[:-1]).any())
             and not runs_hint(spl_pos))
    if not plain:
        return dict(out, why="map")
    if 2 * fullest > 3 * os:
        return dict(out, why="samples")
    return dict(out, take=True)
