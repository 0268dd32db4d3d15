"""A plain numpy restatement of the first partition level's slot-map decision (csrc/dsort_bucket.h,
bucket_slotmap_kernel), from the input keys alone -- the reference of tests/test_gpu_slotmaps.py, held
in place by the pins of tests/test_slotmap_model.py.

  samples    S = B * os regular samples: sample k is the key at position ((2k + 1) n) // (2S)
             (bucket_sample_kernel, pair_sample_keys_kernel), sorted by (key, position);
  splitters  splitter b < B - 1 is the sorted sample (b + 1) os - 1 (bucket_splitter_kernel,
             pair_splitter_kernel);
  slots      of the sign-flipped key u, 2048 of them: fixed (the top 11 bits), linear
             (min((u - ulo) >> sh, 2047)), log (d = u - ulo itself below 2^M, else its bit length and the
             M bits after the leading one; M = 6 for int32, 5 for int64), ulo = the first splitter's
             flipped key and sh the smallest shift that brings the last splitter into the table;
  int32      the cost of a map is its largest slot among those with splitters of two or more keys;
             fixed when that is <= 8, else the cheaper adaptive map (log only when strictly cheaper) --
             unless the fixed map without its most crowded slot costs no more than that adaptive map:
             then the fixed map with that slot refined (first_level_map 3);
  int64      log when its most crowded slot (in distinct splitter keys) is strictly less crowded than
             the linear map's, else linear.

The key shapes of the tests (KEYS32, KEYS64) and the maps they are meant to reach (PINS) live here too, so
that the CPU pins and the GPU cases see the same inputs.
"""
import zlib

import numpy as np

SLOTB = 11
SLOTS = 1 << SLOTB
AD_MIX = 8            # int32: the fixed map is kept while no mixed slot holds more splitters
R2, R2_BITS = 256, 8  # sub-slots of the refined slot

I32_MIN, I32_MAX = -(2**31), 2**31 - 1
I64_MIN, I64_MAX = -(2**63), 2**63 - 1

_U64 = np.uint64


def key_bits(dtype):
    return 8 * np.dtype(dtype).itemsize


def log_m(kb):
    """Mantissa bits of the log map: the largest M with (kb - M + 1) 2^M slots in the table."""
    m = 0
    while m < 16 and (kb - (m + 1) + 1) * (1 << (m + 1)) <= SLOTS:
        m += 1
    return m


def flip(keys):
    """Sign-flipped keys as uint64 (the unsigned order is the keys' order)."""
    keys = np.asarray(keys)
    kb = key_bits(keys.dtype)
    u = keys.astype(np.int64).view(np.uint64)
    if kb == 32:
        return (u + _U64(1 << 31)) & _U64(0xFFFFFFFF)
    return u ^ _U64(1 << 63)


def bit_length(d):
    d = np.array(d, dtype=np.uint64)
    e = np.zeros(d.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        hi = (d >> _U64(s)) != 0
        e += s * hi
        d = np.where(hi, d >> _U64(s), d)
    return e + (d != 0)


def slot_fixed(u, kb):
    return (u >> _U64(kb - SLOTB)).astype(np.int64)


def _above(u, ulo):
    return np.where(u < _U64(ulo), _U64(0), u - _U64(ulo))


def slot_linear(u, ulo, sh):
    return np.minimum(_above(u, ulo) >> _U64(sh), _U64(SLOTS - 1)).astype(np.int64)


def slot_log(u, ulo, kb):
    m = log_m(kb)
    d = _above(u, ulo)
    e = bit_length(d)
    small = d < _U64(1 << m)
    sh = np.where(small, 0, e - 1 - m).astype(np.uint64)
    big = ((e - m) << m) | ((d >> sh) & _U64((1 << m) - 1)).astype(np.int64)
    return np.where(small, d.astype(np.int64), big)


def sample_positions(n, B, os):
    S = B * os
    k = np.arange(S, dtype=np.uint64)
    return ((_U64(2) * k + _U64(1)) * _U64(n)) // _U64(2 * S)


def splitters(a, B, os):
    """(keys, positions) of the B - 1 splitters of input a."""
    a = np.asarray(a)
    pos = sample_positions(a.size, B, os)
    smp = a[pos.astype(np.int64)]
    order = np.lexsort((pos, smp))
    pick = order[os - 1::os][:B - 1]
    return smp[pick], pos[pick]


def _adaptive(spl_u, kb):
    """ulo and the linear shift of the adaptive maps."""
    ulo, r = int(spl_u[0]), int(spl_u[-1]) - int(spl_u[0])
    return ulo, max(r.bit_length() - SLOTB, 0)


def _tot_dst(slots, first):
    tot = np.bincount(slots, minlength=SLOTS)
    dst = np.bincount(slots[first], minlength=SLOTS)
    return tot, dst


def _cost(tot, dst):
    mixed = dst >= 2
    return int(tot[mixed].max()) if mixed.any() else 0


def decide(spl, dtype):
    """The decision from the splitter keys (ascending).  Returns a dict: map (first_level_map), slot
    (the refined slot, or None), costs (int32: fixed, linear, log; int64: the crowd under linear, log),
    rest (int32 with a refined slot: the fixed map's cost without it)."""
    dtype = np.dtype(dtype)
    kb = key_bits(dtype)
    spl = np.asarray(spl, dtype)
    if spl.size == 0:
        return dict(map=0 if kb == 32 else 1, slot=None, costs=(0, 0, 0)[:3 if kb == 32 else 2], rest=None)
    u = flip(spl)
    first = np.ones(spl.size, bool)
    first[1:] = spl[1:] != spl[:-1]
    ulo, sh = _adaptive(u, kb)
    lin, log = slot_linear(u, ulo, sh), slot_log(u, ulo, kb)
    if kb == 64:
        crowd = (int(np.bincount(lin[first]).max()), int(np.bincount(log[first]).max()))
        return dict(map=2 if crowd[1] < crowd[0] else 1, slot=None, costs=crowd, rest=None)
    td = [_tot_dst(s, first) for s in (slot_fixed(u, kb), lin, log)]
    cost = [_cost(t, d) for t, d in td]
    qa = 2 if cost[2] < cost[1] else 1
    slot = rest = None
    if cost[0] > AD_MIX and cost[qa] > AD_MIX:
        tot, dst = td[0]
        cand = int(np.flatnonzero((dst >= 2) & (tot == cost[0]))[0])
        others = dst >= 2
        others[cand] = False
        rest = int(tot[others].max()) if others.any() else 0
        if rest <= cost[qa]:
            slot = cand
    if slot is not None:
        m = 3
    elif cost[0] <= AD_MIX:
        m = 0
    else:
        # (A linear map that equals the fixed one -- from the bottom of the range, the fixed shift --
        # would leave BkMap.ad at 0 and report map 0.  It never gets here: it costs what the fixed map
        # costs, which is no less than the fixed map's cost without a slot, so the refinement is kept.)
        m = qa
    return dict(map=m, slot=slot, costs=tuple(cost), rest=rest if slot is not None else None)


def predict(a, B, os):
    """decide() for input a sorted with B buckets and os samples per bucket."""
    a = np.asarray(a)
    return decide(splitters(a, B, os)[0], a.dtype)


def refined_table(spl, slot):
    """(r2lo, r2sh) of the refined slot's 256 sub-slots, sub-slot = min((u - r2lo) >> r2sh, 255): linear
    from one key below the slot's first splitter (from that splitter where the slot starts there, and in
    slot 0) to the splitter at 31/32 of the slot's."""
    u = flip(np.asarray(spl, np.int32))
    inside = np.flatnonzero(slot_fixed(u, 32) == slot)
    a0, z = int(inside[0]), int(inside[-1]) + 1
    k0, hi = int(u[a0]), int(u[z - 1 - (z - a0) // 32])
    lo = k0 - 1 if slot > 0 and k0 > (slot << (32 - SLOTB)) else k0
    return lo, max((hi - lo).bit_length() - R2_BITS, 0)


def pure_copies(a, B, os):
    """int32 on the fixed map (first_level_map 0 or 3).  Returns (owned, sure): the number of input keys
    whose value owns at least two splitters, and the number of those that the lookups send to pure buckets
    for certain.  A key K with splitters f .. l (l > f) has the pure buckets f + 1 .. l.  Where K's slot --
    or its sub-slot of the refined slot -- holds splitters of K alone, every copy goes there
    (bucket_onekey, refine_pick); where it holds other keys' splitters too, the lookup searches by
    (key, position), and the copies at positions in (position of splitter f, position of splitter l] do."""
    a = np.asarray(a, np.int32)
    spl, pos = splitters(a, B, os)
    d = decide(spl, np.int32)
    assert d["map"] in (0, 3)
    u = flip(spl)
    fixed = slot_fixed(u, 32)
    keys, f, cnt = np.unique(spl, return_index=True, return_counts=True)
    heavy = cnt >= 2
    keys, f, cnt = keys[heavy], f[heavy], cnt[heavy]
    # the lookup unit of every splitter: its slot, or its sub-slot in the refined slot
    unit = fixed.astype(np.int64) * (R2 + 1)
    if d["slot"] is not None:
        inside = np.flatnonzero(fixed == d["slot"])
        lo, r2sh = refined_table(spl, d["slot"])
        sub = np.minimum(np.maximum(u[inside].astype(np.int64) - lo, 0) >> r2sh, R2 - 1)
        unit[inside] += 1 + sub
    per_unit = dict(zip(*np.unique(unit, return_counts=True)))
    owned = sure = 0
    apos = np.arange(a.size, dtype=np.uint64)
    for K, fi, c in zip(keys, f, cnt):
        where = a == K
        copies = int(where.sum())
        owned += copies
        if per_unit[unit[fi]] == c and np.all(unit[fi:fi + c] == unit[fi]):
            sure += copies
        else:
            p = apos[where]
            sure += int(((p > pos[fi]) & (p <= pos[fi + c - 1])).sum())
    return owned, sure


# ---------------------------------------------------------------------------------------------------
# The key shapes.  "half U": half of the keys uniform over the full range.

def _half(rng, n, dtype, other):
    info = np.iinfo(dtype)
    a = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    m = rng.random(n) < 0.5
    a[m] = other(int(m.sum()))
    return a


def _k32_uniform(rng, n):
    return rng.integers(I32_MIN, I32_MAX, n, dtype=np.int32, endpoint=True)


def _k32_bit0(rng, n):
    return (((rng.integers(0, 1024, n) - 512) << 22) + rng.integers(0, 2, n)).astype(np.int32)


def _k32_zipf(rng, n):
    return (rng.zipf(1.3, n) % (1 << 31)).astype(np.int32)


def _k32_low3(rng, n):
    a = _k32_uniform(rng, n)
    r = rng.random(n)
    a[(r >= 0.49) & (r < 0.51)] = I32_MIN
    m = r >= 0.51
    a[m] = (I32_MIN + (1 << 20) + rng.integers(0, 100, int(m.sum()))).astype(np.int32)
    return a


KEYS32 = {
    "uniform": _k32_uniform,
    "bit0": _k32_bit0,
    "ref100": lambda rng, n: rng.integers(1, 101, n).astype(np.int32),
    "lowedge_only": lambda rng, n: (I32_MIN + rng.integers(0, 100, n)).astype(np.int32),
    "highedge_only": lambda rng, n: (I32_MAX - rng.integers(0, 100, n)).astype(np.int32),
    "zipf": _k32_zipf,
    "zipf_neg": lambda rng, n: (I32_MIN + _k32_zipf(rng, n).astype(np.int64)).astype(np.int32),
    "geom": lambda rng, n: np.floor(2.0 ** rng.uniform(0, 31, n)).astype(np.int64).astype(np.int32),
    "mixed_lowedge": lambda rng, n: _half(rng, n, np.int32, lambda c: I32_MIN + rng.integers(0, 100, c)),
    "mixed100": lambda rng, n: _half(rng, n, np.int32, lambda c: rng.integers(1, 101, c)),
    "mixed_signed": lambda rng, n: _half(rng, n, np.int32, lambda c: rng.integers(-50, 50, c)),
    "mixed_cluster": lambda rng, n: _half(rng, n, np.int32, lambda c: rng.integers(0, 1 << 20, c)),
    "mixed_highedge": lambda rng, n: _half(rng, n, np.int32, lambda c: I32_MAX - rng.integers(0, 100, c)),
    "low3": _k32_low3,
}


def _k64_c4(rng, n):
    z = (rng.zipf(1.2, n) % (1 << 24)).astype(np.uint64)
    return (z * _U64(0x9E3779B97F4A7C15)).view(np.int64)


KEYS64 = {
    "uniform": lambda rng, n: rng.integers(I64_MIN, I64_MAX, n, dtype=np.int64, endpoint=True),
    "small100": lambda rng, n: rng.integers(1, 101, n).astype(np.int64),
    "c4": _k64_c4,
    "zipf": lambda rng, n: rng.zipf(1.3, n).astype(np.int64),
    "zipf_at_min": lambda rng, n: I64_MIN + (rng.zipf(1.3, n) % (1 << 40)).astype(np.int64),
    "geom": lambda rng, n: np.floor(2.0 ** rng.uniform(0, 62, n)).astype(np.int64),
    "extremes_mix": lambda rng, n: _half(rng, n, np.int64, lambda c: I64_MAX - rng.integers(0, 100, c)),
}

# name -> (first_level_map, the refined slot(s) allowed); None: no pin, the model alone decides
PINS32 = {
    "uniform": (0, None), "bit0": (0, None),
    "ref100": (1, None), "lowedge_only": (1, None), "highedge_only": (1, None),
    "zipf": (2, None), "zipf_neg": (2, None), "geom": (2, None), "mixed_lowedge": (2, None),
    "mixed100": (3, (1024,)), "mixed_signed": (3, (1023, 1024)), "mixed_cluster": (3, (1024,)),
    "mixed_highedge": (3, (2047,)), "low3": (3, (0,)),
}
PINS64 = {"uniform": (1, None), "small100": (1, None), "c4": (1, None),
          "zipf": (2, None), "zipf_at_min": (2, None), "geom": (2, None), "extremes_mix": None}

SIZES = [(1024, 500_000), (256, 300_001), (64, 200_003)]
SMALL = (1024, 40_000)  # more samples than keys at the default oversampling
SMALL_SHAPES = ("uniform", "mixed100", "zipf")
OS_DEFAULT = 128


def make_keys(dtype, name, B, n):
    """The keys of case (dtype, name, B, n), as generated: one seeded generator per case."""
    dtype = np.dtype(dtype)
    table = KEYS32 if dtype == np.int32 else KEYS64
    seed = [key_bits(dtype), zlib.crc32(name.encode()), B, n]  # (a new shape leaves the others' keys alone)
    a = table[name](np.random.default_rng(seed), n)
    assert a.dtype == dtype and a.size == n
    return a


def pin_of(dtype, name):
    return (PINS32 if np.dtype(dtype) == np.int32 else PINS64)[name]
