"""The path every sort below 2^25 keys and every merge takes, at the sizes where its code branches:
the tile sort followed by regular k-way passes (mergew_kernel<T, LOGF, REG = true>), and the merge of
arbitrary runs (partk_kernel / mergew_kernel with REG = false behind dsort_merge_dev_*).  Small
shapes only; expected values are numpy's stable sort of the input (of the concatenated runs), with
the oracle on top where n <= 200 000.  Every device buffer is a view into a larger tensor filled
with a sentinel, which is checked afterwards, and every input is checked to be left alone.

The shape tables and generators below are imported by tests/test_abi.py, which checks them on the
CPU (ascending runs, the duplicate shares, the pass and level formulas)."""
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# Constants of csrc/dsort_wave.hip, by key width in bytes.
WK = 1024                        # :60  WK = 64 * R, R = 16 (:59)
TILE = {4: 8192, 8: 8192}        # :81  TILE_OF<T> = WK * WG<T>::WAVES; WAVES = 8 (:71/:74 int32, :79 int64)
MT = {4: 16384, 8: 8192}         # :85  MTILE_OF<T> = WK * WG<T>::MWAVES; MWAVES = 16 (:74) / 8 (:79)
SLACK = {w: MT[w] // 32 for w in MT}             # :86  MSLACK_OF<T> = MTILE_OF<T> / 32: 512 / 256
TNOM = {w: MT[w] - 2 * SLACK[w] for w in MT}     # :87  MTNOM_OF<T>: 15360 / 7680
MAXLOGF = {4: 5, 8: 4}           # :74 / :79  WG<T>::MAXLOGF
MAXF = {w: 1 << MAXLOGF[w] for w in MAXLOGF}     # runs per pass: 32 / 16
KPC = {4: 4, 8: 2}               # :88  keys per 16-byte chunk
DEFAULT_LOGF = 4                 # plan_passes: max_logf(opt, 4, WG<T>::MAXLOGF)
DTYPE = {4: np.int32, 8: np.int64}
SENT = {4: 0x5A5A5A5A, 8: 0x5A5A5A5A5A5A5A5A}
GUARD = 16                       # sentinel elements on either side (a multiple of 16 bytes)
OFFSETS = {4: [0, 1, 2, 3], 8: [0, 1]}  # view offsets in elements: every phase of a 16-byte chunk


def ceil_log2(x):
    p = 0
    while (1 << p) < x:
        p += 1
    return p


def sort_passes(tiles, w, option=-1):
    """Merge passes of a regular-path sort of `tiles` tiles under DSORT_OPT_MAX_FANIN_LOG2 = option."""
    bits = ceil_log2(tiles)
    cap = min(option if option > 0 else DEFAULT_LOGF, MAXLOGF[w])
    return -(-bits // cap)


def merge_levels(k, maxf):
    """Levels of a merge of k runs: how often k is divided by maxf, rounding up, to reach 1."""
    lv = 0
    while k > 1:
        k = -(-k // maxf)
        lv += 1
    return lv


def _rng(*what):
    return np.random.default_rng(zlib.crc32(repr(what).encode()))


# ------------------------------------------------------------------------------ sort inputs
SWEEP_FANIN = [-1, 1, 2, 3, 4, 5]
SWEEP_TILES = [2, 3, 5, 9, 17, 33]
SWEEP_REM = [1, 4097, 8192]
SWEEP_KINDS = ["uniform", "few", "extremes"]
VIEW_SIZES = [8189, 8190, 8191, 8192, 8193, 3 * 8192 + 5, 17 * 8192 + 123]
VIEW_KINDS = ["uniform", "few"]


def sort_keys(kind, n, w):
    """Unsorted keys for the sort tests (the generators of tests/test_gpu_sort.py::_dist)."""
    dt = DTYPE[w]
    info = np.iinfo(dt)
    rng = _rng("sort", kind, n, w)
    if kind == "uniform":
        return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    if kind == "few":  # five values that include the type's min and max
        return rng.choice(np.array([info.min, -1, 0, 1, info.max], dt), n)
    if kind == "extremes":
        a = rng.integers(-3, 3, n).astype(dt)
        a[::3] = info.max
        a[1::5] = info.min
        return a
    raise ValueError(kind)


# ------------------------------------------------------------------------------ merge inputs
K_VALUES = {4: [1, 2, 3, 4, 5, 8, 9, 16, 17, 31, 32, 33, 64, 65, 1024, 1025],
            8: [1, 2, 3, 5, 8, 9, 16, 17, 33, 256, 257]}
FAMILIES = ["tiny", "chunk", "wk", "tnom", "one_long", "empties", "random"]
BIG_K = 256  # from here on only tiny, chunk and short random runs: the three-level cases stay small
BIG_K_FAMILIES = ["tiny", "chunk", "random"]
KINDS = {4: ["uniform", "all_equal", "two_values", "stairs_up", "stairs_down", "dups", "zipf", "limits"]}
KINDS[8] = KINDS[4] + ["low_half", "high_half"]


def families_of(k):
    return BIG_K_FAMILIES if k >= BIG_K else FAMILIES


def run_lengths(family, k, w):
    """The run-length variants of one family for k runs: a list of length lists, each with at least
    one key in total."""
    rng = _rng("lens", family, k, w)
    n, mt, tnom, slack = KPC[w], MT[w], TNOM[w], SLACK[w]
    if family == "tiny":
        out = [rng.integers(0, 4, k)]
    elif family == "chunk":  # segments start at every phase of a 16-byte chunk
        out = [rng.choice([n - 1, n, n + 1], k)]
    elif family == "wk":  # a pair's last window shifted to the pair's end; pairs below one window
        out = [rng.choice([WK - 1, WK, WK + 1, 2 * WK - 1, 2 * WK + 1], k)]
    elif family == "tnom":
        out = [rng.choice([tnom - 1, tnom, tnom + 1, mt, mt + 1, 2 * tnom + slack], k)]
    elif family == "one_long":  # one long run among tiny ones: first, in the middle, last
        out = []
        for pos in sorted({0, k // 2, k - 1}):
            lens = rng.integers(0, 61, k)
            lens[pos] = 5 * tnom + 333
            out.append(lens)
    elif family == "empties":
        every_other = rng.integers(1, 3000, k)
        every_other[1::2] = 0
        ends = rng.integers(1, 3000, k)
        ends[0] = ends[-1] = 0
        one = np.zeros(k, np.int64)
        one[k // 2] = 3 * WK + 7
        out = [every_other, ends, one]
    elif family == "random":
        out = [rng.integers(0, (200 if k >= BIG_K else 3 * mt) + 1, k)]
    else:
        raise ValueError(family)
    out = [[int(x) for x in lens] for lens in out if int(np.sum(lens)) > 0]
    if not out:
        out = [[1] * k]
    return out


def merge_runs(kind, lens, w):
    """k ascending runs of the given lengths, of one key kind."""
    dt = DTYPE[w]
    info = np.iinfo(dt)
    k, n = len(lens), int(sum(lens))
    rng = _rng("keys", kind, tuple(lens[:8]), k, n, w)
    if kind == "uniform":
        a = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    elif kind == "all_equal":  # every cut is the exact tie split
        a = np.full(n, 7, dt)
    elif kind == "two_values":
        a = rng.choice(np.array([-3, 11], dt), n)
    elif kind in ("stairs_up", "stairs_down"):  # the cuts take whole runs, in either order
        j = np.repeat(np.arange(k), lens)
        a = (j if kind == "stairs_up" else k - j).astype(dt)
    elif kind == "dups":
        a = rng.integers(-50, 50, n).astype(dt)
    elif kind == "zipf":  # a heavy head, as in test_gpu_sort.py::test_heavy_duplicates_i32
        pool = np.minimum(rng.zipf(1.3, min(n, 1 << 16)), 2**31 - 1).astype(np.int64)
        z = pool[rng.integers(0, pool.size, n)]  # (drawing n Zipf variates is the slow part on the host)
        a = ((z * 2654435761) % (2**32) - 2**31).astype(dt)
    elif kind == "limits":  # about a third key_min, a third key_max: the kernels' padding values as keys
        a = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
        sel = rng.integers(0, 3, n)
        a[sel == 0] = info.min
        a[sel == 1] = info.max
    elif kind == "low_half":  # int64: one high word, low words over the whole uint32 range
        low = rng.integers(0, 2**32, n, dtype=np.int64)
        low[::2] |= 1 << 31
        a = (np.int64(-0x1234) << 32) | low
    elif kind == "high_half":  # int64: one low word
        a = (rng.integers(-(2**31), 2**31, n, dtype=np.int64) << 32) | np.int64(0x89ABCDEF)
    else:
        raise ValueError(kind)
    assert a.dtype == dt and a.size == n
    runs, o = [], 0
    for m in lens:
        runs.append(np.sort(a[o:o + m]))
        o += m
    return runs


def merge_cases(w):
    return [(k, f, kind) for k in K_VALUES[w] for f in families_of(k) for kind in KINDS[w]]


# ------------------------------------------------------------------------------ device helpers
def _tdt(w):
    import torch
    return torch.int32 if w == 4 else torch.int64


def _frame(a, off):
    """A sentinel-filled tensor with `a` at element GUARD + off; returns (whole, view)."""
    import torch
    w = a.dtype.itemsize
    buf = torch.full((2 * GUARD + off + a.size,), SENT[w], dtype=_tdt(w), device="cuda")
    view = buf[GUARD + off:GUARD + off + a.size]
    if a.size:
        view.copy_(torch.from_numpy(a))
        assert view.data_ptr() % 16 == (off * w) % 16
    return buf, view


def _empty_frame(n, w, off):
    return _frame(np.full(n, SENT[w], DTYPE[w]), off)


def _check_frame(buf, off, exp):
    """The view holds exp, element for element, and the sentinels around it are intact."""
    h = buf.cpu().numpy()
    s = SENT[exp.dtype.itemsize]
    lo, hi = GUARD + off, GUARD + off + exp.size
    assert (h[:lo] == s).all() and (h[hi:] == s).all(), "sentinel overwritten"
    got = h[lo:hi]
    if not np.array_equal(got, exp):
        bad = np.flatnonzero(got != exp)
        raise AssertionError(f"{bad.size} of {exp.size} keys differ, first at {bad[0]}: "
                             f"got {got[bad[0]]}, expected {exp[bad[0]]}")


_expected = {}


def _sorted_ref(oracle, key, a):
    """np.sort(kind='stable') of `a`, computed once per key; the oracle agrees where n <= 200 000."""
    if key not in _expected:
        exp = np.sort(a, kind="stable")
        if 0 < a.size <= 200_000:
            assert np.array_equal(oracle.merge_sort(a), exp)
        exp.setflags(write=False)
        _expected[key] = exp
    return _expected[key]


def _merged_ref(oracle, runs, w):
    cat = np.concatenate(runs) if runs else np.zeros(0, DTYPE[w])
    exp = np.sort(cat, kind="stable")
    if 0 < cat.size <= 200_000:
        # (the oracle's run merge scans all k heads for every key: from BIG_K runs on, its merge
        # sort of the concatenation is the second reference)
        ref = oracle.merge_runs(runs, DTYPE[w]) if len(runs) < BIG_K else oracle.merge_sort(cat)
        assert np.array_equal(ref, exp)
    return cat, exp


def _sort_framed(ctx, a, in_off, out_off, inplace):
    """Sorts a framed copy of `a`; returns (output frame, its offset).  Copy mode checks that the
    input and its frame are unchanged."""
    import torch
    ibuf, iview = _frame(a, in_off)
    if inplace:
        ctx.sort_dev(iview)
        torch.cuda.synchronize()
        return ibuf, in_off
    obuf, oview = _empty_frame(a.size, a.dtype.itemsize, out_off)
    ctx.sort_dev(iview, oview)
    torch.cuda.synchronize()
    _check_frame(ibuf, in_off, a)
    return obuf, out_off


def _merge_frames(cat, w, in_off=0, out_off=0):
    """The framed input (the runs back to back) and the framed output of a merge_dev."""
    ibuf, iview = _frame(cat, in_off)
    obuf, oview = _empty_frame(cat.size, w, out_off)
    return ibuf, iview, obuf, oview


# ------------------------------------------------------------------------------ (a) fan-in sweep
@pytest.mark.parametrize("kind", SWEEP_KINDS)
@pytest.mark.parametrize("rem", SWEEP_REM)
@pytest.mark.parametrize("tiles", SWEEP_TILES)
@pytest.mark.parametrize("fanin", SWEEP_FANIN)
@pytest.mark.parametrize("w", [4, 8])
def test_sort_fanin_sweep(gpu_ctx, oracle, w, fanin, tiles, rem, kind):
    """Regular passes of every fan-in the option allows: mergew_kernel<T, LOGF, REG = true> for LOGF
    1..5 (int64: 1..4, 5 acts as 4), chains of LOGF = 1 passes, 32 runs in one int32 pass.  The pass
    count proves the plan the test means was the one that ran."""
    n = (tiles - 1) * TILE[w] + rem
    a = sort_keys(kind, n, w)
    exp = _sorted_ref(oracle, ("sort", kind, n, w), a)
    P = sort_passes(tiles, w, fanin)
    with gpu_ctx.options(max_fanin_log2=fanin):
        obuf, off = _sort_framed(gpu_ctx, a, 0, 0, False)
        st = gpu_ctx.stats()
        stages = gpu_ctx.sort_stages(n, w)
    _check_frame(obuf, off, exp)
    assert st["merge_passes"] == P, st
    assert st["tile_keys"] == TILE[w] and st["keys_in"] == n and st["keys_out"] == n, st
    assert stages == 1 + P
    if w == 8 and fanin == 5:  # the clamp: exactly as 4
        with gpu_ctx.options(max_fanin_log2=4):
            assert gpu_ctx.sort_stages(n, w) == stages
        assert P == sort_passes(tiles, w, 4)


# ------------------------------------------------------------------------------ (b) unaligned sort
def _view_cases():
    out = []
    for w in (4, 8):
        for i in OFFSETS[w]:
            out.append((w, i, i, True))
            out += [(w, i, o, False) for o in OFFSETS[w]]
    return out


@pytest.mark.parametrize("kind", VIEW_KINDS)
@pytest.mark.parametrize("n", VIEW_SIZES)
@pytest.mark.parametrize("w,in_off,out_off,inplace", _view_cases())
def test_sort_unaligned_views(gpu_ctx, oracle, w, in_off, out_off, inplace, n, kind):
    """Default options (no buckets) on views at every phase of a 16-byte chunk: load_tile's `off` and
    its scalar path (off + valid > TILE), bin_sort_tile's `sh` with the rule that a tile within 3 keys
    of TILE keeps sh = 0, and regular passes that read and write misaligned buffers (mis != 0)."""
    a = sort_keys(kind, n, w)
    exp = _sorted_ref(oracle, ("sort", kind, n, w), a)
    obuf, off = _sort_framed(gpu_ctx, a, in_off, out_off, inplace)
    st = gpu_ctx.stats()
    _check_frame(obuf, off, exp)
    assert st["merge_passes"] == sort_passes(-(-n // TILE[w]), w), st
    assert st["tile_keys"] == TILE[w], st


# ------------------------------------------------------------------------------ (c) merge_dev
def _run_merge(ctx, oracle, runs, w, in_off=0, out_off=0):
    import torch
    lens = [r.size for r in runs]
    cat, exp = _merged_ref(oracle, runs, w)
    ibuf, iview, obuf, oview = _merge_frames(cat, w, in_off, out_off)
    ctx.merge_dev(iview, lens, oview)
    torch.cuda.synchronize()
    st = ctx.stats()
    _check_frame(obuf, out_off, exp)
    _check_frame(ibuf, in_off, cat)  # the input is left alone
    assert st["merge_passes"] == merge_levels(len(runs), MAXF[w]), st
    assert st["keys_in"] == cat.size and st["keys_out"] == cat.size, st
    assert st["tile_keys"] == TILE[w], st


@pytest.mark.parametrize("k,family,kind", merge_cases(4))
def test_merge_dev_i32(gpu_ctx, oracle, k, family, kind):
    """dsort_merge_dev_i32: one, two and three levels (k > 32, k > 1024), unequal runs."""
    for lens in run_lengths(family, k, 4):
        _run_merge(gpu_ctx, oracle, merge_runs(kind, lens, 4), 4)


@pytest.mark.parametrize("k,family,kind", merge_cases(8))
def test_merge_dev_i64(gpu_ctx, oracle, k, family, kind):
    """dsort_merge_dev_i64: one, two and three levels (k > 16, k > 256).  Duplicate-heavy kinds reach
    partk_kernel's exact tie split, its data-interpolation modes and the hi - 1 clamp; `limits` puts
    key_min / key_max, the kernels' padding values, among the keys."""
    for lens in run_lengths(family, k, 8):
        _run_merge(gpu_ctx, oracle, merge_runs(kind, lens, 8), 8)


# ------------------------------------------------------------------------------ (d) unaligned merge
@pytest.mark.parametrize("kind", ["uniform", "dups"])
@pytest.mark.parametrize("family", ["chunk", "tnom"])
@pytest.mark.parametrize("k", [2, 5, 17, 33])
@pytest.mark.parametrize("w,in_off,out_off", [(w, i, o) for w in (4, 8) for i in OFFSETS[w] for o in OFFSETS[w]])
def test_merge_dev_unaligned_views(gpu_ctx, oracle, w, in_off, out_off, k, family, kind):
    """d_in and d_out at every phase of a 16-byte chunk: mergew_kernel's `mis`, edge chunks that
    start below the segment (and below d_in), count_le_window's `end` bound."""
    for lens in run_lengths(family, k, w):
        _run_merge(gpu_ctx, oracle, merge_runs(kind, lens, w), w, in_off, out_off)


# ------------------------------------------------------------------------------ (e) back to back
B2B = [(65, "random_short"), (3, "tnom"), (1025, "random"), (2, "wk")]


def _b2b_inputs(oracle):
    jobs = []
    for k, family in B2B:
        if family == "random_short":
            lens = [int(x) for x in _rng("b2b", k).integers(0, 5001, k)]
        else:
            lens = run_lengths(family, k, 4)[0]
        runs = merge_runs("uniform" if k != 3 else "dups", lens, 4)
        cat, exp = _merged_ref(oracle, runs, 4)
        jobs.append((lens, cat, exp) + _merge_frames(cat, 4))
    return jobs


@pytest.mark.parametrize("streams", [1, 2])
def test_merges_back_to_back_without_sync(gpu_ctx, oracle, streams):
    """Merges of k = 65, 3, 1025, 2 issued with no synchronize in between, into separate outputs:
    every level rewrites the pinned group table (behind groups_ev), and all share the split vectors
    and the merge scratch.  With two streams the second must wait for the first on the device."""
    import torch
    jobs = _b2b_inputs(oracle)
    torch.cuda.synchronize()
    ss = [torch.cuda.Stream() for _ in range(streams)]
    passes = []
    for i, (lens, cat, exp, ibuf, iview, obuf, oview) in enumerate(jobs):
        with torch.cuda.stream(ss[i % streams]):
            gpu_ctx.merge_dev(iview, lens, oview)
        passes.append(gpu_ctx.stats()["merge_passes"])
    torch.cuda.synchronize()
    assert passes == [merge_levels(k, MAXF[4]) for k, _ in B2B] == [2, 1, 3, 1]
    for lens, cat, exp, ibuf, iview, obuf, oview in jobs:
        _check_frame(obuf, 0, exp)
        _check_frame(ibuf, 0, cat)


# ------------------------------------------------------------------------------ (f) host entries
@pytest.mark.parametrize("kind", ["dups", "limits"])
@pytest.mark.parametrize("k", [3, 17, 33])
def test_merge_host_i64(gpu_ctx, oracle, k, kind):
    """dsort_merge_i64 with duplicate-heavy keys and with the key limits."""
    runs = merge_runs(kind, run_lengths("random", k, 8)[0], 8)
    keep = [r.copy() for r in runs]
    cat, exp = _merged_ref(oracle, runs, 8)
    got = gpu_ctx.merge(runs)
    st = gpu_ctx.stats()
    assert np.array_equal(got, exp)
    assert all(np.array_equal(r, c) for r, c in zip(runs, keep))
    assert st["merge_passes"] == merge_levels(k, MAXF[8]) and st["tile_keys"] == TILE[8], st
    assert st["keys_in"] == cat.size, st
