"""C-ABI checks that need no GPU: the library loads, exports every function include/dsort.h
declares, the host-side planning rules behave, and the product fails loudly without a GPU."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import PKG, REPO

HEADER = os.path.join(REPO, "include", "dsort.h")
LIB = os.path.join(PKG, "lib", "libdsort.so")


def declared_functions():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(dsort_[a-z0-9_]+)\s*\(", text)))


def test_header_lists_match_binding(dsort_mod):
    assert declared_functions() == sorted(dsort_mod.EXPORTS)


def test_library_exports_every_declared_symbol():
    assert os.path.exists(LIB), "build first: make -C distributed-sorting-with-fault-tolerance_amd"
    lib = ctypes.CDLL(LIB)
    missing = [f for f in declared_functions() if not hasattr(lib, f)]
    assert not missing, missing


def test_library_is_gfx950_code_object():
    blob = open(LIB, "rb").read()
    assert b"gfx950" in blob
    assert b"sm_" not in blob[:0]  # no CUDA targets are produced by this build


def test_version_string(dsort_mod):
    v = dsort_mod.load().dsort_version().decode()
    assert "gfx950" in v


def test_init_without_gpu_fails_loudly(dsort_mod):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    with pytest.raises(dsort_mod.DsortError):
        dsort_mod.Context(0)


def test_sample_positions(dsort_mod):
    idx = dsort_mod.plan_sample_positions(1000, 4)
    assert idx.tolist() == [200, 400, 600, 800]
    assert dsort_mod.plan_sample_positions(0, 3).tolist() == [0, 0, 0]
    assert dsort_mod.plan_sample_positions(2, 4).tolist() == [0, 0, 1, 1]


@pytest.mark.parametrize("dt", [np.int32, np.int64])
def test_plan_cuts_partition_is_exact_and_balanced(dsort_mod, dt):
    """All ranks' cuts together route every key to exactly one rank and the concatenation of the
    per-rank merges is the sorted input -- including a heavy duplicate spread over ranks."""
    rng = np.random.default_rng(7)
    P, n, S = 4, 20000, 64
    chunks = []
    for r in range(P):
        a = rng.integers(-50, 50, n).astype(dt)
        a[: n // 2] = 7  # heavy hitter on every rank
        chunks.append(np.sort(a))
    samples, idxs = [], []
    for r in range(P):
        idx = dsort_mod.plan_sample_positions(n, S)
        samples.append(chunks[r][idx.astype(np.int64)])
        idxs.append(idx)
    sv, sr, si = dsort_mod.plan_splitters(np.concatenate(samples), np.concatenate(idxs), P)
    assert sv.size == P - 1
    cuts = [dsort_mod.plan_cuts(chunks[r], r, P, sv, sr, si) for r in range(P)]
    pieces = [[chunks[r][int(cuts[r][d]):int(cuts[r][d + 1])] for r in range(P)] for d in range(P)]
    dest = [np.sort(np.concatenate(p)) for p in pieces]
    out = np.concatenate(dest)
    assert np.array_equal(out, np.sort(np.concatenate(chunks)))
    # ranges are ordered: max of rank d <= min of rank d+1
    for d in range(P - 1):
        if dest[d].size and dest[d + 1].size:
            assert dest[d][-1] <= dest[d + 1][0]
    sizes = [x.size for x in dest]
    assert max(sizes) <= 1.2 * (P * n) / P, sizes  # the duplicate is split across ranks


def test_write_text(dsort_mod, tmp_path, oracle):
    a = np.array([3, -1, 2147483647, -2147483648, 0], np.int32)
    p = tmp_path / "output.txt"
    dsort_mod.write_text_i32(str(p), a)
    assert p.read_bytes() == oracle.format(a)


def test_sort_stages(dsort_mod):
    """Kill points of a sort (DSORT_OPT_KILL_AFTER_STAGE) under the default options, no GPU needed:
    the bucketed path (>= 2^25 keys) has three, the merge path one per pass plus the tile sort."""
    lib = dsort_mod.load()

    def stages(n, w):
        m = ctypes.c_int()
        assert lib.dsort_sort_stages(None, n, w, ctypes.byref(m)) == 0
        return m.value

    assert stages(0, 4) == 0 and stages(1, 8) == 0
    assert stages(1 << 30, 4) == 3 and stages(1 << 29, 4) == 3 and stages(1 << 25, 8) == 3
    assert stages(8192, 4) == 1                    # one tile (8192 int32 keys): the tile sort only
    assert stages(16384, 4) == 2                   # two tiles: + one merge pass
    assert stages(1 << 20, 4) == 3                 # 128 tiles: tile sort + 2 merge passes (F <= 16)
    assert stages((1 << 25) - 1, 4) == 1 + 3       # 4096 tiles: 12 bits in 3 passes
    # the tile is 8192 keys for both widths (dsort_wave.hip: TILE_OF<T> = WK * WG<T>::WAVES)
    for w in (8, 4):
        assert stages(8192, w) == 1
        assert stages(8193, w) == 2
        assert stages(16 * 8192, w) == 2           # 16 tiles: one pass of fan-in 16
        assert stages(16 * 8192 + 1, w) == 3
        assert stages(256 * 8192 + 1, w) == 4
    m = ctypes.c_int()
    assert lib.dsort_sort_stages(None, 100, 2, ctypes.byref(m)) == -1

    def ss_stages(n, p, r=0, w=4):
        m = ctypes.c_int()
        assert lib.dsort_sample_sort_stages(None, n, p, r, w, ctypes.byref(m)) == 0
        return m.value

    # the bucket exchange from 2^22 keys per rank: three stages; below, the local sort's
    assert ss_stages(1 << 32, 8) == 3 and ss_stages(3 << 22, 3, 2) == 3 and ss_stages(1 << 30, 1) == 3
    assert ss_stages(1 << 20, 4) == stages(1 << 18, 4)
    assert lib.dsort_sample_sort_stages(None, 100, 2, 2, 4, ctypes.byref(m)) == -1


def test_gpu_merge_tables_and_generators(dsort_mod):
    """The expectations of tests/test_gpu_merge.py, checked before they reach the GPU: its constants
    hang together, every generated run is ascending and of the asked length, the duplicate-heavy
    kinds hold the shares they claim, and its pass and level formulas agree with
    dsort_sort_stages(NULL, ...) under the default options."""
    import test_gpu_merge as gm

    lib = dsort_mod.load()

    def stages(n, w):
        m = ctypes.c_int()
        assert lib.dsort_sort_stages(None, n, w, ctypes.byref(m)) == 0
        return m.value

    assert gm.TILE == {4: 8192, 8: 8192} and gm.MT == {4: 16384, 8: 8192}
    assert gm.SLACK == {4: 512, 8: 256} and gm.TNOM == {4: 15360, 8: 7680}
    assert gm.MAXF == {4: 32, 8: 16} and gm.KPC == {4: 4, 8: 2} and gm.WK == 1024
    for w in (4, 8):
        # the pass formula, at the sweep's sizes, the view sizes and the pass boundaries
        sizes = [(t - 1) * gm.TILE[w] + r for t in gm.SWEEP_TILES for r in gm.SWEEP_REM] + gm.VIEW_SIZES
        sizes += [gm.TILE[w], gm.TILE[w] + 1, 16 * gm.TILE[w], 16 * gm.TILE[w] + 1, 256 * gm.TILE[w] + 1]
        for n in sizes:
            tiles = -(-n // gm.TILE[w])
            assert stages(n, w) == 1 + gm.sort_passes(tiles, w), (n, w)
            assert gm.sort_passes(tiles, w) == gm.sort_passes(tiles, w, 4)  # the default cap is 4
        assert gm.sort_passes(33, w, 1) == 6 and gm.sort_passes(32, w, 1) == 5
        assert gm.sort_passes(33, w, 5) == 2 and gm.sort_passes(32, w, 5) == (1 if w == 4 else 2)  # int64: 5 acts as 4
        # the level formula: a sort of k tiles under the default cap merges 16 runs per pass
        for k in sorted(set(gm.K_VALUES[4] + gm.K_VALUES[8] + [255, 4096, 4097])):
            if k * gm.TILE[w] < (1 << 25):
                assert stages(k * gm.TILE[w], w) == (1 + gm.merge_levels(k, 16) if k > 1 else 1), (k, w)
    assert [gm.merge_levels(k, 32) for k in (1, 2, 32, 33, 1024, 1025)] == [0, 1, 1, 2, 2, 3]
    assert [gm.merge_levels(k, 16) for k in (1, 2, 16, 17, 256, 257)] == [0, 1, 1, 2, 2, 3]

    for w in (4, 8):
        info = np.iinfo(gm.DTYPE[w])
        assert len(gm.merge_cases(w)) == len(set(gm.merge_cases(w)))
        for k in gm.K_VALUES[w]:
            for family in gm.families_of(k):
                variants = gm.run_lengths(family, k, w)
                assert variants == gm.run_lengths(family, k, w)  # the same in every process
                for lens in variants:
                    assert len(lens) == k and min(lens) >= 0 and sum(lens) > 0
                    assert max(lens) <= (5 * gm.TNOM[w] + 333 if k < gm.BIG_K else 200)  # small shapes only
                if family == "empties" and k >= 3:
                    assert len(variants) == 3 and all(0 in v for v in variants)
                    assert sum(1 for x in variants[2] if x) == 1
                if family == "one_long":
                    assert [v.index(5 * gm.TNOM[w] + 333) for v in variants] == sorted({0, k // 2, k - 1})
                if family == "chunk":
                    assert set(variants[0]) <= {gm.KPC[w] - 1, gm.KPC[w], gm.KPC[w] + 1}
        # the kinds, on a shape with short and long runs and an empty one
        lens = [0, 1, 5000, 3, 2 * gm.MT[w] + 1, 700, 0, 4000]
        n = sum(lens)
        for kind in gm.KINDS[w]:
            runs = gm.merge_runs(kind, lens, w)
            assert [r.size for r in runs] == lens and all(r.dtype == gm.DTYPE[w] for r in runs)
            assert all((r[1:] >= r[:-1]).all() for r in runs), kind
            cat = np.concatenate(runs)
            vals, counts = np.unique(cat, return_counts=True)
            if kind == "all_equal":
                assert vals.size == 1
            elif kind == "two_values":
                assert vals.size == 2 and counts.min() > n // 3
            elif kind in ("stairs_up", "stairs_down"):
                assert all(np.unique(r).size == 1 for r in runs if r.size) and vals.size == 6
            elif kind == "dups":
                assert vals.min() >= -50 and vals.max() < 50 and counts.min() > n // 200
            elif kind == "zipf":
                assert counts.max() > n // 5
            elif kind == "limits":
                assert vals[0] == info.min and vals[-1] == info.max
                assert 0.3 < counts[0] / n < 0.37 and 0.3 < counts[-1] / n < 0.37
            elif kind == "low_half":
                assert ((cat >> 32) == -0x1234).all() and vals.size > 0.99 * n
                assert 0.7 < ((cat >> 31) & 1).mean() < 0.8  # bit 31 forced on half, random on the rest
            elif kind == "high_half":
                assert ((cat & 0xFFFFFFFF) == 0x89ABCDEF).all() and vals.size > 0.99 * n
            else:
                assert kind == "uniform" and vals.size > 0.99 * n
    for w in (4, 8):
        for kind in gm.SWEEP_KINDS:
            a = gm.sort_keys(kind, 20001, w)
            assert a.dtype == gm.DTYPE[w] and a.size == 20001
            if kind != "uniform":
                assert a.min() == np.iinfo(a.dtype).min and a.max() == np.iinfo(a.dtype).max
            if kind == "few":
                assert np.unique(a).size == 5
