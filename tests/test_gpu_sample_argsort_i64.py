"""The int64 argsort across ranks (dsort_sample_argsort_dev_i64) and the record sort on top of it.  As
in test_gpu_samplesort_pairs.py the ranks are child processes that share cuda:0 and exchange over the
host transport (gloo); the RCCL exchange runs with one rank.  Every expectation is numpy's stable
argsort of the concatenated inputs, plus the base, compared element for element with the concatenated
rank slices."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "tests", "mp_sample_argsort_i64.py")
MERGE_N = 3_000_017  # below 2^22 keys per rank: sort, exchange, merge the received runs
SMALL_N = 100_003
EINVAL, EHIP, ECOMM, ESTAGE = -1, -3, -4, -7
WIDE_ON = {"all": {"argsort_wide": 1}}


def bx_n(world):  # from 2^22 keys per rank: the bucket exchange
    return world * (1 << 22) + 12_345


def run_ranks(tmp_path, world, steps, transport="host", opts=None, expect_fail=False, tag="sa"):
    """Runs the driver's steps on `world` ranks.  Returns the ranks' JSON reports and, per step that
    produced output, a dict: keys = the concatenated inputs, okeys / ovals (/ orows, g8, g4) = the
    ranks' output slices."""
    store = str(tmp_path / (tag + ".store"))  # (a file rendezvous: no port to lose)
    out = str(tmp_path / tag)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    o = dict(opts or {}, steps=steps)
    procs = [subprocess.Popen([sys.executable, DRIVER, str(r), str(world), store, out, transport, json.dumps(o)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = []
    for p in procs:
        try:
            lg, _ = p.communicate(timeout=150)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            tails = list(logs)
            for q in procs[len(logs):]:
                try:
                    tails.append(q.communicate(timeout=10)[0].decode(errors="replace"))
                except (subprocess.TimeoutExpired, ValueError, OSError):
                    tails.append("(no output)")
            pytest.fail("ranks timed out; their last output:\n" + "\n---\n".join(t[-600:] for t in tails))
        logs.append(lg.decode(errors="replace"))
    for p, lg in zip(procs, logs):
        assert p.returncode == 0, lg[-3000:]
    meta = [json.load(open(out + f".rank{r}.json")) for r in range(world)]
    if expect_fail:
        return meta

    def load(j, what):
        return [np.load(out + f".s{j}.{what}{r}.npy") for r in range(world)]

    res = []
    for j, st in enumerate(steps):
        if "n_out" not in meta[0]["steps"][j]:  # (a step that failed on purpose, "keep_going")
            res.append(None)
            continue
        d = {"keys": np.concatenate(load(j, "keys")), "okeys": load(j, "okeys")}
        if st[0] not in ("keys", "records"):
            d["ovals"] = load(j, "ovals")
        if st[0] == "records":
            d["orows"] = load(j, "orows")
        if st[0] == "hold":
            d["g8"], d["g4"] = load(j, "g8"), load(j, "g4")
        res.append(d)
    return meta, res


def check_argsort(d, n, base=0, dtype=np.int64):
    keys = d["keys"]
    assert keys.size == n and keys.dtype == dtype
    order = np.argsort(keys, kind="stable")
    sizes = [k.size for k in d["okeys"]]
    assert sizes == [v.size for v in d["ovals"]] and sum(sizes) == n, sizes
    got = np.concatenate(d["okeys"])
    assert got.dtype == dtype and np.array_equal(got, keys[order])
    want = ((order.astype(np.uint64) + np.uint64(base)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert np.array_equal(np.concatenate(d["ovals"]).view(np.uint32), want)
    return sizes


def rule_passes(keys, base, forced=False):
    """dsort.h's rule in Python integers: b from E = the end of the global range."""
    if keys.size == 0:
        return 0
    if forced:
        return 2
    E = base + keys.size
    b = 1 if E <= 2 else (E - 1).bit_length()
    return 1 if (int(keys.max()) - int(keys.min())) >> (64 - b) == 0 else 2


def passes(meta, j=0):
    return [m["steps"][j]["stats"]["argsort_passes"] for m in meta]


def paths(meta, j=0):
    return [m["steps"][j]["stats"]["exchange_path"] for m in meta]


def balanced(sizes, n, world):  # (the bound of test_sample_sort_ranks_share_gpu for this sampler)
    assert max(sizes) <= 1.25 * n / world + 1024, sizes


@pytest.mark.parametrize("dist,want", [("narrow", 1), ("wide", 2)])
@pytest.mark.parametrize("world", [1, 2, 4])
def test_merge_path(tmp_path, world, dist, want):
    n = MERGE_N
    meta, (d,) = run_ranks(tmp_path, world, [["argsort", n, dist]])
    sizes = check_argsort(d, n)
    assert rule_passes(d["keys"], 0) == want and passes(meta) == [want] * world
    if world >= 2:
        assert paths(meta) == [2] * world
    balanced(sizes, n, world)


@pytest.mark.parametrize("dist,want", [("narrow", 1), ("few", 1), ("equal", 1), ("wide", 2), ("zipf", 2), ("five", 2)])
@pytest.mark.parametrize("world", [2, 3])
def test_bucket_exchange(tmp_path, world, dist, want):
    """Both paths through the bucket exchange, with the wave fence on.  All keys equal is a globally
    sorted run of distinct words: the heavy key splits between the ranks by position."""
    n = bx_n(world)
    meta, (d,) = run_ranks(tmp_path, world, [["argsort", n, dist]], opts={"all": {"test_wave_fence": 1}})
    assert paths(meta) == [1] * world
    assert all(m["steps"][0]["stats"]["fence_ranges"] >= 1 for m in meta)
    sizes = check_argsort(d, n)
    assert rule_passes(d["keys"], 0) == want and passes(meta) == [want] * world
    if dist in ("narrow", "wide", "equal"):
        balanced(sizes, n, world)


@pytest.mark.parametrize("dist", ["hi_const", "lo_const", "narrow"])
def test_wide_forced_equals_the_automatic_run(tmp_path, dist):
    """Keys the rule sends down the narrow path, forced through the two passes: the low halves order
    as unsigned (neighbours across bit 31), the high halves as signed, bit for bit the same result."""
    n = SMALL_N
    meta, (d,) = run_ranks(tmp_path, 3, [["argsort", n, dist]], tag="auto")
    metaw, (dw,) = run_ranks(tmp_path, 3, [["argsort", n, dist]], opts=WIDE_ON, tag="wide")
    assert passes(meta) == [1] * 3 and passes(metaw) == [2] * 3
    check_argsort(d, n)
    check_argsort(dw, n)
    for what in ("okeys", "ovals"):
        assert np.array_equal(np.concatenate(d[what]), np.concatenate(dw[what]))
    k = d["keys"]
    if dist == "hi_const":
        assert ((k & 0xFFFFFFFF) < 2 ** 31).any() and ((k & 0xFFFFFFFF) >= 2 ** 31).any()
    if dist == "lo_const":
        assert (k < 0).any() and (k > 0).any() and ((k & 0xFFFFFFFF) == 0x89ABCDEF).all()


@pytest.mark.parametrize("span,want", [(2 ** 32 - 1, 1), (2 ** 32, 2)])
def test_boundary_with_b_from_the_end_of_the_range(tmp_path, span, want):
    """The global range ends exactly at 2^32, so b = 32 although the keys number 100 003: a key range of
    2^32 - 1 still fits one pass, 2^32 needs two; the minimum sits on rank 0, the maximum on rank 1.
    One position more is DSORT_EINVAL on every rank before any collective."""
    n = SMALL_N
    base = 2 ** 32 - n
    meta, (d,) = run_ranks(tmp_path, 2, [["argsort", n, f"span:{span}"]], opts={"base": base, "probe_einval": 1})
    assert [m["einval_rc"] for m in meta] == [EINVAL, EINVAL], meta
    k = d["keys"]
    half = meta[0]["steps"][0]["n_in"]
    assert int(k.max()) - int(k.min()) == span and int(k[:half].min()) == int(k.min()) and int(k[half:].max()) == int(k.max())
    assert int(k[:half].max()) < int(k.max()) and int(k[half:].min()) > int(k.min())
    assert rule_passes(k, base) == want and passes(meta) == [want] * 2
    assert rule_passes(k, 0) == 1  # (b from the key count would have said one pass for both)
    check_argsort(d, n, base)
    assert int(np.concatenate(d["ovals"]).view(np.uint32).max()) == 2 ** 32 - 1


@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("world,n", [(4, 3), (2, 1), (2, 0)])
def test_tiny_and_empty(tmp_path, world, n, forced):
    meta, (d,) = run_ranks(tmp_path, world, [["argsort", n, "wide"]], opts=WIDE_ON if forced else None)
    assert meta[-1]["steps"][0]["n_in"] == 0  # (the last rank holds no key and still joins)
    check_argsort(d, n)
    assert passes(meta) == [rule_passes(d["keys"], 0, forced)] * world
    if n == 0:
        assert passes(meta) == [0] * world


@pytest.mark.parametrize("dist", ["narrow", "wide"])
@pytest.mark.parametrize("world", [1, 2])
def test_input_views(tmp_path, world, dist):
    """Keys that start at element 1 of their allocation (8 mod 16), n % 256 non-zero; inputs unchanged."""
    n = SMALL_N
    assert n % 256 and (n // 2) % 256
    meta, (d,) = run_ranks(tmp_path, world, [["argsort", n, dist]], opts={"view": 1})
    check_argsort(d, n)
    assert all(m["steps"][0]["inputs_unchanged"] for m in meta)


@pytest.mark.parametrize("dist", ["narrow", "wide"])
def test_one_rccl_rank_equals_the_local_argsort(tmp_path, dist):
    n = 1_000_003
    meta, (d,) = run_ranks(tmp_path, 1, [["argsort", n, dist]], transport="rccl", opts={"local_argsort": 1})
    check_argsort(d, n)
    assert passes(meta) == [1 if dist == "narrow" else 2]
    out = str(tmp_path / "sa")
    assert np.array_equal(d["okeys"][0], np.load(out + ".s0.lkeys0.npy"))
    assert np.array_equal(d["ovals"][0], np.load(out + ".s0.lidx0.npy"))


def test_sample_sort_records(tmp_path):
    """int64 keys in [1, 100] with 16-byte rows: row i = (position, ~position)."""
    n = SMALL_N
    meta, (d,) = run_ranks(tmp_path, 3, [["records", n, "ref100"]])
    order = np.argsort(d["keys"], kind="stable")
    assert np.array_equal(np.concatenate(d["okeys"]), d["keys"][order])
    rows = np.stack((order.astype(np.int64), ~order.astype(np.int64)), axis=1)
    got = np.concatenate(d["orows"])
    assert got.shape == (n, 2) and np.array_equal(got, rows)


def test_symmetric_errors_leave_the_communicator_usable(tmp_path):
    """Ranks that disagree on DSORT_OPT_ARGSORT_WIDE, then overlapping ranges: DSORT_EINVAL on every
    rank from the same call; a good call follows each on the same communicator."""
    n = SMALL_N
    steps = [["argsort", n, "narrow", {"rank_opts": {"1": {"argsort_wide": 1}}}], ["argsort", n, "narrow"],
             ["overlap", n, "wide"], ["argsort", n, "wide"]]
    meta, res = run_ranks(tmp_path, 3, steps, opts={"keep_going": 1})
    for m in meta:
        assert [s["rc"] for s in m["steps"]] == [EINVAL, 0, EINVAL, 0], m
        assert "disagree on DSORT_OPT_ARGSORT_WIDE" in m["steps"][0]["error"]
        assert "overlap" in m["steps"][2]["error"]
    assert res[0] is None and res[2] is None
    check_argsort(res[1], n)
    check_argsort(res[3], n)
    assert passes(meta, 1) == [1] * 3 and passes(meta, 3) == [2] * 3


@pytest.mark.parametrize("opt", [{"test_fail_exchange": 3}, {"test_fail_leg": 3}, {"test_fail_leg": 5}])
def test_local_failure_fails_every_rank(tmp_path, opt):
    """Rank 1 fails locally on the wide path -- inside the first sort (right before its key all-to-all),
    or between two legs (before the key gather, before the final gather): it returns DSORT_EHIP, its
    peers DSORT_ECOMM naming it at their next gate, nobody blocks."""
    res = run_ranks(tmp_path, 3, [["argsort", SMALL_N, "wide"]], opts={"rank_opts": {"1": opt}}, expect_fail=True)
    name = "DSORT_OPT_TEST_FAIL_EXCHANGE" if "test_fail_exchange" in opt else "DSORT_OPT_TEST_FAIL_LEG"
    assert res[1]["rc"] == EHIP and name in res[1]["error"], res[1]
    for r in (0, 2):
        assert res[r]["rc"] == ECOMM and "rank 1 failed locally" in res[r]["error"], res[r]
    assert max(r["s"] for r in res) < 30, res


def test_failure_leg_the_call_never_reaches_is_ignored(tmp_path):
    n = SMALL_N
    meta, (d,) = run_ranks(tmp_path, 2, [["argsort", n, "narrow"]], opts={"rank_opts": {"1": {"test_fail_leg": 3}}})
    check_argsort(d, n)
    assert passes(meta) == [1, 1]


def test_kill_stage_beyond_the_first_sort(tmp_path):
    """Rank 1 with a kill stage its first sort never reaches, on the wide path: it goes through every
    leg with its peers and returns DSORT_ESTAGE with a valid slice; the peers return 0."""
    n = SMALL_N
    meta, (d,) = run_ranks(tmp_path, 3, [["argsort", n, "wide"]], opts={"rank_opts": {"1": {"kill_after_stage": 50}}})
    assert [m["steps"][0]["rc"] for m in meta] == [0, ESTAGE, 0], meta
    assert "every leg has run" in meta[1]["estage_error"]
    check_argsort(d, n)
    assert passes(meta) == [2] * 3


def test_one_context_through_a_sequence_of_calls(tmp_path):
    """A wide bucket-exchange call, a small narrow one (the arenas keep their size), the int32 sample
    argsort, a keys-only sample sort, then an int64 argsort whose context-owned index slice feeds two
    gathers and is read only after both."""
    big, small = bx_n(2), SMALL_N
    steps = [["argsort", big, "wide"], ["argsort", small, "narrow"], ["argsort32", small, "uniform"],
             ["keys", small, "uniform"], ["hold", small, "wide"]]
    meta, (d0, d1, d2, d3, d4) = run_ranks(tmp_path, 2, steps)
    assert paths(meta, 0) == [1, 1] and passes(meta, 0) == [2, 2] and passes(meta, 1) == [1, 1]
    check_argsort(d0, big)
    check_argsort(d1, small)
    check_argsort(d2, small, dtype=np.int32)
    assert np.array_equal(np.concatenate(d3["okeys"]), np.sort(d3["keys"]))
    check_argsort(d4, small)  # (the slices as they were AFTER the two gathers)
    order = np.argsort(d4["keys"], kind="stable")
    assert np.array_equal(np.concatenate(d4["g8"]), d4["keys"][order])
    assert np.array_equal(np.concatenate(d4["g4"]).view(np.uint32), order.astype(np.uint32))
