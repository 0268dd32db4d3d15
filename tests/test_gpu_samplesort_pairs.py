"""The pair sample sort (dsort.h, ABI 8): dsort_sample_argsort_dev_i32 and
dsort_sample_sort_pairs_dev_i32 with several ranks.  As in test_gpu_multirank.py the ranks are child
processes that share cuda:0 and exchange over the host transport (gloo), the RCCL exchange runs
with one rank.  Every expectation comes from numpy on the concatenated inputs -- np.sort and the
stable np.argsort plus the base for the argsort, np.lexsort on (unsigned value, key) for pairs -- and
is compared element for element with the concatenated rank slices."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "tests", "mp_samplesort_pairs.py")
MERGE_N = 3_000_017  # below 2^22 keys per rank: sort, exchange, merge the received runs


def bx_n(world):  # from 2^22 keys per rank: the bucket exchange
    return world * (1 << 22) + 12_345


def run_ranks(tmp_path, world, steps, transport="host", opts=None, expect_fail=False):
    """Runs the driver's steps on `world` ranks.  Returns the ranks' JSON reports and, per step, a
    dict: keys / vals = the concatenated inputs, okeys / ovals = the ranks' output slices."""
    store = str(tmp_path / "store")  # (a file rendezvous: no port to lose)
    out = str(tmp_path / "sp")
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
    for j, (call, _, _) in enumerate(steps):
        d = {"keys": np.concatenate(load(j, "keys")), "okeys": load(j, "okeys")}
        if call != "keys":
            d["ovals"] = load(j, "ovals")
        if call == "pairs":
            d["vals"] = np.concatenate(load(j, "vals"))
        res.append(d)
    return meta, res


def check_argsort(d, n, base=0):
    keys = d["keys"]
    assert keys.size == n
    order = np.argsort(keys, kind="stable")
    sizes = [k.size for k in d["okeys"]]
    assert sizes == [v.size for v in d["ovals"]] and sum(sizes) == n, sizes
    assert np.array_equal(np.concatenate(d["okeys"]), np.sort(keys))
    want = ((order.astype(np.uint64) + np.uint64(base)) & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    assert np.array_equal(np.concatenate(d["ovals"]).view(np.uint32), want)
    return sizes


def check_pairs(d, n):
    keys, vals = d["keys"], d["vals"]
    assert keys.size == n and vals.size == n
    order = np.lexsort((vals.view(np.uint32), keys))
    sizes = [k.size for k in d["okeys"]]
    assert sizes == [v.size for v in d["ovals"]] and sum(sizes) == n, sizes
    assert np.array_equal(np.concatenate(d["okeys"]), keys[order])
    assert np.array_equal(np.concatenate(d["ovals"]), vals[order])
    return sizes


def paths(meta, j=0):
    return [m["steps"][j]["stats"]["exchange_path"] for m in meta]


def balanced(sizes, n, world):  # (the bound of test_sample_sort_ranks_share_gpu for this sampler)
    assert max(sizes) <= 1.25 * n / world + 1024, sizes


@pytest.mark.parametrize("world", [1, 2, 4])
def test_argsort_merge_path(tmp_path, world):
    n = MERGE_N
    meta, (d,) = run_ranks(tmp_path, world, [["argsort", n, "uniform"]])
    sizes = check_argsort(d, n)
    if world >= 2:
        assert paths(meta) == [2] * world
    balanced(sizes, n, world)


@pytest.mark.parametrize("world,dist", [(2, "uniform"), (3, "uniform"), (3, "few"), (2, "equal"), (3, "ref100")])
def test_argsort_bucket_exchange(tmp_path, world, dist):
    """The packed words through the bucket exchange, with the wave fence on.  All keys equal is a
    globally sorted run of distinct words: the heavy key splits between the ranks by position."""
    n = bx_n(world)
    meta, (d,) = run_ranks(tmp_path, world, [["argsort", n, dist]], opts={"all": {"test_wave_fence": 1}})
    assert paths(meta) == [1] * world
    fr = [m["steps"][0]["stats"]["fence_ranges"] for m in meta]
    assert all(f >= 1 for f in fr), fr
    sizes = check_argsort(d, n)
    if dist in ("uniform", "equal"):
        balanced(sizes, n, world)


@pytest.mark.parametrize("n,path", [(MERGE_N, 2), (bx_n(3), 1)])
def test_pairs_with_identical_words(tmp_path, n, path):
    """8 distinct keys, values {0, 1, 0x80000000, 0xFFFFFFFF}: 32 distinct packed words, so the
    splitters of the bucket exchange fall between identical words (pure buckets), and the values
    order as unsigned."""
    meta, (d,) = run_ranks(tmp_path, 3, [["pairs", n, "few"]], opts={"vals": "quad", "all": {"test_wave_fence": 1}})
    assert paths(meta) == [path] * 3
    check_pairs(d, n)


@pytest.mark.parametrize("call", ["argsort", "pairs"])
@pytest.mark.parametrize("world,n", [(4, 3), (2, 1)])
def test_tiny_and_empty_ranks(tmp_path, world, n, call):
    meta, (d,) = run_ranks(tmp_path, world, [[call, n, "uniform"]], opts={"vals": "rand"})
    assert meta[-1]["steps"][0]["n_in"] == 0  # (the last rank holds no key and still joins)
    (check_argsort if call == "argsort" else check_pairs)(d, n)


def test_one_rccl_rank_equals_the_local_argsort(tmp_path):
    n = 1_000_003
    meta, (d,) = run_ranks(tmp_path, 1, [["argsort", n, "uniform"]], transport="rccl", opts={"local_argsort": 1})
    check_argsort(d, n)
    out = str(tmp_path / "sp")
    assert np.array_equal(d["okeys"][0], np.load(out + ".s0.lkeys0.npy"))
    assert np.array_equal(d["ovals"][0], np.load(out + ".s0.lidx0.npy"))


def test_positions_above_2_31(tmp_path):
    """The global range ends exactly at 2^32: indices compare as uint32.  One position more is
    DSORT_EINVAL on every rank, before any collective, and the context sorts afterwards."""
    n = 100_003
    base = 2 ** 32 - n
    meta, (d,) = run_ranks(tmp_path, 2, [["argsort", n, "uniform"]], opts={"base": base, "probe_einval": 1})
    assert [m["einval_rc"] for m in meta] == [-1, -1], meta
    assert meta[1]["steps"][0]["first"] + meta[1]["steps"][0]["n_in"] == 2 ** 32
    check_argsort(d, n, base)
    assert int(np.concatenate(d["ovals"]).view(np.uint32).max()) == 2 ** 32 - 1


@pytest.mark.parametrize("call", ["argsort", "pairs"])
@pytest.mark.parametrize("world", [1, 2])
def test_input_views(tmp_path, world, call):
    """Keys and values that start at element 1 of their allocation (4-byte aligned only), n % 256
    and a slice length % 4 non-zero (n is odd: with two ranks one slice is); inputs unchanged."""
    n = 100_003
    assert n % 256 and n % 4
    meta, (d,) = run_ranks(tmp_path, world, [[call, n, "uniform"]], opts={"view": 1, "vals": "rand"})
    sizes = (check_argsort if call == "argsort" else check_pairs)(d, n)
    assert any(s % 4 for s in sizes), sizes
    assert all(m["steps"][0]["inputs_unchanged"] for m in meta)


def test_context_reuse(tmp_path):
    """One context: a large pairs sample sort (bucket exchange), a smaller one (merge path; the
    arenas keep their size), then the keys-only sample sort."""
    big, small, bare = bx_n(2), 1_000_003, 500_009
    meta, (d0, d1, d2) = run_ranks(tmp_path, 2, [["pairs", big, "uniform"], ["pairs", small, "ref100"],
                                                 ["keys", bare, "uniform"]], opts={"vals": "rand"})
    assert paths(meta, 0) == [1, 1] and paths(meta, 1) == [2, 2]
    check_pairs(d0, big)
    check_pairs(d1, small)
    assert np.array_equal(np.concatenate(d2["okeys"]), np.sort(d2["keys"]))


def test_local_failure_fails_every_rank(tmp_path):
    """Rank 1 fails locally right before the key all-to-all of the bucket exchange's first wave
    (DSORT_OPT_TEST_FAIL_EXCHANGE = 3) inside the argsort: the status gates of the host transport
    work through the new entry as through dsort_sample_sort_dev_i64."""
    res = run_ranks(tmp_path, 3, [["argsort", bx_n(3), "uniform"]],
                    opts={"rank_opts": {"1": {"test_fail_exchange": 3}}}, expect_fail=True)
    assert res[1]["rc"] == -3 and "DSORT_OPT_TEST_FAIL_EXCHANGE" in res[1]["error"], res[1]
    for r in (0, 2):
        assert res[r]["rc"] == -4 and "rank 1 failed locally" in res[r]["error"], res[r]
    assert max(r["s"] for r in res) < 30, res
