"""The distributed record gather (dsort.h, ABI 9): dsort_sample_gather_dev with several ranks.  As in
test_gpu_samplesort_pairs.py the ranks are child processes that share cuda:0 and exchange over the
host transport (gloo); the RCCL exchange runs with one rank.  Every expectation is numpy on the
concatenated inputs, all_records[all_idx], compared element for element.  One spawn runs a list of
steps on one context (tests/mp_sample_gather.py)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "tests", "mp_sample_gather.py")


def run_ranks(tmp_path, world, steps, transport="host", opts=None):
    """Runs the driver's steps on `world` ranks; returns the ranks' JSON reports and the prefix of the
    files they saved."""
    store = str(tmp_path / "store")  # (a file rendezvous: no port to lose)
    out = str(tmp_path / "sg")
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
    return [json.load(open(out + f".rank{r}.json")) for r in range(world)], out


def load(out, j, what, world):
    return [np.load(out + f".s{j}.{what}{r}.npy") for r in range(world)]


def check_gather(meta, out, j, want_n_idx=None):
    """Step j of every rank against numpy: the records in global order, indexed by each rank's
    indices.  Returns the steps' reports."""
    world = len(meta)
    st = [m["steps"][j] for m in meta]
    assert all(s["rc"] == 0 for s in st), st
    rec, idx, got = (load(out, j, w, world) for w in ("rec", "idx", "out"))
    order = sorted(range(world), key=lambda r: st[r]["first"])
    held = [r for r in order if st[r]["n_src"]]
    start = st[held[0]]["first"]
    pos = start
    for r in held:  # (the ranges tile the global range, whatever the rank order)
        assert st[r]["first"] == pos, st
        pos += st[r]["n_src"]
    all_rec = np.concatenate([rec[r] for r in held])
    for r in range(world):
        assert idx[r].size == st[r]["n_idx"] == got[r].shape[0]
        if want_n_idx is not None:
            assert idx[r].size == want_n_idx[r]
        want = all_rec[idx[r].astype(np.int64) - start]
        assert got[r].shape == want.shape, (got[r].shape, want.shape)
        assert np.array_equal(got[r], want), f"rank {r}: {int((got[r] != want).any(axis=1).sum())} records differ"
        assert st[r]["inputs_unchanged"] and st[r]["sentinels_ok"], st[r]
    assert sum(s["gather_served"] for s in st) == sum(s["n_idx"] for s in st)
    return st


def split(n, world):
    return [n // world + (1 if r < n % world else 0) for r in range(world)]


@pytest.mark.parametrize("world", [1, 2, 3])
def test_widths_and_tails(tmp_path, world):
    """Records of 4, 8 and 16 bytes; 100 003 indices in all (odd: some rank's count is non-zero
    modulo 4); records, indices and the output start at element 1 of their allocation; the sentinels
    around the output and the inputs are unchanged."""
    n_idx = split(100_003, world)
    assert any(n % 4 for n in n_idx)
    n_src = [[40_001], [25_001, 15_000], [9_001, 20_000, 11_000]][world - 1]
    steps = [{"op": "gather", "w": w, "n_src": n_src, "n_idx": n_idx, "idx": "rand"} for w in (4, 8, 16)]
    meta, out = run_ranks(tmp_path, world, steps, opts={"view": 1})
    for j in range(3):
        check_gather(meta, out, j, n_idx)


def test_more_than_one_pass_of_the_grid(tmp_path):
    n = 1_000_003
    meta, out = run_ranks(tmp_path, 2, [{"op": "gather", "w": 16, "n_src": [300_001, 200_000], "n_idx": [n, n],
                                        "idx": "rand"}])
    st = check_gather(meta, out, 0, [n, n])
    assert all(s["gather_sent"] > 0 for s in st), st
    assert sum(s["gather_served"] for s in st) == 2 * n


def test_index_shapes(tmp_path):
    """World 4: a random permutation, every index naming rank 2's range, one index repeated, every
    rank asking for its own records only, the identity."""
    n_src = [5000, 3001, 7002, 1000]
    whole, some = [4000, 4001, 4002, 4000], [3001, 2000, 1003, 4000]
    assert sum(whole) == sum(n_src)
    steps = [{"op": "gather", "w": 8, "n_src": n_src, "n_idx": n, "idx": k}
             for k, n in (("perm", whole), ("owner2", some), ("same", some), ("own", some), ("identity", whole))]
    meta, out = run_ranks(tmp_path, 4, steps)
    sts = [check_gather(meta, out, j) for j in range(5)]
    perm = np.concatenate(load(out, 0, "idx", 4))
    assert np.array_equal(np.sort(perm), np.arange(sum(n_src)))
    assert [s["gather_served"] for s in sts[1]] == [0, 0, sum(some), 0]
    assert len(set(np.concatenate(load(out, 2, "idx", 4)).tolist())) == 1
    assert [s["gather_sent"] for s in sts[3]] == [0, 0, 0, 0]
    assert [s["gather_served"] for s in sts[3]] == some
    assert np.array_equal(np.concatenate(load(out, 4, "idx", 4)), np.arange(sum(n_src)))


def test_range_shapes(tmp_path):
    """Rank r owns chunk P-1-r (`first` descends with the rank), uneven ranges, one rank without
    records and one without indices."""
    steps = [{"op": "gather", "w": 16, "order": "desc", "n_src": [4001, 0, 1234, 777], "n_idx": [1000, 2001, 0, 3],
              "idx": "rand"},
             {"op": "gather", "w": 4, "order": "desc", "n_src": [0, 0, 0, 9], "n_idx": [0, 7, 1, 0], "idx": "rand"}]
    meta, out = run_ranks(tmp_path, 4, steps)
    st = check_gather(meta, out, 0)
    assert [s["first"] for s in st] == [2011, 2011, 777, 0]
    assert [s["gather_served"] for s in st][1] == 0
    check_gather(meta, out, 1)


def test_tiny_and_positions_above_2_31(tmp_path):
    """World 2: 3 records in all; then first + n_src = 2^32 + 1 is DSORT_EINVAL on every rank before
    any collective and the context works afterwards: a global range that ends exactly at 2^32 (the
    owner lookup compares as unsigned)."""
    n_src = [60_001, 40_002]
    base = 2 ** 32 - sum(n_src)
    steps = [{"op": "gather", "w": 16, "n_src": [2, 1], "n_idx": [5, 4], "idx": "rand"},
             {"op": "einval", "n_src": 1000},
             {"op": "gather", "w": 8, "n_src": n_src, "n_idx": [50_001, 50_002], "idx": "rand", "base": base}]
    meta, out = run_ranks(tmp_path, 2, steps)
    check_gather(meta, out, 0)
    assert [m["steps"][1]["rc"] for m in meta] == [-1, -1], meta
    st = check_gather(meta, out, 2)
    assert st[1]["first"] + st[1]["n_src"] == 2 ** 32 and st[0]["first"] > 2 ** 31
    assert int(np.concatenate(load(out, 2, "idx", 2)).max()) > 2 ** 32 - 100


def test_records_follow_their_keys(tmp_path):
    """End to end, world 3: 300 007 keys of [1, 100] (heavy ties) with 16-byte records (key, global
    position, two random words).  The concatenated slices of sample_sort_records_dev are the records
    in stable key order; the argsort's context-owned index array feeds a second gather of an 8-byte
    column and is intact after both."""
    n, world = 300_007, 3
    meta, out = run_ranks(tmp_path, world, [{"op": "records", "n": n}])
    keys = np.concatenate(load(out, 0, "keys", world))
    rec = np.concatenate(load(out, 0, "rec", world))
    assert keys.size == n and np.array_equal(rec[:, 0], keys) and np.array_equal(rec[:, 1], np.arange(n))
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(np.concatenate(load(out, 0, "okeys", world)), keys[order])
    assert np.array_equal(np.concatenate(load(out, 0, "out", world)), rec[order])
    assert np.array_equal(np.concatenate(load(out, 0, "o16", world)), rec[order])
    assert np.array_equal(np.concatenate(load(out, 0, "o8", world)), rec[order][:, 1:3])
    assert np.array_equal(np.concatenate(load(out, 0, "cidx", world)), order.astype(np.int32))
    assert np.array_equal(np.concatenate(load(out, 0, "ckeys", world)), keys[order])
    assert sum(m["steps"][0]["n_out"] for m in meta) == n


def test_one_rccl_rank_equals_the_local_gather(tmp_path):
    n = 1_000_003
    meta, out = run_ranks(tmp_path, 1, [{"op": "gather", "w": 16, "n_src": [n], "n_idx": [n], "idx": "perm",
                                        "local": 1}], transport="rccl")
    st = check_gather(meta, out, 0, [n])
    assert st[0]["gather_sent"] == 0 and st[0]["gather_served"] == n
    assert np.array_equal(np.load(out + ".s0.out0.npy"), np.load(out + ".s0.local0.npy"))


def test_symmetric_argument_errors(tmp_path):
    """World 3: 7 indices of rank 1 that nobody owns; ranks 0 and 1 overlapping by one record; rank
    2 passing another elem_bytes.  Every rank returns DSORT_EINVAL from the same call, and the good
    gather that follows each on the same context succeeds."""
    good = {"op": "gather", "w": 16, "n_src": [3001, 2000, 1002], "n_idx": [2000, 1001, 3000], "idx": "rand"}
    steps = [dict(good, bad_idx={"1": 7}), good, dict(good, first_shift={"1": -1}), good, dict(good, w_of={"2": 8}),
             good]
    meta, out = run_ranks(tmp_path, 3, steps)
    for j in (0, 2, 4):
        assert [m["steps"][j]["rc"] for m in meta] == [-1, -1, -1], [m["steps"][j] for m in meta]
    for m in meta:
        assert "rank 1 holds 7 indices" in m["steps"][0]["error"], m["steps"][0]
        assert "overlap" in m["steps"][2]["error"] and "elem_bytes" in m["steps"][4]["error"]
    for j in (1, 3, 5):
        check_gather(meta, out, j)
    assert sum(sum(s["s"] for s in m["steps"]) for m in meta) < 60


def test_local_failure_fails_every_rank(tmp_path):
    """Rank 1 fails locally right before the request all-to-all (DSORT_OPT_TEST_FAIL_EXCHANGE = 2):
    it returns its own error and its peers leave at the status gate naming it."""
    step = {"op": "gather", "w": 16, "n_src": [3001, 2000, 1002], "n_idx": [2000, 1001, 3000], "idx": "rand",
            "fatal": 1}
    meta, _ = run_ranks(tmp_path, 3, [step], opts={"rank_opts": {"1": {"test_fail_exchange": 2}}})
    res = [m["steps"][0] for m in meta]
    assert res[1]["rc"] == -3 and "DSORT_OPT_TEST_FAIL_EXCHANGE" in res[1]["error"], res[1]
    for r in (0, 2):
        assert res[r]["rc"] == -4 and "rank 1 failed locally" in res[r]["error"], res[r]
    assert max(r["s"] for r in res) < 30, res


def test_context_reuse(tmp_path):
    """One context: a large gather (more indices than one tile per workgroup of the routing grid:
    2048 x 1024), a smaller one (the arenas keep their size), a sample argsort, a gather again."""
    big = 2048 * 1024 + 100_003
    steps = [{"op": "gather", "w": 4, "n_src": [50_001, 70_000], "n_idx": [big, big + 1], "idx": "rand"},
             {"op": "gather", "w": 16, "n_src": [5001, 7000], "n_idx": [3000, 2001], "idx": "rand"},
             {"op": "argsort", "n": 200_003},
             {"op": "gather", "w": 8, "n_src": [7000, 5001], "n_idx": [6000, 6001], "idx": "perm"}]
    meta, out = run_ranks(tmp_path, 2, steps)
    for j in (0, 1, 3):
        check_gather(meta, out, j)
    keys = np.concatenate(load(out, 2, "keys", 2))
    assert np.array_equal(np.concatenate(load(out, 2, "okeys", 2)), np.sort(keys))
    assert np.array_equal(np.concatenate(load(out, 2, "oidx", 2)), np.argsort(keys, kind="stable").astype(np.int32))
