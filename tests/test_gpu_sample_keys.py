"""Typed keys across ranks (dsort.h, "Key types and order"): dsort_sample_sort_dev_keys and
dsort_sample_argsort_dev_keys with several ranks.  As in test_gpu_samplesort_pairs.py the ranks are
child processes that share cuda:0 and exchange over the host transport (gloo), and the RCCL exchange
runs with one rank.  The expectation is the checker of keys_model.py on the concatenated inputs:
the concatenated slices are the keys in the typed order, bit for bit, and the indices are the global
positions of the stable argsort."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import keys_model as km
from conftest import REPO
from mp_sample_keys import sample_keys

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "tests", "mp_sample_keys.py")
STEPS = [["sort", "f32", 1], ["argsort", "f32", 1], ["sort", "f64", 0], ["argsort", "f64", 0]]
RUN_LIMIT_S = 120  # of one run of all ranks; every step inside has the exchange deadline of its own


def run_ranks(tmp_path, lens, steps, transport="host"):
    world = len(lens)
    store = str(tmp_path / "store")
    out = str(tmp_path / "sk")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    o = {"lens": lens, "steps": steps}
    procs = [subprocess.Popen([sys.executable, DRIVER, str(r), str(world), store, out, transport, json.dumps(o)],
                              env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = []
    for p in procs:
        try:
            lg, _ = p.communicate(timeout=RUN_LIMIT_S)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            pytest.fail("ranks timed out; the output so far:\n" + "\n---\n".join(t[-600:] for t in logs))
        logs.append(lg.decode(errors="replace"))
        if p.returncode != 0:  # a failing rank ends the run
            for q in procs:
                q.kill()
            pytest.fail(f"a rank exited with {p.returncode}:\n{logs[-1][-3000:]}")
    meta = [json.load(open(out + f".rank{r}.json")) for r in range(world)]
    for m in meta:
        assert "error" not in m, m
    return meta, out


def check(meta, out, lens, steps):
    world, n = len(lens), sum(lens)
    for j, (call, name, desc) in enumerate(steps):
        x = sample_keys(name, n, j)
        order = km.ref_order(x, name, bool(desc))
        okeys = [np.load(out + f".s{j}.okeys{r}.npy") for r in range(world)]
        assert sum(k.size for k in okeys) == n, [k.size for k in okeys]
        assert np.array_equal(np.concatenate(okeys), km.bits(x[order])), (call, name)
        if call == "argsort":
            oidx = [np.load(out + f".s{j}.oidx{r}.npy") for r in range(world)]
            assert [i.size for i in oidx] == [k.size for k in okeys]
            assert np.array_equal(np.concatenate(oidx).view(np.uint32).astype(np.int64), order), (call, name)
        for r, m in enumerate(meta):
            s = m["steps"][j]
            assert s["n_in"] == lens[r] and s["inputs_unchanged"], s
    # the heavy tie lies across a rank boundary of the output (it is half of the keys)
    if world > 1 and n > 100:
        j = 1
        x = sample_keys(steps[j][1], n, j)
        heavy = km.bits(km.curated(steps[j][1]))[len(km.curated(steps[j][1])) // 2 + 3]
        holders = [r for r in range(world) if (np.load(out + f".s{j}.okeys{r}.npy") == heavy).any()]
        assert (km.bits(x) == heavy).sum() > n // 3 and len(holders) >= 2, holders


@pytest.mark.parametrize("lens", [[0, 257, 8193], [5000, 1, 4097], [257, 8193], [5000, 4097]],
                         ids=["3-empty-first", "3-one-key", "2-a", "2-b"])
def test_sample_sort_and_argsort(tmp_path, lens):
    meta, out = run_ranks(tmp_path, lens, STEPS)
    check(meta, out, lens, STEPS)


def test_one_rccl_rank(tmp_path):
    lens = [8193]
    meta, out = run_ranks(tmp_path, lens, STEPS, transport="rccl")
    check(meta, out, lens, STEPS)
