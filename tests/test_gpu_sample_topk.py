"""Top-k across ranks (dsort_sample_topk_dev_keys; dsort.h, "top-k").  As in
test_gpu_sample_keys.py the ranks are child processes that share cuda:0 and exchange over the host
transport (gloo), and the RCCL exchange runs with one rank.  Every rank's output must equal the
checker of keys_model.py on the concatenated input: the first k of the stable argsort in the typed
order, as global positions, and their keys bit for bit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import keys_model as km
from conftest import REPO
from mp_sample_keys import sample_keys
from mp_sample_topk import firsts_of

pytestmark = pytest.mark.gpu
DRIVER = os.path.join(REPO, "tests", "mp_sample_topk.py")
EINVAL = -1
RUN_LIMIT_S = 120  # of one run of all ranks; every step inside has the exchange deadline of its own


def steps_for(total):
    """f32 descending and f64 ascending; k = 1, 300 (more than one rank holds winners) and the total;
    then one step in which rank 0 passes another k, and one more on the same communicator."""
    ks = [1, min(300, total), total]
    steps = [[name, desc, k, -1] for name, desc in (("f32", 1), ("f64", 0)) for k in ks]
    return steps + [["f32", 1, 7, 0], ["f64", 0, 7, -1]]


def run_ranks(tmp_path, lens, steps, transport="host", reverse=False):
    world = len(lens)
    store = str(tmp_path / "store")
    out = str(tmp_path / "tk")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    o = {"lens": lens, "steps": steps, "reverse": reverse}
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


def check(meta, out, lens, steps, reverse=False):
    world, n = len(lens), sum(lens)
    firsts = firsts_of(lens, reverse)
    for j, (name, desc, k, odd) in enumerate(steps):
        for r, m in enumerate(meta):
            s = m["steps"][j]
            assert s["n_in"] == lens[r] and s["first"] == firsts[r] and s["inputs_unchanged"], s
            if odd >= 0:  # the ranks disagreed on k: DSORT_EINVAL on every rank
                assert s["rc"] == EINVAL and "disagree on k" in s["error"], s
                continue
            assert s["rc"] == 0, s
        if odd >= 0:
            continue
        x = sample_keys(name, n, j)
        order = km.ref_order(x, name, bool(desc))[:k]
        for r in range(world):
            okeys = np.load(out + f".s{j}.okeys{r}.npy")
            oidx = np.load(out + f".s{j}.oidx{r}.npy")
            assert np.array_equal(oidx.view(np.uint32).astype(np.int64), order), (j, r, name, k)
            assert np.array_equal(okeys, km.bits(x[order])), (j, r, name, k)
    if world > 1 and n > 1000:
        # step 1 (k = 300): the winners come from more than one rank
        x = sample_keys(steps[1][0], n, 1)
        order = km.ref_order(x, steps[1][0], bool(steps[1][1]))[:steps[1][2]]
        bounds = sorted((firsts[r], firsts[r] + lens[r]) for r in range(world) if lens[r])
        holders = {i for i, (lo, hi) in enumerate(bounds) if ((order >= lo) & (order < hi)).any()}
        assert len(holders) >= 2, holders


@pytest.mark.parametrize("lens,reverse", [([0, 257, 8193], False), ([5000, 1, 4097], False), ([257, 8193], False),
                                          ([5000, 1, 4097], True)],
                         ids=["3-empty-first", "3-one-key", "2", "3-reverse-ranges"])
def test_sample_topk(tmp_path, lens, reverse):
    steps = steps_for(sum(lens))
    meta, out = run_ranks(tmp_path, lens, steps, reverse=reverse)
    check(meta, out, lens, steps, reverse)


def test_one_rccl_rank(tmp_path):
    lens = [8193]
    steps = [["f32", 1, 1, -1], ["f32", 1, 300, -1], ["f64", 0, sum(lens), -1]]
    meta, out = run_ranks(tmp_path, lens, steps, transport="rccl")
    check(meta, out, lens, steps)
