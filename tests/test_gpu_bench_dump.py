"""bench.py --dump-outputs on the GPU: the files hold the sorted keys of the last timed step at
the positions sample_blocks.npy lists, for the one-GPU sort (a plain run, whose line is the metric
alone, above the size at which the dump becomes a sample) and for the sample sort on one GPU
(--full: verified, with its roofline).  The expected keys are the oracle's generator, sorted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import REPO

pytestmark = pytest.mark.gpu

BENCH = os.path.join(REPO, "bench.py")


def _run(tmp_path, *argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = str(tmp_path / "dump")
    p = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "2", "--warmup", "1", "--dump-outputs", out,
                        *argv], capture_output=True, text=True, timeout=240, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout
    files = sorted(os.listdir(out))
    assert sum(os.path.getsize(os.path.join(out, f)) for f in files) <= 64 << 20
    return json.loads(lines[0]), out, files


def _expected(oracle, n, blocks):
    sys.path.insert(0, REPO)
    import bench

    keys = np.sort(oracle.gen_uniform(bench.SEED, 0, n))
    return np.concatenate([keys[int(s):int(e)] for s, e in blocks]).astype(np.float64)


def test_plain_single_run_dumps_the_sampled_sorted_keys(tmp_path, oracle):
    sys.path.insert(0, REPO)
    import bench

    n = (1 << 22) + 12345  # (one key range above the whole-output dump: 1024 blocks of 4096 keys)
    d, out, files = _run(tmp_path, "--keys", str(n))
    assert files == ["sample_blocks.npy", "sorted_keys.npy"]
    assert d["unit"] == "keys/s" and d["dtype"] == "int32" and d["higher_is_better"] is True and d["steps"] == 2
    assert d["ms_per_step"] > 0 and abs(d["value"] - n / (d["ms_per_step"] * 1e-3)) <= 1e-6 * d["value"]
    assert not {"roofline", "cpu_baseline", "gpu_library_reference", "legs"} & set(d)
    blocks = np.load(os.path.join(out, "sample_blocks.npy"))
    assert blocks.dtype == np.float64 and [tuple(map(int, b)) for b in blocks] == bench.sample_blocks(n, 4)
    got = np.load(os.path.join(out, "sorted_keys.npy"))
    assert got.dtype == np.float64 and got.size == 1 << 22
    assert np.array_equal(got, _expected(oracle, n, blocks))


def test_full_samplesort_run_dumps_the_whole_sorted_output(tmp_path, oracle):
    n = (1 << 20) + 3
    d, out, files = _run(tmp_path, "--keys", str(n), "--path", "samplesort", "--full", "--no-legs", "--no-cpu-baseline")
    assert files == ["sample_blocks.npy", "sorted_keys.npy"]
    assert d["ms_per_step"] > 0 and "roofline" in d and "legs" not in d and "cpu_baseline" not in d
    blocks = np.load(os.path.join(out, "sample_blocks.npy"))
    assert blocks.tolist() == [[0.0, float(n)]]
    assert np.array_equal(np.load(os.path.join(out, "sorted_keys.npy")), _expected(oracle, n, blocks))
