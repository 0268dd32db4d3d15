"""The second level's arithmetic sub-bucket map on the host, CPU only.

arith_sub, arith_splitter_key, slot_entry and sub_of / sub_pick (csrc/dsort_sub.h) are __host__ __device__,
so tests/subarith/subarith_harness.cpp runs the very code the kernels run (the properties are spelled out at
the top of the harness).  The rule a bucket takes the map by is restated in numpy (tests/subarith_model.py),
pinned on uniform, clustered and narrow samples, and compared with the harness's restatement over the same
helper functions the kernel uses.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import PKG, REPO
from subarith_model import arith_sub, arith_take, clumped

HARNESS_SRC = os.path.join(REPO, "tests", "subarith", "subarith_harness.cpp")
HARNESS_DIR = os.path.join(REPO, "tests", "subarith", "build")
HEADERS = ["dsort_bucket.h", "dsort_sub.h", "dsort_internal.h"]


@pytest.fixture(scope="module")
def harness():
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", "/opt/rocm"),
                                                                              "bin", "hipcc")
    os.makedirs(HARNESS_DIR, exist_ok=True)
    out = os.path.join(HARNESS_DIR, "subarith_harness")
    deps = [HARNESS_SRC] + [os.path.join(PKG, "csrc", h) for h in HEADERS]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(PKG, "csrc"),
                               "-I" + os.path.join(REPO, "include"), "-o", out, HARNESS_SRC])
    return out


def test_map_monotone_in_range_and_restated_by_the_tables(harness):
    r = subprocess.run([harness], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.fullmatch(r"ok (\d+)\s*", r.stdout)
    assert m, r.stdout[-4000:]
    # 4 sub-bucket counts x at least 12 buckets that fit the key range; the nsub = 1024 ones alone check
    # 3 x 1023 splitter neighbours at 3 positions each: a run that checked less did not cover the map
    assert int(m.group(1)) > 12 * 3 * 1023 * 5


def test_model_matches_the_definition():
    # equal widths over [klo, klo + span], clamped outside, for a span above 2^31
    klo, span, nsub = -(2**31), 2**32 - 1, 1024
    keys = np.array([-(2**31), -(2**31) + 2**22 - 1, -(2**31) + 2**22, 0, 2**31 - 1], np.int64)
    assert arith_sub(keys, klo, span, nsub).tolist() == [0, 0, 1, 512, 1023]
    assert arith_sub([5, 10, 14, 15, 19, 20, 99], 10, 9, 2).tolist() == [0, 0, 0, 0, 1, 1, 1]  # (scale is rounded down: offset 5 still maps to 0)


def _samples(kind, nsub, osamp, seed):
    rng = np.random.default_rng(seed)
    ns = nsub * osamp
    if kind == "uniform":  # a 1/1024 slice of the key space
        return rng.integers(1 << 21, 1 << 22, ns)
    if kind == "uniform_wide":  # half the key space: a span above 2^31 - 1 needs the unsigned arithmetic
        return rng.integers(-(2**31), 2**31, ns)
    if kind == "smooth":  # a density rising from 0.85 to 1.15 of the mean across the slice
        u = rng.random(ns)
        u = np.where(rng.random(ns) < 0.15, np.maximum(u, rng.random(ns)), u)
        return (1 << 21) + (u * (1 << 21)).astype(np.int64)
    if kind == "clustered":  # 30 % of the samples in 4096 adjacent values
        k = rng.integers(1 << 21, 1 << 22, ns)
        k[: ns * 3 // 10] = rng.integers(3 << 20, (3 << 20) + 4096, ns * 3 // 10)
        return k
    if kind == "narrow":  # fewer values than 2 nsub
        return rng.integers(1, 101, ns)
    if kind == "runs":  # sorted input: nsub runs of 8 adjacent keys, each displaced by up to +-4 sub-buckets
        w = (1 << 21) // nsub
        at = (np.arange(nsub) * w + rng.integers(-4 * w, 4 * w, nsub)).clip(0, (1 << 21) - 8)
        return (1 << 21) + (at[:, None] + np.arange(osamp)[None, :]).ravel()
    if kind == "runs_shuffled":  # the same keys with no run structure left: the plain bound refuses them
        return rng.permutation(_samples("runs", nsub, osamp, seed))
    if kind == "runs_dup":  # ... and eight of the runs inside one duplicate run of 12 K copies
        k = _samples("runs", nsub, osamp, seed)
        k[: 8 * osamp] = (1 << 21) + 777_777
        return k
    if kind == "dup_heavy":  # a span that passes, but half the samples are one key
        k = rng.integers(0, 1 << 16, ns)
        k[::2] = 777
        return k
    raise AssertionError(kind)


def test_clumped_samples_are_known_by_their_order():
    assert clumped(_samples("runs", 85, 8, 1)) and not clumped(_samples("runs_shuffled", 85, 8, 1))
    assert not clumped(_samples("uniform", 1024, 8, 1)) and not clumped(_samples("clustered", 85, 8, 1))


RULE_CASES = [("runs", 683, True), ("runs_shuffled", 683, False), ("runs_dup", 683, False), ("uniform", 85, True), ("uniform", 683, True), ("uniform", 1024, True), ("uniform_wide", 683, True),
              ("smooth", 512, True), ("clustered", 85, False), ("clustered", 1024, False), ("narrow", 85, False),
              ("dup_heavy", 85, False)]


@pytest.mark.parametrize("kind,nsub,want", RULE_CASES)
def test_rule_pinned(kind, nsub, want, harness, tmp_path):
    for seed in (1, 2, 3):
        s = _samples(kind, nsub, 8, seed).astype(np.int32)
        assert arith_take(s, nsub, 8) == want, (kind, nsub, seed)
        # the harness's restatement: the kernel's own form, a binary search per synthetic splitter
        p = tmp_path / f"{kind}_{nsub}_{seed}.bin"
        s.tofile(p)
        r = subprocess.run([harness, "rule", str(nsub), "8", str(p)], stdout=subprocess.PIPE, text=True)
        assert r.returncode == 0 and r.stdout.strip() == ("take" if want else "refuse"), (kind, nsub, seed, r.stdout)
