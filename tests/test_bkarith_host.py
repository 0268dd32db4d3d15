"""The first level's arithmetic bucket map on the host, CPU only.

arith_bucket, arith_splitter_key and arith_bucket_full (csrc/dsort_bucket.h) are __host__ __device__, so
tests/bkarith/bkarith_harness.cpp runs the very code the kernels run (the properties are spelled out at the
top of the harness), once as built and once under the address and undefined-behaviour sanitizers, as a
stand-alone program.  The rule a sort takes the map by is restated in numpy (tests/bkarith_model.py) and
pinned on the key shapes of tests/slotmap_model.py at its sizes, with 128 samples per bucket.
"""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bkarith_model as bm
import slotmap_model as sm
from conftest import PKG, REPO

HARNESS_SRC = os.path.join(REPO, "tests", "bkarith", "bkarith_harness.cpp")
HARNESS_DIR = os.path.join(REPO, "tests", "bkarith", "build")
HEADERS = ["dsort_bucket.h", "dsort_internal.h"]
OS = sm.OS_DEFAULT
TAKERS = ("uniform", "bit0")


def _build(name, extra):
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", "/opt/rocm"),
                                                                              "bin", "hipcc")
    os.makedirs(HARNESS_DIR, exist_ok=True)
    out = os.path.join(HARNESS_DIR, name)
    deps = [HARNESS_SRC] + [os.path.join(PKG, "csrc", h) for h in HEADERS]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(PKG, "csrc"),
                               "-I" + os.path.join(REPO, "include"), *extra, "-o", out, HARNESS_SRC])
    return out


def _ok(binary):
    r = subprocess.run([binary], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.fullmatch(r"ok (\d+)\s*", r.stdout)
    assert m, r.stdout[-4000:]
    # 4 bucket counts x at least 10 sorts that fit the key range; the B = 1024 ones alone look 3 x 1023
    # splitter neighbours up at 3 indices each: a run that checked less did not cover the map
    assert int(m.group(1)) > 10 * 3 * 1023 * 4


def test_map_bounded_monotone_and_restated_by_the_splitters():
    _ok(_build("bkarith_harness", []))


def test_harness_clean_under_the_sanitizers():
    _ok(_build("bkarith_harness_san", ["-g", "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host",
                                       "-fno-sanitize-recover=undefined", "-Xarch_host", "-fno-omit-frame-pointer"]))


def test_model_matches_the_definition():
    klo, span, B = -(2**31), 2**32 - 1, 1024
    keys = np.array([-(2**31), -(2**31) + 2**22 - 1, -(2**31) + 2**22, 0, 2**31 - 1], np.int64)
    assert bm.arith_bucket(keys, klo, span, B).tolist() == [0, 0, 1, 512, 1023]
    assert bm.arith_bucket([5, 10, 14, 15, 19, 20, 99], 10, 9, 2).tolist() == [0, 0, 0, 0, 1, 1, 1]


@pytest.mark.parametrize("B,n", sm.SIZES)
@pytest.mark.parametrize("name", list(sm.KEYS32))
def test_rule_pinned_at_the_slotmap_sizes(name, B, n):
    """uniform and bit0 take the map (their fullest arithmetic bucket holds 154-165 samples against the cap
    of 192); every other shape refuses: ref100 and the edge-only shapes by the span, the rest by their
    samples (24 to 1013 x os in one bucket) where the sampled map has not refused them already."""
    d = bm.decide(sm.make_keys(np.int32, name, B, n), B, OS)
    print(name, B, n, d)
    assert d["take"] == (name in TAKERS), d
    if name in TAKERS:
        assert 154 <= d["fullest"] <= 165, d
    elif name in ("ref100", "lowedge_only", "highedge_only"):
        assert d["why"] == "span", d
    else:
        assert d["fullest"] >= 24 * OS, d


def test_more_samples_than_keys_refuses_by_the_sample_count():
    """131072 samples of 40000 uniform keys: every key is sampled about three times, the counts are three
    times as coarse, and the fullest arithmetic bucket holds 201 samples -- above the cap."""
    B, n = sm.SMALL
    d = bm.decide(sm.make_keys(np.int32, "uniform", B, n), B, OS)
    assert not d["take"] and d["why"] == "samples" and d["fullest"] == 201, d


@pytest.mark.parametrize("order", ["ascending", "descending"])
def test_sorted_input_refuses_by_the_runs_hint(order):
    B, n = sm.SIZES[0]
    a = np.sort(sm.make_keys(np.int32, "uniform", B, n))
    d = bm.decide(a if order == "ascending" else a[::-1].copy(), B, OS)
    assert not d["take"] and d["why"] == "map", d
    assert bm.decide(a, B, OS, mode=2)["take"] and not bm.decide(a, B, OS, mode=0)["take"]
