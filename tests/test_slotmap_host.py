"""The slot maps of both partition levels on the host, CPU only.

log_m, slot_mode, slot_first (csrc/dsort_bucket.h) and the second level's slot_of (csrc/dsort_sub.h) are
__host__ __device__, so tests/slotmap/slotmap_harness.cpp -- a program of its own that includes the two
headers -- runs the very code the kernels run: every slot below the table size, slots monotone in the key,
and slot_first the exact inverse that build_slots counts the splitters of a slot with; at ulo = 0, 1,
UMAX - 5, UMAX, around 2^(KB-1) and 1000 random values, every linear shift and the log map, both key widths
(the properties are spelled out at the top of the harness).
"""
import os
import re
import shutil
import subprocess

import pytest

from conftest import PKG, REPO

HARNESS_SRC = os.path.join(REPO, "tests", "slotmap", "slotmap_harness.cpp")
HARNESS_DIR = os.path.join(REPO, "tests", "slotmap", "build")
HEADERS = ["dsort_bucket.h", "dsort_sub.h", "dsort_internal.h"]


@pytest.fixture(scope="module")
def harness():
    # (the compiler as the package's Makefile finds it)
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or os.path.join(os.environ.get("ROCM", "/opt/rocm"),
                                                                              "bin", "hipcc")
    os.makedirs(HARNESS_DIR, exist_ok=True)
    out = os.path.join(HARNESS_DIR, "slotmap_harness")
    deps = [HARNESS_SRC] + [os.path.join(PKG, "csrc", h) for h in HEADERS]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I" + os.path.join(PKG, "csrc"),
                               "-I" + os.path.join(REPO, "include"), "-o", out, HARNESS_SRC])
    return out


def test_slot_maps_bounded_monotone_and_inverted_by_slot_first(harness):
    r = subprocess.run([harness], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.fullmatch(r"ok (\d+)\s*", r.stdout)
    assert m, r.stdout[-4000:]
    # 1006 ulo values x (22 + 1 and 54 + 1 maps) x (2 x 4200 key checks + 2047 slots): a run that
    # checked less did not cover the maps
    assert int(m.group(1)) > 1006 * (23 + 55) * (2 * 4200 + 2047)
