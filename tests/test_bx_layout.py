"""The bucket exchange's wave layout, every rank against every other, CPU only.

sample_sort_bx (csrc/dsort_exchange.hip) lays its waves out with bx_layout (csrc/dsort_bxlayout.h):
which keys of the partition go to which rank in which wave, and where the pieces of the others
land.  With the ranks of a test sharing one GPU the RCCL path runs with one rank only, so no GPU
test sees whether what rank q sends is what rank r expects.  tests/tx/bxlayout_harness.cpp computes
the layout of every rank of one seeded exchange with that very header and checks:
  * what q sends to r in wave w is what r expects from q, in count and bucket range;
  * a rank's landing zones are pairwise disjoint, inside [n_local, n_local + recv_room) when they
    lie behind its partition and inside [0, nrecv) when not;
  * sum(rlen) = nrecv; nout = the real sizes of the rank's buckets over all sources; pure buckets
    count for nout alone.
"""
import ctypes
import os
import subprocess

import pytest

from conftest import PKG, REPO

HARNESS_SRC = os.path.join(REPO, "tests", "tx", "bxlayout_harness.cpp")
HARNESS_DIR = os.path.join(REPO, "tests", "tx", "build")

SIZES = {"equal": 0, "skewed": 1, "empty-rank": 2}
PURES = {"none": 0, "some": 1, "nearly-all": 2}
ROOMS = {"no-room": 0, "ample": 1, "exact": 2, "one-short": 3}


@pytest.fixture(scope="module")
def harness():
    os.makedirs(HARNESS_DIR, exist_ok=True)
    out = os.path.join(HARNESS_DIR, "libbxlayout.so")
    deps = [HARNESS_SRC, os.path.join(PKG, "csrc", "dsort_bxlayout.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-shared", "-fPIC",
                               "-I" + os.path.join(PKG, "csrc"), "-o", out, HARNESS_SRC])
    lib = ctypes.CDLL(out)
    lib.bxl_check.argtypes = [ctypes.c_int] * 5 + [ctypes.c_uint64, ctypes.c_char_p, ctypes.c_size_t,
                                                   ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    return lib


def check(lib, P, Bl, sizes, pures, room, seed):
    msg = ctypes.create_string_buffer(512)
    behind, apart = ctypes.c_int(0), ctypes.c_int(0)
    rc = lib.bxl_check(P, Bl, SIZES[sizes], PURES[pures], ROOMS[room], seed, msg, len(msg), ctypes.byref(behind),
                       ctypes.byref(apart))
    assert rc == 0, (P, Bl, sizes, pures, room, msg.value.decode())
    assert behind.value + apart.value == P
    return behind.value, apart.value


@pytest.mark.parametrize("P", [1, 2, 3, 8])
@pytest.mark.parametrize("Bl", [1, 2, 5])
def test_every_rank_expects_what_its_peers_send(harness, P, Bl):
    behind = apart = 0
    for sizes in SIZES:
        for pures in PURES:
            for room in ROOMS:
                b, a = check(harness, P, Bl, sizes, pures, room, seed=1000 * P + 10 * Bl)
                behind, apart = behind + b, apart + a
                if room == "ample" or P == 1:  # (a single rank receives nothing from others)
                    assert a == 0, (sizes, pures, room)
    assert behind > 0
    assert apart > 0 or P == 1


def test_both_landing_layouts_occur(harness):
    """recv_room decides: the others' pieces behind the partition, or everything in a receive buffer."""
    assert check(harness, 3, 5, "skewed", "some", "ample", seed=7) == (3, 0)
    assert check(harness, 3, 5, "skewed", "some", "exact", seed=7) == (3, 0)
    assert check(harness, 3, 5, "skewed", "some", "one-short", seed=7) == (0, 3)
    assert check(harness, 3, 5, "skewed", "some", "no-room", seed=7) == (0, 3)
