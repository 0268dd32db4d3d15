"""The peer model of the distributed gather (tests/peer_model.py) without a GPU: a rank restated in
numpy (numpy_rank: the library's two host rules plus the documented sequence of callbacks) runs
against the modeled peers at up to 256 owners -- a clean model and the expected output -- and, broken
on purpose in each of peer_model.FAULTS, is caught by the model's checks.  The same cases that
tests/test_gpu_gather_owners.py runs with positions up to 2^32 are checked here first."""
import numpy as np
import pytest

import peer_model as pm


def run_numpy(dsort, P, me, W, first, count, idx, asks=None, fault=None, **kw):
    model = pm.PeerModel(dsort, P, me, first, count, W, idx, asks, **kw)
    records = pm.record_rule(int(first[me]) + np.arange(int(count[me]), dtype=np.uint64), W)
    out = pm.numpy_rank(dsort, model.transport(), P, me, int(first[me]), records, idx, W, fault=fault)
    return model, out


def ranks_of(P):
    return sorted({0, P // 2, P - 1})


def test_record_rule_and_owner_lookup():
    r = pm.record_rule([0, 1, 2 ** 32 - 1], 16)
    assert r.dtype == np.uint32 and r.shape == (3, 4)
    assert r[0].tolist() == [1, 0x9E3779B9 + 1, (2 * 0x9E3779B9 + 1) % 2 ** 32, (3 * 0x9E3779B9 + 1) % 2 ** 32]
    assert r[1, 0] == 2654435762 and r[2, 0] == ((2 ** 32 - 1) * 2654435761 + 1) % 2 ** 32
    assert np.array_equal(pm.record_rule([7], 4), pm.record_rule([7], 16)[:, :1])
    # ranges in descending rank order, one empty, one ending at 2^32
    first, count = [2 ** 32 - 10, 100, 50, 0], [10, 20, 0, 5]
    bins, loc = pm.owners_of(first, count, np.array([0, 4, 5, 99, 100, 119, 120, 2 ** 32 - 11, 2 ** 32 - 10,
                                                     2 ** 32 - 1], np.uint64).astype(np.uint32))
    assert bins.tolist() == [3, 3, 4, 4, 1, 1, 4, 4, 0, 0]
    assert loc.tolist() == [0, 4, 0, 0, 0, 19, 0, 0, 0, 9]


@pytest.mark.parametrize("P", [1, 2, 3, 5, 64, 256])
def test_numpy_rank_against_the_model(dsort_mod, P):
    rng = np.random.default_rng(P)
    k = 0
    for me in ranks_of(P):
        for tk in pm.TABLES:
            for n in (0, 1, 257, 4 * 1024 + 5):
                k += 1
                W = (4, 8, 16)[k % 3]
                first, count = pm.table(tk, P, me, rng=rng)
                idx = pm.indices(pm.PATTERNS[k % len(pm.PATTERNS)], first, count, me, n, rng)
                if idx is None:
                    idx = pm.indices("uniform", first, count, me, n if count.any() else 0, rng)
                asks = pm.script(pm.SCRIPTS[k % len(pm.SCRIPTS)], P, me, int(count[me]), rng)
                model, out = run_numpy(dsort_mod, P, me, W, first, count, idx, asks)
                what = (P, me, tk, n, W)
                assert model.done() == [], what
                assert model.log == list(pm.SEQUENCE) and model.sent_status == [0, 0, 0, 0], what
                assert np.array_equal(out, pm.record_rule(idx, W)), what
                assert model.sent == int((pm.owners_of(first, count, idx)[0] != me).sum()), what


def test_positions_up_to_2_32_are_consistent(dsort_mod):
    """The tables and indices that the GPU test uses at and above 2^31: the last range ends exactly
    at 2^32, the first and last position of every range are asked for."""
    seen = 0
    for P, me, W, first, count, idx, asks in pm.top_cases():
        assert int(first.max() + count[np.argmax(first)]) == 2 ** 32 and int(first.min()) < 2 ** 31 or P == 1
        assert int(idx.max()) == 2 ** 32 - 1 and (P == 1 or int(idx.min()) < 2 ** 31)
        model, out = run_numpy(dsort_mod, P, me, W, first, count, idx, asks)
        assert model.done() == [], (P, me)
        assert np.array_equal(out, pm.record_rule(idx, W)), (P, me)
        assert model.want_cnt[P] == 0
        seen += 1
    assert seen >= 6


def faulty_case(P):
    """Every owner gets several distinct requests; peers 0 and 1 ask for as many, but other, records."""
    me, W = 2, 8
    rng = np.random.default_rng(5)
    first, count = pm.table("equal", P, me)
    idx = pm.indices("uniform", first, count, me, 40 * P, rng)
    asks = pm.script("some", P, me, 37, rng)
    asks.update({0: [1, 2, 3], 1: [4, 5, 6], P - 1: [0, 0]})
    return P, me, W, first, count, idx, asks


@pytest.mark.parametrize("P", [5, 256])
@pytest.mark.parametrize("fault,names", [("reverse_owner", "requests to owner"), ("swap_segments", "sdispls"),
                                         ("off_by_one", "requests to owner"), ("swap_counts", "counts row"),
                                         ("wrong_peer_order", "replies to peer"), ("skip_callback", "'gate'")])
def test_a_broken_rank_is_caught(dsort_mod, P, fault, names):
    case = faulty_case(P)
    model, out = run_numpy(dsort_mod, *case)  # (the case itself is fine)
    assert model.done() == [] and np.array_equal(out, pm.record_rule(case[5], case[2]))
    model = pm.PeerModel(dsort_mod, P, case[1], case[3], case[4], case[2], case[5], case[6])
    records = pm.record_rule(int(case[3][2]) + np.arange(37, dtype=np.uint64), 8)
    try:
        out = pm.numpy_rank(dsort_mod, model.transport(), P, 2, int(case[3][2]), records, case[5], 8, fault=fault)
    except pm.RankStopped:
        out = None
    errors = model.done()
    assert errors and any(names in e for e in errors), errors
    if fault in ("reverse_owner", "off_by_one"):  # the model answers what was asked: the output shows it too
        assert out is not None and not np.array_equal(out, pm.record_rule(case[5], 8))


def test_callbacks_out_of_turn_are_caught(dsort_mod):
    P, me, W, first, count, idx, asks = faulty_case(5)
    model, _ = run_numpy(dsort_mod, P, me, W, first, count, idx, asks)
    t = model.transport()
    st, every = np.zeros(1, np.int64), np.zeros(P, np.int64)
    assert t.allgather(None, st.ctypes.data, every.ctypes.data, 8) != 0  # one more gate behind the last collective
    assert any("after the call's last collective" in e for e in model.done())
    model.expect(first, count, W, idx, asks)
    z = (np.zeros(P, np.uintp).ctypes.data_as(pm.ctypes.POINTER(pm.ctypes.c_size_t)),) * 4
    assert t.alltoallv(None, every.ctypes.data, z[0], z[1], every.ctypes.data, z[2], z[3]) != 0
    assert any("arrives where 'gate' is due" in e for e in model.done(0)) and model.log == ["misplaced alltoallv"]


def test_scripted_failures_stop_the_numpy_rank(dsort_mod):
    """What the GPU test scripts for its error cases: an unowned count in a peer's row, another
    elem_bytes, an overlap, a peer's status at the gate of collective 2 -- the model plays them and
    sees exactly the collectives up to there."""
    P, me, W, first, count, idx, asks = faulty_case(5)
    for kw, log in (({"unowned": {3: 2}}, pm.SEQUENCE[:4]), ({"elem_bytes": {4: 16}}, pm.SEQUENCE[:2]),
                    ({"gate_status": {(2, 1): -5}}, pm.SEQUENCE[:5])):
        with pytest.raises(pm.RankStopped):
            run_numpy(dsort_mod, P, me, W, first, count, idx, asks, **kw)
    model = pm.PeerModel(dsort_mod, P, me, first, count, W, idx, asks, gate_status={(2, 1): -5})
    with pytest.raises(pm.RankStopped):
        pm.numpy_rank(dsort_mod, model.transport(), P, me, int(first[me]), pm.record_rule(first[me] + np.arange(
            37, dtype=np.uint64), W), idx, W)
    assert model.log == list(pm.SEQUENCE[:5]) and model.errors == []
    shifted = first.copy()
    shifted[3] -= 1  # ranks 2 and 3 overlap by one record
    model = pm.PeerModel(dsort_mod, P, me, shifted, count, W, idx, asks)
    assert model.want_row is None
    with pytest.raises(dsort_mod.DsortError):
        pm.numpy_rank(dsort_mod, model.transport(), P, me, int(first[me]), pm.record_rule(first[me] + np.arange(
            37, dtype=np.uint64), W), idx, W)
    assert model.log == list(pm.SEQUENCE[:2]) and model.errors == []
    with pytest.raises(ValueError):  # a script that asks for a record the rank does not hold
        pm.PeerModel(dsort_mod, P, me, first, count, W, idx, {0: [37]})
