"""The distributed gather's routing at up to 256 owners in ONE process (dsort_sample_gather_dev,
dsort_gather.hip): the library runs its real kernels and host code as rank `me` of P on the host
transport, and tests/peer_model.py plays the other P - 1 ranks through the transport's two
callbacks, checking every byte the rank sends (the counts row against the host rule, the requests
owner-major and in input order, the served records peer by peer) and answering as the peers would.
Records are a pure function of the global position, so the expected output is that function of idx,
compared bit for bit; only this rank's records exist.

A context of this file's own carries the communicators (the session-wide gpu_ctx never gets one).
Sizes are the smallest at which a piece can go wrong: a lane's 4 indices, a wave's 256, a tile's
1024, partial last tiles at each record width, and two sizes past one tile per workgroup (2048
workgroups) at P = 256.  tests/test_peer_model.py checks the model itself, and these tables and
indices, without a GPU."""
import numpy as np
import pytest

import peer_model as pm

pytestmark = pytest.mark.gpu

EINVAL, ECOMM = -1, -4
OWNERS = [1, 2, 3, 4, 5, 63, 64, 65, 255, 256]
N_IDX = [0, 1, 2, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, 4 * 1024 + 5]
N_LARGE = [2048 * 1024 + 1024 + 3,  # more than one tile per workgroup, 2048 workgroups, a short last chunk
           2048 * 1024 - 1]
SOME = 4 * 1024 + 5


class Rank:
    """The context of this file and its current communicator."""

    def __init__(self, dsort):
        self.dsort = dsort
        self.ctx = dsort.Context(0)
        self.ctx.set_option("comm_timeout_ms", 8000)  # (the modeled peers never wait)
        self.has_comm = False
        self.calls = 0

    def comm(self, P, me, transport):
        if self.has_comm:
            self.ctx.comm_destroy()
            self.has_comm = False
        self.ctx.comm_init_transport(P, me, transport)
        self.has_comm = True

    def close(self):
        if self.has_comm:
            self.ctx.comm_destroy()
        self.ctx.close()


@pytest.fixture(scope="module")
def rank(dsort_mod):
    import torch
    if not torch.cuda.is_available():
        pytest.fail("gpu test selected but no GPU visible (tests marked gpu must run on the MI355X box)")
    rk = Rank(dsort_mod)
    yield rk
    print(f"\n{rk.calls} modeled gather calls")
    rk.close()


def ranks_of(P):
    return sorted({0, P // 2, P - 1})


def width_of(k):
    return (4, 8, 16)[k % 3]


def call(rk, model, view=0):
    """One dsort_sample_gather_dev as the rank scripted in `model`, on rk's communicator; records,
    indices and the output start at element `view` of their allocations, zero guards of one record
    around the output.  Returns (the DsortError or None, out as uint32).  Asserts what holds after
    every call, failed or not: the inputs are unchanged and the guards are zero."""
    import torch
    me, W = model.me, model.W
    D, n_src, n = W // 4, model.n_src, model.idx.size

    def flat(words):
        return torch.empty(max(words, 1) + view, dtype=torch.int32, device="cuda")[view:view + words]

    rec_np = pm.record_rule(int(model.first[me]) + np.arange(n_src, dtype=np.uint64), W)
    rec, idx = flat(n_src * D), flat(n)
    if n_src:
        rec.copy_(torch.from_numpy(rec_np.reshape(-1).view(np.int32)))
    if n:
        idx.copy_(torch.from_numpy(model.idx.view(np.int32)))
    full = torch.zeros(view + (n + 2) * D, dtype=torch.int32, device="cuda")
    out = full[view + D:view + D + n * D].view(n, D)
    err = None
    try:
        rk.ctx.sample_gather_dev(rec.view(n_src, D), int(model.first[me]), idx, out=out)
    except rk.dsort.DsortError as e:
        err = e
    torch.cuda.synchronize()
    rk.calls += 1
    full_h = full.cpu().numpy().view(np.uint32)
    assert np.array_equal(rec.cpu().numpy().view(np.uint32), rec_np.reshape(-1)), "records changed"
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), model.idx), "idx changed"
    assert not full_h[:view + D].any() and not full_h[view + D + n * D:].any(), "the guards around out changed"
    return err, full_h[view + D:view + D + n * D].reshape(n, D)


def check_ok(rk, model, view=0, what=None):
    err, out = call(rk, model, view)
    assert err is None, (what, str(err))
    want = pm.record_rule(model.idx, model.W)
    assert np.array_equal(out, want), (what, f"{int((out != want).any(axis=1).sum())} records differ")
    assert model.done() == [], what
    st = rk.ctx.stats()
    assert st["gather_sent"] == model.sent and st["gather_served"] == model.served, (what, st, model.sent, model.served)
    return model


def case(rk, P, me, W, tk, pat, n, sk="some", view=0):
    """Builds table `tk`, index pattern `pat` of n indices and peer script `sk` (peer_model) and
    runs the call on a fresh communicator.  Returns the model, or None where the table cannot give
    the pattern."""
    rng = np.random.default_rng([P, me, W, n, len(tk), len(pat)])
    first, count = pm.table(tk, P, me, rng=rng)
    idx = pm.indices(pat, first, count, me, n, rng)
    if idx is None:
        return None
    model = pm.PeerModel(rk.dsort, P, me, first, count, W, idx, pm.script(sk, P, me, int(count[me]), rng))
    rk.comm(P, me, model.transport())
    return check_ok(rk, model, view, (P, me, W, tk, pat, n, sk, view))


# ------------------------------------------------------------------------------ owner counts
@pytest.mark.parametrize("P", OWNERS)
def test_owner_counts(rank, P):
    """Every P at one width, the three widths at P = 5 and 256; rank 0, a middle one and the last.
    Round robin: a wave of 256 indices meets min(256, P) distinct owners, one ranking round each."""
    widths = (4, 8, 16) if P in (5, 256) else (width_of(OWNERS.index(P)),)
    for me in ranks_of(P):
        for W in widths:
            m = case(rank, P, me, W, "equal", "round_robin", SOME)
            assert len(set(m.bins[:256].tolist())) == min(256, P)
            assert case(rank, P, me, W, "equal", "uniform", 1025)


# ------------------------------------------------------------------------------ index counts
@pytest.mark.parametrize("P", [5, 256])
def test_index_counts(rank, P):
    for W in (4, 8, 16):
        for n in N_IDX:
            for pat in ("round_robin", "uniform"):
                assert case(rank, P, P // 2, W, "equal", pat, n)


@pytest.mark.parametrize("n", N_LARGE)
def test_index_counts_past_one_tile_per_workgroup(rank, n):
    k = N_LARGE.index(n)
    assert case(rank, 256, (0, 255)[k], (4, 8)[k], "equal", "round_robin", n)
    assert case(rank, 256, 128, (16, 4)[k], "equal", ("uniform", "sorted")[k], n, sk="each_once")


# ------------------------------------------------------------------------------ index patterns
@pytest.mark.parametrize("P", [5, 256])
def test_index_patterns(rank, P):
    for me in ranks_of(P):
        for k, pat in enumerate(pm.PATTERNS):
            m = case(rank, P, me, width_of(k + me), "equal", pat, SOME)
            assert m is not None, pat
            if pat in ("one_me", "own"):
                assert m.sent == 0 and m.want_cnt[me] == SOME
            if pat == "others":
                assert m.sent == SOME and m.want_cnt[me] == 0
            if pat in ("one_first", "one_last"):
                assert m.want_cnt[0 if pat == "one_first" else P - 1] == SOME
            if pat == "repeats":
                assert np.unique(m.idx, return_counts=True)[1].max() > SOME // 2


# ------------------------------------------------------------------------------ table shapes
@pytest.mark.parametrize("P", [5, 64, 256])
def test_table_shapes(rank, P):
    ran = 0
    for me in ranks_of(P):
        for k, tk in enumerate(pm.TABLES):
            for pat, n in (("uniform", 1025), ("edges", 2 * P + 3)):
                m = case(rank, P, me, width_of(k), tk, pat, n)
                assert m is not None, (tk, pat)
                ran += 1
                if tk.startswith("alt_"):  # fewer ranges than ranks
                    assert 0 < np.count_nonzero(m.count) < P and (m.n_src == 0) == (tk == "alt_me_empty")
                if tk == "top":
                    assert int(m.idx.max()) >= 2 ** 31
    assert ran == 3 * len(pm.TABLES) * 2


def test_positions_up_to_2_32(rank):
    """The last range ends exactly at 2^32, the first starts below 2^31; the first and last position
    of every range are among the indices.  The peers' ranges are huge and exist as a rule only."""
    for P, me, W, first, count, idx, asks in pm.top_cases():
        model = pm.PeerModel(rank.dsort, P, me, first, count, W, idx, asks)
        rank.comm(P, me, model.transport())
        check_ok(rank, model, 0, (P, me, W))
        assert int(idx.max()) == 2 ** 32 - 1


# ------------------------------------------------------------------------------ scripted peers
@pytest.mark.parametrize("P", [5, 256])
def test_scripted_peers(rank, P):
    for me in ranks_of(P):
        for k, sk in enumerate(pm.SCRIPTS):
            m = case(rank, P, me, width_of(k + me), "equal", "uniform", 1025, sk=sk)
            asked = {"none": 0, "each_once": P - 1, "one_all_twice": 2 * 37}  # (37 records per rank)
            assert sk not in asked or m.served - m.want_cnt[me] == asked[sk]
            # the peers ask while this rank has no index
            m = case(rank, P, me, width_of(k + me), "equal", "uniform", 0, sk=sk)
            assert m.sent == 0 and m.served == sum(a.size for a in m.asks)
        # this rank holds no record and only asks
        m = case(rank, P, me, width_of(me), "alt_me_empty", "uniform", 1025)
        assert m.n_src == 0 and m.served == 0 and m.sent == 1025


# ------------------------------------------------------------------------------ views
@pytest.mark.parametrize("W", [4, 8, 16])
def test_views_at_element_offsets(rank, W):
    """idx, records and out start 4 and 12 bytes into their allocations: nothing may assume more
    than dword alignment of the caller's arrays."""
    for view in (1, 3):
        assert case(rank, 256, 128, W, "equal", "uniform", SOME, view=view)
        assert case(rank, 256, 128, W, "equal", "round_robin", 1023, view=view)


# ------------------------------------------------------------------------------ errors
def expect_error(rk, model, rc, text, log):
    err, out = call(rk, model)
    assert err is not None and err.rc == rc and all(t in str(err) for t in text), (rc, text, str(err))
    assert model.log == list(log) and model.errors == [], (model.log, model.errors)
    assert not out.any(), "out was written by a failing call"


@pytest.mark.parametrize("P", [5, 256])
def test_errors_at_modeled_owner_counts(rank, P):
    """Each error is seen by every rank of a real communicator alike, so the call ends right behind
    the collective that revealed it -- no all-to-all runs -- and leaves `out` alone; a valid call on
    the same context and communicator succeeds afterwards."""
    me, W, peer = P // 2, 8, P - 1
    rng = np.random.default_rng(P)
    first, count = pm.table("gaps", P, me, rng=rng)
    good = pm.indices("uniform", first, count, me, 1025, rng)
    asks = pm.script("some", P, me, int(count[me]), rng)
    model = pm.PeerModel(rank.dsort, P, me)
    rank.comm(P, me, model.transport())

    def valid():
        check_ok(rank, model.expect(first, count, W, good, asks))

    valid()
    # three indices in gaps, on this rank
    holes = np.array([first[me] + count[me], first[0] - 1, first[P - 1] + count[P - 1] + 2], np.uint64)
    bad = np.concatenate([good[:500], holes.astype(np.uint32), good[500:]])
    model.expect(first, count, W, bad, asks)
    assert model.want_cnt[P] == 3
    expect_error(rank, model, EINVAL, [f"rank {me} holds 3 indices that no rank owns"], pm.SEQUENCE[:4])
    valid()
    # an unowned count in a peer's row
    model.expect(first, count, W, good, asks, unowned={peer: 7})
    expect_error(rank, model, EINVAL, [f"rank {peer} holds 7 indices that no rank owns"], pm.SEQUENCE[:4])
    valid()
    # a peer's range row with another elem_bytes
    model.expect(first, count, W, good, asks, elem_bytes={peer: 16})
    expect_error(rank, model, EINVAL, ["disagree on elem_bytes", f"rank {peer} 16"], pm.SEQUENCE[:2])
    valid()
    # two peers' ranges overlapping by one record
    tight, tcount = pm.table("equal", P, me)
    tight[peer] -= 1
    model.expect(tight, tcount, W, good, asks)
    assert model.want_row is None
    expect_error(rank, model, EINVAL, ["ranges overlap"], pm.SEQUENCE[:2])
    valid()
    # a peer reports a local failure at the gate of collective 2: no further callback runs
    model.expect(first, count, W, good, asks, gate_status={(2, peer): -5})
    expect_error(rank, model, ECOMM, [f"rank {peer} failed locally (error -5)"], pm.SEQUENCE[:5])
    valid()


def test_more_than_256_ranks_is_refused_before_any_callback(rank):
    P, me = 257, 128
    first, count = pm.table("equal", P, me)
    idx = pm.indices("uniform", first, count, me, 1025, np.random.default_rng(257))
    model = pm.PeerModel(rank.dsort, P, me, first, count, 8, idx)
    rank.comm(P, me, model.transport())
    expect_error(rank, model, EINVAL, ["more than 256 ranks"], [])
    assert model.sent_status == []  # not even a gate
    assert case(rank, 2, 1, 8, "equal", "uniform", 1025)  # (destroys that communicator first)


# ------------------------------------------------------------------------------ reuse
def test_one_communicator_several_calls(rank):
    """One context, one communicator of 256 ranks, four calls of other widths, sizes, tables and
    patterns back to back: the arenas grow, the routing tables are rewritten."""
    P, me = 256, 77
    model = pm.PeerModel(rank.dsort, P, me)
    rank.comm(P, me, model.transport())
    for W, tk, pat, n, sk in ((4, "equal", "round_robin", 1025, "some"), (16, "reverse", "uniform", 64 * 1024 + 7,
                                                                           "one_all_twice"),
                              (8, "ones", "edges", 5, "each_once"), (4, "gaps", "sorted", SOME, "none")):
        rng = np.random.default_rng(n)
        first, count = pm.table(tk, P, me, rng=rng)
        idx = pm.indices(pat, first, count, me, n, rng)
        check_ok(rank, model.expect(first, count, W, idx, pm.script(sk, P, me, int(count[me]), rng)), 0, (W, tk, pat))
