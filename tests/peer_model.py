"""One rank of the distributed record gather against MODELED peers (dsort_sample_gather_dev on the
host transport, dsort_gather.hip): a dsort.Transport whose two callbacks play the other P - 1 ranks.

On the host transport every exchange of the call goes through dsort_transport's all-gather and
all-to-all-v callbacks, the rank's own part included.  PeerModel answers them as the peers of a
scripted communicator would, so the library runs its real kernels and host code as rank `me` of P
in one process -- and it CHECKS every byte the rank sends against the layout the file header of
dsort_gather.hip promises (owner-major, input order inside an owner), recording each mismatch as a
string in `errors` (an exception inside a ctypes callback would be swallowed).

The call's sequence (dsort_gather.hip, dsort_tx.h, a2av_peers in dsort_exchange.hip): every
collective is preceded by a gate, an 8-byte all-gather of an int64 status (0 = fine);
  0  "ranges"    all-gather of (first, n_src, elem_bytes) as uint64
  1  "counts"    all-gather of the P + 1 uint64 counts, column P = indices nobody owns
  2  "requests"  all-to-all-v of the uint32 requests (the owner's local indices)
  3  "replies"   all-to-all-v of the W-byte records
Counts and displacements of the all-to-all-v arrive in bytes.  The steps are told apart by their
order, not by their size (at P = 2 both all-gathers carry 24 bytes).

Records are a pure function of the global position (record_rule), so a peer's range may be as large
as the 32-bit position space without anything of that size existing.

numpy_rank restates a rank in plain numpy on the same callbacks: tests/test_peer_model.py runs it
against the model without a GPU, also broken on purpose (FAULTS) to show that the checks have teeth.
table / indices / script build the cases of both test files."""
import ctypes

import numpy as np

SEQUENCE = ("gate", "ranges", "gate", "counts", "gate", "requests", "gate", "replies")
M32 = np.uint64(0xFFFFFFFF)


def record_rule(g, W):
    """The records at global positions g, as (len(g), W / 4) uint32: dword d of the record at g is
    (g * 2654435761 + d * 0x9E3779B9 + 1) mod 2^32."""
    g = np.asarray(g, np.uint64).reshape(-1, 1)
    d = np.arange(W // 4, dtype=np.uint64).reshape(1, -1)
    return ((g * np.uint64(2654435761) + d * np.uint64(0x9E3779B9) + np.uint64(1)) & M32).astype(np.uint32)


def owners_of(first, count, idx):
    """numpy's owner lookup: (bin, local index) per index; bin = the owning rank, or P for nobody."""
    first, count = np.asarray(first, np.uint64).astype(np.int64), np.asarray(count, np.uint64).astype(np.int64)
    P = first.size
    g = np.asarray(idx, np.uint32).astype(np.int64)
    held = np.flatnonzero(count)
    order = held[np.argsort(first[held], kind="stable")]
    if order.size == 0:
        return np.full(g.size, P, np.int64), np.zeros(g.size, np.int64)
    lo = first[order]
    hi = lo + count[order]
    sl = np.searchsorted(lo, g, side="right") - 1
    at = np.maximum(sl, 0)
    ok = (sl >= 0) & (g < hi[at])
    return np.where(ok, order[at], P), np.where(ok, g - lo[at], 0)


def _excl(a):
    out = np.zeros(len(a), np.int64)
    np.cumsum(np.asarray(a, np.int64)[:-1], out=out[1:])
    return out


def _view(ptr, nbytes, dtype):
    """The caller's memory at ptr as a writable numpy array."""
    if not nbytes:
        return np.empty(0, dtype)
    return np.frombuffer((ctypes.c_ubyte * int(nbytes)).from_address(int(ptr)), dtype=dtype)


class PeerModel:
    """The peers of rank `me` in a communicator of P ranks.  expect() scripts one call; transport()
    is the dsort.Transport to give to Context.comm_init_transport; after the call, done() returns the
    list of mismatches (empty: the rank sent what the contract says, in order, and nothing more)."""

    def __init__(self, dsort, P, me, *call, **script):
        self.dsort, self.P, self.me = dsort, int(P), int(me)
        self._ag = dsort.ALLGATHER_FN(self._allgather)
        self._a2a = dsort.ALLTOALLV_FN(self._alltoallv)
        self.errors, self.log, self.step = [], [], 0
        if call or script:
            self.expect(*call, **script)

    def transport(self):
        t = self.dsort.Transport(None, self._ag, self._a2a)
        t._keep = (self._ag, self._a2a, self)  # the C side holds raw function pointers
        t.deadline_fn = None
        return t

    def expect(self, first, count, W, idx, asks=None, unowned=None, gate_status=None, elem_bytes=None):
        """Scripts the next call.  first / count: the range table of all ranks (row `me` is what this
        rank must send); idx: this rank's indices; asks: {peer: local indices into this rank's
        records}; unowned: {peer: column P of that peer's counts row}; gate_status: {(collective,
        peer): status} at the gate in front of that collective; elem_bytes: {peer: the elem_bytes of
        that peer's range row}."""
        P, me = self.P, self.me
        self.first = np.asarray(first, np.uint64).copy()
        self.count = np.asarray(count, np.uint64).copy()
        assert self.first.size == P and self.count.size == P
        self.W = int(W)
        self.idx = np.asarray(idx, np.uint32).copy()
        self.n_src = int(self.count[me])
        self.asks = [np.zeros(0, np.uint32)] * P
        for r, a in (asks or {}).items():
            a = np.asarray(a, np.int64)
            if r == me or not 0 <= r < P or (a.size and (a.min() < 0 or a.max() >= self.n_src)):
                raise ValueError(f"peer {r} is scripted to ask for records this rank does not hold")
            self.asks[r] = a.astype(np.uint32)
        self.unowned = dict(unowned or {})
        self.gate_status = dict(gate_status or {})
        self.elem_bytes = dict(elem_bytes or {})
        self.errors, self.log, self.step = [], [], 0
        self.sent_status, self.sent_req = [], None
        # what the rank must route: numpy's partition, and the host rule's counts
        bins, loc = owners_of(self.first, self.count, self.idx)
        self.bins = bins
        self.want_cnt = np.bincount(bins, minlength=P + 1).astype(np.int64)
        order = np.argsort(bins, kind="stable")
        self.want_req = loc[order][:int(self.want_cnt[:P].sum())].astype(np.uint32)  # owner-major, input order
        try:
            lo, hi, owner = self.dsort.plan_gather_table(self.first, self.count)
            self.want_row = self.dsort.plan_gather_route(lo, hi, owner, P, self.idx)[0].astype(np.int64)
            if not np.array_equal(self.want_row, self.want_cnt):
                self.errors.append("dsort_plan_gather_route's counts differ from numpy's bincount of the owners")
        except self.dsort.DsortError:
            self.want_row = None  # the table is refused: the call ends behind collective 0
        return self

    # what a successful call leaves in dsort_stats
    @property
    def sent(self):
        return int(self.want_cnt[:self.P].sum() - self.want_cnt[self.me])

    @property
    def served(self):
        return int(sum(a.size for a in self.asks) + self.want_cnt[self.me])

    def done(self, steps=len(SEQUENCE)):
        if self.step != steps:
            self.errors.append(f"the call made {self.step} callbacks ({self.log}), {steps} expected")
        return self.errors

    # ------------------------------------------------------------------ the callbacks
    def _next(self, kind):
        if self.step >= len(SEQUENCE):
            self.errors.append(f"{kind} callback after the call's last collective")
            self.log.append("extra " + kind)
            return None
        what = SEQUENCE[self.step]
        if kind != ("alltoallv" if what in ("requests", "replies") else "allgather"):
            self.errors.append(f"callback {self.step}: {kind} arrives where '{what}' is due")
            self.log.append("misplaced " + kind)
            return None
        self.step += 1
        self.log.append(what)
        return what

    def _allgather(self, user, send, recv, nbytes):
        try:
            return self._on_allgather(send, recv, int(nbytes))
        except BaseException as e:  # (an exception inside a ctypes callback is swallowed)
            self.errors.append(f"exception in the all-gather callback: {e!r}")
            return 1

    def _alltoallv(self, user, send, sc, sd, recv, rc, rd):
        try:
            return self._on_alltoallv(send, sc, sd, recv, rc, rd)
        except BaseException as e:
            self.errors.append(f"exception in the all-to-all-v callback: {e!r}")
            return 1

    def _on_allgather(self, send, recv, nbytes):
        P, me = self.P, self.me
        coll = self.step // 2
        what = self._next("allgather")
        if what is None:
            return 1
        size = {"gate": 8, "ranges": 24, "counts": (P + 1) * 8}[what]
        if nbytes != size:
            self.errors.append(f"'{what}' (callback {self.step - 1}): {nbytes} bytes per rank, {size} expected")
            return 1
        if what == "gate":
            st = int(_view(send, 8, np.int64)[0])
            self.sent_status.append(st)
            if st:
                self.errors.append(f"the rank reports status {st} at the gate of collective {coll}")
            out = _view(recv, 8 * P, np.int64)
            out[:] = 0
            for (k, r), v in self.gate_status.items():
                if k == coll:
                    out[r] = v
            out[me] = st
        elif what == "ranges":
            row = _view(send, 24, np.uint64).copy()
            want = [int(self.first[me]), self.n_src, self.W]
            if row.tolist() != want:
                self.errors.append(f"range row {row.tolist()}, expected (first, n_src, elem_bytes) = {want}")
            out = _view(recv, 24 * P, np.uint64).reshape(P, 3)
            out[:, 0], out[:, 1], out[:, 2] = self.first, self.count, self.W
            for r, w in self.elem_bytes.items():
                out[r, 2] = w
            out[me] = row
        else:
            row = _view(send, nbytes, np.uint64).copy()
            if self.want_row is None:
                self.errors.append("the counts all-gather runs although the range table must be refused")
            elif not np.array_equal(row.astype(np.int64), self.want_row):
                b = int(np.flatnonzero(row.astype(np.int64) != self.want_row)[0])
                self.errors.append(f"counts row: column {b} is {int(row[b])}, the host rule gives {int(self.want_row[b])}")
            out = _view(recv, nbytes * P, np.uint64).reshape(P, P + 1)
            out[:] = 0
            out[:, me] = [a.size for a in self.asks]
            for r, k in self.unowned.items():
                out[r, P] = k
            out[me] = row
        return 0

    def _layout(self, what, name, got, want):
        if np.array_equal(got, want):
            return True
        r = int(np.flatnonzero(got != want)[0])
        self.errors.append(f"'{what}': {name}[{r}] is {int(got[r])} bytes, expected {int(want[r])}")
        return False

    def _on_alltoallv(self, send, sc, sd, recv, rc, rd):
        P, me = self.P, self.me
        what = self._next("alltoallv")
        if what is None:
            return 1
        sc, sd, rc, rd = (np.ctypeslib.as_array(p, shape=(P,)).astype(np.int64) for p in (sc, sd, rc, rd))
        out_cnt = self.want_cnt[:P]                                   # this rank's requests per owner
        in_cnt = np.array([a.size for a in self.asks], np.int64)      # the requests it receives per peer
        in_cnt[me] = out_cnt[me]
        unit = 4 if what == "requests" else self.W
        scnt, rcnt = (out_cnt, in_cnt) if what == "requests" else (in_cnt, out_cnt)
        soff, roff = _excl(scnt), _excl(rcnt)
        ok = self._layout(what, "scounts", sc, scnt * unit)
        ok = self._layout(what, "sdispls", sd, soff * unit) and ok
        ok = self._layout(what, "rcounts", rc, rcnt * unit) and ok
        ok = self._layout(what, "rdispls", rd, roff * unit) and ok
        if not ok:
            return 1  # (the buffers are laid out otherwise: nothing can be read or answered safely)
        sbuf = _view(send, int(scnt.sum()) * unit, np.uint32)
        rbuf = _view(recv, int(rcnt.sum()) * unit, np.uint32)
        if what == "requests":
            self.sent_req = sbuf.copy()
            if not np.array_equal(sbuf, self.want_req):
                k = int(np.flatnonzero(sbuf != self.want_req)[0])
                r = int(np.searchsorted(soff + scnt, k, side="right"))
                self.errors.append(f"requests to owner {r}: request {k - int(soff[r])} is {int(sbuf[k])}, expected "
                                   f"{int(self.want_req[k])} (idx - lo of the owner, in input order)")
            for r in range(P):
                if r != me and rcnt[r]:
                    rbuf[roff[r]:roff[r] + rcnt[r]] = self.asks[r]
            rbuf[roff[me]:roff[me] + rcnt[me]] = sbuf[soff[me]:soff[me] + scnt[me]]
        else:
            D = self.W // 4
            sbuf, rbuf = sbuf.reshape(-1, D), rbuf.reshape(-1, D)
            # the serve leg: for each peer in rank order, records[its requests]
            asked = [self.asks[r] for r in range(P)]
            asked[me] = self.sent_req[roff[me]:roff[me] + rcnt[me]]
            want = record_rule(self.first[me] + np.concatenate(asked).astype(np.uint64), self.W)
            if not np.array_equal(sbuf, want):
                k = int(np.flatnonzero((sbuf != want).any(axis=1))[0])
                r = int(np.searchsorted(soff + scnt, k, side="right"))
                self.errors.append(f"replies to peer {r}: record {k - int(soff[r])} is {sbuf[k].tolist()}, expected "
                                   f"{want[k].tolist()}")
            # the peers' replies: the records of the requests this rank sent, owner by owner
            rbuf[:] = record_rule(np.repeat(self.first, rcnt) + self.sent_req.astype(np.uint64), self.W)
            rbuf[roff[me]:roff[me] + rcnt[me]] = sbuf[soff[me]:soff[me] + scnt[me]]
        return 0


# ---------------------------------------------------------------------- a rank in numpy
FAULTS = ("reverse_owner", "swap_segments", "off_by_one", "swap_counts", "wrong_peer_order", "skip_callback")


class RankStopped(Exception):
    pass


def numpy_rank(dsort, t, P, me, first, records, idx, W, fault=None):
    """What dsort_sample_gather_dev does as rank `me`, in numpy, on the transport's two callbacks:
    the table by dsort.plan_gather_table, the routing by dsort.plan_gather_route, the documented
    sequence of callbacks, the unroute.  Returns out, (len(idx), W / 4) uint32; raises RankStopped
    when a callback or a gate fails.  fault: one of FAULTS, a deliberately wrong rank."""
    D = W // 4
    idx = np.asarray(idx, np.uint32)
    records = np.ascontiguousarray(records, np.uint32).reshape(-1, D)
    size_p = ctypes.POINTER(ctypes.c_size_t)

    def gate():
        st, every = np.zeros(1, np.int64), np.empty(P, np.int64)
        if t.allgather(None, st.ctypes.data, every.ctypes.data, 8) or every.any():
            raise RankStopped("gate")

    def allgather(row):
        row = np.ascontiguousarray(row, np.uint64)
        out = np.empty((P, row.size), np.uint64)
        if t.allgather(None, row.ctypes.data, out.ctypes.data, row.nbytes):
            raise RankStopped("all-gather")
        return out

    def alltoallv(sbuf, scnt, soff, rcnt, roff, unit):
        sbuf = np.ascontiguousarray(sbuf, np.uint32)
        rbuf = np.zeros(max(int(np.sum(rcnt)) * unit // 4, 1), np.uint32)
        a = [np.ascontiguousarray(np.asarray(x, np.int64) * unit, np.uintp) for x in (scnt, soff, rcnt, roff)]
        sp = sbuf.ctypes.data if sbuf.size else rbuf.ctypes.data
        if t.alltoallv(None, sp, a[0].ctypes.data_as(size_p), a[1].ctypes.data_as(size_p), rbuf.ctypes.data,
                       a[2].ctypes.data_as(size_p), a[3].ctypes.data_as(size_p)):
            raise RankStopped("all-to-all-v")
        return rbuf[:int(np.sum(rcnt)) * unit // 4]

    # 0. the range table
    gate()
    rows = allgather([int(first), records.shape[0], W])
    if (rows[:, 2] != rows[0, 2]).any():
        raise RankStopped("elem_bytes")
    lo, hi, owner = dsort.plan_gather_table(rows[:, 0], rows[:, 1])
    # 1. route
    counts, pos = dsort.plan_gather_route(lo, hi, owner, P, idx)
    counts, pos = counts.astype(np.int64), pos.astype(np.int64)
    bins, loc = owners_of(rows[:, 0], rows[:, 1], idx)
    owned = bins < P
    scnt = counts[:P].copy()
    soff = _excl(scnt)
    req = np.zeros(int(scnt.sum()), np.uint32)
    req[pos[owned]] = loc[owned]
    row = counts.copy()
    if fault == "swap_counts":
        a, b = _two_different(row[:P])
        row[[a, b]] = row[[b, a]]
    if fault != "skip_callback":
        gate()
    mat = allgather(row).astype(np.int64)
    if mat[:, P].any():
        raise RankStopped("unowned")
    rcnt = mat[:, me].copy()
    roff = _excl(rcnt)
    # 2. the requests
    seg = [req[soff[r]:soff[r] + scnt[r]] for r in range(P)]
    if fault == "reverse_owner":
        r = next(r for r in range(P) if not np.array_equal(seg[r], seg[r][::-1]))
        req[soff[r]:soff[r] + scnt[r]] = seg[r][::-1].copy()
    elif fault == "off_by_one":
        req[req.size // 2] += 1
    elif fault == "swap_segments":  # owner b's requests where owner a's belong, the displacements say so
        a, b = np.flatnonzero(scnt)[:2]
        place = list(range(P))
        place[a], place[b] = b, a
        at, soff = 0, soff.copy()
        for r in place:
            soff[r] = at
            at += scnt[r]
        req = np.concatenate([seg[r] for r in place])
    gate()
    rreq = alltoallv(req, scnt, soff, rcnt, roff, 4)
    # 3. serve, and the replies
    if fault == "wrong_peer_order":
        a, b = next((a, b) for a in range(P) for b in range(a + 1, P) if rcnt[a] == rcnt[b] and not np.array_equal(
            rreq[roff[a]:roff[a] + rcnt[a]], rreq[roff[b]:roff[b] + rcnt[b]]))
        rreq = rreq.copy()
        sa, sb = rreq[roff[a]:roff[a] + rcnt[a]].copy(), rreq[roff[b]:roff[b] + rcnt[b]].copy()
        rreq[roff[a]:roff[a] + rcnt[a]], rreq[roff[b]:roff[b] + rcnt[b]] = sb, sa
    rep = records[rreq.astype(np.int64)] if rreq.size else np.zeros((0, D), np.uint32)
    gate()
    back = alltoallv(rep.reshape(-1), rcnt, roff, scnt, soff, W).reshape(-1, D)
    # 4. unroute
    out = np.zeros((idx.size, D), np.uint32)
    if fault == "swap_segments":  # (its own layout: the position inside the owner's segment, at the moved start)
        pos = pos - _excl(counts[:P])[np.minimum(bins, P - 1)] + soff[np.minimum(bins, P - 1)]
    out[owned] = back[pos[owned]]
    return out


def _two_different(a):
    for i in range(len(a)):
        for j in range(i + 1, len(a)):
            if a[i] != a[j]:
                return i, j
    raise ValueError("all columns are equal")


# ---------------------------------------------------------------------- the cases
TABLES = ("equal", "reverse", "random", "alt_me_empty", "alt_me_owner", "gaps", "ones", "top")
PATTERNS = ("one_first", "one_last", "one_me", "round_robin", "uniform", "sorted", "own", "others", "repeats", "edges")
SCRIPTS = ("none", "each_once", "one_all_twice", "some")


def table(kind, P, me, c=37, rng=None):
    """(first, count) of P ranks, uint64; c records per range unless the kind says otherwise.
      equal         rank r owns [r c, (r + 1) c)
      reverse       ... chunk P - 1 - r: first descends with the rank
      random        ... chunk perm[r]
      alt_me_empty  every second rank holds nothing, `me` among them  (the table has fewer ranges than ranks)
      alt_me_owner  every second rank holds nothing, `me` holds records
      gaps          5 positions that nobody owns between two ranges, 11 before the first
      ones          ranges of one record
      top           the last range ends exactly at 2^32, the first starts below 2^31: the peers' ranges
                    are huge, only this rank's c records exist"""
    r = np.arange(P, dtype=np.uint64)
    count = np.full(P, c, np.uint64)
    if kind == "equal":
        first = r * np.uint64(c)
    elif kind == "reverse":
        first = (np.uint64(P - 1) - r) * np.uint64(c)
    elif kind == "random":
        first = rng.permutation(P).astype(np.uint64) * np.uint64(c)
    elif kind in ("alt_me_empty", "alt_me_owner"):
        keep = (r % 2 == me % 2) == (kind == "alt_me_owner")
        count = np.where(keep, c, 0).astype(np.uint64)
        first = _excl(count).astype(np.uint64)
    elif kind == "gaps":
        first = np.uint64(11) + r * np.uint64(c + 5)
    elif kind == "ones":
        count = np.ones(P, np.uint64)
        first = r + np.uint64(3)
    elif kind == "top":
        start = 2 ** 31 - 1000
        if P == 1:
            start = 2 ** 32 - c
        else:
            share = (2 ** 32 - start - c) // (P - 1)
            count = np.full(P, share, np.uint64)
            count[me] = c
            count[P - 1 if me != P - 1 else P - 2] += np.uint64(2 ** 32 - start - c - share * (P - 1))
        first = (np.uint64(start) + _excl(count).astype(np.uint64))
        assert int(first[-1]) + int(count[-1]) == 2 ** 32
    else:
        raise ValueError(kind)
    return first, count


def indices(kind, first, count, me, n, rng):
    """n indices (uint32) into the table; None when the table cannot give the pattern.
      one_first / one_last / one_me   all in the range of the first / last rank that holds records / of `me`
      round_robin   index j goes to the (j mod owners)-th owner: a wave of 256 meets min(256, owners) owners
      uniform       a random owner, a random position in its range
      sorted        ... in ascending order: long runs per owner across wave, tile and workgroup seams
      own / others  ranges of `me` only / of every rank but `me`
      repeats       nine in ten name ONE position
      edges         the first and the last position of every range, shuffled, cycled to n"""
    first, count = np.asarray(first, np.uint64).astype(np.int64), np.asarray(count, np.uint64).astype(np.int64)
    own = np.flatnonzero(count)
    if kind == "one_first":
        own = own[:1]
    elif kind == "one_last":
        own = own[-1:]
    elif kind in ("one_me", "own"):
        own = own[own == me]
    elif kind == "others":
        own = own[own != me]
    if own.size == 0:
        return None if n else np.zeros(0, np.uint32)
    j = np.arange(n, dtype=np.int64)
    if kind == "round_robin":
        r = own[j % own.size]
        g = first[r] + (j // own.size) % count[r]
    elif kind == "edges":
        e = np.concatenate([first[own], first[own] + count[own] - 1])
        g = rng.permutation(e)[j % e.size] if n else e[:0]
    else:
        r = own[rng.integers(0, own.size, n)]
        g = first[r] + (rng.random(n) * count[r]).astype(np.int64)
        if kind == "sorted":
            g = np.sort(g)
        elif kind == "repeats" and n:
            g[rng.random(n) < 0.9] = g[n // 2]
    assert g.size == n and (g >= 0).all() and (g < 2 ** 32).all()
    return g.astype(np.uint64).astype(np.uint32)


def top_cases():
    """(P, me, W, first, count, idx, asks) of the cases at the top of the position space: table
    "top", the first and last position of every range among uniform and sorted indices."""
    k = 0
    for P in (1, 2, 5, 256):
        for me in sorted({0, P // 2, P - 1}):
            rng = np.random.default_rng(1000 * P + me)
            first, count = table("top", P, me)
            idx = np.concatenate([indices("edges", first, count, me, 2 * P, rng),
                                  indices("uniform", first, count, me, 1500, rng),
                                  indices("sorted", first, count, me, 1100 + me, rng)])
            yield P, me, (4, 8, 16)[k % 3], first, count, idx, script("some", P, me, int(count[me]), rng)
            k += 1


def script(kind, P, me, n_src, rng):
    """{peer: requests} -- none: no peer asks; each_once: every peer asks for one record;
    one_all_twice: one peer asks for every record of this rank, twice over; some: a third of the
    peers ask for 1 .. 5 records, with repeats."""
    peers = [r for r in range(P) if r != me]
    if not n_src or not peers or kind == "none":
        return {}
    if kind == "each_once":
        return {r: rng.integers(0, n_src, 1) for r in peers}
    if kind == "one_all_twice":
        return {peers[len(peers) // 2]: np.concatenate([np.arange(n_src), np.arange(n_src)])}
    if kind == "some":
        return {r: rng.integers(0, n_src, int(rng.integers(1, 6))) for r in peers if rng.random() < 0.34}
    raise ValueError(kind)
