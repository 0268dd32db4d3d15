// dsort_exchange.hip -- the exchange layer (dsort_exch.h): the call scope, the bounded waits and
// the collectives over either transport, and on top of them the multi-GPU sample sort -- the bucket
// exchange (sample_sort_bx) and the sort-then-merge path (sample_sort).
#include <signal.h>
#include <string.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "dsort_bxlayout.h"
#include "dsort_exch.h"

namespace dsort {

static_assert(std::is_same<size_t, uint64_t>::value, "counts go to RCCL, the transport and the merge as they are");

void abort_comm_locked(dsort_ctx *ctx) {
    if (ctx->comm) ncclCommAbort(ctx->comm);
    ctx->comm = nullptr;
    ctx->has_transport = false;
    ctx->nranks = 1;
    ctx->rank = 0;
}

// (under the comm mutex: held by a running exchange or communicator set-up; dsort_comm_abort from
// another thread finds it taken and only raises ctx->abort_req, dsort.h)
static int refuse_call(dsort_ctx *ctx) {
    if (ctx->abort_req.load()) {
        abort_comm_locked(ctx);
        return set_err(ctx, DSORT_ECOMM, "communicator aborted (dsort_comm_abort)");
    }
    if (!ctx->comm && !ctx->has_transport)
        return set_err(ctx, DSORT_ECOMM, "communicator not initialised (dsort_comm_init)");
    return DSORT_OK;
}

ExchCall::ExchCall(dsort_ctx *ctx, void *stream, int ncoll)
    : lock(ctx->comm_mu),
      rc(refuse_call(ctx)),
      P(ctx->nranks),
      me(ctx->rank),
      host_tx(ctx->has_transport),
      s(pick_stream(ctx, stream)),
      deadline(ctx->opt.comm_timeout_ms > 0 ? tx_now_ms() + (double)ctx->opt.comm_timeout_ms : 0.0),
      seq(ctx->transport, P, deadline, ncoll),
      scope{ctx} {
    if (!rc && host_tx) {
        ctx->tx = &seq;
        guard.seq = &seq;
    }
}

int exch_leave(dsort_ctx *ctx, void *stream, int code) {
    const std::string err = ctx->err;
    {
        ExchCall call(ctx, stream, 1);
        call.failed(code);
    }  // (the guard's report, at the gate of the collective this rank never runs)
    ctx->err = err;
    return code;
}

// Every wait of an exchange: polls the stream, RCCL's asynchronous error (non-blocking
// communicator), the abort flag and the deadline, and aborts the communicator on a failure,
// instead of a hipStreamSynchronize that a dead peer would block forever.
// hold (DSORT_OPT_TEST_HOLD_EXCHANGE): the wait reports "not done" as if a peer never sent, until
// the abort flag or the deadline ends it.
int exch_wait(dsort_ctx *ctx, hipStream_t s, bool with_stream, double deadline, const char *what, bool hold) {
    PollPause pause;
    for (;;) {
        const hipError_t q0 = with_stream ? hipStreamQuery(s) : hipSuccess;
        const hipError_t q = hold && q0 == hipSuccess ? hipErrorNotReady : q0;
        ncclResult_t ae = ncclSuccess;
        if (ctx->comm) ncclCommGetAsyncError(ctx->comm, &ae);
        if (q == hipSuccess && ae != ncclInProgress && (ae == ncclSuccess || !ctx->comm)) return DSORT_OK;
        if (q != hipSuccess && q != hipErrorNotReady) return hip_err(ctx, q, what);
        if (ae != ncclSuccess && ae != ncclInProgress) {
            abort_comm_locked(ctx);
            return set_err(ctx, DSORT_ECOMM, std::string(what) + ": RCCL error " + ncclGetErrorString(ae) +
                                                 " (a peer failed); communicator aborted");
        }
        if (ctx->abort_req.load()) {
            abort_comm_locked(ctx);
            return set_err(ctx, DSORT_ECOMM, std::string(what) + ": aborted by dsort_comm_abort");
        }
        if (deadline > 0 && tx_now_ms() > deadline) {
            abort_comm_locked(ctx);
            return set_err(ctx, DSORT_ETIMEOUT, std::string(what) + ": no progress before the deadline "
                                                    "(DSORT_OPT_COMM_TIMEOUT_MS); communicator aborted");
        }
        pause();  // (a wait on the critical path of every exchange step)
    }
}

static void exchange_fault_point(dsort_ctx *ctx, int stage) {
    if (ctx->opt.kill_in_exchange == stage) raise(SIGKILL);
}

// DSORT_OPT_TEST_FAIL_EXCHANGE = k (host transport): a local error of this rank right before its
// k-th collective (0 = the key-count all-gather), returned like any other local error -- the
// sequence's guard reports it to the peers at the next gate (dsort_tx.h)
static int tx_fault_point(dsort_ctx *ctx) {
    if (ctx->tx && ctx->opt.test_fail_exchange >= 0 && ctx->opt.test_fail_exchange == ctx->tx->collectives_done())
        return set_err(ctx, DSORT_EHIP, "injected local failure before collective " +
                                            std::to_string(ctx->opt.test_fail_exchange) +
                                            " of the exchange (DSORT_OPT_TEST_FAIL_EXCHANGE)");
    return DSORT_OK;
}

int host_allgather(dsort_ctx *ctx, const void *send, void *recv, size_t bytes, const char *what) {
    if (int rc = tx_fault_point(ctx)) return rc;
    const int rc = ctx->tx->allgather(send, recv, bytes, what);
    return rc ? set_err(ctx, rc, ctx->tx->error()) : DSORT_OK;
}

int host_alltoallv(dsort_ctx *ctx, const void *send, const size_t *sc, const size_t *sd, void *recv,
                   const size_t *rcn, const size_t *rd, const char *what) {
    if (int rc = tx_fault_point(ctx)) return rc;
    const int rc = ctx->tx->alltoallv(send, sc, sd, recv, rcn, rd, what);
    return rc ? set_err(ctx, rc, ctx->tx->error()) : DSORT_OK;
}

int allgather_u64(dsort_ctx *ctx, const uint64_t *src, size_t count, uint64_t *out, hipStream_t s, double deadline,
                  const char *what) {
    const int P = ctx->nranks;
    if (ctx->has_transport) {
        if (!ctx->tx) return set_err(ctx, DSORT_EINVAL, std::string(what) + ": no sample sort running");
        return host_allgather(ctx, src, out, count * 8, what);
    }
    const size_t bytes = count * 8 * (size_t)(P + 1);
    int rc = ensure(ctx, ctx->small, bytes, "sample-sort small buffers");
    if (rc) return rc;
    if ((rc = ensure_small_host(ctx, bytes))) return rc;
    uint64_t *d = ctx->small.as<uint64_t>(), *h = ctx->small_host.as<uint64_t>();
    memcpy(h, src, count * 8);
    DSORT_HIP(ctx, hipMemcpyAsync(d, h, count * 8, hipMemcpyHostToDevice, s));
    DSORT_NCCLNB(ctx, ncclAllGather(d, d + count, count, ncclUint64, ctx->comm, s));
    rc = exch_wait(ctx, s, false, deadline, what);
    if (rc) return rc;
    DSORT_HIP(ctx, hipMemcpyAsync(h + count, d + count, count * 8 * (size_t)P, hipMemcpyDeviceToHost, s));
    rc = exch_wait(ctx, s, true, deadline, what);
    if (rc) return rc;
    memcpy(out, h + count, count * 8 * (size_t)P);
    return DSORT_OK;
}

int rccl_group(dsort_ctx *ctx, const A2av &a, hipStream_t s, double deadline, const char *what) {
    const int P = ctx->nranks, me = ctx->rank;
    const size_t per = a.unit / (a.type == ncclInt64 || a.type == ncclUint64 ? 8 : 4);  // wire elements of one
    const char *sb = static_cast<const char *>(a.sbuf);
    char *rb = static_cast<char *>(a.rbuf);
    DSORT_NCCLNB(ctx, ncclGroupStart());
    for (int r = 0; r < P; ++r) {
        if (r == me) continue;
        if (a.scnt[r]) DSORT_NCCLNB(ctx, ncclSend(sb + a.soff[r] * a.unit, a.scnt[r] * per, a.type, r, ctx->comm, s));
        if (a.rcnt[r]) DSORT_NCCLNB(ctx, ncclRecv(rb + a.roff[r] * a.unit, a.rcnt[r] * per, a.type, r, ctx->comm, s));
    }
    DSORT_NCCLNB(ctx, ncclGroupEnd());
    // (a non-blocking communicator may still be enqueueing the group: whatever the caller puts on
    // the stream next goes behind its kernels)
    return exch_wait(ctx, s, false, deadline, (std::string(what) + " (enqueue)").c_str());
}

int a2av_peers(dsort_ctx *ctx, const A2av &a, hipStream_t s, double deadline, const char *what, const char *staging) {
    if (!ctx->has_transport) return rccl_group(ctx, a, s, deadline, what);
    const int P = ctx->nranks;
    int rc = ensure_host(ctx, ctx->xfer, (a.stotal ? a.stotal : 1) * a.unit);
    if (rc) return rc;
    rc = ensure_host(ctx, ctx->xfer2, (a.rtotal ? a.rtotal : 1) * a.unit);
    if (rc) return rc;
    if (a.stotal) DSORT_HIP(ctx, hipMemcpyAsync(ctx->xfer.p, a.sbuf, a.stotal * a.unit, hipMemcpyDeviceToHost, s));
    rc = exch_wait(ctx, s, true, deadline, staging);
    if (rc) return rc;
    std::vector<size_t> sc(P), sd(P), rcn(P), rd(P);
    for (int r = 0; r < P; ++r) {
        sc[r] = a.scnt[r] * a.unit;
        sd[r] = a.soff[r] * a.unit;
        rcn[r] = a.rcnt[r] * a.unit;
        rd[r] = a.roff[r] * a.unit;
    }
    rc = host_alltoallv(ctx, ctx->xfer.p, sc.data(), sd.data(), ctx->xfer2.p, rcn.data(), rd.data(), what);
    if (rc) return rc;
    if (a.rtotal) DSORT_HIP(ctx, hipMemcpyAsync(a.rbuf, ctx->xfer2.p, a.rtotal * a.unit, hipMemcpyHostToDevice, s));
    return DSORT_OK;
}

int a2av_own(dsort_ctx *ctx, const A2av &a, hipStream_t s) {
    const int me = ctx->rank;
    if (!ctx->has_transport && a.scnt[me])
        DSORT_HIP(ctx, hipMemcpyAsync(static_cast<char *>(a.rbuf) + a.roff[me] * a.unit,
                                      static_cast<const char *>(a.sbuf) + a.soff[me] * a.unit, a.scnt[me] * a.unit,
                                      hipMemcpyDeviceToDevice, s));
    return DSORT_OK;
}

// ------------------------------------------------------------------ sample sort ---------
static const int kSamplesPerRank = 512;

template <typename T> static ncclDataType_t nccl_type();
template <> ncclDataType_t nccl_type<int32_t>() { return ncclInt32; }
template <> ncclDataType_t nccl_type<int64_t>() { return ncclInt64; }

// (the splitter rule is the C ABI's restatement, dsort_api.hip)
static int plan_splitters(int P, int S, const int32_t *hs, const uint64_t *idx, int32_t *sv, int32_t *sr, uint64_t *si) {
    return dsort_plan_splitters_i32(P, S, hs, idx, sv, sr, si);
}
static int plan_splitters(int P, int S, const int64_t *hs, const uint64_t *idx, int64_t *sv, int32_t *sr, uint64_t *si) {
    return dsort_plan_splitters_i64(P, S, hs, idx, sv, sr, si);
}

// Regular samples of a sorted local run: sample j = keys[(j+1)*n/(s+1)].
template <typename T>
__global__ void sample_kernel(const T *keys, uint64_t n, int s, T *out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= s) return;
    if (n == 0) {
        out[j] = sizeof(T) == 4 ? (T)INT32_MAX : (T)INT64_MAX;
        return;
    }
    uint64_t idx = (uint64_t)(j + 1) * n / (uint64_t)(s + 1);
    if (idx >= n) idx = n - 1;
    out[j] = keys[idx];
}

// Composite-splitter cut positions in a sorted local run (same rule as dsort_plan_cuts_*):
// keys of this rank below splitter (v, r, i) in (value, rank, index) order.
template <typename T>
__global__ void cuts_kernel(const T *keys, uint64_t n, int my_rank, int nsplit, const T *sv,
                            const int32_t *sr, const uint64_t *si, uint64_t *cuts) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j > nsplit) return;
    if (j == 0) {
        cuts[0] = 0;
        cuts[nsplit + 1] = n;
    }
    if (j == nsplit) return;
    const T v = sv[j];
    const int r = sr[j];
    uint64_t pos;
    if (r == my_rank) {
        pos = si[j] < n ? si[j] : n;
    } else {
        const bool upper = my_rank < r;  // equal keys of lower ranks go left
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            const bool left = upper ? (keys[mid] <= v) : (keys[mid] < v);
            if (left) lo = mid + 1;
            else hi = mid;
        }
        pos = lo;
    }
    cuts[j + 1] = pos;
}

// The context's comm stream (the bucket exchange's sends and receives) and its events.
static int comm_stream(dsort_ctx *ctx) {
    // (the highest priority: a hardware queue of its own -- a stream created after the sort's may
    // share its queue, and then nothing on it runs beside the sort's kernels)
    int lo = 0, hi = 0;
    if (!ctx->xs && (hipDeviceGetStreamPriorityRange(&lo, &hi) != hipSuccess ||
                     hipStreamCreateWithPriority(&ctx->xs.h, hipStreamNonBlocking, hi) != hipSuccess))
        return set_err(ctx, DSORT_EHIP, "hipStreamCreate (comm stream)");
    for (auto &e : ctx->xev)
        if (!e && hipEventCreateWithFlags(&e.h, hipEventDisableTiming) != hipSuccess)
            return set_err(ctx, DSORT_EHIP, "hipEventCreate (comm stream)");
    return DSORT_OK;
}

// DSORT_OPT_TEST_WAVE_FENCE (test only): fingerprints (fingerprint_kernel: sum and xor of
// splitmix64, order independent) of device ranges taken on the sort stream before and after a step
// of the exchange; any range that changed fails the sort with DSORT_EHIP naming it.  Value 2 tests
// the fence itself: one key of the first range is flipped between the two prints.
template <typename T>
__global__ void fence_poke_kernel(T *p) {
    p[0] ^= (T)1;
}

template <typename T>
struct WaveFence {
    struct R {
        const T *p;
        uint64_t n;
        std::string what;
    };
    std::vector<R> r;
    bool on() const { return !r.empty(); }
    void add(const T *p, uint64_t n, std::string what) {
        if (n) r.push_back(R{p, n, std::move(what)});
    }
    int prepare(dsort_ctx *ctx) {
        if (r.empty()) return DSORT_OK;
        const size_t bytes = r.size() * 4 * sizeof(unsigned long long);
        int rc = ensure(ctx, ctx->fence, bytes, "wave fence");
        return rc ? rc : ensure_host(ctx, ctx->fence_host, bytes);
    }
    // which = 0: before, 1: after
    int print(dsort_ctx *ctx, hipStream_t s, int which) {
        auto *acc = ctx->fence.as<unsigned long long>() + (size_t)which * 2 * r.size();
        DSORT_HIP(ctx, hipMemsetAsync(acc, 0, r.size() * 2 * sizeof(unsigned long long), s));
        for (size_t i = 0; i < r.size(); ++i)
            if (int rc = fingerprint_launch<T>(ctx, r[i].p, r[i].n, acc + 2 * i, s)) return rc;
        return DSORT_OK;
    }
    int check(dsort_ctx *ctx, hipStream_t s, double deadline) {
        if (ctx->opt.test_wave_fence == 2) {
            hipLaunchKernelGGL((fence_poke_kernel<T>), dim3(1), dim3(1), 0, s, const_cast<T *>(r[0].p));
            DSORT_HIP(ctx, hipGetLastError());
        }
        int rc = print(ctx, s, 1);
        if (rc) return rc;
        const size_t m = r.size() * 4;
        DSORT_HIP(ctx, hipMemcpyAsync(ctx->fence_host.p, ctx->fence.p, m * sizeof(unsigned long long),
                                      hipMemcpyDeviceToHost, s));
        if ((rc = exch_wait(ctx, s, true, deadline, "wave fence"))) return rc;
        const auto *h = ctx->fence_host.as<const unsigned long long>();
        const size_t R2 = 2 * r.size();
        for (size_t i = 0; i < r.size(); ++i)
            if (h[2 * i] != h[R2 + 2 * i] || h[2 * i + 1] != h[R2 + 2 * i + 1])
                return set_err(ctx, DSORT_EHIP, "DSORT_OPT_TEST_WAVE_FENCE: wave 0's second level / tile sort changed " +
                                                    r[i].what + " (" + std::to_string(r[i].n) + " keys)");
        ctx->stats.fence_ranges += (int)r.size();
        return DSORT_OK;
    }
};

// The bucket exchange (dsort_internal.h): samples of the unsorted keys from every
// rank -> the same Btot global splitters everywhere -> this rank's keys partitioned into the Btot
// buckets (the first level of the one-GPU sort) -> buckets [q Bl, (q+1) Bl) to rank q (RCCL
// grouped send/recv over xGMI) -> the received pieces of this rank's Bl buckets finished by the
// second level and the tile sort.  Replaces the gather + merge_chunks of server.c:414-415 and
// 500-515: nothing is merged.
template <typename T>
static int sample_sort_bx(dsort_ctx *ctx, const T *d_in, const BxPlan &pl, T **d_out, size_t *n_out, hipStream_t s,
                          double deadline) {
    const int P = pl.P, me = pl.me, Bl = pl.Bl, Bt = pl.Btot;
    const bool host_tx = ctx->has_transport;
    if (host_tx) ctx->tx->plan(2 + bx_waves(Bl));  // samples, bucket starts, the waves (dsort_tx.h)
    const size_t rec = (size_t)pl.s_max * sizeof(BxSample);
    int rc = ensure(ctx, ctx->bxs, rec * (size_t)(P + 1), "bucket-exchange samples");
    if (rc) return rc;
    BxSample *mine = ctx->bxs.as<BxSample>(), *all = mine + pl.s_max;
    // 1. samples, all-gathered
    if ((rc = bx_sample<T>(ctx, d_in, pl, mine, s))) return rc;
    if (!host_tx) {
        DSORT_NCCLNB(ctx, ncclAllGather(mine, all, (size_t)pl.s_max * 2, ncclInt64, ctx->comm, s));
        rc = exch_wait(ctx, s, false, deadline, "sample all-gather (enqueue)");
        if (rc) return rc;
    } else {
        rc = ensure_host(ctx, ctx->xfer, rec * (size_t)(P + 1));
        if (rc) return rc;
        char *hm = ctx->xfer.as<char>(), *ha = hm + rec;
        DSORT_HIP(ctx, hipMemcpyAsync(hm, mine, rec, hipMemcpyDeviceToHost, s));
        rc = exch_wait(ctx, s, true, deadline, "samples");
        if (rc) return rc;
        if ((rc = host_allgather(ctx, hm, ha, rec, "samples all-gather"))) return rc;
        DSORT_HIP(ctx, hipMemcpyAsync(all, ha, rec * (size_t)P, hipMemcpyHostToDevice, s));
    }
    exchange_fault_point(ctx, 1);
    // 2. global splitters and this rank's first partition level (the host waits for the bucket
    //    starts while the scatter runs); kill stage 0
    const uint64_t *hb;
    T *part;
    std::vector<uint8_t> pure;
    rc = bx_partition<T>(ctx, d_in, pl, all, s, true, &hb, &part, pure);
    if (rc) return rc;
    // 3. every rank's bucket starts, on the comm stream: they are on the host before the scatter
    //    ends, so the all-gather, the exchange's enqueue and the first wave's tables overlap it (on
    //    the sort stream they queued behind it: about 0.14 ms of idle GPU per 2^27-key rank)
    if (!host_tx && (rc = comm_stream(ctx))) return rc;
    std::vector<uint64_t> hb_all((size_t)P * (Bt + 1));
    {
        const std::vector<uint64_t> mine_hb(hb, hb + Bt + 1);
        rc = allgather_u64(ctx, mine_hb.data(), (size_t)Bt + 1, hb_all.data(), host_tx ? s : ctx->xs, deadline,
                           "bucket starts all-gather");
        if (rc) return rc;
    }
    // The layout of the waves (dsort_bxlayout.h): over RCCL the second level of wave 0 runs while
    // wave 1's keys are on the links (the sends and receives go on the comm stream; the sort stream
    // waits for each wave's event).  (The host transport and a single rank run the same waves one
    // after the other: the same layout and second-level calls as the 8-GPU run.)
    const BxLayout L = bx_layout(P, me, Bl, pl.n_local, pl.recv_room, hb_all, pure);
    const int W = L.W;
    const int *jb = L.jb;
    if (!L.behind) {
        rc = ensure(ctx, ctx->recv, (L.nrecv ? L.nrecv : 1) * sizeof(T) + 16, "receive buffer");
        if (rc) return rc;
    }
    rc = ensure(ctx, ctx->recv2, (L.nout ? L.nout : 1) * sizeof(T), "sorted slice");
    if (rc) return rc;
    T *rb = L.behind ? part : ctx->recv.as<T>();  // (the second level's source)
    T *outp = ctx->recv2.as<T>();
    exchange_fault_point(ctx, 2);
    // DSORT_OPT_TEST_WAVE_FENCE: what wave 1 still needs while wave 0's second level and tile sort
    // run -- its sends (part, every q != me), this rank's own wave-1 buckets (read in place when
    // `behind`) and its landing zone -- fingerprinted before and after wave 0 (dsort.h).  Set up before anything is
    // enqueued on the comm stream (the arena may grow)
    WaveFence<T> fence;
    if (ctx->opt.test_wave_fence && W == 2) {
        for (int q = 0; q < P; ++q) {
            const size_t k = (size_t)P + q;  // (wave 1)
            fence.add(part + L.soff[k], L.scnt[k], q != me ? "wave-1 send range of part to rank " + std::to_string(q)
                                                           : std::string("this rank's own wave-1 buckets in part"));
            // (over RCCL with peers the landing zone fills while wave 0 runs: not fenced there)
            if (!(L.behind && q == me) && (host_tx || P == 1))
                fence.add(rb + L.rpos[k], L.rcnt[k], "wave-1 landing zone of the keys from rank " + std::to_string(q));
        }
        if ((rc = fence.prepare(ctx))) return rc;
    }
    // wave w's keys are in rb on s: its second level and tile sort, under the fence around wave 0's
    uint64_t out_off = 0;
    auto finish_wave = [&](int w) -> int {
        int rc = DSORT_OK;
        if (w == 0 &&  // (its keys are in)
            ((rc = stage_event(ctx, s, true, kEvAllToAll1)) || (rc = stage_event(ctx, s, true, kEvExchangeDone))))
            return rc;
        if (w == 0 && fence.on() && (rc = fence.print(ctx, s, 0))) return rc;
        uint64_t nw = 0;
        rc = bx_local_sort<T>(ctx, rb, outp, pl, hb_all.data(), L.hc_all.data(), L.base.data() + (size_t)w * P, jb[w],
                              jb[w + 1], out_off, w, W, s, true, &nw);
        if (rc) return rc;
        out_off += nw;
        return w == 0 && fence.on() ? fence.check(ctx, s, deadline) : DSORT_OK;
    };
    // 4. the buckets to their ranks: per wave one send and one receive per peer (all-to-all-v over
    //    xGMI), on the comm stream after the partition
    if ((rc = stage_event(ctx, s, true, kEvAllToAll0))) return rc;
    if (host_tx) {
        // The same order as RCCL's: wave w's send ranges are staged from `part` right
        // before its all-to-all, and wave w's second level and tile sort are queued before wave
        // w+1 is staged -- so wave 1's sends are read from `part` after wave 0's kernels ran on it,
        // as the 8-GPU run reads them while those kernels run.  The host buffer mirrors `part`
        // (send displacements = positions in part); the receive layout is the device one minus
        // the partition (behind: the other sources from n_local on, this rank's own buckets not
        // shipped).
        rc = ensure_host(ctx, ctx->xfer, (pl.n_local ? pl.n_local : 1) * sizeof(T));
        if (rc) return rc;
        rc = ensure_host(ctx, ctx->xfer2, (L.nrecv ? L.nrecv : 1) * sizeof(T));
        if (rc) return rc;
        const uint64_t shift = L.behind ? pl.n_local : 0;
        for (int w = 0; w < W; ++w) {
            std::vector<size_t> sc(P), sd(P), rcn(P), rd(P);
            uint64_t lo = ~0ull, hi = 0;
            for (int q = 0; q < P; ++q) {
                const size_t k = (size_t)w * P + q;
                const bool self = L.behind && q == me;
                sd[q] = L.soff[k] * sizeof(T);
                sc[q] = self ? 0 : L.scnt[k] * sizeof(T);
                rcn[q] = self ? 0 : L.rcnt[k] * sizeof(T);
                rd[q] = self ? 0 : (L.rpos[k] - shift) * sizeof(T);
                if (sc[q])  // (stage this wave's range for q, and nothing else)
                    DSORT_HIP(ctx, hipMemcpyAsync(ctx->xfer.as<char>() + sd[q], part + L.soff[k], sc[q],
                                                  hipMemcpyDeviceToHost, s));
                if (!self && L.rcnt[k]) {
                    lo = std::min<uint64_t>(lo, L.rpos[k]);
                    hi = std::max<uint64_t>(hi, L.rpos[k] + L.rcnt[k]);
                }
            }
            rc = exch_wait(ctx, s, true, deadline, w ? "key staging (wave 1)" : "key staging (wave 0)");
            if (rc) return rc;
            rc = host_alltoallv(ctx, ctx->xfer.p, sc.data(), sd.data(), ctx->xfer2.p, rcn.data(), rd.data(),
                                w ? "key all-to-all (wave 1)" : "key all-to-all (wave 0)");
            if (rc) return rc;
            if (hi > lo)
                DSORT_HIP(ctx, hipMemcpyAsync(rb + lo, ctx->xfer2.as<char>() + (lo - shift) * sizeof(T),
                                              (hi - lo) * sizeof(T), hipMemcpyHostToDevice, s));
            if ((rc = finish_wave(w))) return rc;
        }
    } else {
        const hipStream_t cs = ctx->xs;
        DSORT_HIP(ctx, hipEventRecord(ctx->xev[2], s));
        DSORT_HIP(ctx, hipStreamWaitEvent(cs, ctx->xev[2], 0));
        for (int w = 0; w < W; ++w) {
            const size_t k0 = (size_t)w * P;
            const A2av a{part, L.scnt.data() + k0, L.soff.data() + k0, 0, rb, L.rcnt.data() + k0, L.rpos.data() + k0, 0,
                         sizeof(T), nccl_type<T>()};  // (the totals: the host transport's staging only)
            // (the wave's event goes on the stream behind the group's kernels and its own part)
            if ((rc = rccl_group(ctx, a, cs, deadline, "key all-to-all"))) return rc;
            if (!L.behind && (rc = a2av_own(ctx, a, cs))) return rc;
            DSORT_HIP(ctx, hipEventRecord(ctx->xev[w], cs));
        }
        // 5. the second level and the tile sort of this rank's buckets, wave by wave, each queued behind
        //    its receives while later waves are in flight (the host builds and uploads a wave's tables
        //    meanwhile); the host waits inside poll the abort flag and the deadline, as a dead peer never
        //    completes the stream.  Kill stages 1 and 2 (after the first wave's).
        ctx->poll_waits = true;
        ctx->poll_deadline = deadline;
        ctx->poll_stream = s;
        for (int w = 0; w < W && !rc; ++w) {
            const hipError_t e = hipStreamWaitEvent(s, ctx->xev[w], 0);
            rc = e != hipSuccess ? hip_err(ctx, e, "hipStreamWaitEvent (wave)") : finish_wave(w);
        }
        ctx->poll_waits = false;
        if (rc) {
            // The arenas the second level replaced while the keys were in flight (release_dev) are
            // freed once no kernel can touch them (a faulted sort kept its multi-GB scratch
            // until the next good exchange, so the recovery ran at twice the footprint).  After a
            // communicator failure the abort ends the comm stream's kernels; after a local failure
            // every send and receive was enqueued and still completes: wait for it, bounded by the
            // deadline and the abort flag (a failing wait aborts the communicator).
            if (rc == DSORT_ECOMM || rc == DSORT_ETIMEOUT) {
                abort_comm_locked(ctx);
            } else {
                const std::string err = ctx->err;
                (void)exch_wait(ctx, cs, true, deadline, "key all-to-all (after a local failure)");
                ctx->err = err;
            }
        } else {
            // the receives have landed (and the test hold, DSORT_OPT_TEST_HOLD_EXCHANGE, is released)
            rc = exch_wait(ctx, cs, true, deadline, "key all-to-all", ctx->opt.test_hold_exchange != 0);
        }
        if (rc) {
            // (a failed final wait has aborted the communicator, or met a HIP error: the arenas the
            // second level replaced go once the sort stream is idle, as on the failures above --
            // tests/test_gpu_faults.py::test_faulted_exchanges_release_replaced_arenas)
            if (hipStreamSynchronize(s) == hipSuccess) flush_later(ctx);
            return rc;
        }
    }
    flush_later(ctx);  // (the buffers the second level replaced while the keys were in flight)
    ctx->last_stream = s;
    ctx->stats.keys_in = pl.n_local;
    ctx->stats.keys_out = L.nout;
    ctx->stats.keys_sent = L.sent;
    ctx->stats.exchange_path = 1;
    *d_out = outp;
    *n_out = L.nout;
    return DSORT_OK;
}

template <typename T>
static int sample_sort(dsort_ctx *ctx, const T *d_in, size_t n_local, T **d_out, size_t *n_out,
                       void *stream, bool presorted) {
    if (!ctx || !d_out || !n_out || (n_local && !d_in)) return set_err(ctx, DSORT_EINVAL, "null argument");
    // The first collective is the key-count all-gather (the presorted entry starts with the samples).
    ExchCall call(ctx, stream, presorted ? 3 : 1);
    if (call.rc) return call.rc;
    const hipStream_t s = call.s;
    const double deadline = call.deadline;
    const int P = call.P, me = call.me, S = kSamplesPerRank;
    const bool host_tx = call.host_tx;
    int rc;
    if (!presorted) {
        // every rank's key count decides the path, the same on every rank: the bucket exchange, or
        // (small inputs, partition switched off) sort locally and merge the received runs
        std::vector<uint64_t> n_of(P);
        const uint64_t nl = n_local;
        rc = allgather_u64(ctx, &nl, 1, n_of.data(), s, deadline, "key count all-gather");
        if (rc) return rc;
        BxPlan pl;
        if (bx_make_plan(ctx->opt, P, me, n_of.data(), (int)sizeof(T), pl)) {
            ctx->stats = fresh_stats();
            return sample_sort_bx<T>(ctx, d_in, pl, d_out, n_out, s, deadline);
        }
        if (host_tx) call.seq.plan(3);  // samples, count matrix, keys
    }
    const T *d_keys;
    dsort_stats st = fresh_stats();
    if (presorted) {
        // the caller already holds a sorted local run (fault recovery: a survivor merged the
        // chunks it sorted)
        d_keys = d_in;
        ctx->ev_mask = 0;
        ctx->last_stream = s;
        for (int e = kEvStart; e <= kEvLocalDone; ++e)  // (no local sort: its three events at once)
            if ((rc = stage_event(ctx, s, true, StageEv(e)))) return rc;
        st.keys_in = n_local;
    } else {
        // 1. local sort (the worker's merge_sort) into the context's local arena
        rc = ensure(ctx, ctx->local, (n_local ? n_local : 1) * sizeof(T), "local run");
        if (rc) return rc;
        T *dk = ctx->local.as<T>();
        rc = sort_device<T>(ctx, d_in, dk, n_local, s, true);
        if (rc) return rc;
        d_keys = dk;
        st = ctx->stats;
    }
    // device small-area layout
    const size_t off_samp = 0;                                   // S keys
    const size_t off_all = off_samp + (size_t)S * sizeof(T);      // P*S keys
    const size_t off_n = off_all + (size_t)P * S * sizeof(T);     // P uint64 (n_local of all)
    const size_t off_sv = off_n + (size_t)P * 8;                  // P keys (splitter values)
    const size_t off_sr = off_sv + (size_t)P * sizeof(T);         // P int32
    const size_t off_si = off_sr + (size_t)P * 8;                 // P uint64
    const size_t off_cut = off_si + (size_t)P * 8;                // P+1 uint64
    const size_t off_cnt = off_cut + (size_t)(P + 1) * 8;         // 1 uint64 (n_local)
    // (and room for the count all-gather, P + P*P uint64 from 0 on: it never regrows the arenas)
    const size_t total_small = off_cnt + (size_t)P * 8 + (size_t)P * P * 8 + 64;
    rc = ensure(ctx, ctx->small, total_small, "sample-sort small buffers");
    if (rc) return rc;
    if ((rc = ensure_small_host(ctx, total_small))) return rc;
    char *dsm = ctx->small.as<char>();
    char *hsm = ctx->small_host.as<char>();
    // 2. regular samples + local size
    hipLaunchKernelGGL((sample_kernel<T>), dim3((S + 255) / 256), dim3(256), 0, s, d_keys,
                       (uint64_t)n_local, S, reinterpret_cast<T *>(dsm + off_samp));
    DSORT_HIP(ctx, hipGetLastError());
    uint64_t nl = n_local;
    DSORT_HIP(ctx, hipMemcpyAsync(dsm + off_cnt, &nl, 8, hipMemcpyHostToDevice, s));
    // 3. all-gather samples and sizes
    if (!host_tx) {
        DSORT_NCCLNB(ctx, ncclGroupStart());
        DSORT_NCCLNB(ctx, ncclAllGather(dsm + off_samp, dsm + off_all, (size_t)S, nccl_type<T>(), ctx->comm, s));
        DSORT_NCCLNB(ctx, ncclAllGather(dsm + off_cnt, dsm + off_n, 1, ncclUint64, ctx->comm, s));
        DSORT_NCCLNB(ctx, ncclGroupEnd());
        rc = exch_wait(ctx, s, false, deadline, "sample all-gather (enqueue)");
        if (rc) return rc;
        DSORT_HIP(ctx, hipMemcpyAsync(hsm + off_all, dsm + off_all, (size_t)P * S * sizeof(T) + (size_t)P * 8,
                                      hipMemcpyDeviceToHost, s));
        rc = exch_wait(ctx, s, true, deadline, "sample all-gather");
        if (rc) return rc;
    } else {
        // [S samples | n_local] per rank through the caller's all-gather
        const size_t rec = (size_t)S * sizeof(T) + 8;
        rc = ensure_host(ctx, ctx->xfer, rec * (size_t)(P + 1));
        if (rc) return rc;
        char *mine = ctx->xfer.as<char>(), *all = mine + rec;
        DSORT_HIP(ctx, hipMemcpyAsync(mine, dsm + off_samp, (size_t)S * sizeof(T), hipMemcpyDeviceToHost, s));
        rc = exch_wait(ctx, s, true, deadline, "local sort");
        if (rc) return rc;
        memcpy(mine + (size_t)S * sizeof(T), &nl, 8);
        if ((rc = host_allgather(ctx, mine, all, rec, "samples all-gather"))) return rc;
        for (int r = 0; r < P; ++r) {
            memcpy(hsm + off_all + (size_t)r * S * sizeof(T), all + (size_t)r * rec, (size_t)S * sizeof(T));
            memcpy(hsm + off_n + (size_t)r * 8, all + (size_t)r * rec + (size_t)S * sizeof(T), 8);
        }
    }
    exchange_fault_point(ctx, 1);
    // 4. splitters on the host (tiny: P*S composites)
    {
        const T *hs = reinterpret_cast<const T *>(hsm + off_all);
        const uint64_t *hn = reinterpret_cast<const uint64_t *>(hsm + off_n);
        std::vector<uint64_t> idx((size_t)P * S);
        for (int r = 0; r < P; ++r) dsort_plan_sample_positions(hn[r], S, &idx[(size_t)r * S]);
        T *sv = reinterpret_cast<T *>(hsm + off_sv);
        int32_t *sr = reinterpret_cast<int32_t *>(hsm + off_sr);
        uint64_t *si = reinterpret_cast<uint64_t *>(hsm + off_si);
        rc = plan_splitters(P, S, hs, idx.data(), sv, sr, si);
        if (rc) return set_err(ctx, rc, "splitter planning failed");
        DSORT_HIP(ctx, hipMemcpyAsync(dsm + off_sv, hsm + off_sv, off_cut - off_sv, hipMemcpyHostToDevice, s));
    }
    // 5. cuts and send counts (out of the small arenas: the count all-gather uses them from 0 on)
    hipLaunchKernelGGL((cuts_kernel<T>), dim3(1), dim3(((P + 63) / 64) * 64), 0, s, d_keys,
                       (uint64_t)n_local, me, P - 1, reinterpret_cast<const T *>(dsm + off_sv),
                       reinterpret_cast<const int32_t *>(dsm + off_sr),
                       reinterpret_cast<const uint64_t *>(dsm + off_si),
                       reinterpret_cast<uint64_t *>(dsm + off_cut));
    DSORT_HIP(ctx, hipGetLastError());
    DSORT_HIP(ctx, hipMemcpyAsync(hsm + off_cut, dsm + off_cut, (size_t)(P + 1) * 8, hipMemcpyDeviceToHost, s));
    rc = exch_wait(ctx, s, true, deadline, "cut search");
    if (rc) return rc;
    const uint64_t *cut0 = reinterpret_cast<const uint64_t *>(hsm + off_cut);
    const std::vector<uint64_t> hcut(cut0, cut0 + P + 1);
    std::vector<uint64_t> hcnt(P);
    for (int r = 0; r < P; ++r) hcnt[r] = hcut[r + 1] - hcut[r];
    // 6. count matrix
    std::vector<uint64_t> mat((size_t)P * P);  // mat[src*P + dst]
    rc = allgather_u64(ctx, hcnt.data(), (size_t)P, mat.data(), s, deadline, "count all-gather");
    if (rc) return rc;
    std::vector<size_t> rlen(P);
    std::vector<uint64_t> roff(P + 1, 0);
    for (int r = 0; r < P; ++r) {
        rlen[r] = mat[(size_t)r * P + me];
        roff[r + 1] = roff[r] + rlen[r];
    }
    const uint64_t nrecv = roff[P];
    rc = ensure(ctx, ctx->recv, (nrecv ? nrecv : 1) * sizeof(T), "receive buffer");
    if (rc) return rc;
    rc = ensure(ctx, ctx->recv2, (nrecv ? nrecv : 1) * sizeof(T), "merge output");
    if (rc) return rc;
    T *rb = ctx->recv.as<T>();
    exchange_fault_point(ctx, 2);
    uint64_t sent = 0;
    for (int r = 0; r < P; ++r) sent += r == me ? 0 : hcnt[r];
    if ((rc = stage_event(ctx, s, true, kEvAllToAll0))) return rc;
    // 7. key exchange: one send and one receive per peer link, grouped (RCCL all-to-all-v), or
    //    host-staged: D2H the sorted run, exchange, H2D the received runs.  Stage event 6 sits behind
    //    the peers' keys: in front of RCCL's own part.
    const A2av a{d_keys, hcnt.data(), hcut.data(), n_local, rb, rlen.data(), roff.data(), nrecv, sizeof(T), nccl_type<T>()};
    if ((rc = a2av_peers(ctx, a, s, deadline, "key all-to-all", "key staging"))) return rc;
    if ((rc = stage_event(ctx, s, true, kEvAllToAll1)) || (rc = a2av_own(ctx, a, s)) ||
        (rc = stage_event(ctx, s, true, kEvExchangeDone)))
        return rc;
    // 8. merge the P received runs (source-rank order keeps the merge deterministic); the
    // local sort's statistics and per-launch events stay
    T *outp = ctx->recv2.as<T>();
    rc = merge_device<T>(ctx, rb, rlen.data(), P, outp, s, true);
    if (rc) return rc;
    if (!host_tx) {  // the receives must have landed before the caller reads the slice
        rc = exch_wait(ctx, s, true, deadline, "key all-to-all", ctx->opt.test_hold_exchange != 0);
        if (rc) return rc;
    }
    if ((rc = stage_event(ctx, s, true, kEvFinalDone))) return rc;
    ctx->last_stream = s;
    st.keys_out = nrecv;
    st.keys_sent = sent;
    st.exchange_path = 2;
    ctx->stats = st;
    *d_out = outp;
    *n_out = nrecv;
    return DSORT_OK;
}

template <typename T>
int sample_sort_entry(dsort_ctx *ctx, const T *d, size_t n, T **o, size_t *no, void *st, bool presorted) {
    if (!ctx) return DSORT_EINVAL;
    const uint64_t d0 = ctx->deferred_n;
    const int rc = sample_sort<T>(ctx, d, n, o, no, st, presorted);
    ctx->stats.deferred_frees = (int)(ctx->deferred_n - d0);
    ctx->stats.pending_frees = (int)(ctx->dev_later.size() + ctx->host_later.size());
    return rc;
}
template int sample_sort_entry<int32_t>(dsort_ctx *, const int32_t *, size_t, int32_t **, size_t *, void *, bool);
template int sample_sort_entry<int64_t>(dsort_ctx *, const int64_t *, size_t, int64_t **, size_t *, void *, bool);

int sample_sort_packed(dsort_ctx *ctx, const int64_t *d_in, size_t n_local, int64_t **d_out, size_t *n_out,
                       void *stream) {
    return sample_sort_entry<int64_t>(ctx, d_in, n_local, d_out, n_out, stream, false);
}

}  // namespace dsort
