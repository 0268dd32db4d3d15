// dsort_exch.h -- the exchange layer (dsort_exchange.hip): what a collective call over either
// transport -- RCCL on the stream, or the caller's host transport through a TxSeq with its status
// gates (dsort_tx.h) -- is driven with.  Private to the sample sort (dsort_exchange.hip), the
// distributed gather (dsort_gather.hip) and the C ABI (dsort_api.hip).
#pragma once

#include <rccl/rccl.h>

#include <mutex>
#include <string>

#include "dsort_internal.h"
#include "dsort_tx.h"

namespace dsort {

// Aborts the communicator; the caller holds ctx->comm_mu.
void abort_comm_locked(dsort_ctx *ctx);

// An RCCL call on the non-blocking communicator: ncclInProgress is success-so-far.
#define DSORT_NCCLNB(ctx, call)                                                           \
    do {                                                                                  \
        ncclResult_t r_ = (call);                                                         \
        if (r_ != ncclSuccess && r_ != ncclInProgress) {                                  \
            dsort::abort_comm_locked(ctx);                                                \
            return dsort::set_err((ctx), DSORT_ECOMM,                                     \
                                  std::string(#call) + ": " + ncclGetErrorString(r_));    \
        }                                                                                 \
    } while (0)

// One collective call (a sample sort, a gather) from its first line to its return: holds the comm
// mutex, refuses an aborted or missing communicator (rc), picks the stream and the deadline, and on
// the host transport runs the sequence of `ncoll` collectives with their gates (seq; plan() adds
// more once the path is known) as ctx->tx.  Leaving the call before the last collective on any
// error reports the failure to the peers at the next gate (the guard), so none of them blocks in a
// collective this rank never joins; an exit that every rank takes alike says finished() first.
struct ExchCall {
    std::unique_lock<std::mutex> lock;
    const int rc;  // not DSORT_OK: the call is refused (the error is set), return it
    const int P, me;
    const bool host_tx;
    const hipStream_t s;
    const double deadline;  // on the tx_now_ms() scale, 0 = none
    TxSeq seq;
    ExchCall(dsort_ctx *ctx, void *stream, int ncoll);
    void finished() { guard.finished = true; }
    void failed(int code) { guard.code = code; }  // what the guard reports instead of DSORT_ECOMM

  private:
    struct TxScope {
        dsort_ctx *c;
        ~TxScope() { c->tx = nullptr; }
    } scope;        // (destroyed after the guard: its report still sees the sequence's deadline)
    TxGuard guard;
};

// A call made of several exchange calls one after the other (the int64 sample argsort's legs) that
// fails locally BETWEEN two of them -- an arena, a kernel launch -- must not leave its peers blocked
// in the next one: the failing rank opens that next call, of one collective, and leaves it
// unfinished, so that its guard reports `code` at the peers' first gate there.  Returns `code`, the
// context's error message untouched.  (RCCL has no gates: the deadline and the abort flag.)
int exch_leave(dsort_ctx *ctx, void *stream, int code);

// Every wait of an exchange (stream, RCCL's asynchronous error, abort flag, deadline).
int exch_wait(dsort_ctx *ctx, hipStream_t s, bool with_stream, double deadline, const char *what,
              bool hold = false);
// A collective of the host transport: the fault point (DSORT_OPT_TEST_FAIL_EXCHANGE), the collective
// through ctx->tx (its gate in front), the sequence's error as the context's.
int host_allgather(dsort_ctx *ctx, const void *send, void *recv, size_t bytes, const char *what);
int host_alltoallv(dsort_ctx *ctx, const void *send, const size_t *sc, const size_t *sd, void *recv,
                   const size_t *rcn, const size_t *rd, const char *what);
// All-gather of `count` uint64 per rank over either transport: out[r * count + i] = rank r's src[i].
// (RCCL: through the context's small arenas, device and pinned, from offset 0.)
int allgather_u64(dsort_ctx *ctx, const uint64_t *src, size_t count, uint64_t *out, hipStream_t s,
                  double deadline, const char *what);

// An all-to-all-v of `unit`-byte elements, `type` on the wire (unit a multiple of its size):
// sbuf[soff[r] .. + scnt[r]) goes to rank r, which receives it at rbuf[roff[s] .. + rcnt[s]) for
// source s; counts and offsets in elements, arrays of P.
struct A2av {
    const void *sbuf;
    const uint64_t *scnt, *soff;
    uint64_t stotal;
    void *rbuf;
    const uint64_t *rcnt, *roff;
    uint64_t rtotal;
    size_t unit;
    ncclDataType_t type;
};
// RCCL: one grouped send and receive per peer (not the own part) on s, then the enqueue wait.
int rccl_group(dsort_ctx *ctx, const A2av &a, hipStream_t s, double deadline, const char *what);
// The exchange in two pieces, for a caller that records an event between them: a2av_peers is
// rccl_group, or the whole exchange on the host transport (D2H, the caller's all-to-all-v, H2D
// through the pinned staging buffers; its staging wait reports as `staging`); a2av_own is RCCL's
// own part, a D2D copy.
int a2av_peers(dsort_ctx *ctx, const A2av &a, hipStream_t s, double deadline, const char *what, const char *staging);
int a2av_own(dsort_ctx *ctx, const A2av &a, hipStream_t s);
inline int alltoallv(dsort_ctx *ctx, const A2av &a, hipStream_t s, double deadline, const char *what,
                     const char *staging) {
    const int rc = a2av_peers(ctx, a, s, deadline, what, staging);
    return rc ? rc : a2av_own(ctx, a, s);
}

// The sample sort behind the C ABI (presorted: dsort_sample_merge_dev_*), with the call's
// stats.deferred_frees / pending_frees whatever it returns.  int32_t and int64_t.
template <typename T>
int sample_sort_entry(dsort_ctx *ctx, const T *d, size_t n, T **o, size_t *no, void *stream, bool presorted);

// fingerprint_kernel<T> (dsort_api.hip) of keys[0, n) into acc[0..1] on s, for the wave fence.
template <typename T>
int fingerprint_launch(dsort_ctx *ctx, const T *keys, uint64_t n, unsigned long long *acc, hipStream_t s);

}  // namespace dsort
