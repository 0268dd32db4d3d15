// dsort_internal.h -- private declarations shared by the libdsort translation units.
// gfx950 only (MI355X, CDNA4, wave64).  No CUDA shims, no dual platform paths.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "dsort.h"

struct ncclComm;
namespace dsort {
class TxSeq;
}

namespace dsort {

// ----------------------------------------------------------------------------------------
// k-way merge passes.  A pass merges GROUPS of up to F sorted runs (F a power of two <= kMaxF)
// that lie back to back; every group's output is cut into TILE-key output tiles, one workgroup
// per tile.  Regular passes (the sort): runs of length R, groups of F runs, so every group is
// a multiple of TILE long and tile j covers output [j*TILE, (j+1)*TILE).  Irregular passes (the
// master merge, the multi-GPU receive merge): a table of groups with arbitrary run lengths.
// ----------------------------------------------------------------------------------------
constexpr int kMaxLogF = 5;
constexpr int kMaxF = 1 << kMaxLogF;

struct GroupK {
    uint64_t base;        // first key of the group (input and output index)
    uint64_t first_tile;  // global index of the group's first output tile
    uint64_t total;       // keys in the group
    uint32_t nruns;       // runs in the group (<= F of the pass)
    uint32_t pad;
    uint64_t roff[kMaxF + 1];  // run i = [base + roff[i], base + roff[i+1])
};

struct PassDesc {
    uint64_t n;              // keys in the whole array
    uint64_t R;              // regular: run length (a multiple of TILE)
    int F;                   // runs per group, power of two
    int ngroups;             // irregular: entries in `groups`
    const GroupK *groups;    // irregular: group table (device memory)
    const uint32_t *tile_group = nullptr;  // irregular, optional: group of every output tile
};

// ----------------------------------------------------------------------------------------
// What the context owns.  Each member frees or destroys itself when the context is deleted, so
// dsort_finalize keeps no list of them.
// ----------------------------------------------------------------------------------------
// A grow-only arena and its size: device memory (DevBuf) or pinned host memory (HostBuf).  ensure()
// and ensure_host() below grow them; a buffer they replace goes through release_dev / release_host.
template <hipError_t (*Free)(void *)>
struct Buf {
    void *p = nullptr;
    size_t bytes = 0;
    Buf() = default;
    Buf(const Buf &) = delete;
    Buf &operator=(const Buf &) = delete;
    ~Buf() {
        if (p) (void)Free(p);
    }
    template <class T>
    T *as() const {
        return static_cast<T *>(p);
    }
    void swap(Buf &o) {
        std::swap(p, o.p);
        std::swap(bytes, o.bytes);
    }
};
using DevBuf = Buf<hipFree>;
using HostBuf = Buf<hipHostFree>;

// An event or a stream the context created (`h` is null until then); reads as the plain handle.
template <class H, hipError_t (*Destroy)(H)>
struct Owned {
    H h = nullptr;
    Owned() = default;
    Owned(const Owned &) = delete;
    Owned &operator=(const Owned &) = delete;
    ~Owned() {
        if (h) (void)Destroy(h);
    }
    operator H() const { return h; }
};
using Event = Owned<hipEvent_t, hipEventDestroy>;
using Stream = Owned<hipStream_t, hipStreamDestroy>;

// Stage events of a sort (dsort_ctx::ev; dsort_get_stats reads the times between them).
enum StageEv {
    kEvStart = 0,
    kEvTileSortDone = 1,
    kEvLocalDone = 2,     // the local sort done
    kEvExchangeDone = 3,
    kEvFinalDone = 4,     // the final merge (the bucket exchange: the last wave) done
    kEvAllToAll0 = 5, kEvAllToAll1 = 6,  // around the key all-to-all
    kEvTile0 = 7, kEvTile1 = 8,          // around the tile sort kernel
    kEvHist0 = 9, kEvHist1 = 10,         // around the first-level histogram
    kEvScatter0 = 11, kEvScatter1 = 12,  // around the first-level scatter
    kEvSub0 = 13, kEvSub1 = 14,          // around the second-level partition
    kWave0Offset = 15,  // the bucket exchange's first wave records kEvTileSortDone, kEvTile0/1 and kEvSub0/1
                        // this much higher (dsort_ctx::ev_off), and its end at kEvWave0Done
    kEvWave0Done = 16,
    kStageEvents = 30
};

// The leg timer of a feature: HIP events around the legs of its last call, created on first use,
// for its dsort_*_leg_ms reader.  start() opens a recording, mark() appends the next event; an
// event that fails ends the recording, and count() is then 0, as it is when nothing was recorded.
struct LegClock {
    static constexpr int kMax = 14;  // (the top-k select: two per histogram pass of six, and 12 / 13)
    Event ev[kMax];
    int n = 0;        // events of the recording so far (mark_at: one past the highest index)
    bool ok = false;  // recording, and every event so far went in
    void start(bool enabled) {
        n = 0;
        ok = enabled;
    }
    void mark(hipStream_t s) { mark_at(n, s); }
    void mark_at(int i, hipStream_t s) {
        if (!ok || i >= kMax) return;
        ok = (ev[i].h || hipEventCreate(&ev[i].h) == hipSuccess) && hipEventRecord(ev[i], s) == hipSuccess;
        if (ok) n = i + 1;
    }
    int count() const { return ok ? n : 0; }
    bool complete(int events) const { return count() == events; }
    // for the readers: blocks until the last event, then ms between events a and b
    int wait_last(dsort_ctx *ctx) const;
    int elapsed(dsort_ctx *ctx, int a, int b, double *ms) const;
};

}  // namespace dsort

// Per-context options (dsort_set_option; defaults = the tuned values).
struct dsort_opts {
    int64_t buckets = -1;           // DSORT_OPT_BUCKETS: -1 auto, 0 off, B forced
    int64_t bucket_keys = 1 << 20;  // DSORT_OPT_BUCKET_KEYS
    static constexpr int64_t BUCKET_OS_DEFAULT = 128;
    int64_t bucket_os = BUCKET_OS_DEFAULT;  // DSORT_OPT_BUCKET_OVERSAMPLE
    int64_t max_logf = -1;          // DSORT_OPT_MAX_FANIN_LOG2: -1 = per key type default
    int64_t kill_after_pass = -1;   // DSORT_OPT_KILL_AFTER_STAGE
    int64_t stage_timing = 1;       // DSORT_OPT_STAGE_TIMING
    int64_t kill_in_exchange = -1;  // DSORT_OPT_KILL_IN_EXCHANGE
    int64_t comm_timeout_ms = 0;    // DSORT_OPT_COMM_TIMEOUT_MS
    int64_t test_hold_exchange = 0; // DSORT_OPT_TEST_HOLD_EXCHANGE
    int64_t test_fail_exchange = -1; // DSORT_OPT_TEST_FAIL_EXCHANGE
    int64_t test_tile_cap = 0;      // DSORT_OPT_TEST_TILE_CAP
    int64_t test_wave_fence = 0;    // DSORT_OPT_TEST_WAVE_FENCE
    int64_t sub_keys = -1;          // DSORT_OPT_SUB_KEYS: -1 = 3/16 of a tile, 0 = no second level
    int64_t sub_os = -1;            // DSORT_OPT_SUB_OVERSAMPLE: -1 = 8 (4 at sub-buckets <= TILE/8)
    int64_t sub_gather = 1;         // DSORT_OPT_SUB_GATHER
    int64_t argsort_wide = 0;       // DSORT_OPT_ARGSORT_WIDE
    int64_t test_fail_leg = -1;     // DSORT_OPT_TEST_FAIL_LEG
    int64_t topk_path = -1;         // DSORT_OPT_TOPK_PATH: -1 dsort_plan_topk's rule, 0 full argsort, 1 select
    int64_t sub_arith = -1;         // not an ABI option (dsort_debug_sub_arith_mode): the second level's arithmetic
                                    // sub-bucket map: -1 per bucket by the sample rule, 0 off, 2 (tests) every
                                    // bucket whose span allows it
    int64_t bk_arith = -1;          // likewise (dsort_debug_bucket_arith_mode): the first level's arithmetic
                                    // bucket map: -1 by the rule, 0 off, 2 (tests) whenever the span allows it
};

// The context.  One per host thread, bound to one device.
struct dsort_ctx {
    using DevBuf = dsort::DevBuf;
    using HostBuf = dsort::HostBuf;
    using Event = dsort::Event;
    using Stream = dsort::Stream;
    using LegClock = dsort::LegClock;

    dsort_opts opt;
    int nested = 0;  // > 0 inside a sort the library runs for itself (the splitter-sample sort):
                     // such a sort never buckets and never fires the fault injection
    int stages_done = 0;            // kill points the running (outermost) sort has passed
    std::atomic<int> abort_req{0};  // dsort_comm_abort from another thread during an exchange
    std::mutex comm_mu;             // held by a running exchange / communicator set-up (dsort.h)
    int device = 0;
    std::string err;

    // Members are destroyed last to first (dsort_finalize: delete ctx, on the context's device): the
    // buffers below go first, then the events, then the streams.
    Stream stream;
    Stream side;   // copies that overlap the first-level scatter (both directions)
    Stream xs;     // bucket exchange: the comm stream of its sends and receives

    Event groups_ev;   // last H2D copy out of groups_host
    Event bucket_ev;
    Event sub_ev;
    Event side_ev;     // side -> sort stream
    Event ready_ev;    // sort stream -> side
    // End of the last sort / merge on its stream: a call on another stream waits for it, since
    // the arenas are shared and a call returns while its last kernels still run.
    Event done_ev;
    Event a64_mm_ev;   // the int64 argsort's min/max read-back into small_host
    Event xev[3];      // bucket exchange: a wave's receives done (0, 1), the partition done (2)
    Event ev[dsort::kStageEvents];  // stage timing (StageEv)
    static constexpr int kMaxKev = 128;  // per-launch events of the merge kernel (2 per pass)
    Event kev[kMaxKev];
    // the legs' events of the last call of a feature (its dsort_*_leg_ms reader)
    LegClock pairs_clk;  // the pair sort (dsort_pairs.hip): pack, sort and unpack
    LegClock a64_clk;    // the int64 argsort (dsort_pairs64.hip)
    LegClock s64_clk;    // the int64 argsort across ranks
    LegClock tk_clk;     // the top-k select's histogram kernels and compaction (on request)
    LegClock gat_clk;    // the distributed gather's five legs

    // grow-only device arenas
    DevBuf scratch;
    DevBuf splits;   // per-tile split vectors of a k-way pass (uint32 x F per tile)
    DevBuf groups;   // irregular group tables (device)
    HostBuf groups_host;  // pinned staging of the group tables
    bool groups_ev_pending = false;
    DevBuf scratch2; // second scratch for multi-level irregular merges
    DevBuf io;        // staging for the host-buffer entry points
    DevBuf io2;
    DevBuf pairs;     // packed (key, value) words of the pair sort (dsort_pairs.hip): 8 B each
    DevBuf spairs_k;     // the pair sample sort's slice, unpacked: sorted keys (4 B each) ...
    DevBuf spairs_v;     // ... and their indices / values
    // the int64 argsort and record sort (dsort_pairs64.hip); its first arena is `pairs`
    DevBuf a64_b;        // the wide path's second arena of packed words: 8 B each
    DevBuf a64_idx;      // the record sort's permutation: 4 B each
    DevBuf a64_part;     // the min/max reduction's per-workgroup partials and its result
    bool a64_minmax = false;      // the last call ran the reduction (the automatic mode)
    // the int64 argsort across ranks (dsort_sample_argsort_dev_i64, dsort_pairs64.hip); its packed
    // words start in `pairs`
    DevBuf s64_k;        // this rank's slice: sorted keys (8 B each) ...
    DevBuf s64_i;        // ... and their global positions (4 B each)
    DevBuf s64_sa;       // wide: the first sort's slice, saved (the second sort reuses recv2)
    DevBuf s64_pos;      // wide: the low words of a slice, the indices of a gather (4 B each)
    DevBuf s64_got;      // wide: what a gather brought (8 B per index)
    // the typed-key sample sort and sample argsort (dsort_keys.hip): this rank's chunk, encoded -- the
    // input of the integer call behind them
    DevBuf kenc;
    // top-k selection (dsort_topk.hip); the 4-byte candidates' packed words go to `pairs`, the order
    // of the 8-byte candidates to `a64_idx`
    DevBuf tk_rows;      // one pass's histogram rows: 2048 bins per workgroup (4 B each)
    DevBuf tk_small;     // the state, the partial column sums, less / eq / quota / offsets
    DevBuf tk_ck;        // the candidates: 8-byte keys, or the packed words a rank sends (8 B each);
                         // the full path's sorted keys
    DevBuf tk_cp;        // ... and the positions of 8-byte candidates (4 B each)
    DevBuf tk_rk;        // across ranks, 8-byte keys: every rank's candidates ...
    DevBuf tk_rp;        // ... their positions ...
    DevBuf tk_sk;        // ... and the candidates in key order
    bool tk_timing = false;       // dsort_topk_leg_timing
    int tk_passes = 0;            // histogram passes the last select timed (0: none)
    // the distributed gather (dsort_gather.hip): arenas of its own, so that a gather leaves the
    // slices of the preceding sample sort / argsort (recv2, spairs_k, spairs_v) alone
    DevBuf gat_req;      // this rank's requests, owner-major (4 B per index)
    DevBuf gat_rreq;     // the requests received (4 B each)
    DevBuf gat_rep;      // the records served (W bytes per request received)
    DevBuf gat_back;     // the records that came back (W bytes per index)
    DevBuf gat_small;    // owner table, per-workgroup counts, bin starts and totals
    HostBuf gat_host;    // pinned: the owner table and the bin totals
    DevBuf bucket;       // partition pass of the bucketed int32 sort (dsort_bucket.h)
    HostBuf bucket_host; // pinned: bucket starts
    DevBuf sub;          // second partition level (dsort_sub.h)
    DevBuf sub_alt;      // the bucket exchange's second wave uses the other of the two
                         // (the first wave's kernels still read theirs)
    DevBuf stmp;         // merge output of a split sub-bucket (merge_split_subbuckets)
    HostBuf sub_host;    // pinned: bucket table, chunk table, tile / merge-record counts
    hipStream_t done_stream = nullptr;  // (done_ev)
    bool done_pending = false;
    DevBuf tfb;          // tiles the bin sort declined (+ their count, on the device)
    DevBuf text_status;  // per-tile counts and their prefixes of the text codec
    DevBuf red;       // 64 B of reduction accumulators
    HostBuf red_host; // pinned mirror
    // sample sort (multi-GPU)
    ncclComm *comm = nullptr;
    bool has_transport = false;   // host transport instead of RCCL (dsort_comm_init_transport)
    dsort_transport transport = {};
    dsort::TxSeq *tx = nullptr;   // the running sample sort's host-transport sequence (dsort_tx.h)
    HostBuf xfer;         // pinned host staging of the host transport
    HostBuf xfer2;
    DevBuf fence;        // DSORT_OPT_TEST_WAVE_FENCE: fingerprints (device, pinned mirror)
    HostBuf fence_host;
    int nranks = 1;
    int rank = 0;
    DevBuf local;  // locally sorted chunk
    DevBuf recv;
    DevBuf recv2;
    DevBuf small;  // samples / splitters / counts on device
    HostBuf small_host;  // pinned
    DevBuf bxs;    // bucket exchange: this rank's and every rank's splitter samples
    const uint32_t *bk_hot = nullptr;  // the last first level's runs flag (device, BkMap.hot)
    uint32_t sub_arith_n[2] = {0, 0};  // the last bucketed sort: buckets of several sub-buckets, and those of
                                       // them on the arithmetic map (dsort_debug_sub_arith)
    uint32_t bk_arith_on = 0;          // the last bucketed sort's first level ran on the arithmetic bucket map
                                       // (dsort_debug_bucket_arith)
    int ev_off = 0;               // kWave0Offset while the bucket exchange's first wave runs its second
                                  // level and tile sort (dsort_get_stats adds the two waves up)
    int ev_done = dsort::kEvLocalDone;  // the stage event a sort's second level records at its end (the
                                        // bucket exchange: kEvWave0Done, then kEvFinalDone)
    // The bucket exchange runs its second level while the keys are still in flight: the sort's
    // host waits then poll (abort flag, deadline) instead of blocking on a stream a dead peer
    // would never complete (sync_event / sync_stream, dsort_wave.hip).
    bool poll_waits = false;
    double poll_deadline = 0.0;  // ms on the CLOCK_MONOTONIC scale, 0 = none
    hipStream_t poll_stream = nullptr;  // the sort stream of those waits (ensure() polls it, and the
                                        // side stream, instead of a device-wide synchronize)
    // buffers replaced while poll_waits is set: hipFree / hipHostFree synchronize the device, which
    // would wait for the comm stream, so they are released once the exchange is over (flush_later)
    std::vector<void *> dev_later, host_later;
    uint64_t deferred_n = 0;  // arenas whose release was deferred so far (stats.deferred_frees)
    // stage timing
    unsigned ev_mask = 0;             // events recorded by the last call (bit i = ev[i])
    hipStream_t last_stream = nullptr;  // stream of the last asynchronous call
    int kev_used = 0;
    bool ev_ok = false;       // stage events recorded: created, and DSORT_OPT_STAGE_TIMING on
    bool ev_created = false;
    dsort_stats stats = {};
};

namespace dsort {

// Inclusive sum over a wave (DPP row shifts, then the row broadcasts of lane 15 and 31).
__device__ __forceinline__ uint32_t wave_incl_sum(uint32_t v) {
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x111, 0xF, 0xF, false);  // row_shr:1
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x112, 0xF, 0xF, false);  // row_shr:2
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x114, 0xF, 0xF, false);  // row_shr:4
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x118, 0xF, 0xF, false);  // row_shr:8
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x142, 0xA, 0xF, false);  // row_bcast:15
    v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x143, 0xC, 0xF, false);  // row_bcast:31
    return v;
}

// The statistics of a call before it records anything (first_level_map -1: no bucketed sort ran).
inline dsort_stats fresh_stats() {
    dsort_stats s{};
    s.first_level_map = -1;
    return s;
}

int set_err(dsort_ctx *ctx, int code, const std::string &msg);
// the stream argument of the C-ABI: NULL = the context's stream, DSORT_NULL_STREAM = stream 0
hipStream_t pick_stream(dsort_ctx *ctx, void *stream);
int hip_err(dsort_ctx *ctx, hipError_t e, const char *what);
// grow-only: at least `need` bytes in the arena (the old contents are not kept)
int ensure(dsort_ctx *ctx, DevBuf &buf, size_t need, const char *what);
int ensure_host(dsort_ctx *ctx, HostBuf &buf, size_t need);
// the pinned mirror of ctx->small (sized before any keys are in flight: it never grows while
// ctx->poll_waits)
inline int ensure_small_host(dsort_ctx *ctx, size_t need) { return ensure_host(ctx, ctx->small_host, need); }
// hipFree / hipHostFree of a buffer that is being replaced, deferred while ctx->poll_waits (see
// dsort_ctx); the buffer is empty afterwards
void release_dev(dsort_ctx *ctx, DevBuf &buf);
void release_host(dsort_ctx *ctx, HostBuf &buf);
void flush_later(dsort_ctx *ctx);
// Stage event e of a timed call on s, when stage timing is on (ctx->ev_ok); `timed` also opens and
// closes the profiler ranges around the sort's kernels.  Records exactly ev[e]: the callers inside
// the bucket exchange's waves add ctx->ev_off themselves.
int stage_event(dsort_ctx *ctx, hipStream_t s, bool timed, StageEv e);

// The sort and the k-way merge (dsort_wave.hip), both key widths.  All asynchronous on `s`.
// sort_device sorts d_in[0..n) into d_keys (d_in may equal d_keys).  merge_device with
// keep_stats leaves the statistics and per-launch events of the preceding local sort alone (the
// sample sort's final merge).
template <typename T>
int sort_device(dsort_ctx *ctx, const T *d_in, T *d_keys, size_t n, hipStream_t s, bool timed);
template <typename T>
int merge_device(dsort_ctx *ctx, const T *d_in, const size_t *lens, int k, T *d_out,
                 hipStream_t s, bool keep_stats = false);
// Fault injection for the fault-tolerance tests and bench (BASELINE config C5): with
// DSORT_OPT_KILL_AFTER_STAGE = k the process SIGKILLs itself right after stage k of a local
// (non-nested) sort has finished on the GPU -- a worker dying mid-sort.  The stages of a sort, in
// order (sort_stages counts them):
//   bucketed sort (>= 2^25 keys)  0 first-level partition, 1 second-level partition, 2 tile sort
//     (with DSORT_OPT_SUB_KEYS = 0: 0 partition, 1 tile sort, 2 + p merge pass p)
//   merge path                    0 tile sort, 1 + p merge pass p
// A kill stage the sort never reaches makes the sort return DSORT_EINVAL (sort_device).
void fault_point(dsort_ctx *ctx, hipStream_t s, int stage);
// Kill points of a top-level sort of n keys of key_bytes bytes under `opt` (the bucketed path
// without the second level has data-dependent merge passes: the guaranteed minimum).
int sort_stages(const dsort_opts &opt, uint64_t n, int key_bytes);
// The cross-stream rule of the shared arenas (dsort_ctx::done_ev): a top-level call waits on its
// stream for the context's previous call when that ran on another stream (order_begin), and marks
// its own end (order_end).  sort_device and merge_device bracket themselves; a call that uses an
// arena around them (the pair sort) brackets its whole sequence as well.
int order_begin(dsort_ctx *ctx, hipStream_t s);
int order_end(dsort_ctx *ctx, hipStream_t s);
// dsort_sample_sort_dev_i64 for the pair sample sort (dsort_pairs.hip; the sample sort and the rest
// of the exchange layer: dsort_exch.h).  Takes the comm mutex itself: the caller must not hold it.
int sample_sort_packed(dsort_ctx *ctx, const int64_t *d_in, size_t n_local, int64_t **d_out, size_t *n_out,
                       void *stream);
// The pair sort of 4-byte keys (dsort_pairs.hip) and the argsort of 8-byte keys (dsort_pairs64.hip)
// behind the argument checks of their entry points, for the typed-key entry points
// (dsort_keys.hip).  kc = the key codec (dsort_keycodec.h), 0 = the signed integer, ascending; the
// key pointers are typed as the integer of the key's width whatever the key type.
namespace pr {
int pairs_sort(dsort_ctx *ctx, const int32_t *keys_in, const uint32_t *vals_in, int32_t *keys_out,
               uint32_t *vals_out, size_t n, hipStream_t s, int kc = 0);
// The pair sort's unpack alone, for the top-k select (dsort_topk.hip): keys_out[i] = the decoded high
// word (NULL: not wanted), vals_out[i] = the low word of packed[i], i < n.
int unpack_words(dsort_ctx *ctx, const uint64_t *packed, int32_t *keys_out, uint32_t *vals_out, size_t n,
                 hipStream_t s, int kc);
}
namespace p64 {
int argsort64(dsort_ctx *ctx, const int64_t *keys, int64_t *keys_out, uint32_t *idx_out, size_t n, hipStream_t s,
              int kc = 0);
}
// Host waits of the sort: blocking, or (ctx->poll_waits) polling with the abort flag and deadline
// (DSORT_ECOMM / DSORT_ETIMEOUT).
int sync_event(dsort_ctx *ctx, hipEvent_t e, const char *what);
int sync_stream(dsort_ctx *ctx, hipStream_t s, const char *what);
// The pause between two polls of a polled wait: yield for the first POLL_SPIN_MS of the wait,
// then sleep.  (A usleep of a few us sleeps about 60 us with the default timer slack: measured
// as 40-85 us of idle GPU after every polled tile-count and all-gather wait of the bucket
// exchange -- 0.2 ms of a 2^27-key rank's 1.7 ms.)
struct PollPause {
    static constexpr double POLL_SPIN_MS = 20.0;
    double t0 = -1.0;
    void operator()();
};
// Largest log2 fan-in of one merge pass: the option, else the key type's default.
int max_logf(const dsort_opts &opt, int type_default, int type_cap);

// ----------------------------------------------------------------------------------------
// Bucket exchange (the multi-GPU sample sort): every rank cuts its UNSORTED keys
// into Btot = P * Bl global buckets by splitters taken from every rank's samples (the first
// partition level of the one-GPU sort, with global splitters), ships buckets [q Bl, (q+1) Bl) to
// rank q, and finishes its own Bl buckets with the second level and the tile sort -- the received
// pieces of a bucket are its chunks.  No sorted runs are merged anywhere.
// ----------------------------------------------------------------------------------------
struct BxSample {  // a splitter sample: key (sign-extended) and position in its rank's keys
    int64_t k;
    uint64_t i;
};
struct BxPlan {
    int P, me, Bl, Btot;
    uint64_t n_local, n_total;
    uint32_t s_max;                 // sample records per rank (the all-gather's unit)
    uint64_t recv_room;             // keys the partition buffer holds past this rank's own: the
                                    // other ranks' pieces land there (no copy of its own buckets)
    std::vector<uint64_t> n_of;     // keys of every rank
    std::vector<uint64_t> ioff;     // composite index of every rank's first key (prefix of n_of)
    std::vector<uint32_t> s_of;     // real samples of every rank (the rest of its s_max: padding)
};
// The plan from every rank's key count; false when the bucket exchange does not apply (too few
// keys, the second level or the partition switched off): the caller takes the sort-then-merge path.
bool bx_make_plan(const dsort_opts &opt, int P, int me, const uint64_t *n_of, int key_bytes, BxPlan &plan);
// 1. this rank's s_of[me] regular samples of d_in into d_smp (s_max records, the rest padded)
template <typename T>
int bx_sample(dsort_ctx *ctx, const T *d_in, const BxPlan &pl, BxSample *d_smp, hipStream_t s);
// 2. the global splitters from every rank's records (d_all: P * s_max), then the first partition
//    level of d_in into ctx->scratch (bucket-major, Btot buckets; recv_room more keys fit behind
//    them).  *hb = this rank's bucket starts (host, Btot + 1), *part = the partitioned keys.  Kill
//    stage 0 fires here.
//    pure[g] (Btot): global bucket g lies between two splitters of one key.  Its keys are dropped
//    (the scatter's pure-bucket drop, round 6): part holds the others at the compacted starts -- every pure
//    bucket of size 0 -- and the owner fills a pure bucket with its key, so its keys never cross
//    the links.
template <typename T>
int bx_partition(dsort_ctx *ctx, const T *d_in, const BxPlan &pl, const BxSample *d_all, hipStream_t s, bool timed,
                 const uint64_t **hb, T **part, std::vector<uint8_t> &pure);
// 3. after the exchange: src holds the pieces of this rank's buckets from every source r, source
//    r's in bucket order from src[base[r]] on (base: of the wave's first bucket);
//    hb_all[r * (Btot + 1) + g] = source r's bucket starts, hc_all its compacted starts (the pieces'
//    positions: a pure bucket has none).  Sorts them into out (nrecv keys; src holds at least nrecv
//    keys: the second level's scratch).  Kill stages 1 and 2 fire here.
//    The buckets [j_lo, j_hi) of this rank (wave w of W) into out + out_off; *n_out = their keys.
template <typename T>
int bx_local_sort(dsort_ctx *ctx, T *src, T *out, const BxPlan &pl, const uint64_t *hb_all, const uint64_t *hc_all,
                  const uint64_t *base, int j_lo, int j_hi, uint64_t out_off, int w, int W, hipStream_t s,
                  bool timed, uint64_t *n_out);

}  // namespace dsort

#define DSORT_HIP(ctx, call)                                      \
    do {                                                          \
        hipError_t e_ = (call);                                   \
        if (e_ != hipSuccess) return dsort::hip_err((ctx), e_, #call); \
    } while (0)
