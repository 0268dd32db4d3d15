/*
 * dsort.h -- C ABI of libdsort, the MI355X (gfx950) sort path of the distributed sort.
 *
 * Drop-in boundary for khimansusinha/Distributed-sorting-with-fault-tolerance
 * (reference snapshot 2025-10-24).  The reference has two in-process calls on its hot path:
 *
 *   client.c:117   merge_sort(chunk, 0, num_integers - 1);            (worker, L3)
 *   server.c:266   merge_chunks(MAX_WORKERS, received_chunks,
 *                               chunk_sizes, total_integers);        (master, L4)
 *
 * dsort_sort_i32() replaces the first and dsort_merge_i32() replaces the merge half of the
 * second (the text write of output.txt, server.c:517-519, stays in host C: dsort_write_text()).
 * The multi-GPU entry points replace the single-master gather (server.c:414-415) by a sample
 * sort whose key exchange is an RCCL all-to-all over xGMI.
 *
 * Conventions (differences from the reference are deliberate and listed in DESIGN.md):
 *   - plain C types only: no HIP, RCCL or torch types cross this boundary; streams are passed
 *     as `void *` holding a hipStream_t (NULL = the context's own stream,
 *     DSORT_NULL_STREAM = HIP's legacy default stream, i.e. hipStream_t 0);
 *   - all sizes are size_t (the reference uses int, client.c:166, server.c:481);
 *   - every call returns 0 on success or a negative DSORT_E* code; dsort_last_error(ctx)
 *     gives the message.  Nothing inside the library calls exit() (server.c:485-498 does);
 *   - the *_i32 / *_i64 entry points take signed keys, compared as signed integers, sorted
 *     ascending; the full range is valid (the reference cannot take -1 or INT_MAX).
 *     The *_keys entry points ("Key types and order" below) take float, unsigned and signed keys of
 *     4 and 8 bytes, ascending or descending;
 *   - one context per thread; one context drives one GPU.
 */
#ifndef DSORT_H
#define DSORT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DSORT_ABI_VERSION 10

#define DSORT_OK 0
#define DSORT_EINVAL (-1)   /* bad argument */
#define DSORT_ENOMEM (-2)   /* device or host allocation failed */
#define DSORT_EHIP (-3)     /* HIP runtime error (kernel launch, copy, ...) */
#define DSORT_ECOMM (-4)    /* RCCL error or communicator not initialised */
#define DSORT_ENODEV (-5)   /* no gfx950 device / device index out of range */
#define DSORT_ETIMEOUT (-6) /* a peer did not answer in time (fault path) */
#define DSORT_ESTAGE (-7)   /* ABI 4: DSORT_OPT_KILL_AFTER_STAGE names a stage this sort never
                               reached (the sort itself finished: its output is valid)        */

typedef struct dsort_ctx dsort_ctx;

/* Stream argument meaning "the HIP null stream" (a NULL argument selects the context's own
 * non-blocking stream instead). */
#define DSORT_NULL_STREAM ((void *)1)

/* Per-call stage timings of the last sort/merge on this context (device time, ms). */
typedef struct dsort_stats {
    double block_sort_ms;   /* LDS tile sort (the worker's merge_sort leaves)            */
    double merge_ms;        /* global merge-path passes                                   */
    double exchange_ms;     /* multi-GPU: sampling + splitters + RCCL all-to-all          */
    double final_merge_ms;  /* multi-GPU: merge of the runs received from every rank      */
    double total_ms;
    double merge_kernel_ms; /* sum of the merge kernel's own launch durations (HIP events) */
    int merge_kernel_launches;
    int merge_passes;       /* number of global merge passes executed                     */
    int tile_keys;          /* keys per tile of the tile sort (int32 8192, or 16384 when a */
                            /* bucket exceeds 2M keys; int64 8192)                         */
    size_t keys_in;         /* keys handed to the call                                    */
    size_t keys_out;        /* keys produced (multi-GPU: this rank's key range)           */
    double alltoall_ms;     /* multi-GPU: the key all-to-all alone (grouped send/recv)    */
    size_t keys_sent;       /* multi-GPU: keys this rank shipped to other ranks           */
    double tile_sort_kernel_ms; /* the tile sort kernel alone (HIP events around its launch) */
    double partition_ms;    /* bucketed sort: the partition passes before the tile sort   */
    size_t tile_sort_keys;  /* keys the tile sort sorted (bucketed sort: a bucket of one key
                               value -- a heavy duplicate -- is not tile-sorted)             */
    /* ABI 3: the partition kernels alone (HIP events around their launches; 0 when the sort
     * did not run them) */
    double bucket_hist_ms;    /* first-level histogram                                      */
    double bucket_scatter_ms; /* first-level scatter                                        */
    double sub_partition_ms;  /* second-level partition (local partition, or hist + scatter) */
    /* ABI 4: the second level's rare paths */
    int sub_split_subbuckets; /* sub-buckets above a tile (a sampling outlier): tile-sorted in
                                 pieces and merged (merge_passes counts that merge)            */
    int sub_scatter_fallback; /* 1 when the sort left the default local partition for the
                                 scatter path on its own (a bucket of too many chunks, or more
                                 split tiles than the tile tables hold)                         */
    int exchange_path;        /* the last sample sort: 1 = bucket exchange (partition, exchange,
                                 sort the received buckets), 2 = sort, exchange, merge the received
                                 runs (small inputs, dsort_sample_merge_dev), 0 = not a sample sort */
    /* ABI 5 */
    int first_level_map;      /* slot map of the last bucketed sort's first partition level: 0 the fixed
                                 top-11-bit map (int32 only), 1 linear over the splitters' key range, 2
                                 logarithmic (bucket_slotmap_kernel; int32 leaves the fixed map when it
                                 crowds the splitters of several keys into one slot); ABI 6: 3 the fixed map
                                 with one refined slot (a second table over the most crowded slot, when
                                 no map thins it: small keys mixed with uniform ones); -1 none */
    /* ABI 6 */
    int fence_ranges;         /* DSORT_OPT_TEST_WAVE_FENCE: device ranges the last sample sort's wave
                                 fence found unchanged across its first wave (0: no fence ran) */
    int deferred_frees;       /* the last sample sort: arenas it replaced while keys were in flight,
                                 whose release waited for the exchange's end */
    int pending_frees;        /* ... of those, still held when it returned (0, failed or not) */
    /* ABI 10 (in the four bytes that were padding here: no other field moves) */
    int argsort_passes;       /* the last int64 argsort or record sort: 1 = the narrow word, one int64
                                 sort; 2 = the wide path, two (0: it had no keys); 0 after every
                                 other call (a sort resets it) */
    /* ABI 9: set by the last dsort_sample_gather_dev, which touches no other field (a sort
     * resets them to 0) */
    size_t gather_sent;       /* requests this rank shipped to OTHER ranks                      */
    size_t gather_served;     /* requests it served from its own records, its own included      */
} dsort_stats;

/* ---------------------------------------------------------------- lifecycle ---------- */
/* Creates a context bound to HIP device `device` (its own stream, scratch arenas). */
int dsort_init(dsort_ctx **ctx, int device);
int dsort_finalize(dsort_ctx *ctx);
const char *dsort_last_error(const dsort_ctx *ctx);
const char *dsort_version(void);
int dsort_get_stats(const dsort_ctx *ctx, dsort_stats *out);
/* Blocks until all work queued by this context has finished. */
int dsort_synchronize(dsort_ctx *ctx);

/* Per-context options (tuning and fault injection).  Defaults are the tuned values; nothing in
 * the library reads the environment.  dsort_set_option returns DSORT_EINVAL for an unknown
 * option or a value out of range. */
#define DSORT_OPT_BUCKETS 1           /* partition pass: -1 automatic (default), 0 off, B >= 2 forces B
                                         buckets at any size (<= 1024)                               */
#define DSORT_OPT_BUCKET_KEYS 2       /* nominal keys per bucket (default 2^20)                        */
#define DSORT_OPT_BUCKET_OVERSAMPLE 3 /* splitter samples per bucket, 1..4096 (default 128; 256 before   
                                         round 5)                                                    */
/* 4: retired (skewed bucket sizes of the round-1 merge plan); rejected as unknown               */
#define DSORT_OPT_MAX_FANIN_LOG2 5    /* cap on log2(F) of one merge pass; -1 = per key type default   */
#define DSORT_OPT_KILL_AFTER_STAGE 6  /* fault injection (config C5): SIGKILL the calling process right
                                         after stage k of a local sort has finished on the GPU; -1 =
                                         off (default).  Stages: bucketed sort (>= 2^25 keys) 0 first-
                                         level partition, 1 second-level partition, 2 tile sort; below
                                         2^25 keys 0 tile sort, 1 + p merge pass p (dsort_sort_stages).
                                         A stage the sort never reaches makes it return DSORT_ESTAGE
                                         (ABI 3: DSORT_EINVAL) */
/* ABI 2's DSORT_OPT_KILL_AFTER_PASS (option 6, merge passes) was kept as a deprecated alias of
 * DSORT_OPT_KILL_AFTER_STAGE through ABI 5 and is gone from ABI 6. */
#define DSORT_OPT_KILL_IN_EXCHANGE 7  /* fault injection: SIGKILL inside the sample-sort exchange, at
                                         stage 1 (samples all-gathered) or 2 (counts exchanged, keys
                                         about to move); -1 = off (default)                            */
#define DSORT_OPT_COMM_TIMEOUT_MS 8   /* deadline of every wait inside one sample-sort exchange on
                                         RCCL (ms); on expiry the communicator is aborted and the call
                                         returns DSORT_ETIMEOUT.  0 = no deadline (default)            */
#define DSORT_OPT_SUB_KEYS 9          /* second partition level: nominal keys per sub-bucket inside
                                         every bucket; consecutive sub-buckets are packed into tiles
                                         and the tile sort finishes the sort (no merge pass).  -1 =
                                         tile/8 (default), 0 = off (k-way merge passes in buckets) */
#define DSORT_OPT_SUB_OVERSAMPLE 10   /* splitter samples per sub-bucket, 1..64; -1 = 4 (default)       */
#define DSORT_OPT_SUB_GATHER 11       /* second level: 1 = chunks partitioned in place and gathered by
                                         the tile sort (default), 0 = keys scattered to sub-buckets  */
#define DSORT_OPT_TEST_HOLD_EXCHANGE 12 /* test only: 1 = the sample sort's last exchange wait (keys
                                         in flight) reports "not done" until the communicator is
                                         aborted (dsort_comm_abort from another thread) or the deadline
                                         passes -- the survivor's blocked wait of a peer failure, made
                                         deterministic.  0 = off (default)                          */
#define DSORT_OPT_TEST_FAIL_EXCHANGE 13 /* test only (ABI 5, host transport): k >= 0 = this rank fails
                                         locally (DSORT_EHIP) right before the k-th collective of its
                                         sample sort (0 = the key-count all-gather); its peers must
                                         leave at the next status gate with DSORT_ECOMM instead of
                                         blocking.  -1 = off (default)                               */
#define DSORT_OPT_STAGE_TIMING 14      /* ABI 5: 1 = every sort records its per-stage HIP events for
                                         dsort_get_stats (default); 0 = none (the *_ms statistics read
                                         0).  Each event sits between two kernels of the sort: about
                                         6 us of idle GPU apiece, ~1 % of a 2^30-key sort */
#define DSORT_OPT_TEST_TILE_CAP 15     /* test only (ABI 5): t > 0 = the local second level's tile
                                         tables hold at most t tiles, so a sort needing more takes
                                         the scatter path (stats.sub_scatter_fallback), as a
                                         pathological sampling would.  0 = off (default)            */
#define DSORT_OPT_TEST_WAVE_FENCE 16   /* test only (ABI 6): 1 = the bucket exchange fingerprints what
                                         its second wave still needs -- every wave-1 send range of the
                                         partition buffer, this rank's own wave-1 buckets and (host
                                         transport, or one rank) the wave-1 landing zone -- before and
                                         after the first wave's second level and tile sort, and fails
                                         with DSORT_EHIP naming a range that changed (over RCCL those
                                         kernels run while wave 1 is on the links).  stats.fence_ranges
                                         counts the ranges checked.  2 = the same, with one key of the
                                         first range flipped in between (the fence's own test: the
                                         sort must fail).  0 = off (default)                         */
#define DSORT_OPT_ARGSORT_WIDE 17      /* ABI 10: the int64 argsort and record sort: 0 = one pass when the
                                         keys' range allows it, else two (default; the call then reads
                                         the keys' min and max first and waits for them on the host);
                                         1 = always two passes (correct on any input, no host wait):
                                         for tests and for the bench's A/B of the two paths.  Across
                                         ranks (dsort_sample_argsort_dev_i64) every rank must set
                                         the same value                                              */
#define DSORT_OPT_TEST_FAIL_LEG 18     /* test only (an ABI 10 addition): k >= 0 = this rank fails
                                         locally with DSORT_EHIP right before leg k of
                                         dsort_sample_argsort_dev_i64 (0 decision, 1 first sort, 2
                                         slice-length all-gather, 3 key gather, 4 second sort, 5 final
                                         gather); a leg the call never reaches is ignored.  -1 = off
                                         (default)                                                   */
#define DSORT_OPT_TOPK_PATH 19         /* an ABI 10 addition: the path of dsort_topk_dev_keys / dsort_topk_keys:
                                         -1 = dsort_plan_topk's rule (default), 0 = always the full
                                         argsort, 1 = always the select path (tests, A/B)            */
int dsort_set_option(dsort_ctx *ctx, int option, int64_t value);
int dsort_get_option(const dsort_ctx *ctx, int option, int64_t *value);

/* ---------------------------------------------------------------- worker sort -------- */
/* Number of stages (fault-injection kill points, DSORT_OPT_KILL_AFTER_STAGE) a sort of n keys of
 * key_bytes (4 or 8) bytes passes through under ctx's options (ctx NULL: the defaults).  With
 * DSORT_OPT_SUB_KEYS = 0 the bucketed sort's merge passes depend on the data: the guaranteed
 * minimum. */
int dsort_sort_stages(const dsort_ctx *ctx, size_t n, int key_bytes, int *stages);
/* ABI 4: kill points of rank `rank`'s part of a sample sort of n_total keys over nranks ranks in the
 * reference's equal contiguous chunks (server.c:185-216): the bucket exchange's three stages (first
 * partition level, second level of the received buckets, their tile sort), or below 2^22 keys per
 * rank those of its local sort (dsort_sort_stages). */
int dsort_sample_sort_stages(const dsort_ctx *ctx, size_t n_total, int nranks, int rank, int key_bytes,
                             int *stages);

/* Drop-in for `merge_sort(chunk, 0, n-1)` (client.c:117 -> client.c:166-173): sorts the
 * caller-owned HOST buffer in place, ascending.  Copies to HBM, sorts on the GPU, copies
 * back; returns when `host_keys` holds the result. */
int dsort_sort_i32(dsort_ctx *ctx, int32_t *host_keys, size_t n);
int dsort_sort_i64(dsort_ctx *ctx, int64_t *host_keys, size_t n);

/* Device-resident variants: `d_keys` is device memory of this context's GPU, sorted in
 * place, asynchronously on `stream` (NULL = context stream).  Scratch of n keys is taken
 * from the context's arena (allocated on first use, reused afterwards). */
int dsort_sort_dev_i32(dsort_ctx *ctx, int32_t *d_keys, size_t n, void *stream);
int dsort_sort_dev_i64(dsort_ctx *ctx, int64_t *d_keys, size_t n, void *stream);
/* Out-of-place: sorts d_in[0..n) into d_out (d_in is not modified; d_in == d_out allowed). */
int dsort_sort_dev_copy_i32(dsort_ctx *ctx, const int32_t *d_in, int32_t *d_out, size_t n,
                            void *stream);
int dsort_sort_dev_copy_i64(dsort_ctx *ctx, const int64_t *d_in, int64_t *d_out, size_t n,
                            void *stream);

/* ---------------------------------------------------------------- argsort, pairs ----- */
/* ABI 7: the permutation of a sort, and records of a key and a payload.  int32 keys only, with a
 * 32-bit value; wider payloads follow their key by an argsort and dsort_gather_dev.  A key and
 * its value are packed into one int64, (int64)key << 32 | (uint32)value, which the int64 sort
 * orders by key, then by value as unsigned.  Memory: an arena of 8 * n bytes in the context
 * (grow-only, like the others), on top of the int64 sort's own scratch for n keys.  int64 keys
 * with a payload: ABI 10, below.  All device pointers need the alignment of their elements only
 * (records of dsort_gather_dev: 4 bytes).
 * DSORT_OPT_KILL_AFTER_STAGE acts as on an int64 sort of n keys: dsort_sort_stages(ctx, n, 8, ..)
 * gives the stage count, and with DSORT_ESTAGE the outputs are valid as for a sort.
 * dsort_get_stats afterwards shows that int64 sort's statistics (keys_in = keys_out = n). */

/* Stable argsort: d_idx_out[j] = position in d_keys of the j-th smallest key, equal keys in
 * input order; d_keys_out (NULL: not wanted; may equal d_keys) gets the sorted keys.  n <= 2^32
 * (else DSORT_EINVAL, before any memory is touched).  Asynchronous on `stream`. */
int dsort_argsort_dev_i32(dsort_ctx *ctx, const int32_t *d_keys, int32_t *d_keys_out,
                          uint32_t *d_idx_out, size_t n, void *stream);
/* Key-value sort: ascending by key, equal keys ascending by value as UNSIGNED 32-bit
 * (deterministic, independent of input order).  Outputs may alias the inputs; d_keys_out may be
 * NULL (not wanted).  No bound on n beyond memory.  Asynchronous on `stream`. */
int dsort_sort_pairs_dev_i32(dsort_ctx *ctx, const int32_t *d_keys_in, const uint32_t *d_vals_in,
                             int32_t *d_keys_out, uint32_t *d_vals_out, size_t n, void *stream);
/* d_dst[i] = d_src[d_idx[i]], i < n, for records of elem_bytes in {4, 8, 16} (else DSORT_EINVAL);
 * no overlap; an index >= the source length is the caller's error (not checked).  Applies an
 * argsort's permutation to the caller's payload records.  Asynchronous on `stream`. */
int dsort_gather_dev(dsort_ctx *ctx, const void *d_src, const uint32_t *d_idx, void *d_dst,
                     size_t n, int elem_bytes, void *stream);
/* Host form (synchronous, staged through the context's arenas like dsort_sort_i32): writes
 * idx (n entries) and, if non-NULL, keys_out (may equal keys).  n <= 2^32. */
int dsort_argsort_i32(dsort_ctx *ctx, const int32_t *keys, int32_t *keys_out, uint32_t *idx, size_t n);

/* ABI 10: the stable argsort and the record sort of int64 keys.  No 128-bit composite: a position
 * needs only b = ceil(log2 n) bits of a 64-bit word (dsort_plan_argsort_i64), so
 *   narrow, one pass:  when max - min of the keys fits the other 64 - b bits, one int64 sort of
 *                      u = (uint64)(key - min) << b | position, handed to the sort as
 *                      (int64)(u ^ 1 << 63) (signed order = unsigned order of u), is the stable
 *                      argsort; unpack: position = u & (2^b - 1), key = (int64)((u >> b) + min);
 *   wide, two passes:  any other keys take two stable passes, least significant half first: an
 *                      int64 sort of (lo32(key) ^ 0x80000000) << 32 | position, then one of
 *                      hi32(key) << 32 | j over the keys in that order, j their rank in it.
 * Every packed word is distinct, as those of the int32 argsort.  n = 2^30 keys go narrow when they
 * span less than 2^34, n = 2^20 less than 2^44.
 *
 * Memory (context arenas, grow-only, freed by dsort_finalize): narrow 8 n bytes (the pair arena of
 * the int32 calls), wide 16 n bytes, the record sort 4 n bytes more for its permutation; on top of
 * the int64 sort's own scratch for n keys and 32 KiB of reduction partials.
 *
 * Host wait: with DSORT_OPT_ARGSORT_WIDE = 0 (default) the call first reduces the keys' min and max
 * on `stream` and WAITS for the 16 bytes on the host, once, as the bucketed sort waits for its own
 * read-backs; everything else is queued on `stream`.  With DSORT_OPT_ARGSORT_WIDE = 1 nothing waits.
 *
 * DSORT_OPT_KILL_AFTER_STAGE acts inside the inner int64 sorts of n keys; the wide path's two sorts
 * count one after the other, the second's stages continuing the first's numbering (2 x
 * dsort_sort_stages(ctx, n, 8, ..) in all).  A stage never reached: DSORT_ESTAGE, every leg has
 * run and the outputs are valid.  dsort_get_stats afterwards: argsort_passes, and the LAST inner
 * sort's statistics (keys_in = keys_out = n). */

/* The host rule: *idx_bits = b = 1 for n <= 2, else the bit length of n - 1 (2^32 keys: 32);
 * with R = (uint64)key_max - (uint64)key_min, *passes = 1 if R >> (64 - b) is 0, else 2; n = 0: 0
 * passes.  n > 2^32 or key_min > key_max: DSORT_EINVAL.  Either output may be NULL. */
int dsort_plan_argsort_i64(size_t n, int64_t key_min, int64_t key_max, int *idx_bits, int *passes);
/* Stable argsort, the contract of dsort_argsort_dev_i32: d_idx_out[j] = position in d_keys of the
 * j-th smallest key, equal keys in input order; d_keys_out (NULL: not wanted; may equal d_keys)
 * gets the sorted keys; d_keys is not modified unless aliased.  n <= 2^32 (else DSORT_EINVAL,
 * before any memory is touched); n = 0 touches nothing.  Keys need 8-byte, indices 4-byte
 * alignment only. */
int dsort_argsort_dev_i64(dsort_ctx *ctx, const int64_t *d_keys, int64_t *d_keys_out,
                          uint32_t *d_idx_out, size_t n, void *stream);
/* Host form (synchronous, staged like dsort_argsort_i32). */
int dsort_argsort_i64(dsort_ctx *ctx, const int64_t *keys, int64_t *keys_out, uint32_t *idx, size_t n);
/* Stable sort of records by an int64 key: d_dst[j] = d_src[idx[j]] for the argsort's idx (kept in
 * a context arena), by dsort_gather_dev's kernel; record i of elem_bytes in {4, 8, 16} (else
 * DSORT_EINVAL, checked first) belongs to d_keys[i].  Records of EQUAL keys keep their input order
 * -- not the "by value as unsigned" rule of dsort_sort_pairs_dev_i32.  d_dst must not overlap
 * d_src; d_keys_out may be NULL or equal d_keys.  n <= 2^32. */
int dsort_sort_records_dev_i64(dsort_ctx *ctx, const int64_t *d_keys, int64_t *d_keys_out,
                               const void *d_src, void *d_dst, size_t n, int elem_bytes, void *stream);

/* ---------------------------------------------------------------- master merge ------- */
/* Drop-in for the merge half of merge_chunks (server.c:481-515): merges k sorted host runs
 * into `out` (sum(lens) keys).  Ties take the lowest run index first, like the reference's
 * strict `<` argmin scan (server.c:504), which for keys-only data is the sorted multiset.
 * Unlike the reference, INT_MAX keys are kept. */
int dsort_merge_i32(dsort_ctx *ctx, const int32_t *const runs[], const size_t lens[], int k,
                    int32_t *out);
int dsort_merge_i64(dsort_ctx *ctx, const int64_t *const runs[], const size_t lens[], int k,
                    int64_t *out);
/* Device-resident: the k runs lie back to back in d_in (run j has lens[j] keys, host array);
 * the merged result goes to d_out (no overlap with d_in). */
int dsort_merge_dev_i32(dsort_ctx *ctx, const int32_t *d_in, const size_t lens[], int k,
                        int32_t *d_out, void *stream);
int dsort_merge_dev_i64(dsort_ctx *ctx, const int64_t *d_in, const size_t lens[], int k,
                        int64_t *d_out, void *stream);

/* ---------------------------------------------------------------- multi-GPU ---------- */
/* One process per GPU.  Rank 0 creates the 128-byte RCCL unique id and ships it to the other
 * ranks by any side channel (the bench uses torch.distributed's store; the C master of
 * `dsort_master --mode samplesort` creates it and sends it in every worker's JOB frame over its
 * TCP control socket, host/ss_master.c); every rank then calls dsort_comm_init.  The communicator
 * is non-blocking: every wait of the exchange polls the stream, RCCL's asynchronous error and the
 * abort flag (dsort_comm_abort from another thread), so a dead peer surfaces as DSORT_ECOMM or,
 * with DSORT_OPT_COMM_TIMEOUT_MS, DSORT_ETIMEOUT instead of a hang. */
#define DSORT_UNIQUE_ID_BYTES 128
int dsort_comm_unique_id(char id[DSORT_UNIQUE_ID_BYTES]);
int dsort_comm_init(dsort_ctx *ctx, int nranks, int rank, const char id[DSORT_UNIQUE_ID_BYTES]);
/* Host transport: the sample sort's exchanges (counts, samples, bucket starts, keys) through caller
 * callbacks on HOST buffers instead of RCCL.  RCCL needs one GPU per rank; this serves ranks
 * that share a GPU (tests on a 1-GPU box drive it with gloo) or hosts without a usable RCCL.
 * All sizes in bytes; every callback returns 0 on success, DSORT_ETIMEOUT when it gave up at the
 * exchange deadline (see dsort_comm_deadline_ms), anything else on a transport failure (the sort
 * then returns DSORT_ETIMEOUT / DSORT_ECOMM and runs no further collective on this transport).
 *   allgather: rank r's `bytes` from `send` land at recv + r*bytes on every rank.
 *   alltoallv: send[sdispls[d] .. +scounts[d]) goes to rank d, which receives it at
 *              recv[rdispls[s] .. +rcounts[s]) for source s.
 * ABI 6: every collective of a sample sort, its first included (ABI 5: the 2nd..last), is preceded
 * by an 8-byte all-gather of every rank's status (a gate): a rank that fails locally before or
 * between collectives reports it at the next gate, and every rank then returns (the failing one its
 * own error, the others DSORT_ECOMM) instead of blocking in a collective the failed rank never joins.
 * The bucket exchange's key waves run in the order of the RCCL path: wave w's send ranges are read
 * from the partition buffer after the second level and tile sort of wave w-1 were queued. */
typedef struct dsort_transport {
    void *user;
    int (*allgather)(void *user, const void *send, void *recv, size_t bytes);
    int (*alltoallv)(void *user, const void *send, const size_t *scounts, const size_t *sdispls,
                     void *recv, const size_t *rcounts, const size_t *rdispls);
} dsort_transport;
int dsort_comm_init_transport(dsort_ctx *ctx, int nranks, int rank, const dsort_transport *t);
/* ABI 5: for transport callbacks, called on the thread running the sample sort: the milliseconds
 * left before the sort's exchange deadline (DSORT_OPT_COMM_TIMEOUT_MS; 0 = passed), or -1 when it
 * has none or no sample sort is running.  A callback bounds its waits by it and returns
 * DSORT_ETIMEOUT when it runs out, so a peer that hangs surfaces as a timeout, not as a hang. */
int dsort_comm_deadline_ms(const dsort_ctx *ctx, int64_t *remaining_ms);
/* Abort in-flight collectives (fault path: a peer died) and drop the communicator.  Safe to
 * call from another thread while this context is inside a sample sort: the call only raises the
 * abort flag, and the sample sort aborts the communicator itself and returns DSORT_ECOMM. */
int dsort_comm_abort(dsort_ctx *ctx);
int dsort_comm_destroy(dsort_ctx *ctx);

/* Sample sort over the communicator: every rank holds an equal contiguous
 * chunk (server.c:185-216 partitioning); local sort, regular samples, all-gathered splitters
 * with (value, rank, index) tie-splitting, RCCL all-to-all of key ranges, merge of the
 * received runs.  On return *d_out points to this rank's slice of the global sorted order
 * (owned by the context, valid until the next sample sort or dsort_finalize) and *n_out is its
 * length; concatenating the slices of ranks 0..nranks-1 gives the sorted input.  `d_keys` is
 * not modified (the local run is sorted into a context arena). */
int dsort_sample_sort_dev_i32(dsort_ctx *ctx, const int32_t *d_keys, size_t n_local,
                              int32_t **d_out, size_t *n_out, void *stream);
int dsort_sample_sort_dev_i64(dsort_ctx *ctx, const int64_t *d_keys, size_t n_local,
                              int64_t **d_out, size_t *n_out, void *stream);
/* The exchange half alone: `d_sorted` is this rank's already sorted local run (e.g. a fault
 * survivor that sorted its own chunk and a dead rank's chunk, then merged them).  Same output
 * contract as dsort_sample_sort_dev_*. */
int dsort_sample_merge_dev_i32(dsort_ctx *ctx, const int32_t *d_sorted, size_t n_local,
                               int32_t **d_out, size_t *n_out, void *stream);
int dsort_sample_merge_dev_i64(dsort_ctx *ctx, const int64_t *d_sorted, size_t n_local,
                               int64_t **d_out, size_t *n_out, void *stream);

/* ABI 8: the argsort and the key-value sort of int32 keys (ABI 7) across the ranks of the
 * communicator.  Every rank packs its chunk into the context's pair arena as for the local pair
 * sort -- (int64)key << 32 | (uint32)value, the value of the argsort being the key's GLOBAL position
 * -- and the packed words go through the int64 sample sort, whichever exchange path and transport it
 * takes; the rank's slice is then unpacked into two arrays of the context.  The packed words of an
 * argsort are all distinct, so a heavy key is split between ranks by position and the global order
 * is stable.
 *
 * Contract, as for dsort_sample_sort_dev_*: the inputs are not modified; on return *n_out is this
 * rank's slice length and *d_keys_out, *d_idx_out / *d_vals_out point to context-owned arrays of
 * *n_out elements, valid until the next sample sort or pair call (a gather is neither) on this
 * context or dsort_finalize.  The unpack is queued on `stream`: the arrays are ready after the stream.
 * d_keys_out == NULL: the sorted keys are not wanted.  Concatenating the slices of ranks
 * 0..nranks-1 gives the global order -- argsort: ascending by key, equal keys in ascending global
 * position (stable); pairs: ascending by key, equal keys by value as UNSIGNED 32-bit.  A rank with
 * n_local == 0 (its inputs may be NULL) still takes part in every collective.
 *
 * Errors (DSORT_ECOMM / DSORT_ETIMEOUT and the status gates of the host transport included),
 * DSORT_OPT_KILL_AFTER_STAGE -- with dsort_sample_sort_stages(.., key_bytes = 8, ..) -- and
 * dsort_get_stats behave as on dsort_sample_sort_dev_i64 of the same key counts.  An argument
 * error, or a failure to allocate the pair arena, returns before the first collective, as a NULL
 * argument of dsort_sample_sort_dev_* does.
 *
 * Memory: the pair arena (8 * n_local bytes) and 8 * n_out bytes of output arrays (4 * n_out
 * without the keys), all grow-only, on top of the int64 sample sort's memory for these counts.
 *
 * Wider payload records reach the rank that holds their key through dsort_sample_gather_dev (ABI 9,
 * below); int64 keys take dsort_sample_argsort_dev_i64 and the same gather.  Not offered across
 * ranks: the presorted / fault-survivor entry (dsort_sample_merge_dev_*) for pairs; the C master and
 * workers, which move bare keys. */

/* Global stable argsort.  The rank's chunk d_keys[0..n_local) holds the global positions
 * first .. first + n_local - 1 (`first` as in dsort_gen_uniform_*); (*d_idx_out)[j] is the global
 * position of the j-th key of this rank's slice.  first + n_local > 2^32 returns DSORT_EINVAL
 * before any memory or collective is touched; ranks passing overlapping ranges is the caller's
 * error (not checked). */
int dsort_sample_argsort_dev_i32(dsort_ctx *ctx, const int32_t *d_keys, size_t n_local, uint64_t first,
                                 int32_t **d_keys_out, uint32_t **d_idx_out, size_t *n_out,
                                 void *stream);
/* Global key-value sort.  No bound on the counts beyond memory. */
int dsort_sample_sort_pairs_dev_i32(dsort_ctx *ctx, const int32_t *d_keys, const uint32_t *d_vals,
                                    size_t n_local, int32_t **d_keys_out, uint32_t **d_vals_out,
                                    size_t *n_out, void *stream);

/* An ABI 10 addition (new symbols only): the global stable argsort of int64 keys, and with
 * dsort_sample_gather_dev the record sort of int64 keys across ranks.  The contract of
 * dsort_sample_argsort_dev_i32: collective, a rank with n_local == 0 (d_keys may be NULL) joins every
 * collective; the inputs are not modified; d_keys_out may be NULL (keys not wanted); *d_keys_out
 * (int64) and *d_idx_out (uint32 global positions) are context-owned arrays of *n_out elements in
 * arenas of this call's own, ready after `stream` and valid until the next sample sort, pair call
 * or argsort call on the context (a gather invalidates nothing) or dsort_finalize; concatenating the
 * slices of ranks 0..nranks-1 gives the keys ascending, equal keys in ascending global position.
 * Keys need 8-byte alignment only.
 *
 * Algorithm.  Every rank takes the same branch, decided in leg 0: one all-gather of every rank's
 * (first, n_local, local min, local max, DSORT_OPT_ARGSORT_WIDE), to which every rank applies
 * dsort_plan_sample_argsort_i64.  The min and max come from the local argsort's reduction and one
 * host wait; a rank without keys, or with the option set, skips it.
 *   narrow, 1 pass     the local argsort's narrow word with b from E = the end of the global range
 *                      and the GLOBAL minimum, position = first + i, through the int64 sample sort
 *                      (leg 1); the slice is unpacked into the output arenas.
 *   wide, 2 passes     least significant half first.  A = (lo32 ^ 0x80000000) : (first + i) through
 *                      the sample sort (leg 1) gives the slice SA of mA words, which is saved; the
 *                      ranks all-gather mA (leg 2; offA = the exclusive prefix); a distributed
 *                      gather of the caller's keys by SA's low words (leg 3) gives the whole keys in
 *                      pass-A order; B[j] = hi32 : (offA + j) goes through the sample sort (leg 4);
 *                      a gather of the saved SA by SB's low words (leg 5) brings every SB word its SA
 *                      word: index = its low word, key = hi32(SB) : (hi32(SA) ^ 0x80000000).
 * All words of both sorts are distinct, so a heavy key splits between ranks by position.
 *
 * Limits: first + n_local <= 2^32 (else DSORT_EINVAL before any memory or collective is touched);
 * on the wide path fewer than 2^32 keys in all (a slice is the index array of a gather) and at most
 * 256 ranks (the gather's owner table) -- both DSORT_EINVAL on every rank after leg 0.
 *
 * Errors.  Checked symmetrically in leg 0 -- every rank returns DSORT_EINVAL from the same call and
 * the communicator stays usable: ranks that disagree on DSORT_OPT_ARGSORT_WIDE, two non-empty ranges
 * that overlap.  Every leg is an exchange call of its own with the host transport's status gates,
 * the deadline (DSORT_OPT_COMM_TIMEOUT_MS, per leg) and dsort_comm_abort as in a sample sort; a rank
 * that fails locally BETWEEN two legs (an arena, a kernel launch, DSORT_OPT_TEST_FAIL_LEG) reports
 * at the gate of the next leg, so its peers return DSORT_ECOMM naming it instead of blocking (RCCL
 * has no gates: the deadline and the abort flag).  DSORT_OPT_TEST_FAIL_EXCHANGE = k counts the
 * collectives of each leg from 0 and fires in the first leg that reaches collective k.
 * DSORT_OPT_KILL_AFTER_STAGE and DSORT_OPT_KILL_IN_EXCHANGE act inside the FIRST inner sample sort,
 * as on dsort_sample_sort_dev_i64 of the same counts, and are off during the second.  A kill stage
 * beyond that sort's stages (dsort_sample_sort_stages; with DSORT_OPT_SUB_KEYS = 0 its guaranteed
 * minimum) does not stop the call, whose peers are in the legs that follow: every leg runs, the
 * outputs are valid and the call returns DSORT_ESTAGE at the end.
 *
 * dsort_get_stats: argsort_passes = 1 or 2 (0: no keys on any rank), the other fields as the last
 * inner sample sort left them.
 *
 * Memory (context arenas, grow-only), with n = n_local, m = this rank's slice (mA, mB on the wide
 * path): the pair arena 8 max(n, mA), the outputs 12 m (4 m without the keys); wide: 8 mA for the
 * saved slice, 4 max(mA, mB) of indices and 8 max(mA, mB) of gathered words; on top of the int64
 * sample sort's and the gather's memory for these counts.
 *
 * The RCCL path has run with one rank only. */
int dsort_sample_argsort_dev_i64(dsort_ctx *ctx, const int64_t *d_keys, size_t n_local, uint64_t first,
                                 int64_t **d_keys_out, uint32_t **d_idx_out, size_t *n_out,
                                 void *stream);
/* The host rule of leg 0, exported so that the CPU tests run the code the GPU path runs.  Ranks with
 * count[r] == 0 are ignored, their key_min / key_max included.  With E = the largest
 * first[r] + count[r] and the smallest key_min / largest key_max over the other ranks, the result
 * is that of dsort_plan_argsort_i64(E, min, max): b comes from E, not from the key count, so that
 * every global position fits b bits.  All counts 0: 0 passes (b = 1).  DSORT_EINVAL: nranks < 1, a
 * NULL array, two non-empty ranges that overlap or one that ends beyond 2^32
 * (dsort_plan_gather_table's rule), a non-empty rank with key_min > key_max.  Either output may be
 * NULL. */
int dsort_plan_sample_argsort_i64(int nranks, const uint64_t first[], const uint64_t count[],
                                  const int64_t key_min[], const int64_t key_max[], int *idx_bits,
                                  int *passes);

/* ---------------------------------------------------------------- key types and order --
 * An ABI 10 addition (new symbols only; no struct, option or existing call changes): every sort
 * entry for typed keys -- float32, float64, uint32, uint64, int32, int64 -- ascending or descending.
 *
 * The codec.  A key's bits b, as an integer of the key's width W, map to a word w whose SIGNED order
 * is the order of the keys, and back (csrc/dsort_keycodec.h, one rule for host and device):
 *
 *     DSORT_KEY_I32, _I64    w = b
 *     DSORT_KEY_U32, _U64    w = b ^ sign_bit
 *     DSORT_KEY_F32, _F64    w = b ^ ((b >> (W-1)) & ~sign_bit), the shift arithmetic: a negative
 *                            float flips every bit but the sign
 *     DSORT_ORDER_DESCENDING ~w of the ascending word
 *
 * Every step is an involution, so decoding applies the same steps in reverse order and the round
 * trip is bit-exact: NaN payloads and the sign of zero survive a sort.
 *
 * The order.  Integers: numeric.  Floats: IEEE 754 totalOrder -- negative NaNs (larger payload
 * first), -inf, ..., -0.0, +0.0, ..., +inf, positive NaNs (larger payload last).  Descending is the
 * exact reverse.  This differs from numpy and torch, which treat -0.0 == +0.0 and put every NaN last:
 *   - -0.0 sorts before +0.0 (descending: after), so an argsort is not stable ACROSS the two zeros;
 *   - NaNs with the sign bit set come first (descending: last), not last.
 * Inputs without NaN and without -0.0 give results bit-identical to np.sort,
 * np.argsort(kind="stable") and torch.sort(stable=True, descending=...).  Stability: keys of equal
 * BITS keep ascending input position in either order (ties stay ties under ~w), so a stable
 * descending argsort lists equal keys by ascending position, as torch does.
 *
 * The calls.  Each keeps the contract of the integer call of the same width -- dsort_sort_dev_*,
 * dsort_sort_dev_copy_*, dsort_sort_*, dsort_argsort_dev_*, dsort_argsort_*, dsort_sort_pairs_dev_i32,
 * dsort_sort_records_dev_i64, dsort_sample_sort_dev_*, dsort_sample_argsort_dev_* -- with "key" now
 * meaning the typed key and its order the one above: aliasing rules, NULL for d_keys_out, alignment
 * (elements only), n <= 2^32 for positions, n == 0 touching nothing, the arenas, the stream rules,
 * DSORT_OPT_KILL_AFTER_STAGE / DSORT_ESTAGE, the statistics (argsort_passes included) and, across
 * ranks, the collectives with their gates.  Key pointers are void *: n elements of the type's width.
 * With DSORT_KEY_I32 / _I64 and flags 0 a call IS the integer call.  In addition:
 *   - an unknown key_type, a flag bit other than DSORT_ORDER_DESCENDING, or an 8-byte type given to
 *     dsort_sort_pairs_dev_keys is DSORT_EINVAL before any memory or collective is touched; a NULL
 *     context is a plain DSORT_EINVAL;
 *   - dsort_sort_pairs_dev_keys: equal keys stay ordered by value as unsigned 32-bit ASCENDING, in
 *     either key order;
 *   - dsort_sort_records_dev_keys with a 4-byte type is the argsort into a context arena (4 n bytes)
 *     and the kernel of dsort_gather_dev -- which also gives int32 keys a record sort; with an
 *     8-byte type it is dsort_sort_records_dev_i64's path;
 *   - 8-byte types: the choice between one and two passes is dsort_plan_argsort_i64 applied to the
 *     min and max of the ENCODED words.  uint64 ids around 2^63 are narrow (the encoding removes the
 *     sign-bit straddle); float64 values of one binade are narrow, but float64 data that spans many
 *     binades has a wide encoded range and takes the two-pass path.
 *
 * Where the codec runs.  Argsort, pair sort and record sort: inside the pack and unpack kernels
 * those paths already stream every key through -- no extra pass over memory.  The keys-only sorts
 * (dsort_sort_dev_keys, _copy_keys, dsort_sort_keys): an encode kernel, the integer sort, a decode
 * kernel, i.e. two extra streaming passes over the keys (the out-of-place form encodes d_in into
 * d_out and sorts and decodes d_out in place: no arena, d_in unmodified); signed keys ascending
 * call the integer sort directly.  Across ranks: this rank's chunk is encoded into a grow-only
 * context arena of its own (n_local elements), the integer sample sort / sample argsort runs on it,
 * and the returned key slice is decoded in place on `stream` -- context-owned and ready after the
 * stream, as it is for the integer call.  A rank with n_local == 0 still joins every collective.
 * Ranks that disagree on key_type or flags are the caller's error and are NOT checked: the result
 * is then not an order of anything.
 *
 * Not offered: the codec fused into the keys-only sort's own kernels; typed keys in the C master and
 * workers and in the text codec. */
#define DSORT_KEY_I32 0
#define DSORT_KEY_U32 1
#define DSORT_KEY_F32 2
#define DSORT_KEY_I64 3
#define DSORT_KEY_U64 4
#define DSORT_KEY_F64 5
#define DSORT_ORDER_DESCENDING 1   /* flags bit 0; every other bit must be 0 */

/* The host rule, exported so that the CPU tests run the code the GPU runs: words[i] = the codec's
 * word of keys[i] (a signed integer of the key's width) and back; words may alias keys.  No
 * context.  DSORT_EINVAL, nothing written: an unknown key_type or flag bit, a NULL array with
 * n > 0. */
int dsort_key_encode(int key_type, int flags, const void *keys, void *words, size_t n);
int dsort_key_decode(int key_type, int flags, const void *words, void *keys, size_t n);

/* keys only: in place, out of place (d_in may equal d_out), and from a host buffer (staged) */
int dsort_sort_dev_keys(dsort_ctx *ctx, void *d_keys, size_t n, int key_type, int flags, void *stream);
int dsort_sort_dev_copy_keys(dsort_ctx *ctx, const void *d_in, void *d_out, size_t n, int key_type,
                             int flags, void *stream);
int dsort_sort_keys(dsort_ctx *ctx, void *host_keys, size_t n, int key_type, int flags);
/* stable argsort, device and host form */
int dsort_argsort_dev_keys(dsort_ctx *ctx, const void *d_keys, void *d_keys_out, uint32_t *d_idx_out,
                           size_t n, int key_type, int flags, void *stream);
int dsort_argsort_keys(dsort_ctx *ctx, const void *keys, void *keys_out, uint32_t *idx, size_t n,
                       int key_type, int flags);
/* key-value sort: 4-byte key types only */
int dsort_sort_pairs_dev_keys(dsort_ctx *ctx, const void *d_keys_in, const uint32_t *d_vals_in,
                              void *d_keys_out, uint32_t *d_vals_out, size_t n, int key_type, int flags,
                              void *stream);
/* stable record sort, records of 4, 8 or 16 bytes */
int dsort_sort_records_dev_keys(dsort_ctx *ctx, const void *d_keys, void *d_keys_out, const void *d_src,
                                void *d_dst, size_t n, int elem_bytes, int key_type, int flags,
                                void *stream);
/* across ranks */
int dsort_sample_sort_dev_keys(dsort_ctx *ctx, const void *d_keys, size_t n_local, int key_type,
                               int flags, void **d_out, size_t *n_out, void *stream);
int dsort_sample_argsort_dev_keys(dsort_ctx *ctx, const void *d_keys, size_t n_local, uint64_t first,
                                  int key_type, int flags, void **d_keys_out, uint32_t **d_idx_out,
                                  size_t *n_out, void *stream);

/* ---------------------------------------------------------------- top-k ----------------
 * An ABI 10 addition (new symbols and option 19; no struct, existing option or call changes): the
 * first k entries of the stable argsort in the typed order, without sorting the other n - k keys.
 *
 * Contract.  d_idx_out[j], j < k, is exactly what dsort_argsort_dev_keys of the same keys, key_type
 * and flags returns in position j, and d_keys_out[j] its key, bit for bit: the output is sorted
 * (DSORT_ORDER_DESCENDING: the k largest, largest first); keys of equal bits come in ascending
 * position, and where the cut falls inside a run of equal keys the lowest positions win; floats in
 * totalOrder, with the rules on NaN and -0.0 of "Key types and order".
 *
 * Local calls.  d_keys_out (k keys) may be NULL, d_idx_out (k positions) is required; both are
 * caller-owned and must not overlap d_keys, which is not modified.  Exactly k elements of each
 * output are written.  DSORT_EINVAL before any memory is touched: a NULL ctx (plain return), an
 * unknown key_type or flag bit, k > n, n > 2^32, a NULL pointer whose count is non-zero.  k == 0
 * touches nothing.  Asynchronous on `stream` under the argsort's stream rules (with an 8-byte type
 * and DSORT_OPT_ARGSORT_WIDE = 0 the inner argsort's one host wait for min/max remains).
 * dsort_get_stats afterwards shows the inner sort's statistics: keys_in == k on the select path, n
 * on the full path; the fault-injection options act inside the inner sort as when it is called
 * directly.
 *
 * The select path (csrc/dsort_topk.hip).  With w the codec's word of a key, a radix select on
 * u = w ^ sign_bit, most significant digit first, digits of 11 bits: 3 histogram passes over the
 * keys for 4-byte types, 6 for 8-byte types (dsort_plan_topk's `digits`), each counting only the
 * keys whose higher digits equal the prefix chosen so far; the prefix lives on the device and
 * nothing waits on the host.  After the last pass the prefix is the threshold T; one more read of
 * the keys writes the k winners -- u < T, and the first k_rest copies of T -- in ascending
 * position, and these are sorted: 4-byte keys as the pair sort's packed words by the int64 sort, 8-
 * byte keys by the int64 argsort of the k candidate keys and a gather of their positions.
 * Memory (context arenas, grow-only): 16 MiB of histogram rows (2048 workgroups x 2048 bins; fewer
 * workgroups below 2^23 keys) and 0.3 MiB of tables, plus 8 k bytes (4-byte keys: the pair arena) or
 * 16 k bytes (8-byte keys: candidates, positions and their order), on top of the inner sort's memory
 * for k keys.
 * The full path is dsort_argsort_dev_keys into context arenas (4 n bytes of indices, and n keys
 * when d_keys_out is given) and a copy of the first k.
 *
 * dsort_plan_topk, the host rule: *path = 0 nothing to do (k == 0), 1 the select path, 2 the full
 * argsort and its first k; topk_path_opt is DSORT_OPT_TOPK_PATH's value: 0 and 1 force a path, -1
 * takes the full argsort below 2^24 keys and when k > n / 2 (where the two paths were measured to
 * cross with a margin; below 2^24 keys a small k is still faster through the select path, which
 * the option forces).  *digits = the histogram
 * passes of the select path for the width.  Either output may be NULL.  DSORT_EINVAL: key_bytes not
 * 4 or 8, n > 2^32, k > n, an option value outside -1..1.
 *
 * Across ranks: dsort_sample_topk_dev_keys is collective.  Every rank passes its chunk, holding the
 * global positions first .. first + n_local - 1, and receives the same global top-k -- k keys
 * (d_keys_out, may be NULL) and their GLOBAL positions (d_idx_out) -- in caller-owned memory.  A
 * rank with n_local == 0 (d_keys may be NULL) still joins.  One exchange call:
 *   collective 0   all-gather of every rank's (first, n_local, k, key_type, flags);
 *   collective 1   all-to-all-v of the candidates: every rank selects its own min(k, n_local)
 *                  winners with the select path above (positions offset by `first`) and sends the
 *                  same block to every rank; the counts follow from the table.  4-byte keys travel as
 *                  packed words; 8-byte keys as their keys (collective 1) and their positions
 *                  (collective 2) -- the numbering of DSORT_OPT_TEST_FAIL_EXCHANGE.
 * The blocks land in the order of the ranges' starts, not of the ranks, so that equal keys are in
 * ascending global position; every rank then sorts the candidates as the local call does and takes
 * the first k.  Checked symmetrically after collective 0 -- DSORT_EINVAL on every rank from the same
 * call, the communicator stays usable: ranks that disagree on k, key_type or flags, overlapping
 * ranges (dsort_plan_gather_table's rule), k above the total key count, more than 256 ranks,
 * nranks * k >= 2^32.  Before any collective: the local calls' argument checks, and
 * first + n_local > 2^32.  Gates, deadline, dsort_comm_abort and DSORT_OPT_TEST_FAIL_EXCHANGE work as
 * in a gather; the kill options do not act on it; DSORT_OPT_TOPK_PATH does not either (a rank's
 * candidates always come from the select path).  The RCCL path has run with one rank only. */
int dsort_plan_topk(size_t n, size_t k, int key_bytes, int topk_path_opt, int *path, int *digits);
int dsort_topk_dev_keys(dsort_ctx *ctx, const void *d_keys, size_t n, size_t k, int key_type, int flags,
                        void *d_keys_out, uint32_t *d_idx_out, void *stream);
/* host form (synchronous, staged like dsort_argsort_keys) */
int dsort_topk_keys(dsort_ctx *ctx, const void *keys, size_t n, size_t k, int key_type, int flags,
                    void *keys_out, uint32_t *idx);
int dsort_sample_topk_dev_keys(dsort_ctx *ctx, const void *d_keys, size_t n_local, uint64_t first, size_t k,
                               int key_type, int flags, void *d_keys_out, uint32_t *d_idx_out, void *stream);

/* ABI 9: the distributed record gather -- payloads follow their keys across ranks.
 *   d_dst[j] = the record at GLOBAL position d_idx[j], j < n_idx, wherever it lives.
 * This rank owns the records at global positions first .. first + n_src - 1 (d_src[0..n_src)), and
 * d_idx holds the n_idx global positions it wants, e.g. the index slice of
 * dsort_sample_argsort_dev_i32: argsort, then one gather per payload column.
 *
 * Algorithm, a request/reply exchange over the communicator (either transport): 0. all-gather of
 * every rank's (first, n_src, elem_bytes) -- the range table; 1. all-gather of every rank's request
 * counts per owner, plus one column counting its indices nobody owns; 2. all-to-all-v of the
 * requests (uint32 local indices, routed by a stable partition of d_idx by owner); the owners serve
 * them with the kernel of dsort_gather_dev; 3. the reverse all-to-all-v of the records, which are
 * then put back into the order of d_idx.  At one rank nothing is sent and every kernel still runs.
 *
 * Contract: collective -- every rank of the communicator calls it.  A rank with n_src == 0 and/or
 * n_idx == 0 (its pointers may then be NULL) still joins every collective.  elem_bytes is 4, 8 or
 * 16 as for dsort_gather_dev; records and indices need 4-byte alignment only.  The inputs are not
 * modified; d_dst (caller-owned, n_idx records, no overlap with the inputs) is ready after
 * `stream`.  d_idx may be the context-owned index array of dsort_sample_argsort_dev_i32: a gather
 * uses arenas of its own and invalidates no slice of a sample sort, so several payload columns can
 * be gathered from one argsort.  The ranks' ranges may come in any rank order; indices may repeat,
 * may all name one owner and need not be a permutation.  n_idx < 2^32.
 *
 * Errors.  Checked before any memory or collective is touched, DSORT_EINVAL: a NULL ctx (plain
 * return), elem_bytes not 4 / 8 / 16, first + n_src > 2^32, n_idx >= 2^32, a NULL pointer whose
 * count is non-zero.  Without a communicator: DSORT_ECOMM, as dsort_sample_sort_dev_*.  More than
 * 256 ranks (the owner table's fixed size): DSORT_EINVAL on every rank before the first collective.
 * Checked symmetrically -- every rank returns DSORT_EINVAL from the same call, the communicator and
 * the context stay usable: two non-empty ranges that overlap, ranks that disagree on elem_bytes
 * (both seen by every rank in the range table) and an index that no rank owns (any non-zero entry
 * of the count matrix's extra column; the message names the first such rank and its count; no
 * request has moved by then).  This does not rely on the host transport's status gates.
 * DSORT_OPT_COMM_TIMEOUT_MS, dsort_comm_abort, dsort_comm_deadline_ms, the host transport's status
 * gates and DSORT_OPT_TEST_FAIL_EXCHANGE work as in a sample sort, k counting the gather's own four
 * collectives as numbered above (0 = the range-table all-gather).  DSORT_OPT_KILL_AFTER_STAGE and
 * DSORT_OPT_KILL_IN_EXCHANGE do not act on a gather.
 *
 * dsort_get_stats: the call sets gather_sent and gather_served and nothing else, so the preceding
 * sample sort's statistics stay readable.
 *
 * Memory (context arenas of the gather's own, grow-only): with W = elem_bytes and m the requests
 * this rank receives, 4 n_idx + 4 m + W m + W n_idx bytes, plus at most 2.1 MB of routing tables;
 * on the host transport the pinned staging of the sample sort (max(4 n_idx, W m) and
 * max(4 m, W n_idx) bytes).
 *
 * Not offered: records wider than 16 bytes in one call (gather the columns one by one).  The RCCL
 * path has run with one rank only. */
int dsort_sample_gather_dev(dsort_ctx *ctx, const void *d_src, size_t n_src, uint64_t first,
                            const uint32_t *d_idx, size_t n_idx, void *d_dst, int elem_bytes,
                            void *stream);

/* ---------------------------------------------------------------- sample-sort planning  */
/* Host-side planning rules of the sample sort, exported so that the CPU tests (gloo, no GPU)
 * exercise the exact code the GPU path runs.
 *
 * dsort_plan_splitters_*: `samples` holds nranks*s keys, s per rank, each rank's block sorted,
 * sample j of rank r having local index idx[r*s+j].  Writes nranks-1 splitters as
 * (value, rank, index) triples: the composite order (value, rank, index) is total, so ranks
 * holding a heavy duplicate split it between them instead of one rank receiving it all. */
int dsort_plan_splitters_i32(int nranks, int s, const int32_t *samples, const uint64_t *idx,
                             int32_t *split_val, int32_t *split_rank, uint64_t *split_idx);
int dsort_plan_splitters_i64(int nranks, int s, const int64_t *samples, const uint64_t *idx,
                             int64_t *split_val, int32_t *split_rank, uint64_t *split_idx);
/* dsort_plan_cuts_*: for a sorted local run of rank `my_rank`, cuts[0..nranks] (cuts[0]=0,
 * cuts[nranks]=n) such that keys [cuts[r], cuts[r+1]) go to rank r. */
int dsort_plan_cuts_i32(const int32_t *sorted, size_t n, int my_rank, int nranks,
                        const int32_t *split_val, const int32_t *split_rank,
                        const uint64_t *split_idx, uint64_t *cuts);
int dsort_plan_cuts_i64(const int64_t *sorted, size_t n, int my_rank, int nranks,
                        const int64_t *split_val, const int32_t *split_rank,
                        const uint64_t *split_idx, uint64_t *cuts);
/* Regular sample positions of a local run of n keys: s indices (j+1)*n/(s+1), j<s. */
int dsort_plan_sample_positions(size_t n, int s, uint64_t *idx);
/* The distributed gather's host rules (ABI 9).
 * dsort_plan_gather_table: from every rank's range [first[r], first[r] + count[r]) the owner table:
 * the non-empty ranges sorted by their start, range i = [lo[i], hi[i]) owned by rank owner[i]
 * (arrays of nranks entries, *nranges of them written).  DSORT_EINVAL when two ranges overlap or one
 * ends beyond 2^32.
 * dsort_plan_gather_route: the routing of n indices by that table, as the kernels do it (the same
 * owner lookup: a binary search over lo, compared as unsigned, and a check against hi):
 * counts[r] = the indices rank r owns, counts[nranks] = those nobody owns; pos[j] = the place of
 * index j in the request layout -- owner-major, input order inside an owner (stable), the unowned
 * ones last. */
int dsort_plan_gather_table(int nranks, const uint64_t first[], const uint64_t count[], uint64_t lo[],
                            uint64_t hi[], int32_t owner[], int *nranges);
int dsort_plan_gather_route(int nranges, const uint64_t lo[], const uint64_t hi[], const int32_t owner[],
                            int nranks, const uint32_t *idx, size_t n, uint64_t counts[], uint64_t pos[]);

/* ---------------------------------------------------------------- utilities ---------- */
/* Synthetic workload generators on the GPU: key i = f(splitmix64(seed+first+i)).
 * uniform i32 = high 32 bits, uniform i64 = all 64 bits; zipf i64 = s=1.2 over 2^24 ranks,
 * key = rank * 0x9E3779B97F4A7C15 (an odd multiplier, so ranks map to distinct keys). */
int dsort_gen_uniform_i32(dsort_ctx *ctx, int32_t *d_keys, size_t n, uint64_t seed,
                          uint64_t first, void *stream);
int dsort_gen_uniform_i64(dsort_ctx *ctx, int64_t *d_keys, size_t n, uint64_t seed,
                          uint64_t first, void *stream);
int dsort_gen_zipf_i64(dsort_ctx *ctx, int64_t *d_keys, size_t n, uint64_t seed, uint64_t first,
                       void *stream);
/* Size-independent parity checks on device data: order-independent multiset fingerprint
 * (sum and xor of splitmix64 of each key) and the number of adjacent descents (0 = sorted).
 * Blocking: results are on the host when the call returns. */
int dsort_fingerprint_i32(dsort_ctx *ctx, const int32_t *d_keys, size_t n, uint64_t *sum,
                          uint64_t *xr);
int dsort_fingerprint_i64(dsort_ctx *ctx, const int64_t *d_keys, size_t n, uint64_t *sum,
                          uint64_t *xr);
int dsort_count_descents_i32(dsort_ctx *ctx, const int32_t *d_keys, size_t n, uint64_t *count);
int dsort_count_descents_i64(dsort_ctx *ctx, const int64_t *d_keys, size_t n, uint64_t *count);

/* Device memory helpers for hosts without another allocator (C master/worker, ctypes). */
int dsort_dev_alloc(dsort_ctx *ctx, void **d_ptr, size_t bytes);
int dsort_dev_free(dsort_ctx *ctx, void *d_ptr);
int dsort_copy_h2d(dsort_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
int dsort_copy_d2h(dsort_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
int dsort_copy_d2d(dsort_ctx *ctx, void *d_dst, const void *d_src, size_t bytes);
/* Pins a host range for DMA (hipHostRegister) and releases it: the master's chunk replicas,
 * mapped from shared memory by every worker of the C sample sort (host/ss.h). */
int dsort_host_register(dsort_ctx *ctx, void *host, size_t bytes);
int dsort_host_unregister(dsort_ctx *ctx, void *host);

/* Text output of the reference (server.c:517-519): one "%d\n" per key into `path`.
 * Host-only helper; returns DSORT_EINVAL if the file cannot be written. */
int dsort_write_text_i32(const char *path, const int32_t *keys, size_t n);

/* GPU text codec, asynchronous on `stream` (NULL: the context's stream) up to
 * the returned length/count, which synchronizes.
 *
 * dsort_format_text_dev_i32 replaces the output loop of merge_chunks (server.c:517-519,
 * fprintf(output, "%d\n", merged[i])): writes the output.txt bytes of n device keys to d_text
 * (cap >= 12 * n bytes, else DSORT_EINVAL) and their count to *out_len.
 *
 * dsort_parse_text_dev_i32 replaces the two fscanf("%d") passes of main (server.c:179-182 and
 * 212-214): parses whitespace-separated [+-]?[0-9]+ tokens of d_text (16-byte aligned, len bytes)
 * into d_keys in file order; *n_out = the number of tokens (keys past cap are counted, not
 * stored).  Values beyond int32 saturate at 2^32 and wrap (the oracle's rule; %d overflow is
 * undefined in the reference).  A token that is not an integer returns DSORT_EINVAL, with its
 * byte offset in dsort_last_error (the reference loops forever there). */
int dsort_format_text_dev_i32(dsort_ctx *ctx, const int32_t *d_keys, size_t n, char *d_text,
                              size_t cap, size_t *out_len, void *stream);
int dsort_parse_text_dev_i32(dsort_ctx *ctx, const char *d_text, size_t len, int32_t *d_keys,
                             size_t cap, size_t *n_out, void *stream);

/* Host-buffer forms of the codec (synchronous; staged through the context's device arenas), for
 * the C master at the server.c:179/213 parse and server.c:517-519 write positions.
 * dsort_format_text_i32 returns DSORT_EINVAL if the text needs more than cap bytes (12 per key
 * always suffice). */
int dsort_parse_text_i32(dsort_ctx *ctx, const char *text, size_t len, int32_t *keys, size_t cap,
                         size_t *n_out);
int dsort_format_text_i32(dsort_ctx *ctx, const int32_t *keys, size_t n, char *text, size_t cap,
                          size_t *len_out);

#ifdef __cplusplus
}
#endif
#endif /* DSORT_H */
