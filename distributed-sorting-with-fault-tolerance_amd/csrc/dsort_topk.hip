// dsort_topk.hip -- top-k selection (dsort.h, "Top-k", an ABI 10 addition): the first k entries of
// the stable argsort in the typed order, without sorting the other n - k keys.
//
// A most-significant-digit radix select.  A key goes through the codec (dsort_keycodec.h, a
// template parameter as in the pack kernels) to its word w, and u = w ^ sign_bit, compared as
// unsigned, is what the select works on.  Digits of 11 bits (a workgroup histogram is 8 KiB of LDS):
// 3 passes for 4-byte keys (11 + 11 + 10 bits), 6 for 8-byte keys (5 x 11 + 9).
//
// Every workgroup owns one contiguous range of positions -- the same range in every kernel of a
// call (select_grid) -- cut in tiles of NT 16-byte loads, typed 4-byte aligned like everything of
// the caller's (dsort_pairs.hip); a range starts at a multiple of the tile, so the loads are
// 16-byte aligned where the pointer is.  Per pass:
//   hist      counts the pass's digit of the keys whose higher digits equal the prefix chosen so
//             far (read from the device state: nothing waits on the host) in LDS and writes its
//             counts as one row per workgroup -- no global atomic.  A wave's lanes that hold the
//             digit of its first active lane count with one LDS atomic (bump: the aggregation of
//             bucket_bump, dsort_bucket.h), so equal keys, keys of [1, 100] and sorted input do not
//             serialise on one counter.
//   colsum    sums the rows by column, 64 rows per workgroup, into at most 32 partial rows
//   pick      one workgroup: sums the partial rows, scans the bins, picks the digit d with
//             count(< d) < k_rest <= count(<= d), appends it to the prefix and takes count(< d)
//             off k_rest
//   less      less[g] += workgroup g's own count of the bins below d; after the last pass
//             eq[g] = its count of bin d
// After the last pass the prefix is the threshold word T and r = k_rest copies of it are wanted.
// `offsets` (one workgroup) scans eq into every workgroup's tie quota and less + quota into its
// output offset.  `compact`, the last read of the keys, writes the winners -- u < T, or u == T with
// a tie rank below r -- in ascending position, stable within a workgroup by a prefix sum per tile
// and across workgroups by those offsets: 4-byte keys as the pair sort's packed word
// (uint64)w << 32 | position, 8-byte keys as the raw key and the position in two arrays.  The k
// candidates are then sorted by the existing paths: sort_device<int64_t> and the pair sort's unpack,
// or p64::argsort64 (stable: the candidates are in ascending position) and the gather kernel.
//
// HBM traffic: 4 reads of the keys (4-byte) or 7 (8-byte), 16 MiB of rows written and read twice
// per pass at the full grid, and the k candidates.  Memory: DESIGN.md 3.9.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dsort_exch.h"
#include "dsort_keycodec.h"

namespace dsort {
namespace tk {

constexpr int NT = 256;           // threads per workgroup
constexpr int WAVES = NT / 64;
constexpr unsigned MAXWG = 2048;  // workgroups of a launch, as in dsort_keys.hip
constexpr int DB = 11;            // bits of a digit
constexpr int NB = 1 << DB;       // bins of a histogram
constexpr int RSL = 64;           // rows one colsum workgroup sums
constexpr int MAXRS = MAXWG / RSL;
constexpr int SEG = MAXWG / NT;   // workgroups per thread of the offsets kernel

// The crossover of dsort_plan_topk: the full argsort below TOPK_MIN_N keys and above one key in
// TOPK_MAX_FRAC.  From profiles/topk_bench.json: at k = n / 2 the select path is 14 %
// (4-byte keys) and 12 % (8-byte keys) ahead at 2^24 keys and further ahead above, against a
// run-to-run spread of 1-2 %; at 2^22 keys it is behind at n / 2 and level at n / 8; at 2^28 keys
// the paths meet near 0.9 n (4-byte) and 0.75 n (8-byte).
constexpr uint64_t TOPK_MIN_N = 1ull << 24;
constexpr uint64_t TOPK_MAX_FRAC = 2;

typedef uint32_t u4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// the device state of a call
struct State {
    uint64_t prefix;  // the digits chosen so far, in their place in u (the other bits 0)
    uint64_t k_rest;  // what is still wanted among the keys that match the prefix
    uint32_t d;       // the digit the last pick chose
    uint32_t pad;
};

template <int W>
struct Word;
template <>
struct Word<4> {
    using U = uint32_t;
    static constexpr int E = 4;  // elements of one 16-byte load
    static constexpr U SIGN = 0x80000000u;
};
template <>
struct Word<8> {
    using U = uint64_t;
    static constexpr int E = 2;
    static constexpr U SIGN = 1ull << 63;
};

// A lane's 16 bytes of the tile at element e0 (the elements at or beyond `end` read as 0).
template <int W>
__device__ __forceinline__ u4_a4 load_raw(const uint32_t *keys, uint64_t e0, uint64_t end) {
    constexpr int E = Word<W>::E, D = W / 4;
    if (e0 + E <= end) return *reinterpret_cast<const u4_a4 *>(keys + e0 * D);
    uint32_t r[4] = {0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < E; ++e)
        if (e0 + e < end) {
#pragma unroll
            for (int d = 0; d < D; ++d) r[e * D + d] = keys[(e0 + e) * D + d];
        }
    return u4_a4{r[0], r[1], r[2], r[3]};
}

// element e of those 16 bytes: the key's bits
template <int W>
__device__ __forceinline__ typename Word<W>::U bits_of(u4_a4 v, int e) {
    if (W == 4) return (typename Word<W>::U)(e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w);
    return (typename Word<W>::U)(e == 0 ? ((uint64_t)v.y << 32) | v.x : ((uint64_t)v.w << 32) | v.z);
}

// One count of bin b for every active lane: the lanes that share the first active lane's bin add
// their number with one atomic, the others one each.
__device__ __forceinline__ void bump(uint32_t *hist, uint32_t b, bool act) {
    const uint64_t am = __ballot(act);
    if (!am) return;
    const int first = (int)__ffsll((long long)am) - 1;
    const uint32_t b0 = (uint32_t)__shfl((int)b, first);
    const uint64_t same = __ballot(act && b == b0);
    if (act && b != b0) atomicAdd(&hist[b], 1u);
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[b0], (uint32_t)__popcll(same));
}

__global__ void topk_init_kernel(State *st, uint64_t k) {
    st->prefix = 0;
    st->k_rest = k;
    st->d = 0;
    st->pad = 0;
}

// rows[g * NB + b] = workgroup g's keys of digit b -- (u >> shift) & mask -- among those whose bits
// from hi_shift up equal the prefix (FIRST: all keys).  Workgroup g owns
// keys[g * chunk, min(n, (g + 1) * chunk)).
template <int KC, int W, bool FIRST>
__global__ void __launch_bounds__(NT) topk_hist_kernel(const uint32_t *__restrict__ keys, uint64_t n, uint64_t chunk,
                                                       const State *__restrict__ st, int shift, uint32_t mask,
                                                       int hi_shift, uint32_t *__restrict__ rows) {
    using U = typename Word<W>::U;
    using C = kc::Codec<KC>;
    constexpr int E = Word<W>::E;
    constexpr uint64_t TILE = (uint64_t)NT * E;
    __shared__ uint32_t hist[NB];
    for (int b = threadIdx.x; b < NB; b += NT) hist[b] = 0;
    const U prefix = FIRST ? (U)0 : (U)st->prefix;
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * chunk;
    const uint64_t end = begin + chunk < n ? begin + chunk : n;
    u4_a4 next = load_raw<W>(keys, begin + (uint64_t)E * threadIdx.x, end);
    for (uint64_t base = begin; base < end; base += TILE) {
        const uint64_t e0 = base + (uint64_t)E * threadIdx.x;
        const u4_a4 v = next;
        if (base + TILE < end) next = load_raw<W>(keys, e0 + TILE, end);
#pragma unroll
        for (int e = 0; e < E; ++e) {
            const U u = C::enc(bits_of<W>(v, e)) ^ Word<W>::SIGN;
            bool act = e0 + e < end;
            if (!FIRST) act = act && ((u ^ prefix) >> hi_shift) == 0;
            bump(hist, (uint32_t)(u >> shift) & mask, act);
        }
    }
    __syncthreads();
    for (int b = threadIdx.x; b < NB; b += NT) rows[(uint64_t)blockIdx.x * NB + b] = hist[b];
}

// part[y * NB + b] = the sum of rows [y * RSL, min(G, (y + 1) * RSL)) of column b; grid (NB / NT, RS)
__global__ void __launch_bounds__(NT) topk_colsum_kernel(const uint32_t *__restrict__ rows, int G,
                                                         uint32_t *__restrict__ part) {
    const int b = blockIdx.x * NT + threadIdx.x;
    const int g0 = blockIdx.y * RSL, g1 = g0 + RSL < G ? g0 + RSL : G;
    uint32_t sum = 0;
    for (int g = g0; g < g1; ++g) sum += rows[(uint64_t)g * NB + b];
    part[(uint64_t)blockIdx.y * NB + b] = sum;
}

// exclusive prefix sum of v over the workgroup's threads (sh: NT words)
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t *sh) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {
        const uint64_t x = t >= o ? sh[t - o] : 0;
        __syncthreads();
        sh[t] += x;
        __syncthreads();
    }
    const uint64_t incl = sh[t];
    __syncthreads();
    return incl - v;
}

// One workgroup: the bins' totals from the RS partial rows, their scan, and the digit d with
// count(< d) < k_rest <= count(<= d).  A thread takes NB / NT consecutive bins.
__global__ void __launch_bounds__(NT) topk_pick_kernel(const uint32_t *__restrict__ part, int RS, State *st,
                                                       int shift) {
    constexpr int PER = NB / NT;
    __shared__ uint64_t sh[NT];
    uint64_t c[PER], sum = 0;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        uint64_t a = 0;
        for (int y = 0; y < RS; ++y) a += part[(uint64_t)y * NB + threadIdx.x * PER + i];
        c[i] = a;
        sum += a;
    }
    const uint64_t k = st->k_rest;  // (read by every thread before the scan's barriers, written behind them)
    uint64_t run = block_excl_scan(sum, sh);
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        if (run < k && k <= run + c[i]) {
            const uint32_t d = threadIdx.x * PER + i;
            st->prefix |= (uint64_t)d << shift;
            st->k_rest = k - run;
            st->d = d;
        }
        run += c[i];
    }
}

// A wave per workgroup row g: less[g] (+)= the row's bins below d; LAST: eq[g] = its bin d.
template <bool FIRST, bool LAST>
__global__ void __launch_bounds__(NT) topk_less_kernel(const uint32_t *__restrict__ rows, int G,
                                                       const State *__restrict__ st, uint32_t *__restrict__ less,
                                                       uint32_t *__restrict__ eq) {
    const int g = blockIdx.x * WAVES + (int)(threadIdx.x >> 6);
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t d = st->d;
    uint32_t sum = 0;
    if (g < G)
        for (uint32_t b = lane; b < d; b += 64) sum += rows[(uint64_t)g * NB + b];
    const uint32_t incl = wave_incl_sum(sum);  // (all 64 lanes: the DPP prefix sum needs them)
    if (g < G && lane == 63) {
        less[g] = FIRST ? incl : less[g] + incl;
        if (LAST) eq[g] = rows[(uint64_t)g * NB + d];
    }
}

// One workgroup: quota[g] = the copies of T workgroup g contributes (the first r in position order),
// off[g] = the winners of the workgroups before g.  A thread takes SEG consecutive workgroups.
__global__ void __launch_bounds__(NT) topk_offsets_kernel(const uint32_t *__restrict__ less,
                                                          const uint32_t *__restrict__ eq, int G,
                                                          const State *__restrict__ st, uint32_t *__restrict__ quota,
                                                          uint64_t *__restrict__ off) {
    __shared__ uint64_t sh[NT];
    const uint64_t r = st->k_rest;
    const int seg = (G + NT - 1) / NT, g0 = (int)threadIdx.x * seg;
    uint64_t e[SEG], w[SEG], sum = 0;
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
        e[i] = i < seg && g0 + i < G ? eq[g0 + i] : 0u;
        sum += e[i];
    }
    uint64_t tb = block_excl_scan(sum, sh);  // the copies of T before this thread's workgroups
    sum = 0;
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
        const uint64_t room = tb < r ? r - tb : 0;
        const uint64_t take = e[i] < room ? e[i] : room;
        tb += e[i];
        w[i] = take;
        if (i < seg && g0 + i < G) {
            quota[g0 + i] = (uint32_t)take;
            w[i] += less[g0 + i];
        }
        sum += w[i];
    }
    uint64_t o = block_excl_scan(sum, sh);
#pragma unroll
    for (int i = 0; i < SEG; ++i)
        if (i < seg && g0 + i < G) {
            off[g0 + i] = o;
            o += w[i];
        }
}

// The winners of workgroup g's range, in ascending position, from slot off[g] on: W == 4
// out_w[slot] = (uint64)w << 32 | (posbase + position); W == 8 out_w[slot] = the key's bits and
// out_p[slot] = posbase + position.  A slot at or beyond cap (= k) is never written.
// Inside a tile a lane counts its keys below T and equal to T; one wave prefix sum of the two
// counts packed in a word (16 bits each: a tile has at most 1024 keys) and the waves' totals through
// LDS give every key its number of smaller and of equal keys before it in the tile.  The ties are
// taken in position order, so a key's slot is: the workgroup's running offset + the smaller ones
// before it + the ties before it that are within the quota.
template <int KC, int W>
__global__ void __launch_bounds__(NT) topk_compact_kernel(const uint32_t *__restrict__ keys, uint64_t n,
                                                          uint64_t chunk, const State *__restrict__ st,
                                                          const uint32_t *__restrict__ quota,
                                                          const uint64_t *__restrict__ off, uint32_t posbase,
                                                          uint64_t cap, uint64_t *__restrict__ out_w,
                                                          uint32_t *__restrict__ out_p) {
    using U = typename Word<W>::U;
    using C = kc::Codec<KC>;
    constexpr int E = Word<W>::E;
    constexpr uint64_t TILE = (uint64_t)NT * E;
    __shared__ uint32_t s_tot[2][WAVES];
    const U T = (U)st->prefix;
    uint64_t wr = off[blockIdx.x];          // the next free slot (every thread keeps its own copy)
    uint32_t ties = quota[blockIdx.x];      // copies of T still to take
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint64_t begin = (uint64_t)blockIdx.x * chunk;
    const uint64_t end = begin + chunk < n ? begin + chunk : n;
    u4_a4 next = load_raw<W>(keys, begin + (uint64_t)E * threadIdx.x, end);
    int par = 0;
    for (uint64_t base = begin; base < end; base += TILE, par ^= 1) {
        const uint64_t e0 = base + (uint64_t)E * threadIdx.x;
        const u4_a4 v = next;
        if (base + TILE < end) next = load_raw<W>(keys, e0 + TILE, end);
        U b[E], u[E];
        uint32_t pk = 0;  // equal to T: bits 16.., below T: bits 0..15
#pragma unroll
        for (int e = 0; e < E; ++e) {
            b[e] = bits_of<W>(v, e);
            u[e] = C::enc(b[e]) ^ Word<W>::SIGN;
            if (e0 + e < end) pk += u[e] < T ? 1u : (u[e] == T ? 0x10000u : 0u);
        }
        const uint32_t incl = wave_incl_sum(pk);
        if (lane == 63) s_tot[par][wv] = incl;
        __syncthreads();
        uint32_t pre = 0, tot = 0;
#pragma unroll
        for (int x = 0; x < WAVES; ++x) {
            const uint32_t t = s_tot[par][x];
            if (x < (int)wv) pre += t;
            tot += t;
        }
        // (the next tile writes the other half of s_tot; the one after it comes behind the next
        // barrier, which every wave reaches only after these reads)
        const uint32_t excl = incl - pk + pre;
        uint32_t lt_b = excl & 0xFFFFu, eq_b = excl >> 16;
#pragma unroll
        for (int e = 0; e < E; ++e) {
            if (e0 + e >= end) continue;
            uint64_t slot = ~0ull;
            if (u[e] < T) {
                slot = wr + lt_b + (eq_b < ties ? eq_b : ties);
                ++lt_b;
            } else if (u[e] == T) {
                if (eq_b < ties) slot = wr + lt_b + eq_b;
                ++eq_b;
            }
            if (slot < cap) {
                const uint32_t pos = posbase + (uint32_t)(e0 + e);
                if (W == 4) {
                    out_w[slot] = ((uint64_t)(u[e] ^ Word<W>::SIGN) << 32) | pos;
                } else {
                    out_w[slot] = (uint64_t)b[e];
                    out_p[slot] = pos;
                }
            }
        }
        const uint32_t t_eq = tot >> 16, take = t_eq < ties ? t_eq : ties;
        wr += (tot & 0xFFFFu) + take;
        ties -= take;
    }
}

// The grid of a call over n keys of W bytes: G workgroups of `chunk` keys each, chunk a multiple of
// the tile and at least MIN_TILES tiles (16 KiB of keys): a workgroup writes an 8 KiB row per pass,
// which two small kernels read again, so a finer grid moves more rows than keys (measured at 2^20
// 8-byte keys with one tile per workgroup: 0.47 ms against the full argsort's 0.41).
constexpr uint64_t MIN_TILES = 4;
static void select_grid(uint64_t n, int W, unsigned *G, uint64_t *chunk) {
    const uint64_t tile = (uint64_t)NT * (16 / W);
    const uint64_t tiles = (n + tile - 1) / tile;
    uint64_t per = (tiles + MAXWG - 1) / MAXWG;  // tiles per workgroup
    if (per < MIN_TILES) per = MIN_TILES;
    *chunk = per * tile;
    *G = (unsigned)((n + *chunk - 1) / *chunk);
    if (*G == 0) *G = 1;
}

static int digits_of(int W) { return (8 * W + DB - 1) / DB; }

// the small arena: state | partial rows | less | eq | quota | off
constexpr size_t OFF_PART = 64;
constexpr size_t OFF_LESS = OFF_PART + (size_t)MAXRS * NB * 4;
constexpr size_t OFF_EQ = OFF_LESS + (size_t)MAXWG * 4;
constexpr size_t OFF_QUOTA = OFF_EQ + (size_t)MAXWG * 4;
constexpr size_t OFF_OFF = OFF_QUOTA + (size_t)MAXWG * 4;
constexpr size_t SMALL_BYTES = OFF_OFF + (size_t)MAXWG * 8;

struct KeySpec {
    int kc = 0, bytes = 4;
};
static bool parse(int key_type, int flags, KeySpec *k) {
    int cls = 0;
    if (!kc::type_info(key_type, &cls, &k->bytes)) return false;
    if (flags & ~DSORT_ORDER_DESCENDING) return false;
    k->kc = kc::id_of(cls, (flags & DSORT_ORDER_DESCENDING) != 0);
    return true;
}
static int bad_spec(dsort_ctx *ctx) {
    return set_err(ctx, DSORT_EINVAL, "unknown key_type (DSORT_KEY_*) or flags (DSORT_ORDER_DESCENDING only)");
}

// the codec id as a template argument, the identity included
#define DSORT_TK_KC(id, ...)                          \
    do {                                              \
        if ((id) == 0) {                              \
            constexpr int KC_ = 0;                    \
            __VA_ARGS__;                              \
        } else {                                      \
            DSORT_KC_SWITCH(id, __VA_ARGS__);         \
        }                                             \
    } while (0)

template <int W>
static void launch_hist(int kc, bool first, unsigned G, hipStream_t s, const uint32_t *keys, uint64_t n,
                        uint64_t chunk, const State *st, int shift, uint32_t mask, int hi_shift, uint32_t *rows) {
    if (first) {
        DSORT_TK_KC(kc, hipLaunchKernelGGL((topk_hist_kernel<KC_, W, true>), dim3(G), dim3(NT), 0, s, keys, n, chunk, st,
                                           shift, mask, hi_shift, rows));
    } else {
        DSORT_TK_KC(kc, hipLaunchKernelGGL((topk_hist_kernel<KC_, W, false>), dim3(G), dim3(NT), 0, s, keys, n, chunk, st,
                                           shift, mask, hi_shift, rows));
    }
}

template <int W>
static void launch_compact(int kc, unsigned G, hipStream_t s, const uint32_t *keys, uint64_t n, uint64_t chunk,
                           const State *st, const uint32_t *quota, const uint64_t *off, uint32_t posbase, uint64_t cap,
                           uint64_t *out_w, uint32_t *out_p) {
    DSORT_TK_KC(kc, hipLaunchKernelGGL((topk_compact_kernel<KC_, W>), dim3(G), dim3(NT), 0, s, keys, n, chunk, st, quota,
                                       off, posbase, cap, out_w, out_p));
}

// The legs' events of the last select (dsort_topk_leg_ms), recorded only when asked for
// (dsort_topk_leg_timing): 2 p and 2 p + 1 around pass p's histogram, 12 and 13 around the compaction.
constexpr int EV_COMPACT = 12, EV_COUNT = 14;

// The select itself: the k (1 <= k <= n) winners of keys[0..n) in ascending position into out_w
// (and, 8-byte keys, out_p), k slots each; positions count from posbase.  Asynchronous on s, inside
// the caller's order bracket.
static int select(dsort_ctx *ctx, const void *d_keys, size_t n, size_t k, KeySpec ks, uint32_t posbase,
                  hipStream_t s, uint64_t *out_w, uint32_t *out_p) {
    const int W = ks.bytes;
    unsigned G = 0;
    uint64_t chunk = 0;
    select_grid((uint64_t)n, W, &G, &chunk);
    int rc = ensure(ctx, ctx->tk_rows, (size_t)G * NB * 4, "top-k histogram rows");
    if (rc) return rc;
    rc = ensure(ctx, ctx->tk_small, SMALL_BYTES, "top-k tables");
    if (rc) return rc;
    char *sm = ctx->tk_small.as<char>();
    State *st = reinterpret_cast<State *>(sm);
    uint32_t *part = reinterpret_cast<uint32_t *>(sm + OFF_PART);
    uint32_t *less = reinterpret_cast<uint32_t *>(sm + OFF_LESS);
    uint32_t *eq = reinterpret_cast<uint32_t *>(sm + OFF_EQ);
    uint32_t *quota = reinterpret_cast<uint32_t *>(sm + OFF_QUOTA);
    uint64_t *off = reinterpret_cast<uint64_t *>(sm + OFF_OFF);
    uint32_t *rows = ctx->tk_rows.as<uint32_t>();
    const uint32_t *keys = static_cast<const uint32_t *>(d_keys);
    const int RS = (int)((G + RSL - 1) / RSL), passes = digits_of(W), bits = 8 * W;
    LegClock &clk = ctx->tk_clk;
    clk.start(ctx->tk_timing);
    ctx->tk_passes = 0;
    hipLaunchKernelGGL(topk_init_kernel, dim3(1), dim3(1), 0, s, st, (uint64_t)k);
    DSORT_HIP(ctx, hipGetLastError());
    for (int p = 0; p < passes; ++p) {
        const int hi_shift = bits - DB * p;                 // the bits from here up are the prefix
        const int shift = hi_shift > DB ? hi_shift - DB : 0;
        const uint32_t mask = (1u << (hi_shift - shift)) - 1u;
        const bool first = p == 0, last = p == passes - 1;
        clk.mark_at(2 * p, s);
        if (W == 4)
            launch_hist<4>(ks.kc, first, G, s, keys, (uint64_t)n, chunk, st, shift, mask, hi_shift, rows);
        else
            launch_hist<8>(ks.kc, first, G, s, keys, (uint64_t)n, chunk, st, shift, mask, hi_shift, rows);
        DSORT_HIP(ctx, hipGetLastError());
        clk.mark_at(2 * p + 1, s);
        hipLaunchKernelGGL(topk_colsum_kernel, dim3(NB / NT, RS), dim3(NT), 0, s, rows, (int)G, part);
        DSORT_HIP(ctx, hipGetLastError());
        hipLaunchKernelGGL(topk_pick_kernel, dim3(1), dim3(NT), 0, s, part, RS, st, shift);
        DSORT_HIP(ctx, hipGetLastError());
        const dim3 lg((G + WAVES - 1) / WAVES);
        if (first)
            hipLaunchKernelGGL((topk_less_kernel<true, false>), lg, dim3(NT), 0, s, rows, (int)G, st, less, eq);
        else if (!last)
            hipLaunchKernelGGL((topk_less_kernel<false, false>), lg, dim3(NT), 0, s, rows, (int)G, st, less, eq);
        else
            hipLaunchKernelGGL((topk_less_kernel<false, true>), lg, dim3(NT), 0, s, rows, (int)G, st, less, eq);
        DSORT_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(topk_offsets_kernel, dim3(1), dim3(NT), 0, s, less, eq, (int)G, st, quota, off);
    DSORT_HIP(ctx, hipGetLastError());
    clk.mark_at(EV_COMPACT, s);
    if (W == 4)
        launch_compact<4>(ks.kc, G, s, keys, (uint64_t)n, chunk, st, quota, off, posbase, (uint64_t)k, out_w, out_p);
    else
        launch_compact<8>(ks.kc, G, s, keys, (uint64_t)n, chunk, st, quota, off, posbase, (uint64_t)k, out_w, out_p);
    DSORT_HIP(ctx, hipGetLastError());
    clk.mark_at(EV_COMPACT + 1, s);
    ctx->tk_passes = clk.complete(EV_COUNT) ? passes : 0;
    return DSORT_OK;
}

static int plan(uint64_t n, uint64_t k, int key_bytes, int opt, int *path, int *digits) {
    if ((key_bytes != 4 && key_bytes != 8) || n > (1ull << 32) || k > n || opt < -1 || opt > 1) return DSORT_EINVAL;
    int p;
    if (k == 0)
        p = 0;
    else if (opt >= 0)
        p = opt ? 1 : 2;
    else
        p = n < TOPK_MIN_N || k > n / TOPK_MAX_FRAC ? 2 : 1;
    if (path) *path = p;
    if (digits) *digits = digits_of(key_bytes);
    return DSORT_OK;
}

// the candidates' sort and the outputs, 4-byte keys: the m packed words of `packed` are sorted in
// place and the first k unpacked
static int finish4(dsort_ctx *ctx, uint64_t *packed, size_t m, size_t k, KeySpec ks, void *keys_out, uint32_t *idx_out,
                   hipStream_t s, int *src) {
    *src = sort_device<int64_t>(ctx, reinterpret_cast<int64_t *>(packed), reinterpret_cast<int64_t *>(packed), m, s, true);
    if (*src && *src != DSORT_ESTAGE) return *src;
    return pr::unpack_words(ctx, packed, static_cast<int32_t *>(keys_out), idx_out, k, s, ks.kc);
}

// dsort_topk_dev_keys behind its argument checks (k >= 1)
static int topk_dev(dsort_ctx *ctx, const void *d_keys, size_t n, size_t k, KeySpec ks, void *d_keys_out,
                    uint32_t *d_idx_out, void *stream) {
    hipStream_t s = pick_stream(ctx, stream);
    int path = 0;
    if (plan((uint64_t)n, (uint64_t)k, ks.bytes, (int)ctx->opt.topk_path, &path, nullptr))
        return set_err(ctx, DSORT_EINVAL, "top-k: no plan for these counts");
    const size_t W = (size_t)ks.bytes;
    int rc = order_begin(ctx, s);
    if (rc) return rc;
    int src = DSORT_OK;
    std::string msg;
    if (path == 2) {
        // the existing argsort into arenas of the context, and its first k
        rc = ensure(ctx, ctx->a64_idx, n * 4, "top-k indices");
        if (rc) return rc;
        if (d_keys_out && (rc = ensure(ctx, ctx->tk_ck, n * W, "top-k sorted keys"))) return rc;
        uint32_t *idx = ctx->a64_idx.as<uint32_t>();
        void *ko = d_keys_out ? ctx->tk_ck.p : nullptr;
        src = W == 4 ? pr::pairs_sort(ctx, static_cast<const int32_t *>(d_keys), nullptr, static_cast<int32_t *>(ko),
                                      idx, n, s, ks.kc)
                     : p64::argsort64(ctx, static_cast<const int64_t *>(d_keys), static_cast<int64_t *>(ko), idx, n, s,
                                      ks.kc);
        if (src && src != DSORT_ESTAGE) return src;
        msg = ctx->err;
        if (d_keys_out) DSORT_HIP(ctx, hipMemcpyAsync(d_keys_out, ko, k * W, hipMemcpyDeviceToDevice, s));
        DSORT_HIP(ctx, hipMemcpyAsync(d_idx_out, idx, k * 4, hipMemcpyDeviceToDevice, s));
    } else if (W == 4) {
        rc = ensure(ctx, ctx->pairs, k * 8, "pair arena");
        if (rc) return rc;
        uint64_t *packed = ctx->pairs.as<uint64_t>();
        if ((rc = select(ctx, d_keys, n, k, ks, 0, s, packed, nullptr))) return rc;
        if ((rc = finish4(ctx, packed, k, k, ks, d_keys_out, d_idx_out, s, &src))) return rc;
        msg = ctx->err;
    } else {
        rc = ensure(ctx, ctx->tk_ck, k * 8, "top-k candidate keys");
        if (rc) return rc;
        if ((rc = ensure(ctx, ctx->tk_cp, k * 4, "top-k candidate positions"))) return rc;
        if ((rc = ensure(ctx, ctx->a64_idx, k * 4, "top-k candidate order"))) return rc;
        uint64_t *ck = ctx->tk_ck.as<uint64_t>();
        uint32_t *cp = ctx->tk_cp.as<uint32_t>(), *ord = ctx->a64_idx.as<uint32_t>();
        if ((rc = select(ctx, d_keys, n, k, ks, 0, s, ck, cp))) return rc;
        // stable over candidates in ascending position: equal keys stay in position order
        src = p64::argsort64(ctx, reinterpret_cast<const int64_t *>(ck), static_cast<int64_t *>(d_keys_out), ord, k, s,
                             ks.kc);
        if (src && src != DSORT_ESTAGE) return src;
        msg = ctx->err;
        if ((rc = dsort_gather_dev(ctx, cp, ord, d_idx_out, k, 4, stream))) return rc;
    }
    if ((rc = order_end(ctx, s))) return rc;
    return src ? set_err(ctx, src, msg) : DSORT_OK;
}

// dsort_sample_topk_dev_keys behind its argument checks.  One exchange call (dsort_exch.h), like
// the gather: collective 0 the table all-gather, 1 the candidates' all-to-all-v (8-byte keys: 1
// the keys', 2 the positions').  Every rank sends its min(k, n_local) candidates, unsorted and in
// ascending position, to every rank; the blocks land in the order of the ranges' starts, so that
// equal keys are in ascending global position for the stable sort that follows.
template <int W>
static int sample_topk(dsort_ctx *ctx, const void *d_keys, size_t n_local, uint64_t first, size_t k, KeySpec ks,
                       int key_type, int flags, void *d_keys_out, uint32_t *d_idx_out, void *stream) {
    ExchCall call(ctx, stream, W == 4 ? 2 : 3);
    if (call.rc) return call.rc;
    const int P = call.P, me = call.me;
    const hipStream_t s = call.s;
    const double deadline = call.deadline;
    if (P > 256) {
        call.finished();  // (every rank leaves here)
        return set_err(ctx, DSORT_EINVAL, "sample top-k: more than 256 ranks");
    }
    int rc = order_begin(ctx, s);
    if (rc) return rc;

    // 0. the table
    const uint64_t mine[5] = {first, (uint64_t)n_local, (uint64_t)k, (uint64_t)(uint32_t)key_type,
                              (uint64_t)(uint32_t)flags};
    std::vector<uint64_t> all((size_t)5 * P);
    rc = allgather_u64(ctx, mine, 5, all.data(), s, deadline, "sample top-k table all-gather");
    if (rc) return rc;
    auto leave = [&](const std::string &m) {
        call.finished();  // (every rank sees the same table and leaves here)
        return set_err(ctx, DSORT_EINVAL, m);
    };
    for (int r = 0; r < P; ++r)
        for (int j = 2; j < 5; ++j)
            if (all[5 * r + j] != all[j])
                return leave(std::string("sample top-k: the ranks disagree on ") +
                             (j == 2 ? "k" : j == 3 ? "key_type" : "flags") + " (rank 0 passes " +
                             std::to_string(all[j]) + ", rank " + std::to_string(r) + " " +
                             std::to_string(all[5 * r + j]) + ")");
    std::vector<uint64_t> f(P), c(P), lo(P), hi(P);
    std::vector<int32_t> own(P);
    int nr = 0;
    uint64_t total = 0;
    for (int r = 0; r < P; ++r) f[r] = all[5 * r], c[r] = all[5 * r + 1], total += c[r];
    if (dsort_plan_gather_table(P, f.data(), c.data(), lo.data(), hi.data(), own.data(), &nr))
        return leave("sample top-k: the ranks' key ranges overlap or end beyond 2^32");
    if ((uint64_t)k > total)
        return leave("sample top-k: k = " + std::to_string(k) + " exceeds the " + std::to_string(total) +
                     " keys of all ranks");
    if ((uint64_t)P * (uint64_t)k >= (1ull << 32)) return leave("sample top-k: nranks * k must stay below 2^32");
    if (k == 0) {
        call.finished();
        return order_end(ctx, s);
    }
    // every rank's candidates, and where its block lands: in the order of the ranges' starts
    std::vector<uint64_t> scnt(P), soff(P, 0), rcnt(P, 0), roff(P, 0);
    uint64_t M = 0;
    for (int i = 0; i < nr; ++i) {
        const int r = own[i];
        rcnt[r] = std::min<uint64_t>((uint64_t)k, c[r]);
        roff[r] = M;
        M += rcnt[r];
    }
    const uint64_t cm = rcnt[me];
    for (int r = 0; r < P; ++r) scnt[r] = cm;

    // this rank's candidates
    rc = ensure(ctx, ctx->tk_ck, (cm ? cm : 1) * 8, "top-k candidate keys");
    if (rc) return rc;
    if (W == 8 && (rc = ensure(ctx, ctx->tk_cp, (cm ? cm : 1) * 4, "top-k candidate positions")))
        return rc;
    uint64_t *ck = ctx->tk_ck.as<uint64_t>();
    uint32_t *cp = ctx->tk_cp.as<uint32_t>();
    if (cm && (rc = select(ctx, d_keys, n_local, (size_t)cm, ks, (uint32_t)first, s, ck, W == 8 ? cp : nullptr)))
        return rc;

    int src = DSORT_OK;
    std::string msg;
    if (W == 4) {
        rc = ensure(ctx, ctx->pairs, M * 8, "pair arena");
        if (rc) return rc;
        uint64_t *packed = ctx->pairs.as<uint64_t>();
        rc = alltoallv(ctx, A2av{ck, scnt.data(), soff.data(), cm, packed, rcnt.data(), roff.data(), M, 8, ncclUint64}, s,
                       deadline, "sample top-k candidate all-to-all", "sample top-k candidate all-to-all (staging)");
        if (rc) return rc;
        call.finished();
        if ((rc = finish4(ctx, packed, (size_t)M, k, ks, d_keys_out, d_idx_out, s, &src))) return rc;
        msg = ctx->err;
    } else {
        rc = ensure(ctx, ctx->tk_rk, M * 8, "top-k candidates received");
        if (rc) return rc;
        if ((rc = ensure(ctx, ctx->tk_rp, M * 4, "top-k positions received"))) return rc;
        if ((rc = ensure(ctx, ctx->a64_idx, M * 4, "top-k candidate order"))) return rc;
        if (d_keys_out && (rc = ensure(ctx, ctx->tk_sk, M * 8, "top-k sorted candidates"))) return rc;
        uint64_t *rk = ctx->tk_rk.as<uint64_t>();
        uint32_t *rp = ctx->tk_rp.as<uint32_t>(), *ord = ctx->a64_idx.as<uint32_t>();
        rc = alltoallv(ctx, A2av{ck, scnt.data(), soff.data(), cm, rk, rcnt.data(), roff.data(), M, 8, ncclUint64}, s,
                       deadline, "sample top-k key all-to-all", "sample top-k key all-to-all (staging)");
        if (rc) return rc;
        rc = alltoallv(ctx, A2av{cp, scnt.data(), soff.data(), cm, rp, rcnt.data(), roff.data(), M, 4, ncclUint32}, s,
                       deadline, "sample top-k position all-to-all", "sample top-k position all-to-all (staging)");
        if (rc) return rc;
        call.finished();
        int64_t *sk = d_keys_out ? ctx->tk_sk.as<int64_t>() : nullptr;
        src = p64::argsort64(ctx, reinterpret_cast<const int64_t *>(rk), sk, ord, (size_t)M, s, ks.kc);
        if (src && src != DSORT_ESTAGE) return src;
        msg = ctx->err;
        if ((rc = dsort_gather_dev(ctx, rp, ord, d_idx_out, k, 4, stream))) return rc;
        if (d_keys_out) DSORT_HIP(ctx, hipMemcpyAsync(d_keys_out, sk, k * 8, hipMemcpyDeviceToDevice, s));
    }
    if (!call.host_tx) {  // the receives must have landed before the caller reads the outputs
        rc = exch_wait(ctx, s, true, deadline, "sample top-k candidate all-to-all");
        if (rc) return rc;
    }
    if ((rc = order_end(ctx, s))) return rc;
    return src ? set_err(ctx, src, msg) : DSORT_OK;
}

}  // namespace tk
}  // namespace dsort

using namespace dsort;

extern "C" {

int dsort_plan_topk(size_t n, size_t k, int key_bytes, int topk_path_opt, int *path, int *digits) {
    return tk::plan((uint64_t)n, (uint64_t)k, key_bytes, topk_path_opt, path, digits);
}

int dsort_topk_dev_keys(dsort_ctx *ctx, const void *d_keys, size_t n, size_t k, int key_type, int flags,
                        void *d_keys_out, uint32_t *d_idx_out, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    tk::KeySpec ks;
    if (!tk::parse(key_type, flags, &ks)) return tk::bad_spec(ctx);
    if (k > n) return set_err(ctx, DSORT_EINVAL, "top-k: k exceeds n");
    if ((uint64_t)n > (1ull << 32))
        return set_err(ctx, DSORT_EINVAL, "top-k: more than 2^32 keys (a position must fit 32 bits)");
    if ((n && !d_keys) || (k && !d_idx_out)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (k == 0) return DSORT_OK;
    return tk::topk_dev(ctx, d_keys, n, k, ks, d_keys_out, d_idx_out, stream);
}

int dsort_topk_keys(dsort_ctx *ctx, const void *keys, size_t n, size_t k, int key_type, int flags, void *keys_out,
                    uint32_t *idx) {
    if (!ctx) return DSORT_EINVAL;
    tk::KeySpec ks;
    if (!tk::parse(key_type, flags, &ks)) return tk::bad_spec(ctx);
    if (k > n) return set_err(ctx, DSORT_EINVAL, "top-k: k exceeds n");
    if ((uint64_t)n > (1ull << 32))
        return set_err(ctx, DSORT_EINVAL, "top-k: more than 2^32 keys (a position must fit 32 bits)");
    if ((n && !keys) || (k && !idx)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (k == 0) return DSORT_OK;
    const size_t W = (size_t)ks.bytes, idx_bytes = (k * 4 + 15) & ~(size_t)15;
    int rc = ensure(ctx, ctx->io, n * W, "staging");
    if (rc) return rc;
    rc = ensure(ctx, ctx->io2, idx_bytes + k * W, "staging 2");
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    uint32_t *di = ctx->io2.as<uint32_t>();
    void *dk = ctx->io2.as<char>() + idx_bytes;
    DSORT_HIP(ctx, hipMemcpyAsync(ctx->io.p, keys, n * W, hipMemcpyHostToDevice, s));
    const int src = tk::topk_dev(ctx, ctx->io.p, n, k, ks, keys_out ? dk : nullptr, di, nullptr);
    if (src && src != DSORT_ESTAGE) return src;
    if (keys_out) DSORT_HIP(ctx, hipMemcpyAsync(keys_out, dk, k * W, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipMemcpyAsync(idx, di, k * 4, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipStreamSynchronize(s));
    return src;
}

int dsort_sample_topk_dev_keys(dsort_ctx *ctx, const void *d_keys, size_t n_local, uint64_t first, size_t k,
                               int key_type, int flags, void *d_keys_out, uint32_t *d_idx_out, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    tk::KeySpec ks;
    if (!tk::parse(key_type, flags, &ks)) return tk::bad_spec(ctx);
    if (first > (1ull << 32) || (uint64_t)n_local > (1ull << 32) - first)
        return set_err(ctx, DSORT_EINVAL,
                       "sample top-k: first + n_local exceeds 2^32 (a global position must fit 32 bits)");
    if ((uint64_t)k >= (1ull << 32)) return set_err(ctx, DSORT_EINVAL, "sample top-k: nranks * k must stay below 2^32");
    if ((n_local && !d_keys) || (k && !d_idx_out)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (ks.bytes == 4)
        return tk::sample_topk<4>(ctx, d_keys, n_local, first, k, ks, key_type, flags, d_keys_out, d_idx_out, stream);
    return tk::sample_topk<8>(ctx, d_keys, n_local, first, k, ks, key_type, flags, d_keys_out, d_idx_out, stream);
}

// Not part of the ABI (like dsort_pairs_leg_ms), for scripts/bench_pairs.py --topk.
// dsort_topk_leg_timing: on != 0 = the select records HIP events around each histogram kernel and
// around the compaction (each costs a few us of idle GPU: off by default).
// dsort_topk_leg_ms: those of the last select: hist_ms[p] for its *passes histogram passes and
// the compaction.  Blocks until that call has finished; DSORT_EINVAL when it recorded none.
int dsort_topk_leg_timing(dsort_ctx *ctx, int on) {
    if (!ctx) return DSORT_EINVAL;
    ctx->tk_timing = on != 0;
    return DSORT_OK;
}

int dsort_topk_leg_ms(dsort_ctx *ctx, double hist_ms[6], int *passes, double *compact_ms) {
    if (!ctx || !hist_ms || !passes || !compact_ms) return DSORT_EINVAL;
    if (!ctx->tk_passes) return set_err(ctx, DSORT_EINVAL, "no timed top-k select on this context");
    const LegClock &c = ctx->tk_clk;
    int rc = c.wait_last(ctx);
    for (int p = 0; p < ctx->tk_passes && !rc; ++p) rc = c.elapsed(ctx, 2 * p, 2 * p + 1, &hist_ms[p]);
    if (!rc) rc = c.elapsed(ctx, tk::EV_COMPACT, tk::EV_COMPACT + 1, compact_ms);
    *passes = ctx->tk_passes;
    return rc;
}

}  // extern "C"
