// dsort_gather.hip -- the distributed record gather (dsort.h, ABI 9): payloads follow their keys
// across ranks.  out[j] = the record at GLOBAL position idx[j], wherever it lives.
//
// Every rank owns a contiguous range of global positions.  The call is a request/reply exchange:
//   0. range table   all-gather of (first, n_src, elem_bytes); the owner table is planned on the
//                    host (dsort_plan_gather_table) and uploaded
//   1. route         a stable P-way partition of this rank's indices by owner into requests,
//                    req[pos(j)] = idx[j] - lo(owner): the owner's local index
//      counts        all-gather of the P + 1 counts (the last: indices nobody owns)
//   2. requests      all-to-all-v of the uint32 requests
//   3. serve         gather_kernel<W> (dsort_gather_dev) on the owner's records
//      replies       the reverse all-to-all-v of the W-byte records
//   4. unroute       dst[j] = reply[pos(j)], pos recomputed by the routing code
//
// Routing is three launches and no global atomic, so the layout is deterministic: owner-major, and
// inside an owner in input order.  A fixed grid of at most MAXWG workgroups, each owning one
// contiguous range of idx cut into tiles of 1024 (a lane takes four consecutive indices: one
// 16-byte load, typed 4-byte aligned like everything of the caller's, dsort_pairs.hip):
//   count    per workgroup, the indices per owner (+ the unowned bin)
//   scan     a workgroup per owner: its per-workgroup bases and total; then the owners' starts
//   place    walks the same range in the same order: an index's rank among those of its owner is
//            (a) inside its wave by a loop over the distinct owners present -- the lanes' match
//            counts through a wave prefix sum, (b) across the four waves of a tile through LDS,
//            (c) across tiles by a running LDS counter that starts at the workgroup's base.
// `place` is one templated kernel with two actions: ROUTE writes the request, UNROUTE reads the
// reply at that position and stores the record -- 4 bytes per index are recomputed instead of
// stored and read back, and the stores to dst are contiguous.  Both hand a wave's 256 positions
// through LDS first, so that each store instruction of the wave covers consecutive elements.
//
// HBM bytes per index at one rank (W = record bytes): count 4, route 4 + 4, requests' own part
// (D2D) 4 + 4, serve 4 + W + W, replies' own part W + W, unroute 4 + W + W: 28 + 6 W in all, of
// which the routing reads idx three times.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "dsort_exch.h"

namespace dsort {
namespace ga {

constexpr int NT = 256;           // threads per workgroup
constexpr int WAVES = NT / 64;
constexpr int TILE = NT * 4;      // indices per tile: four per lane
constexpr unsigned MAXWG = 2048;  // workgroups of a launch, as in dsort_pairs.hip
constexpr int MAXR = 256;         // ranges of the owner table (= ranks of the communicator)
constexpr uint32_t NONE = 0xFFFFFFFFu;

typedef uint32_t u4_a4 __attribute__((ext_vector_type(4), aligned(4)));

// The owner lookup, shared by the kernels and the host restatement (dsort_plan_gather_route): the
// non-empty ranges sorted by start, range i = [lo[i], last[i]] (last inclusive, so that a range
// ending at 2^32 fits 32 bits).  Binary search for the last range that starts at or before g --
// UNSIGNED comparison: positions above 2^31 -- then the check against its end.  -1: nobody owns g.
__host__ __device__ __forceinline__ int owner_slot(const uint32_t *lo, const uint32_t *last, int nr, uint32_t g) {
    int a = 0, b = nr;  // a = the ranges known to start at or before g
    while (a < b) {
        const int m = (a + b) >> 1;
        if (lo[m] <= g)
            a = m + 1;
        else
            b = m;
    }
    if (a == 0) return -1;
    return g <= last[a - 1] ? a - 1 : -1;
}

enum { COUNT = 0, ROUTE = 1, UNROUTE = 2 };

// tab: lo[MAXR] | last[MAXR] | owner[MAXR].  NB = P + 1 bins: owner ranks 0..P-1 and P = unowned.
// Workgroup g owns idx[g * chunk, min(n, (g + 1) * chunk)), chunk a multiple of TILE.
//   COUNT    wgcnt[g * NB + b] = its indices of bin b
//   ROUTE    req[pos(j)] = idx[j] - lo(owner)                 (nothing for an unowned index)
//   UNROUTE  dst[j] = reply[pos(j)], records of W bytes
// with pos(j) = binstart[b] + wgcnt[g * NB + b] (after the scan: the exclusive prefix over g) + the
// number of earlier indices of bin b in the workgroup's range.
template <int MODE, int W>
__global__ void __launch_bounds__(NT) place_kernel(const uint32_t *__restrict__ idx, uint64_t n, uint64_t chunk,
                                                   const uint32_t *__restrict__ tab, int nr, int P,
                                                   uint32_t *__restrict__ wgcnt,
                                                   const uint32_t *__restrict__ binstart,
                                                   uint32_t *__restrict__ req,
                                                   const uint32_t *__restrict__ reply,
                                                   uint32_t *__restrict__ dst) {
    constexpr int D = W / 4;  // dwords per record
    __shared__ uint32_t s_lo[MAXR], s_last[MAXR];
    __shared__ int32_t s_own[MAXR];
    __shared__ uint32_t run[MAXR + 1];          // COUNT: the bin's count; else: the next position of the bin
    __shared__ uint32_t wcnt[WAVES][MAXR + 1];  // a tile's count per wave and bin (zero between tiles)
    __shared__ __attribute__((aligned(16))) uint32_t t_pos[WAVES][256];  // a wave's positions, in input order
    __shared__ __attribute__((aligned(16))) uint32_t t_loc[WAVES][256];  // ROUTE: and its requests
    const int NB = P + 1;
    const uint32_t tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    for (int i = tid; i < nr; i += NT) {
        s_lo[i] = tab[i];
        s_last[i] = tab[MAXR + i];
        s_own[i] = (int32_t)tab[2 * MAXR + i];
    }
    for (int b = tid; b < NB; b += NT) {
        run[b] = MODE == COUNT ? 0u : binstart[b] + wgcnt[(uint64_t)blockIdx.x * NB + b];
        for (int v = 0; v < WAVES; ++v) wcnt[v][b] = 0;
    }
    __syncthreads();
    const uint64_t begin = (uint64_t)blockIdx.x * chunk;
    const uint64_t end = begin + chunk < n ? begin + chunk : n;
    for (uint64_t base = begin; base < end; base += TILE) {
        const uint64_t e0 = base + 4 * tid;
        const bool whole = e0 + 4 <= end;
        uint32_t g[4] = {0, 0, 0, 0};
        if (whole) {
            const u4_a4 v = *reinterpret_cast<const u4_a4 *>(idx + e0);
            g[0] = v.x, g[1] = v.y, g[2] = v.z, g[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (e0 + k < end) g[k] = idx[e0 + k];
        }
        uint32_t bin[4], loc[4], rank[4] = {0, 0, 0, 0};
        uint32_t todo = 0;  // bit k: element k is still to be ranked
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            bin[k] = NONE;
            loc[k] = 0;
            if (e0 + k < end) {
                const int sl = owner_slot(s_lo, s_last, nr, g[k]);
                bin[k] = sl < 0 ? (uint32_t)P : (uint32_t)s_own[sl];
                loc[k] = sl < 0 ? 0u : g[k] - s_lo[sl];
                todo |= 1u << k;
            }
        }
        // (a) inside the wave: one round per distinct bin present.  All 64 lanes stay in the loop
        // (its condition is a ballot), as the DPP prefix sum needs.
        for (;;) {
            uint32_t cand = NONE;
#pragma unroll
            for (int k = 3; k >= 0; --k)
                if (todo & (1u << k)) cand = bin[k];
            const unsigned long long act = __ballot(cand != NONE);
            if (!act) break;
            const int leader = __ffsll((long long)act) - 1;
            const uint32_t b = (uint32_t)__shfl((int)cand, leader);
            uint32_t c = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) c += ((todo >> k) & 1u) & (uint32_t)(bin[k] == b);
            const uint32_t incl = wave_incl_sum(c);
            const uint32_t total = (uint32_t)__shfl((int)incl, 63);
            uint32_t r = incl - c;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (((todo >> k) & 1u) && bin[k] == b) {
                    rank[k] = r++;
                    todo &= ~(1u << k);
                }
            if (lane == 0) {
                if (MODE == COUNT)
                    atomicAdd(&run[b], total);  // (LDS; a sum: the order of the waves does not matter)
                else
                    wcnt[w][b] = total;
            }
        }
        if (MODE == COUNT) continue;
        // (b), (c): the waves before this one in the tile, the tiles before this one
        __syncthreads();
        uint32_t pos[4], mine[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pos[k] = NONE;
            mine[k] = 0;
            if (bin[k] != NONE) {
                uint32_t off = run[bin[k]];
                for (uint32_t v = 0; v < w; ++v) off += wcnt[v][bin[k]];
                // (NONE: nothing to move -- an unowned index; a position past the end cannot happen
                // while idx is the array that was counted)
                if (bin[k] < (uint32_t)P && off + rank[k] < n) pos[k] = off + rank[k];
                if (rank[k] == 0) mine[k] = wcnt[w][bin[k]];  // the first of its bin in the wave
            }
        }
        // The wave's 256 positions (ROUTE: and local indices) go through LDS, so that one store
        // instruction of the wave covers consecutive elements instead of every fourth: lane l then
        // moves element 64 q + l (requests), or the 16 / W records of one 16-byte store.
        *reinterpret_cast<uint4 *>(&t_pos[w][4 * lane]) = make_uint4(pos[0], pos[1], pos[2], pos[3]);
        if (MODE == ROUTE) *reinterpret_cast<uint4 *>(&t_loc[w][4 * lane]) = make_uint4(loc[0], loc[1], loc[2], loc[3]);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (bin[k] != NONE && rank[k] == 0) {
                atomicAdd(&run[bin[k]], mine[k]);
                wcnt[w][bin[k]] = 0;
            }
        // (the next tile reads run[] behind its first barrier, and writes its own rows of wcnt,
        // t_pos and t_loc only)
        if (MODE == ROUTE) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const uint32_t p = t_pos[w][64 * q + lane];
                if (p != NONE) req[p] = t_loc[w][64 * q + lane];
            }
        } else {
            constexpr int E = 16 / W;  // records of one 16-byte store
            const uint64_t wbase = base + 256 * w;
#pragma unroll
            for (int q = 0; q < D; ++q) {
                const uint32_t o = (uint32_t)(q * 64 + lane) * E;
                uint32_t p[E], r[4] = {0, 0, 0, 0};
                __builtin_memcpy(p, &t_pos[w][o], sizeof(p));
#pragma unroll
                for (int e = 0; e < E; ++e)
                    if (p[e] != NONE) __builtin_memcpy(r + e * D, reply + (uint64_t)p[e] * D, W);
                const uint64_t j = wbase + o;
                if (j + E <= end) {
                    u4_a4 v;
                    __builtin_memcpy(&v, r, 16);
                    __builtin_nontemporal_store(v, reinterpret_cast<u4_a4 *>(dst + j * D));
                } else {
#pragma unroll
                    for (int e = 0; e < E; ++e)
                        if (j + e < end) {
#pragma unroll
                            for (int d = 0; d < D; ++d) dst[(j + e) * D + d] = r[e * D + d];
                        }
                }
            }
        }
    }
    if (MODE == COUNT) {
        __syncthreads();
        for (int b = tid; b < NB; b += NT) wgcnt[(uint64_t)blockIdx.x * NB + b] = run[b];
    }
}

// Workgroup b scans bin b: wgcnt[g][b] becomes its exclusive prefix over g, tot[b] the bin's total.
// A thread takes SEG consecutive workgroups' counts (G <= MAXWG = NT * SEG).
constexpr int SEG = MAXWG / NT;
__global__ void __launch_bounds__(NT) scan_kernel(uint32_t *__restrict__ wgcnt, int G, int NB,
                                                  uint64_t *__restrict__ tot) {
    __shared__ uint32_t s_w[WAVES];
    const int b = blockIdx.x;
    const int seg = (G + NT - 1) / NT, g0 = (int)threadIdx.x * seg;
    const uint32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t c[SEG], sum = 0;
#pragma unroll
    for (int i = 0; i < SEG; ++i) {
        c[i] = i < seg && g0 + i < G ? wgcnt[(uint64_t)(g0 + i) * NB + b] : 0u;
        sum += c[i];
    }
    const uint32_t incl = wave_incl_sum(sum);
    if (lane == 63) s_w[w] = incl;
    __syncthreads();
    uint32_t off = incl - sum;
    for (uint32_t v = 0; v < w; ++v) off += s_w[v];
#pragma unroll
    for (int i = 0; i < SEG; ++i)
        if (i < seg && g0 + i < G) {
            wgcnt[(uint64_t)(g0 + i) * NB + b] = off;
            off += c[i];
        }
    if (threadIdx.x == NT - 1) tot[b] = off;  // (the last thread's prefix and its own: everything)
}

// binstart[b] = the totals of the bins before b (one workgroup; NB <= MAXR + 1)
__global__ void __launch_bounds__(NT) starts_kernel(const uint64_t *__restrict__ tot, int NB,
                                                    uint32_t *__restrict__ binstart) {
    __shared__ uint32_t s_tot[MAXR + 1];
    for (int b = threadIdx.x; b < NB; b += NT) s_tot[b] = (uint32_t)tot[b];
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t acc = 0;
        for (int b = 0; b < NB; ++b) {
            binstart[b] = acc;
            acc += s_tot[b];
        }
    }
}

// the grid of the routing kernels over n indices: G workgroups of `chunk` indices each
static void route_grid(uint64_t n, unsigned *G, uint64_t *chunk) {
    const uint64_t tiles = (n + TILE - 1) / TILE;
    const uint64_t g0 = tiles > MAXWG ? MAXWG : (tiles ? tiles : 1);
    const uint64_t per = (tiles + g0 - 1) / g0;  // tiles per workgroup
    *chunk = (per ? per : 1) * TILE;
    *G = (unsigned)((n + *chunk - 1) / *chunk);
}

template <int MODE, int W>
static void launch_place(hipStream_t s, unsigned G, const uint32_t *idx, uint64_t n, uint64_t chunk,
                         const uint32_t *tab, int nr, int P, uint32_t *wgcnt, const uint32_t *binstart, uint32_t *req,
                         const uint32_t *reply, uint32_t *dst) {
    hipLaunchKernelGGL((place_kernel<MODE, W>), dim3(G), dim3(NT), 0, s, idx, n, chunk, tab, nr, P, wgcnt, binstart,
                       req, reply, dst);
}

static int plan_table(int nranks, const uint64_t *first, const uint64_t *count, uint64_t *lo, uint64_t *hi,
                      int32_t *owner, int *nranges) {
    std::vector<int> order;
    for (int r = 0; r < nranks; ++r) {
        if (first[r] > (1ull << 32) || count[r] > (1ull << 32) - first[r]) return DSORT_EINVAL;
        if (count[r]) order.push_back(r);
    }
    std::sort(order.begin(), order.end(), [&](int a, int b) { return first[a] < first[b]; });
    for (size_t i = 0; i < order.size(); ++i) {
        const int r = order[i];
        if (i && first[r] < hi[i - 1]) return DSORT_EINVAL;  // overlaps the range before it
        lo[i] = first[r];
        hi[i] = first[r] + count[r];
        owner[i] = r;
    }
    *nranges = (int)order.size();
    return DSORT_OK;
}

// dsort_sample_gather_dev behind its argument checks.  One order bracket around the whole sequence:
// the arenas are shared by calls that may run on other streams.  One exchange call (dsort_exch.h),
// like the sample sort.
template <int W>
static int sample_gather(dsort_ctx *ctx, const uint32_t *src, size_t n_src, uint64_t first, const uint32_t *idx,
                         size_t n_idx, uint32_t *dst, void *stream) {
    // the gather's four collectives: range table, counts, requests, replies
    ExchCall call(ctx, stream, 4);
    if (call.rc) return call.rc;
    const int P = call.P, me = call.me, NB = P + 1;
    const hipStream_t s = call.s;
    const double deadline = call.deadline;
    if (P > MAXR) {
        call.finished();  // (every rank leaves here)
        return set_err(ctx, DSORT_EINVAL, "gather: more than 256 ranks (the owner table's fixed size)");
    }
    ctx->gat_clk.start(ctx->ev_ok && ctx->opt.stage_timing);  // (the legs' events, for dsort_sample_gather_leg_ms)
    int rc = order_begin(ctx, s);
    if (rc) return rc;

    // 0. the range table
    const uint64_t mine[3] = {first, (uint64_t)n_src, (uint64_t)W};
    std::vector<uint64_t> all((size_t)3 * P);
    rc = allgather_u64(ctx, mine, 3, all.data(), s, deadline, "gather range-table all-gather");
    if (rc) return rc;
    for (int r = 0; r < P; ++r)
        if (all[3 * r + 2] != all[2]) {
            call.finished();  // (every rank sees the same table and leaves here)
            return set_err(ctx, DSORT_EINVAL, "gather: the ranks disagree on elem_bytes (rank 0 passes " +
                                                  std::to_string(all[2]) + ", rank " + std::to_string(r) + " " +
                                                  std::to_string(all[3 * r + 2]) + ")");
        }
    std::vector<uint64_t> f(P), c(P), lo(P), hi(P);
    std::vector<int32_t> own(P);
    int nr = 0;
    for (int r = 0; r < P; ++r) f[r] = all[3 * r], c[r] = all[3 * r + 1];
    if (plan_table(P, f.data(), c.data(), lo.data(), hi.data(), own.data(), &nr)) {
        call.finished();
        return set_err(ctx, DSORT_EINVAL, "gather: the ranks' record ranges overlap or end beyond 2^32");
    }

    // arenas: the table and the routing tables, the requests
    unsigned G = 0;
    uint64_t chunk = TILE;
    if (n_idx) route_grid(n_idx, &G, &chunk);
    const size_t off_cnt = (size_t)3 * MAXR * 4;                                   // G * NB uint32
    const size_t off_bs = off_cnt + (((size_t)(G ? G : 1) * NB * 4 + 7) & ~(size_t)7);  // NB uint32
    const size_t off_tot = off_bs + (((size_t)NB * 4 + 7) & ~(size_t)7);            // NB uint64
    const size_t small_total = off_tot + (size_t)NB * 8;
    rc = ensure(ctx, ctx->gat_small, small_total, "gather routing tables");
    if (rc) return rc;
    rc = ensure_host(ctx, ctx->gat_host, off_cnt + (size_t)(MAXR + 1) * 8);
    if (rc) return rc;
    rc = ensure(ctx, ctx->gat_req, (n_idx ? n_idx : 1) * 4, "gather requests");
    if (rc) return rc;
    char *dsm = ctx->gat_small.as<char>();
    uint32_t *htab = ctx->gat_host.as<uint32_t>();
    uint64_t *htot = reinterpret_cast<uint64_t *>(ctx->gat_host.as<char>() + off_cnt);
    for (int i = 0; i < MAXR; ++i) {
        htab[i] = i < nr ? (uint32_t)lo[i] : 0u;
        htab[MAXR + i] = i < nr ? (uint32_t)(hi[i] - 1) : 0u;
        htab[2 * MAXR + i] = i < nr ? (uint32_t)own[i] : 0u;
    }
    const uint32_t *tab = reinterpret_cast<const uint32_t *>(dsm);
    uint32_t *wgcnt = reinterpret_cast<uint32_t *>(dsm + off_cnt);
    uint32_t *binstart = reinterpret_cast<uint32_t *>(dsm + off_bs);
    uint64_t *dtot = reinterpret_cast<uint64_t *>(dsm + off_tot);
    uint32_t *req = ctx->gat_req.as<uint32_t>();
    DSORT_HIP(ctx, hipMemcpyAsync(dsm, htab, off_cnt, hipMemcpyHostToDevice, s));

    // 1. route: count, scan, starts, place
    ctx->gat_clk.mark(s);
    if (G) {
        launch_place<COUNT, 4>(s, G, idx, n_idx, chunk, tab, nr, P, wgcnt, binstart, nullptr, nullptr, nullptr);
        DSORT_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(scan_kernel, dim3(NB), dim3(NT), 0, s, wgcnt, (int)G, NB, dtot);
    DSORT_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(starts_kernel, dim3(1), dim3(NT), 0, s, dtot, NB, binstart);
    DSORT_HIP(ctx, hipGetLastError());
    if (G) {
        launch_place<ROUTE, 4>(s, G, idx, n_idx, chunk, tab, nr, P, wgcnt, binstart, req, nullptr, nullptr);
        DSORT_HIP(ctx, hipGetLastError());
    }
    ctx->gat_clk.mark(s);
    DSORT_HIP(ctx, hipMemcpyAsync(htot, dtot, (size_t)NB * 8, hipMemcpyDeviceToHost, s));
    rc = exch_wait(ctx, s, true, deadline, "gather routing");
    if (rc) return rc;

    // the counts, with the unowned column: mat[src * NB + owner]
    std::vector<uint64_t> row(htot, htot + NB), mat((size_t)NB * P);
    rc = allgather_u64(ctx, row.data(), (size_t)NB, mat.data(), s, deadline, "gather count all-gather");
    if (rc) return rc;
    for (int r = 0; r < P; ++r)
        if (mat[(size_t)r * NB + P]) {
            call.finished();  // (every rank sees the same matrix and leaves here)
            return set_err(ctx, DSORT_EINVAL, "gather: rank " + std::to_string(r) + " holds " +
                                                  std::to_string(mat[(size_t)r * NB + P]) +
                                                  " indices that no rank owns");
        }
    std::vector<uint64_t> scnt(P), soff(P), rcnt(P), roff(P);
    uint64_t m = 0, sent = 0, so = 0;
    for (int r = 0; r < P; ++r) {
        scnt[r] = mat[(size_t)me * NB + r];
        soff[r] = so;
        so += scnt[r];
        rcnt[r] = mat[(size_t)r * NB + me];
        roff[r] = m;
        m += rcnt[r];
        if (r != me) sent += scnt[r];
    }
    if (so != (uint64_t)n_idx) return set_err(ctx, DSORT_EHIP, "gather: the routing counts do not add up");
    rc = ensure(ctx, ctx->gat_rreq, (m ? m : 1) * 4, "gather requests received");
    if (rc) return rc;
    rc = ensure(ctx, ctx->gat_rep, (m ? m : 1) * (size_t)W, "gather replies");
    if (rc) return rc;
    rc = ensure(ctx, ctx->gat_back, (n_idx ? n_idx : 1) * (size_t)W, "gather records received");
    if (rc) return rc;
    uint32_t *rreq = ctx->gat_rreq.as<uint32_t>();
    uint32_t *rep = ctx->gat_rep.as<uint32_t>();
    uint32_t *back = ctx->gat_back.as<uint32_t>();

    // 2. the requests
    // (requests and records travel as dwords)
    rc = alltoallv(ctx, A2av{req, scnt.data(), soff.data(), n_idx, rreq, rcnt.data(), roff.data(), m, 4, ncclUint32}, s,
                   deadline, "gather request all-to-all", "gather request all-to-all (staging)");
    if (rc) return rc;
    ctx->gat_clk.mark(s);

    // 3. serve them from this rank's records (m > 0: it owns some, so src is not NULL)
    if (m) {
        rc = dsort_gather_dev(ctx, src, rreq, rep, (size_t)m, W, stream);
        if (rc) return rc;
    }
    ctx->gat_clk.mark(s);

    // the replies: the reverse exchange
    rc = alltoallv(ctx, A2av{rep, rcnt.data(), roff.data(), m, back, scnt.data(), soff.data(), n_idx, W, ncclUint32}, s,
                   deadline, "gather reply all-to-all", "gather reply all-to-all (staging)");
    if (rc) return rc;
    call.finished();
    ctx->gat_clk.mark(s);

    // 4. unroute: dst[j] = back[pos(j)]
    if (G) {
        launch_place<UNROUTE, W>(s, G, idx, n_idx, chunk, tab, nr, P, wgcnt, binstart, nullptr, back, dst);
        DSORT_HIP(ctx, hipGetLastError());
    }
    ctx->gat_clk.mark(s);
    if (!call.host_tx) {  // the receives must have landed before the caller reads dst
        rc = exch_wait(ctx, s, true, deadline, "gather reply all-to-all");
        if (rc) return rc;
    }
    if ((rc = order_end(ctx, s))) return rc;
    ctx->stats.gather_sent = (size_t)sent;
    ctx->stats.gather_served = (size_t)m;
    return DSORT_OK;
}

}  // namespace ga
}  // namespace dsort

using namespace dsort;

extern "C" {

int dsort_sample_gather_dev(dsort_ctx *ctx, const void *d_src, size_t n_src, uint64_t first, const uint32_t *d_idx,
                            size_t n_idx, void *d_dst, int elem_bytes, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16)
        return set_err(ctx, DSORT_EINVAL, "gather: elem_bytes must be 4, 8 or 16");
    if (first > (1ull << 32) || (uint64_t)n_src > (1ull << 32) - first)
        return set_err(ctx, DSORT_EINVAL,
                       "gather: first + n_src exceeds 2^32 (a global position must fit 32 bits)");
    if ((uint64_t)n_idx >= (1ull << 32))
        return set_err(ctx, DSORT_EINVAL, "gather: 2^32 or more indices in one call");
    if ((n_src && !d_src) || (n_idx && (!d_idx || !d_dst))) return set_err(ctx, DSORT_EINVAL, "null argument");
    const uint32_t *src = static_cast<const uint32_t *>(d_src);
    uint32_t *dst = static_cast<uint32_t *>(d_dst);
    if (elem_bytes == 4) return ga::sample_gather<4>(ctx, src, n_src, first, d_idx, n_idx, dst, stream);
    if (elem_bytes == 8) return ga::sample_gather<8>(ctx, src, n_src, first, d_idx, n_idx, dst, stream);
    return ga::sample_gather<16>(ctx, src, n_src, first, d_idx, n_idx, dst, stream);
}

int dsort_plan_gather_table(int nranks, const uint64_t first[], const uint64_t count[], uint64_t lo[], uint64_t hi[],
                            int32_t owner[], int *nranges) {
    if (nranks < 1 || !first || !count || !lo || !hi || !owner || !nranges) return DSORT_EINVAL;
    return ga::plan_table(nranks, first, count, lo, hi, owner, nranges);
}

int dsort_plan_gather_route(int nranges, const uint64_t lo[], const uint64_t hi[], const int32_t owner[], int nranks,
                            const uint32_t *idx, size_t n, uint64_t counts[], uint64_t pos[]) {
    if (nranges < 0 || nranks < 1 || !counts || (nranges && (!lo || !hi || !owner)) || (n && (!idx || !pos)))
        return DSORT_EINVAL;
    std::vector<uint32_t> l32((size_t)nranges + 1), last((size_t)nranges + 1);
    for (int i = 0; i < nranges; ++i) {
        if (hi[i] <= lo[i] || hi[i] > (1ull << 32) || (i && lo[i] < hi[i - 1]) || owner[i] < 0 || owner[i] >= nranks)
            return DSORT_EINVAL;
        l32[i] = (uint32_t)lo[i];
        last[i] = (uint32_t)(hi[i] - 1);
    }
    auto bin_of = [&](uint32_t g) {
        const int sl = ga::owner_slot(l32.data(), last.data(), nranges, g);
        return sl < 0 ? nranks : (int)owner[sl];
    };
    for (int b = 0; b <= nranks; ++b) counts[b] = 0;
    for (size_t j = 0; j < n; ++j) ++counts[bin_of(idx[j])];
    std::vector<uint64_t> next((size_t)nranks + 1);
    uint64_t acc = 0;
    for (int b = 0; b <= nranks; ++b) {
        next[b] = acc;
        acc += counts[b];
    }
    for (size_t j = 0; j < n; ++j) pos[j] = next[bin_of(idx[j])]++;
    return DSORT_OK;
}

// Not part of the ABI (like dsort_pairs_leg_ms): device time of the last gather's five legs -- route
// (count, scan, place) | request exchange (the count all-gather and its host wait included) | serve
// | reply exchange | unroute -- from HIP events between them, for scripts/bench_pairs.py.  Blocks
// until that call has finished; DSORT_EINVAL when it recorded none.
int dsort_sample_gather_leg_ms(dsort_ctx *ctx, double ms[5]) {
    if (!ctx || !ms) return DSORT_EINVAL;
    const LegClock &c = ctx->gat_clk;
    if (!c.complete(6)) return set_err(ctx, DSORT_EINVAL, "no timed gather on this context");
    int rc = c.wait_last(ctx);
    for (int i = 0; i < 5 && !rc; ++i) rc = c.elapsed(ctx, i, i + 1, &ms[i]);
    return rc;
}

}  // extern "C"
