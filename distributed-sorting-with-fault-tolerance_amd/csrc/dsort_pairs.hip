// dsort_pairs.hip -- stable argsort and key-value sort of int32 keys, and the record gather.
//
// An int32 key and a 32-bit value fit in one int64, (int64)key << 32 | (uint32)value, and signed
// int64 order on that word is signed order on the key, then unsigned order on the value.  So a
// pair sort is: pack into an arena of the context, sort the arena with the int64 sort
// (sort_device<int64_t>, untouched: every packed word of an argsort is distinct, which is the
// input the int64 sort has the least to say about), unpack.  With value = input position the
// order is the stable argsort.  Records wider than 32 bits follow their key by an argsort and a
// gather (gather_kernel).  Across ranks the packed words go through the int64 sample sort instead
// (sample_pairs_sort, ABI 8), the argsort's value being the global position.
//
// The three kernels are streaming: grid-stride, 16 bytes per store and, but for the pack's keys
// and values, per load; outputs as non-temporal stores.  The caller's pointers are only
// element-aligned (a tensor view that starts at element 1), and the keys, the values and the two
// outputs can each sit at another phase, so no head could align them all: their vector accesses
// are typed 4-byte aligned instead (a multi-dword global access needs dword alignment on gfx950,
// and a wave's 1 KiB then touches nine 128-byte lines instead of eight).  Vector groups count from
// element 0, where the arena is 16-byte aligned, and the elements behind the last whole group
// (pack: n % 256, unpack: n % 4, gather: n % (16 / record bytes)) go one by one.
//
// HBM bytes per element: pack reads 4 (argsort) or 8 (pairs) and writes 8; unpack reads 8 and
// writes 4 per wanted output; on top of the int64 sort's own traffic.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "dsort_internal.h"
#include "dsort_keycodec.h"

namespace dsort {
namespace pr {

constexpr int NT = 256;          // threads per workgroup
constexpr unsigned MAXWG = 2048; // workgroups of a launch (256 CUs x 8), the rest by grid stride

// 16 bytes of caller memory: four dwords at dword alignment
typedef uint32_t u4_a4 __attribute__((ext_vector_type(4), aligned(4)));
// 16 bytes of the arena
typedef uint64_t l2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint64_t pack1(int32_t k, uint32_t v) {
    return ((uint64_t)(uint32_t)k << 32) | (uint64_t)v;
}

// 8 bytes of caller memory
typedef uint32_t u2_a4 __attribute__((ext_vector_type(2), aligned(4)));

// packed[i] = keys[i] : (ARG ? (uint32_t)(base + i) : vals[i]); base is the global position of
// keys[0] in a sample argsort, 0 in a local one.  A wave takes 256 elements, lane l the pairs at 2l
// and at 128 + 2l: each of its two 16-byte stores is then contiguous over the wave (1 KiB), at the
// price of 8-byte loads.  (Four consecutive elements per lane -- one 16-byte key load, two stores
// 32 bytes apart, so that every store instruction fills half of each line it touches -- measured
// 3.73 against 2.60 ms at 2^30 keys, 0.84 against 0.61 ms at 2^28, 2 of 2 alternating runs;
// DESIGN.md 3.9.)
//
// KC is the key codec (dsort_keycodec.h): the caller's keys are encoded as they are read.  The
// body is shared by two kernels so that the int32 entry points keep launching the kernel they
// always have (the identity codec: the same name, the same machine code) and the typed ones
// (dsort_keys.hip) a kernel per codec.
// (The pointers are the kernels' __restrict__ parameters.)
template <bool ARG, int KC>
__device__ __forceinline__ void pairs_pack_body(const int32_t *keys, const uint32_t *vals, uint64_t *packed,
                                                uint64_t n, uint32_t base) {
    using C = kc::Codec<KC>;
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        const u2_a4 k0 = *reinterpret_cast<const u2_a4 *>(keys + e0);
        const u2_a4 k1 = *reinterpret_cast<const u2_a4 *>(keys + e1);
        u2_a4 v0, v1;
        if (ARG) {
            v0 = u2_a4{base + (uint32_t)e0, base + (uint32_t)e0 + 1};
            v1 = u2_a4{base + (uint32_t)e1, base + (uint32_t)e1 + 1};
        } else {
            v0 = *reinterpret_cast<const u2_a4 *>(vals + e0);
            v1 = *reinterpret_cast<const u2_a4 *>(vals + e1);
        }
        __builtin_nontemporal_store(
            l2{pack1((int32_t)C::enc(k0.x), v0.x), pack1((int32_t)C::enc(k0.y), v0.y)},
            reinterpret_cast<l2 *>(packed + e0));
        __builtin_nontemporal_store(
            l2{pack1((int32_t)C::enc(k1.x), v1.x), pack1((int32_t)C::enc(k1.y), v1.y)},
            reinterpret_cast<l2 *>(packed + e1));
    }
    const uint64_t i = (chunks << 8) + t;  // the n % 256 last elements, one each
    if (i < n) packed[i] = pack1((int32_t)C::enc((uint32_t)keys[i]), ARG ? base + (uint32_t)i : vals[i]);
}

template <bool ARG>
__global__ void __launch_bounds__(NT) pairs_pack_kernel(const int32_t *__restrict__ keys,
                                                        const uint32_t *__restrict__ vals,
                                                        uint64_t *__restrict__ packed, uint64_t n,
                                                        uint32_t base) {
    pairs_pack_body<ARG, 0>(keys, vals, packed, n, base);
}

template <bool ARG, int KC>
__global__ void __launch_bounds__(NT) pairs_pack_keys_kernel(const int32_t *__restrict__ keys,
                                                             const uint32_t *__restrict__ vals,
                                                             uint64_t *__restrict__ packed, uint64_t n,
                                                             uint32_t base) {
    pairs_pack_body<ARG, KC>(keys, vals, packed, n, base);
}

// keys_out[i] = high word (decoded by the codec KC), vals_out[i] = low word of packed[i]; a NULL
// output is not written
template <int KC>
__global__ void __launch_bounds__(NT) pairs_unpack_keys_kernel(const uint64_t *__restrict__ packed,
                                                               int32_t *__restrict__ keys_out,
                                                               uint32_t *__restrict__ vals_out, uint64_t n) {
    using C = kc::Codec<KC>;
    const uint64_t groups = n >> 2;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    for (uint64_t g = t; g < groups; g += stride) {
        const uint64_t i = g << 2;
        const l2 *src = reinterpret_cast<const l2 *>(packed + i);
        const l2 a = src[0], b = src[1];
        if (keys_out) {
            const u4_a4 k = {C::dec((uint32_t)(a.x >> 32)), C::dec((uint32_t)(a.y >> 32)),
                             C::dec((uint32_t)(b.x >> 32)), C::dec((uint32_t)(b.y >> 32))};
            __builtin_nontemporal_store(k, reinterpret_cast<u4_a4 *>(keys_out + i));
        }
        if (vals_out) {
            const u4_a4 v = {(uint32_t)a.x, (uint32_t)a.y, (uint32_t)b.x, (uint32_t)b.y};
            __builtin_nontemporal_store(v, reinterpret_cast<u4_a4 *>(vals_out + i));
        }
    }
    const uint64_t i = (groups << 2) + t;
    if (i < n) {
        const uint64_t p = packed[i];
        if (keys_out) keys_out[i] = (int32_t)C::dec((uint32_t)(p >> 32));
        if (vals_out) vals_out[i] = (uint32_t)p;
    }
}

// The same without a codec: the kernel of the int32 entry points, kept word for word.  (As one body
// shared with the kernel above, its instructions came out of the compiler in a slightly different
// order; scripts/asm_digest.py compares it with the parent's.)
__global__ void __launch_bounds__(NT) pairs_unpack_kernel(const uint64_t *__restrict__ packed,
                                                          int32_t *__restrict__ keys_out,
                                                          uint32_t *__restrict__ vals_out, uint64_t n) {
    const uint64_t groups = n >> 2;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    for (uint64_t g = t; g < groups; g += stride) {
        const uint64_t i = g << 2;
        const l2 *src = reinterpret_cast<const l2 *>(packed + i);
        const l2 a = src[0], b = src[1];
        if (keys_out) {
            const u4_a4 k = {(uint32_t)(a.x >> 32), (uint32_t)(a.y >> 32), (uint32_t)(b.x >> 32),
                             (uint32_t)(b.y >> 32)};
            __builtin_nontemporal_store(k, reinterpret_cast<u4_a4 *>(keys_out + i));
        }
        if (vals_out) {
            const u4_a4 v = {(uint32_t)a.x, (uint32_t)a.y, (uint32_t)b.x, (uint32_t)b.y};
            __builtin_nontemporal_store(v, reinterpret_cast<u4_a4 *>(vals_out + i));
        }
    }
    const uint64_t i = (groups << 2) + t;
    if (i < n) {
        const uint64_t p = packed[i];
        if (keys_out) keys_out[i] = (int32_t)(uint32_t)(p >> 32);
        if (vals_out) vals_out[i] = (uint32_t)p;
    }
}


// dst[i] = src[idx[i]] for records of W bytes (4, 8, 16): a lane takes the 16 / W records of one
// 16-byte store.  Records are dword-aligned like everything of the caller's.
template <int W>
__global__ void __launch_bounds__(NT) gather_kernel(const uint32_t *__restrict__ src,
                                                    const uint32_t *__restrict__ idx,
                                                    uint32_t *__restrict__ dst, uint64_t n) {
    constexpr int E = 16 / W;  // records per lane and step
    constexpr int D = W / 4;   // dwords per record
    const uint64_t groups = n / E;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    for (uint64_t g = t; g < groups; g += stride) {
        const uint64_t i = g * E;
        uint32_t j[E];
        __builtin_memcpy(j, idx + i, sizeof(j));
        uint32_t r[4];
#pragma unroll
        for (int e = 0; e < E; ++e) __builtin_memcpy(r + e * D, src + (uint64_t)j[e] * D, W);
        u4_a4 v;
        __builtin_memcpy(&v, r, 16);
        __builtin_nontemporal_store(v, reinterpret_cast<u4_a4 *>(dst + i * D));
    }
    const uint64_t i = groups * E + t;  // the n % E last records (none at W = 16)
    if (i < n) {
        const uint64_t j = idx[i];
#pragma unroll
        for (int d = 0; d < D; ++d) dst[i * D + d] = src[j * D + d];
    }
}

static unsigned grid_for(uint64_t lanes) {
    const uint64_t g = (lanes + NT - 1) / NT;
    return (unsigned)(g > MAXWG ? MAXWG : (g ? g : 1));
}

// The launches of the typed kernels, defined at the end of the file: the int32 entry points'
// kernels then come out of the compiler in the order, and so under the labels, they always had
// (scripts/asm_digest.py compares them with the parent's).
static void launch_pack_keys(int kc, unsigned grid, hipStream_t s, const int32_t *keys_in, const uint32_t *vals_in,
                             uint64_t *packed, uint64_t n, uint32_t base);
static void launch_unpack_keys(int kc, unsigned grid, hipStream_t s, const uint64_t *packed, int32_t *keys_out,
                               uint32_t *vals_out, uint64_t n);

static int pack(dsort_ctx *ctx, const int32_t *keys_in, const uint32_t *vals_in, uint64_t *packed, size_t n,
                uint32_t base, hipStream_t s, int kc = 0) {
    const unsigned grid = grid_for((n + 3) / 4);
    if (kc)
        launch_pack_keys(kc, grid, s, keys_in, vals_in, packed, (uint64_t)n, base);
    else if (vals_in)
        hipLaunchKernelGGL((pairs_pack_kernel<false>), dim3(grid), dim3(NT), 0, s, keys_in, vals_in, packed,
                           (uint64_t)n, base);
    else
        hipLaunchKernelGGL((pairs_pack_kernel<true>), dim3(grid), dim3(NT), 0, s, keys_in, vals_in, packed,
                           (uint64_t)n, base);
    DSORT_HIP(ctx, hipGetLastError());
    return DSORT_OK;
}

// Sorts (keys_in[i], vals_in ? vals_in[i] : i) by key, then by value as unsigned 32-bit, into
// keys_out / vals_out (either may be NULL: not wanted; either may be its input: the pack has
// consumed the inputs before the unpack writes).  Asynchronous on s.  kc: the key codec
// (dsort_keycodec.h; 0 = int32 ascending, the kernels of the int32 entry points), under which
// "key" is the typed key and its order the codec's.
int pairs_sort(dsort_ctx *ctx, const int32_t *keys_in, const uint32_t *vals_in, int32_t *keys_out,
               uint32_t *vals_out, size_t n, hipStream_t s, int kc) {
    if (n == 0) {
        ctx->stats = fresh_stats();
        ctx->ev_mask = 0;
        ctx->kev_used = 0;
        return DSORT_OK;
    }
    if (n > SIZE_MAX / 8) return set_err(ctx, DSORT_EINVAL, "pair sort: n * 8 bytes overflow size_t");
    // The arena is shared by calls that may run on different streams, and this call touches it
    // before and after the sort's own bracket: one bracket around all three legs.
    int rc = order_begin(ctx, s);
    if (rc) return rc;
    rc = ensure(ctx, ctx->pairs, n * 8, "pair arena");
    if (rc) return rc;
    uint64_t *packed = ctx->pairs.as<uint64_t>();
    // the legs' events (pack | sort | unpack), for dsort_pairs_leg_ms below
    ctx->pairs_clk.start(ctx->ev_ok && ctx->opt.stage_timing);
    ctx->pairs_clk.mark(s);
    const unsigned grid = grid_for((n + 3) / 4);
    rc = pack(ctx, keys_in, vals_in, packed, n, 0, s, kc);
    if (rc) return rc;
    ctx->pairs_clk.mark(s);
    // DSORT_OPT_KILL_AFTER_STAGE fires inside, as for any int64 sort of n keys; DSORT_ESTAGE (the
    // stage was never reached) leaves a valid output, so the unpack still runs
    const int src = sort_device<int64_t>(ctx, reinterpret_cast<int64_t *>(packed), reinterpret_cast<int64_t *>(packed),
                                         n, s, true);
    if (src && src != DSORT_ESTAGE) return src;
    ctx->pairs_clk.mark(s);
    if (kc)
        launch_unpack_keys(kc, grid, s, packed, keys_out, vals_out, (uint64_t)n);
    else
        hipLaunchKernelGGL(pairs_unpack_kernel, dim3(grid), dim3(NT), 0, s, packed, keys_out, vals_out, (uint64_t)n);
    DSORT_HIP(ctx, hipGetLastError());
    ctx->pairs_clk.mark(s);
    rc = order_end(ctx, s);
    return rc ? rc : src;
}

// The pair sort across ranks: the packed words go through the int64 sample sort (both exchange
// paths, both transports, untouched) and this rank's slice is unpacked into two arenas of the
// context.  The words of an argsort are all distinct -- base = the global position of keys_in[0] --
// so a heavy key splits between ranks by position and the global order is stable.
//
// The slice the sample sort returns starts at the base of its output arena on both exchange paths
// (ctx->recv2, a hipMalloc of its own: 256-byte aligned), which is what the unpack's 16-byte loads
// need; checked below, since that is the sample sort's business and may change.
//
// The pair arena is the sample sort's input: read on s, and by the comm stream of the RCCL bucket
// exchange, which starts behind an event of s and which the sample sort has waited for when it
// returns 0.  One order bracket around the three legs, as in pairs_sort.  The sample sort takes the
// comm mutex itself (not recursive): nothing here holds it.
//
// A rank without keys (n == 0) packs nothing and joins every collective of the sample sort.
static int sample_pairs_sort(dsort_ctx *ctx, const int32_t *keys_in, const uint32_t *vals_in, uint32_t base, size_t n,
                             int32_t **keys_out, uint32_t **vals_out, size_t *n_out, void *stream) {
    if (n > SIZE_MAX / 8) return set_err(ctx, DSORT_EINVAL, "pair sample sort: n * 8 bytes overflow size_t");
    hipStream_t s = pick_stream(ctx, stream);
    int rc = order_begin(ctx, s);
    if (rc) return rc;
    rc = ensure(ctx, ctx->pairs, (n ? n : 1) * 8, "pair arena");
    if (rc) return rc;
    uint64_t *packed = ctx->pairs.as<uint64_t>();
    // the legs' events (pack | sort | unpack), for dsort_pairs_leg_ms below
    ctx->pairs_clk.start(ctx->ev_ok && ctx->opt.stage_timing);
    ctx->pairs_clk.mark(s);
    if (n && (rc = pack(ctx, keys_in, vals_in, packed, n, base, s))) return rc;
    ctx->pairs_clk.mark(s);
    int64_t *slice = nullptr;
    size_t m = 0;
    rc = sample_sort_packed(ctx, reinterpret_cast<const int64_t *>(packed), n, &slice, &m, stream);
    if (rc) return rc;
    if (m && (reinterpret_cast<uintptr_t>(slice) & 15))
        return set_err(ctx, DSORT_EHIP, "pair sample sort: the sample sort's slice is not 16-byte aligned");
    if (keys_out) {
        rc = ensure(ctx, ctx->spairs_k, (m ? m : 1) * 4, "pair sample sort keys");
        if (rc) return rc;
    }
    rc = ensure(ctx, ctx->spairs_v, (m ? m : 1) * 4, "pair sample sort values");
    if (rc) return rc;
    int32_t *ko = keys_out ? ctx->spairs_k.as<int32_t>() : nullptr;
    uint32_t *vo = ctx->spairs_v.as<uint32_t>();
    ctx->pairs_clk.mark(s);
    if (m) {
        hipLaunchKernelGGL(pairs_unpack_kernel, dim3(grid_for((m + 3) / 4)), dim3(NT), 0, s,
                           reinterpret_cast<const uint64_t *>(slice), ko, vo, (uint64_t)m);
        DSORT_HIP(ctx, hipGetLastError());
    }
    ctx->pairs_clk.mark(s);
    if ((rc = order_end(ctx, s))) return rc;
    if (keys_out) *keys_out = ko;
    *vals_out = vo;
    *n_out = m;
    return DSORT_OK;
}

}  // namespace pr
}  // namespace dsort

using namespace dsort;

extern "C" {

int dsort_argsort_dev_i32(dsort_ctx *ctx, const int32_t *d_keys, int32_t *d_keys_out, uint32_t *d_idx_out, size_t n,
                          void *stream) {
    if (!ctx) return DSORT_EINVAL;
    if ((uint64_t)n > (1ull << 32))
        return set_err(ctx, DSORT_EINVAL, "argsort: more than 2^32 keys (a position must fit 32 bits)");
    if (n && (!d_keys || !d_idx_out)) return set_err(ctx, DSORT_EINVAL, "null argument");
    return pr::pairs_sort(ctx, d_keys, nullptr, d_keys_out, d_idx_out, n, pick_stream(ctx, stream));
}

int dsort_sort_pairs_dev_i32(dsort_ctx *ctx, const int32_t *d_keys_in, const uint32_t *d_vals_in, int32_t *d_keys_out,
                             uint32_t *d_vals_out, size_t n, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    if (n && (!d_keys_in || !d_vals_in || !d_vals_out)) return set_err(ctx, DSORT_EINVAL, "null argument");
    return pr::pairs_sort(ctx, d_keys_in, d_vals_in, d_keys_out, d_vals_out, n, pick_stream(ctx, stream));
}

int dsort_sample_argsort_dev_i32(dsort_ctx *ctx, const int32_t *d_keys, size_t n_local, uint64_t first,
                                 int32_t **d_keys_out, uint32_t **d_idx_out, size_t *n_out, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    if (first > (1ull << 32) || (uint64_t)n_local > (1ull << 32) - first)
        return set_err(ctx, DSORT_EINVAL,
                       "sample argsort: first + n_local exceeds 2^32 (a global position must fit 32 bits)");
    if (!d_idx_out || !n_out || (n_local && !d_keys)) return set_err(ctx, DSORT_EINVAL, "null argument");
    return pr::sample_pairs_sort(ctx, d_keys, nullptr, (uint32_t)first, n_local, d_keys_out, d_idx_out, n_out, stream);
}

int dsort_sample_sort_pairs_dev_i32(dsort_ctx *ctx, const int32_t *d_keys, const uint32_t *d_vals, size_t n_local,
                                    int32_t **d_keys_out, uint32_t **d_vals_out, size_t *n_out, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    if (!d_vals_out || !n_out || (n_local && (!d_keys || !d_vals))) return set_err(ctx, DSORT_EINVAL, "null argument");
    return pr::sample_pairs_sort(ctx, d_keys, d_vals, 0, n_local, d_keys_out, d_vals_out, n_out, stream);
}

int dsort_gather_dev(dsort_ctx *ctx, const void *d_src, const uint32_t *d_idx, void *d_dst, size_t n, int elem_bytes,
                     void *stream) {
    if (!ctx) return DSORT_EINVAL;
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16)
        return set_err(ctx, DSORT_EINVAL, "gather: elem_bytes must be 4, 8 or 16");
    if (n == 0) return DSORT_OK;
    if (!d_src || !d_idx || !d_dst) return set_err(ctx, DSORT_EINVAL, "null argument");
    hipStream_t s = pick_stream(ctx, stream);
    const uint32_t *src = static_cast<const uint32_t *>(d_src);
    uint32_t *dst = static_cast<uint32_t *>(d_dst);
    const unsigned grid = pr::grid_for(((uint64_t)n * elem_bytes + 15) / 16);
    if (elem_bytes == 4)
        hipLaunchKernelGGL((pr::gather_kernel<4>), dim3(grid), dim3(pr::NT), 0, s, src, d_idx, dst, (uint64_t)n);
    else if (elem_bytes == 8)
        hipLaunchKernelGGL((pr::gather_kernel<8>), dim3(grid), dim3(pr::NT), 0, s, src, d_idx, dst, (uint64_t)n);
    else
        hipLaunchKernelGGL((pr::gather_kernel<16>), dim3(grid), dim3(pr::NT), 0, s, src, d_idx, dst, (uint64_t)n);
    DSORT_HIP(ctx, hipGetLastError());
    return DSORT_OK;
}

int dsort_argsort_i32(dsort_ctx *ctx, const int32_t *keys, int32_t *keys_out, uint32_t *idx, size_t n) {
    if (!ctx) return DSORT_EINVAL;
    if ((uint64_t)n > (1ull << 32))
        return set_err(ctx, DSORT_EINVAL, "argsort: more than 2^32 keys (a position must fit 32 bits)");
    if (n && (!keys || !idx)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (n == 0) return DSORT_OK;
    int rc = ensure(ctx, ctx->io, n * 4, "staging");
    if (rc) return rc;
    rc = ensure(ctx, ctx->io2, n * 4, "staging 2");
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    int32_t *dk = ctx->io.as<int32_t>();
    uint32_t *di = ctx->io2.as<uint32_t>();
    DSORT_HIP(ctx, hipMemcpyAsync(dk, keys, n * 4, hipMemcpyHostToDevice, s));
    const int src = pr::pairs_sort(ctx, dk, nullptr, keys_out ? dk : nullptr, di, n, s);
    if (src && src != DSORT_ESTAGE) return src;
    if (keys_out) DSORT_HIP(ctx, hipMemcpyAsync(keys_out, dk, n * 4, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipMemcpyAsync(idx, di, n * 4, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipStreamSynchronize(s));
    return src;
}

// Not part of the ABI (like dsort_debug_stamps): device time of the last pair sort's three legs
// -- pack, int64 sort (a pair sample sort: the whole sample sort, its host waits included), unpack
// -- from HIP events between them, for scripts/bench_pairs.py.
// Blocks until that call has finished; DSORT_EINVAL when it recorded none (no pair sort yet, or
// DSORT_OPT_STAGE_TIMING off).
int dsort_pairs_leg_ms(dsort_ctx *ctx, double ms[3]) {
    if (!ctx || !ms) return DSORT_EINVAL;
    const LegClock &c = ctx->pairs_clk;
    if (!c.complete(4)) return set_err(ctx, DSORT_EINVAL, "no timed pair sort on this context");
    int rc = c.wait_last(ctx);
    for (int i = 0; i < 3 && !rc; ++i) rc = c.elapsed(ctx, i, i + 1, &ms[i]);
    return rc;
}

}  // extern "C"

namespace dsort {
namespace pr {

static void launch_pack_keys(int kc, unsigned grid, hipStream_t s, const int32_t *keys_in, const uint32_t *vals_in,
                             uint64_t *packed, uint64_t n, uint32_t base) {
    if (vals_in) {
        DSORT_KC_SWITCH(kc, hipLaunchKernelGGL((pairs_pack_keys_kernel<false, KC_>), dim3(grid), dim3(NT), 0, s,
                                               keys_in, vals_in, packed, n, base));
    } else {
        DSORT_KC_SWITCH(kc, hipLaunchKernelGGL((pairs_pack_keys_kernel<true, KC_>), dim3(grid), dim3(NT), 0, s,
                                               keys_in, vals_in, packed, n, base));
    }
}

static void launch_unpack_keys(int kc, unsigned grid, hipStream_t s, const uint64_t *packed, int32_t *keys_out,
                               uint32_t *vals_out, uint64_t n) {
    DSORT_KC_SWITCH(kc, hipLaunchKernelGGL((pairs_unpack_keys_kernel<KC_>), dim3(grid), dim3(NT), 0, s, packed,
                                           keys_out, vals_out, n));
}

int unpack_words(dsort_ctx *ctx, const uint64_t *packed, int32_t *keys_out, uint32_t *vals_out, size_t n,
                 hipStream_t s, int kc) {
    if (n == 0) return DSORT_OK;
    const unsigned grid = grid_for((n + 3) / 4);
    if (kc)
        launch_unpack_keys(kc, grid, s, packed, keys_out, vals_out, (uint64_t)n);
    else
        hipLaunchKernelGGL(pairs_unpack_kernel, dim3(grid), dim3(NT), 0, s, packed, keys_out, vals_out, (uint64_t)n);
    DSORT_HIP(ctx, hipGetLastError());
    return DSORT_OK;
}

}  // namespace pr
}  // namespace dsort
