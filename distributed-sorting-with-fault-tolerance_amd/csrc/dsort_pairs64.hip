// dsort_pairs64.hip -- stable argsort and record sort of int64 keys (dsort.h, ABI 10).
//
// No 128-bit composite: a position needs only b = ceil(log2 n) bits of a 64-bit word, which leaves
// room for the key in two cases (plan_argsort64, the rule dsort_plan_argsort_i64 exports).
//
//   narrow, one pass   max - min of the keys fits the other 64 - b bits: one int64 sort of
//                      u = (key - min) << b | position, handed to the sort as (int64)(u ^ 1 << 63)
//                      so that its signed order is the unsigned order of u.
//   wide, two passes   any other keys: two stable passes, least significant half first.
//                      1. A[i] = (lo32(key) ^ 0x80000000) : i, sorted -- the low halves as unsigned;
//                      2. B[j] = hi32(d_keys[p]) : j with p = low word of A[j], sorted -- the high
//                         halves as signed, ties in the order of pass 1;
//                      3. r -> j = low word of B[r], (lo, p) = A[j]: idx_out[r] = p and
//                         keys_out[r] = hi32 : lo.
//
// Both run sort_device<int64_t> untouched on words that are all distinct, as dsort_pairs.hip does.
// The kernels here are the work around it: a min/max reduction (two launches, no atomics), the pack
// and unpack of the narrow word, and the wide path's pack, regroup and final kernels, the last two
// with one random 8-byte read per element and four of them in flight per lane.
//
// Access shapes as in dsort_pairs.hip: a wave takes 256 elements, lane l those at 2l, 2l + 1 and
// 128 + 2l, 128 + 2l + 1, so every 16-byte load and store of 8-byte elements is contiguous over
// the wave (1 KiB) and the indices go out as two 8-byte stores of 512 contiguous bytes.  Outputs
// are non-temporal stores.  The caller's pointers are typed at their element alignment (keys 8,
// indices 4 bytes: a tensor view at element 1); groups count from element 0, where the arenas are
// 16-byte aligned, and the n % 256 last elements go one by one.
//
// HBM bytes per element: min/max reads 8; the narrow pack reads 8 and writes 8, the
// unpack reads 8 and writes 4 + 8 (keys wanted); the wide pack reads 8 and writes 8, the regroup
// reads 8 + a random 8 and writes 8, the final kernel reads 8 + a random 8 and writes 4 + 8.
//
// Across ranks (dsort_sample_argsort_dev_i64; the algorithm: dsort.h) the same words, with global
// positions, go through the int64 sample sort, and the wide path's two random reads become
// distributed gathers (dsort_gather.hip) of the keys and of the first pass's words.  Its kernels
// stream: the split of a slice into a saved copy and its low words reads 8 and writes 8 + 4 (4
// without the copy), the regroup reads 8 and writes 8, the final kernel reads 8 + 8 and writes 4 + 8.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>
#include <vector>

#include "dsort_exch.h"
#include "dsort_internal.h"
#include "dsort_keycodec.h"

namespace dsort {
namespace p64 {

constexpr int NT = 256;          // threads per workgroup
constexpr unsigned MAXWG = 2048; // workgroups of a launch (256 CUs x 8), the rest by grid stride

// 16 bytes of the caller's keys: two int64 at 8-byte alignment
typedef uint64_t k2_a8 __attribute__((ext_vector_type(2), aligned(8)));
// 8 bytes of the caller's indices: two dwords at dword alignment
typedef uint32_t u2_a4 __attribute__((ext_vector_type(2), aligned(4)));
// 16 bytes of an arena
typedef uint64_t l2 __attribute__((ext_vector_type(2)));

constexpr uint64_t SIGN = 1ull << 63;
constexpr uint32_t BIAS = 0x80000000u;

__device__ __forceinline__ uint64_t word(uint32_t hi, uint32_t lo) { return ((uint64_t)hi << 32) | lo; }

// ------------------------------------------------------------------ min / max ------------
__device__ __forceinline__ void wave_minmax(int64_t &lo, int64_t &hi) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        const int64_t a = __shfl_xor((long long)lo, d, 64), b = __shfl_xor((long long)hi, d, 64);
        lo = a < lo ? a : lo;
        hi = b > hi ? b : hi;
    }
}

// the workgroup's (min, max) from every lane's, valid in thread 0
__device__ __forceinline__ void block_minmax(int64_t &lo, int64_t &hi) {
    __shared__ int64_t sh[2 * (NT / 64)];
    wave_minmax(lo, hi);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        sh[2 * w] = lo;
        sh[2 * w + 1] = hi;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 1; i < NT / 64; ++i) {
            lo = sh[2 * i] < lo ? sh[2 * i] : lo;
            hi = sh[2 * i + 1] > hi ? sh[2 * i + 1] : hi;
        }
    }
}

// Every kernel below that reads the caller's keys or writes them back exists twice: the one the
// int64 entry points have always launched, under its name and with its machine code, and a
// *_keys_kernel that takes the key codec KC (dsort_keycodec.h) as a template parameter, for the typed
// entry points (dsort_keys.hip): keys are encoded as they are read and decoded as they are
// written, and everything in between works on the encoded words.  regroup64 and final64 are one
// body behind both kernels (the identity codec compiles to the old code); minmax, pack64 and
// unpack64 keep the old kernel's text beside the templated one.

// part[2 g], part[2 g + 1] = min, max of the (encoded) keys workgroup g saw (grid-stride, 16-byte
// loads, two in flight per lane)
template <int KC>
__global__ void __launch_bounds__(NT) minmax_keys_kernel(const int64_t *__restrict__ keys, uint64_t n,
                                                         int64_t *__restrict__ part) {
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    const uint64_t groups = n >> 1;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    auto take = [&](uint64_t v) {
        const int64_t k = (int64_t)kc::Codec<KC>::enc(v);
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    };
    uint64_t g = t;
    for (; g + stride < groups; g += 2 * stride) {
        const k2_a8 a = *reinterpret_cast<const k2_a8 *>(keys + 2 * g);
        const k2_a8 b = *reinterpret_cast<const k2_a8 *>(keys + 2 * (g + stride));
        take(a.x), take(a.y), take(b.x), take(b.y);
    }
    if (g < groups) {
        const k2_a8 a = *reinterpret_cast<const k2_a8 *>(keys + 2 * g);
        take(a.x), take(a.y);
    }
    if (t == 0 && (n & 1)) take((uint64_t)keys[n - 1]);
    block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = lo;
        part[2 * blockIdx.x + 1] = hi;
    }
}
// The same without a codec: the kernel of the int64 entry points, kept word for word.  (As one body
// shared with the kernel above, its instructions came out of the compiler in a slightly different
// order; scripts/asm_digest.py compares it with the parent's.)
__global__ void __launch_bounds__(NT) minmax_kernel(const int64_t *__restrict__ keys, uint64_t n,
                                                    int64_t *__restrict__ part) {
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    const uint64_t groups = n >> 1;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    auto take = [&](uint64_t v) {
        const int64_t k = (int64_t)v;
        lo = k < lo ? k : lo;
        hi = k > hi ? k : hi;
    };
    uint64_t g = t;
    for (; g + stride < groups; g += 2 * stride) {
        const k2_a8 a = *reinterpret_cast<const k2_a8 *>(keys + 2 * g);
        const k2_a8 b = *reinterpret_cast<const k2_a8 *>(keys + 2 * (g + stride));
        take(a.x), take(a.y), take(b.x), take(b.y);
    }
    if (g < groups) {
        const k2_a8 a = *reinterpret_cast<const k2_a8 *>(keys + 2 * g);
        take(a.x), take(a.y);
    }
    if (t == 0 && (n & 1)) take((uint64_t)keys[n - 1]);
    block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = lo;
        part[2 * blockIdx.x + 1] = hi;
    }
}

// out[0], out[1] = min, max over the m workgroups' partials (one workgroup)
__global__ void __launch_bounds__(NT) minmax_final_kernel(const int64_t *__restrict__ part, uint32_t m,
                                                          int64_t *__restrict__ out) {
    int64_t lo = INT64_MAX, hi = INT64_MIN;
    for (uint32_t g = threadIdx.x; g < m; g += NT) {
        lo = part[2 * g] < lo ? part[2 * g] : lo;
        hi = part[2 * g + 1] > hi ? part[2 * g + 1] : hi;
    }
    block_minmax(lo, hi);
    if (threadIdx.x == 0) {
        out[0] = lo;
        out[1] = hi;
    }
}

// ------------------------------------------------------------------ pack -----------------
// WIDE: the first pass's word, the biased low half over the position.  Else the narrow word.
template <bool WIDE>
__device__ __forceinline__ uint64_t pack_word(uint64_t key, uint64_t i, uint64_t kmin, int b) {
    if (WIDE) return word((uint32_t)key ^ BIAS, (uint32_t)i);
    return (((key - kmin) << b) | i) ^ SIGN;
}

// `base` = the global position of keys[0] (a sample argsort; 0 in a local one): element i packs the
// position base + i.
template <bool WIDE, int KC>
__global__ void __launch_bounds__(NT) pack64_keys_kernel(const int64_t *__restrict__ keys,
                                                         uint64_t *__restrict__ packed, uint64_t n, uint64_t kmin,
                                                         int b, uint64_t base) {
    using C = kc::Codec<KC>;
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        const uint64_t p0 = base + e0, p1 = base + e1;
        const k2_a8 k0 = *reinterpret_cast<const k2_a8 *>(keys + e0);
        const k2_a8 k1 = *reinterpret_cast<const k2_a8 *>(keys + e1);
        __builtin_nontemporal_store(
            l2{pack_word<WIDE>(C::enc(k0.x), p0, kmin, b), pack_word<WIDE>(C::enc(k0.y), p0 + 1, kmin, b)},
            reinterpret_cast<l2 *>(packed + e0));
        __builtin_nontemporal_store(
            l2{pack_word<WIDE>(C::enc(k1.x), p1, kmin, b), pack_word<WIDE>(C::enc(k1.y), p1 + 1, kmin, b)},
            reinterpret_cast<l2 *>(packed + e1));
    }
    const uint64_t i = (chunks << 8) + t;  // the n % 256 last elements, one each
    if (i < n) packed[i] = pack_word<WIDE>(C::enc((uint64_t)keys[i]), base + i, kmin, b);
}
// The same without a codec: the kernel of the int64 entry points, kept word for word.  (As one body
// shared with the kernel above, its instructions came out of the compiler in a slightly different
// order; scripts/asm_digest.py compares it with the parent's.)
template <bool WIDE>
__global__ void __launch_bounds__(NT) pack64_kernel(const int64_t *__restrict__ keys, uint64_t *__restrict__ packed,
                                                    uint64_t n, uint64_t kmin, int b, uint64_t base) {
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        const uint64_t p0 = base + e0, p1 = base + e1;
        const k2_a8 k0 = *reinterpret_cast<const k2_a8 *>(keys + e0);
        const k2_a8 k1 = *reinterpret_cast<const k2_a8 *>(keys + e1);
        __builtin_nontemporal_store(
            l2{pack_word<WIDE>(k0.x, p0, kmin, b), pack_word<WIDE>(k0.y, p0 + 1, kmin, b)},
            reinterpret_cast<l2 *>(packed + e0));
        __builtin_nontemporal_store(
            l2{pack_word<WIDE>(k1.x, p1, kmin, b), pack_word<WIDE>(k1.y, p1 + 1, kmin, b)},
            reinterpret_cast<l2 *>(packed + e1));
    }
    const uint64_t i = (chunks << 8) + t;  // the n % 256 last elements, one each
    if (i < n) packed[i] = pack_word<WIDE>((uint64_t)keys[i], base + i, kmin, b);
}

// ------------------------------------------------------------------ narrow unpack --------
// idx_out[i] = the low b bits of u = packed[i] ^ SIGN, keys_out[i] (NULL: not wanted) = (u >> b) + min
// (the encoded word, which the codec turns back into the caller's key)
template <int KC>
__global__ void __launch_bounds__(NT) unpack64_keys_kernel(const uint64_t *__restrict__ packed,
                                                           int64_t *__restrict__ keys_out,
                                                           uint32_t *__restrict__ idx_out, uint64_t n, uint64_t kmin,
                                                           int b) {
    using C = kc::Codec<KC>;
    const uint64_t mask = (1ull << b) - 1;
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        l2 a = *reinterpret_cast<const l2 *>(packed + e0);
        l2 d = *reinterpret_cast<const l2 *>(packed + e1);
        a ^= SIGN;
        d ^= SIGN;
        __builtin_nontemporal_store(u2_a4{(uint32_t)(a.x & mask), (uint32_t)(a.y & mask)},
                                    reinterpret_cast<u2_a4 *>(idx_out + e0));
        __builtin_nontemporal_store(u2_a4{(uint32_t)(d.x & mask), (uint32_t)(d.y & mask)},
                                    reinterpret_cast<u2_a4 *>(idx_out + e1));
        if (keys_out) {
            __builtin_nontemporal_store(k2_a8{C::dec((a.x >> b) + kmin), C::dec((a.y >> b) + kmin)},
                                        reinterpret_cast<k2_a8 *>(keys_out + e0));
            __builtin_nontemporal_store(k2_a8{C::dec((d.x >> b) + kmin), C::dec((d.y >> b) + kmin)},
                                        reinterpret_cast<k2_a8 *>(keys_out + e1));
        }
    }
    const uint64_t i = (chunks << 8) + t;
    if (i < n) {
        const uint64_t u = packed[i] ^ SIGN;
        idx_out[i] = (uint32_t)(u & mask);
        if (keys_out) keys_out[i] = (int64_t)C::dec((u >> b) + kmin);
    }
}
// The same without a codec: the kernel of the int64 entry points, kept word for word.  (As one body
// shared with the kernel above, its instructions came out of the compiler in a slightly different
// order; scripts/asm_digest.py compares it with the parent's.)
__global__ void __launch_bounds__(NT) unpack64_kernel(const uint64_t *__restrict__ packed, int64_t *__restrict__ keys_out,
                                                      uint32_t *__restrict__ idx_out, uint64_t n, uint64_t kmin,
                                                      int b) {
    const uint64_t mask = (1ull << b) - 1;
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        l2 a = *reinterpret_cast<const l2 *>(packed + e0);
        l2 d = *reinterpret_cast<const l2 *>(packed + e1);
        a ^= SIGN;
        d ^= SIGN;
        __builtin_nontemporal_store(u2_a4{(uint32_t)(a.x & mask), (uint32_t)(a.y & mask)},
                                    reinterpret_cast<u2_a4 *>(idx_out + e0));
        __builtin_nontemporal_store(u2_a4{(uint32_t)(d.x & mask), (uint32_t)(d.y & mask)},
                                    reinterpret_cast<u2_a4 *>(idx_out + e1));
        if (keys_out) {
            __builtin_nontemporal_store(k2_a8{(a.x >> b) + kmin, (a.y >> b) + kmin},
                                        reinterpret_cast<k2_a8 *>(keys_out + e0));
            __builtin_nontemporal_store(k2_a8{(d.x >> b) + kmin, (d.y >> b) + kmin},
                                        reinterpret_cast<k2_a8 *>(keys_out + e1));
        }
    }
    const uint64_t i = (chunks << 8) + t;
    if (i < n) {
        const uint64_t u = packed[i] ^ SIGN;
        idx_out[i] = (uint32_t)(u & mask);
        if (keys_out) keys_out[i] = (int64_t)((u >> b) + kmin);
    }
}

// ------------------------------------------------------------------ wide: regroup --------
// B[j] = hi32(enc(keys[p])) : j, p = the low word of A[j] (A sorted by the low halves): the keys are
// the caller's, read at random, so each is encoded again before its high half is taken
template <int KC>
__device__ __forceinline__ void regroup64_body(const uint64_t *A, const int64_t *keys, uint64_t *B, uint64_t n) {
    using C = kc::Codec<KC>;
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        const l2 a = *reinterpret_cast<const l2 *>(A + e0);
        const l2 d = *reinterpret_cast<const l2 *>(A + e1);
        // four independent random reads in flight
        const uint64_t k0 = C::enc((uint64_t)keys[(uint32_t)a.x]), k1 = C::enc((uint64_t)keys[(uint32_t)a.y]);
        const uint64_t k2 = C::enc((uint64_t)keys[(uint32_t)d.x]), k3 = C::enc((uint64_t)keys[(uint32_t)d.y]);
        __builtin_nontemporal_store(
            l2{word((uint32_t)(k0 >> 32), (uint32_t)e0), word((uint32_t)(k1 >> 32), (uint32_t)e0 + 1)},
            reinterpret_cast<l2 *>(B + e0));
        __builtin_nontemporal_store(
            l2{word((uint32_t)(k2 >> 32), (uint32_t)e1), word((uint32_t)(k3 >> 32), (uint32_t)e1 + 1)},
            reinterpret_cast<l2 *>(B + e1));
    }
    const uint64_t i = (chunks << 8) + t;
    if (i < n) B[i] = word((uint32_t)(C::enc((uint64_t)keys[(uint32_t)A[i]]) >> 32), (uint32_t)i);
}
__global__ void __launch_bounds__(NT) regroup64_kernel(const uint64_t *__restrict__ A, const int64_t *__restrict__ keys,
                                                       uint64_t *__restrict__ B, uint64_t n) {
    regroup64_body<0>(A, keys, B, n);
}
template <int KC>
__global__ void __launch_bounds__(NT) regroup64_keys_kernel(const uint64_t *__restrict__ A,
                                                            const int64_t *__restrict__ keys,
                                                            uint64_t *__restrict__ B, uint64_t n) {
    regroup64_body<KC>(A, keys, B, n);
}

// ------------------------------------------------------------------ wide: final ----------
// r -> j = the low word of B[r] (B sorted by the high halves), A[j] = (lo ^ BIAS) : p:
// idx_out[r] = p, keys_out[r] (NULL: not wanted) = the codec's decoding of hi32 : lo
template <int KC>
__device__ __forceinline__ void final64_body(const uint64_t *B, const uint64_t *A, int64_t *keys_out,
                                             uint32_t *idx_out, uint64_t n) {
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    auto key_of = [](uint64_t bw, uint64_t aw) {
        return kc::Codec<KC>::dec(word((uint32_t)(bw >> 32), (uint32_t)(aw >> 32) ^ BIAS));
    };
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        const l2 x = *reinterpret_cast<const l2 *>(B + e0);
        const l2 y = *reinterpret_cast<const l2 *>(B + e1);
        const uint64_t a0 = A[(uint32_t)x.x], a1 = A[(uint32_t)x.y];
        const uint64_t a2 = A[(uint32_t)y.x], a3 = A[(uint32_t)y.y];
        __builtin_nontemporal_store(u2_a4{(uint32_t)a0, (uint32_t)a1}, reinterpret_cast<u2_a4 *>(idx_out + e0));
        __builtin_nontemporal_store(u2_a4{(uint32_t)a2, (uint32_t)a3}, reinterpret_cast<u2_a4 *>(idx_out + e1));
        if (keys_out) {
            __builtin_nontemporal_store(k2_a8{key_of(x.x, a0), key_of(x.y, a1)},
                                        reinterpret_cast<k2_a8 *>(keys_out + e0));
            __builtin_nontemporal_store(k2_a8{key_of(y.x, a2), key_of(y.y, a3)},
                                        reinterpret_cast<k2_a8 *>(keys_out + e1));
        }
    }
    const uint64_t i = (chunks << 8) + t;
    if (i < n) {
        const uint64_t bw = B[i];
        const uint64_t aw = A[(uint32_t)bw];
        idx_out[i] = (uint32_t)aw;
        if (keys_out) keys_out[i] = (int64_t)key_of(bw, aw);
    }
}
__global__ void __launch_bounds__(NT) final64_kernel(const uint64_t *__restrict__ B, const uint64_t *__restrict__ A,
                                                     int64_t *__restrict__ keys_out, uint32_t *__restrict__ idx_out,
                                                     uint64_t n) {
    final64_body<0>(B, A, keys_out, idx_out, n);
}
template <int KC>
__global__ void __launch_bounds__(NT) final64_keys_kernel(const uint64_t *__restrict__ B,
                                                          const uint64_t *__restrict__ A,
                                                          int64_t *__restrict__ keys_out,
                                                          uint32_t *__restrict__ idx_out, uint64_t n) {
    final64_body<KC>(B, A, keys_out, idx_out, n);
}

// ------------------------------------------------------------------ across ranks ---------
// The wide path of dsort_sample_argsort_dev_i64 has a distributed gather where the local one reads
// at random, so its three kernels stream: 16-byte loads of arenas, the shapes as above.

// low[i] = the low word of S[i] (the indices of the gather that follows); copy (NULL: not wanted)
// = S, which the next sample sort overwrites
__global__ void __launch_bounds__(NT) split64_kernel(const uint64_t *__restrict__ S, uint64_t *__restrict__ copy,
                                                     uint32_t *__restrict__ low, uint64_t n) {
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        const l2 a = *reinterpret_cast<const l2 *>(S + e0);
        const l2 d = *reinterpret_cast<const l2 *>(S + e1);
        __builtin_nontemporal_store(u2_a4{(uint32_t)a.x, (uint32_t)a.y}, reinterpret_cast<u2_a4 *>(low + e0));
        __builtin_nontemporal_store(u2_a4{(uint32_t)d.x, (uint32_t)d.y}, reinterpret_cast<u2_a4 *>(low + e1));
        if (copy) {
            __builtin_nontemporal_store(a, reinterpret_cast<l2 *>(copy + e0));
            __builtin_nontemporal_store(d, reinterpret_cast<l2 *>(copy + e1));
        }
    }
    const uint64_t i = (chunks << 8) + t;
    if (i < n) {
        const uint64_t w = S[i];
        low[i] = (uint32_t)w;
        if (copy) copy[i] = w;
    }
}

// B[j] = hi32(K[j]) : (off + j), K the whole keys in the order of the first pass and off this
// rank's first rank in that order
__global__ void __launch_bounds__(NT) regroup_stream64_kernel(const uint64_t *__restrict__ K, uint64_t *__restrict__ B,
                                                              uint64_t n, uint32_t off) {
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        const uint32_t j0 = off + (uint32_t)e0, j1 = off + (uint32_t)e1;
        const l2 a = *reinterpret_cast<const l2 *>(K + e0);
        const l2 d = *reinterpret_cast<const l2 *>(K + e1);
        __builtin_nontemporal_store(l2{word((uint32_t)(a.x >> 32), j0), word((uint32_t)(a.y >> 32), j0 + 1)},
                                    reinterpret_cast<l2 *>(B + e0));
        __builtin_nontemporal_store(l2{word((uint32_t)(d.x >> 32), j1), word((uint32_t)(d.y >> 32), j1 + 1)},
                                    reinterpret_cast<l2 *>(B + e1));
    }
    const uint64_t i = (chunks << 8) + t;
    if (i < n) B[i] = word((uint32_t)(K[i] >> 32), off + (uint32_t)i);
}

// SB[r] = hi32 : j and AW[r] = the first pass's word of rank j, (lo ^ BIAS) : p:
// idx_out[r] = p, keys_out[r] (NULL: not wanted) = hi32 : lo
__global__ void __launch_bounds__(NT) final_stream64_kernel(const uint64_t *__restrict__ SB,
                                                            const uint64_t *__restrict__ AW,
                                                            int64_t *__restrict__ keys_out,
                                                            uint32_t *__restrict__ idx_out, uint64_t n) {
    const uint64_t chunks = n >> 8;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    const uint64_t nwaves = ((uint64_t)gridDim.x * NT) >> 6;
    const uint32_t l = threadIdx.x & 63;
    auto key_of = [](uint64_t bw, uint64_t aw) { return word((uint32_t)(bw >> 32), (uint32_t)(aw >> 32) ^ BIAS); };
    for (uint64_t c = t >> 6; c < chunks; c += nwaves) {
        const uint64_t e0 = (c << 8) + 2 * l, e1 = e0 + 128;
        const l2 a = *reinterpret_cast<const l2 *>(AW + e0);
        const l2 d = *reinterpret_cast<const l2 *>(AW + e1);
        __builtin_nontemporal_store(u2_a4{(uint32_t)a.x, (uint32_t)a.y}, reinterpret_cast<u2_a4 *>(idx_out + e0));
        __builtin_nontemporal_store(u2_a4{(uint32_t)d.x, (uint32_t)d.y}, reinterpret_cast<u2_a4 *>(idx_out + e1));
        if (keys_out) {
            const l2 x = *reinterpret_cast<const l2 *>(SB + e0);
            const l2 y = *reinterpret_cast<const l2 *>(SB + e1);
            __builtin_nontemporal_store(k2_a8{key_of(x.x, a.x), key_of(x.y, a.y)},
                                        reinterpret_cast<k2_a8 *>(keys_out + e0));
            __builtin_nontemporal_store(k2_a8{key_of(y.x, d.x), key_of(y.y, d.y)},
                                        reinterpret_cast<k2_a8 *>(keys_out + e1));
        }
    }
    const uint64_t i = (chunks << 8) + t;
    if (i < n) {
        const uint64_t aw = AW[i];
        idx_out[i] = (uint32_t)aw;
        if (keys_out) keys_out[i] = (int64_t)key_of(SB[i], aw);
    }
}

// ------------------------------------------------------------------ host -----------------
// The launches of the typed kernels, defined at the end of the file: the int64 entry points'
// kernels then come out of the compiler in the order, and so under the labels, they always had
// (scripts/asm_digest.py compares them with the parent's).
static void launch_minmax_keys(int kc, unsigned grid, hipStream_t s, const int64_t *keys, uint64_t n, int64_t *part);
static void launch_pack64_keys(int kc, bool wide, unsigned grid, hipStream_t s, const int64_t *keys, uint64_t *packed,
                               uint64_t n, uint64_t kmin, int b, uint64_t base);
static void launch_unpack64_keys(int kc, unsigned grid, hipStream_t s, const uint64_t *packed, int64_t *keys_out,
                                 uint32_t *idx_out, uint64_t n, uint64_t kmin, int b);
static void launch_regroup64_keys(int kc, unsigned grid, hipStream_t s, const uint64_t *A, const int64_t *keys,
                                  uint64_t *B, uint64_t n);
static void launch_final64_keys(int kc, unsigned grid, hipStream_t s, const uint64_t *B, const uint64_t *A,
                                int64_t *keys_out, uint32_t *idx_out, uint64_t n);

static unsigned grid_for(uint64_t lanes) {
    const uint64_t g = (lanes + NT - 1) / NT;
    return (unsigned)(g > MAXWG ? MAXWG : (g ? g : 1));
}

// The host rule (dsort_plan_argsort_i64): bits of a position, and the passes the keys' range needs.
static int plan_argsort64(uint64_t n, int64_t kmin, int64_t kmax, int *idx_bits, int *passes) {
    if (n > (1ull << 32) || kmin > kmax) return DSORT_EINVAL;
    int b = 1;
    if (n > 2) b = 64 - __builtin_clzll(n - 1);
    const uint64_t R = (uint64_t)kmax - (uint64_t)kmin;
    if (idx_bits) *idx_bits = b;
    if (passes) *passes = n == 0 ? 0 : ((R >> (64 - b)) == 0 ? 1 : 2);
    return DSORT_OK;
}

// min and max of keys[0..n), n > 0, on the host: two launches, a 16-byte copy into the pinned
// mirror and one host wait.
static int minmax(dsort_ctx *ctx, const int64_t *keys, size_t n, hipStream_t s, int64_t *kmin, int64_t *kmax,
                  int kc = 0) {
    int rc = ensure(ctx, ctx->a64_part, (size_t)(MAXWG + 1) * 16, "argsort min/max partials");
    if (rc) return rc;
    if ((rc = ensure_small_host(ctx, 16))) return rc;
    if (!ctx->a64_mm_ev && hipEventCreateWithFlags(&ctx->a64_mm_ev.h, hipEventDisableTiming) != hipSuccess)
        return set_err(ctx, DSORT_EHIP, "hipEventCreate");
    int64_t *part = ctx->a64_part.as<int64_t>();
    const unsigned grid = grid_for(((uint64_t)n + 3) / 4);
    if (kc) {
        launch_minmax_keys(kc, grid, s, keys, (uint64_t)n, part);
    } else {
        hipLaunchKernelGGL(minmax_kernel, dim3(grid), dim3(NT), 0, s, keys, (uint64_t)n, part);
    }
    DSORT_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(minmax_final_kernel, dim3(1), dim3(NT), 0, s, part, (uint32_t)grid, part + 2 * MAXWG);
    DSORT_HIP(ctx, hipGetLastError());
    DSORT_HIP(ctx, hipMemcpyAsync(ctx->small_host.p, part + 2 * MAXWG, 16, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipEventRecord(ctx->a64_mm_ev, s));
    if ((rc = sync_event(ctx, ctx->a64_mm_ev, "argsort min/max read-back"))) return rc;
    const int64_t *h = ctx->small_host.as<const int64_t>();
    *kmin = h[0];
    *kmax = h[1];
    return DSORT_OK;
}

// One inner sort of the call.  DSORT_OPT_KILL_AFTER_STAGE counts the call's sorts one after the
// other: `done` = the stages of the sorts before this one, which this one's continue.
static int inner_sort(dsort_ctx *ctx, uint64_t *words, size_t n, hipStream_t s, int *done) {
    const int64_t kill = ctx->opt.kill_after_pass;
    if (kill >= 0) ctx->opt.kill_after_pass = kill - *done;  // (>= 0: the earlier sorts never reached it)
    const int rc = sort_device<int64_t>(ctx, reinterpret_cast<int64_t *>(words), reinterpret_cast<int64_t *>(words), n,
                                        s, true);
    ctx->opt.kill_after_pass = kill;
    *done += ctx->stages_done;
    return rc;
}

// d_idx_out[j] = the position in keys of the j-th smallest key, equal keys in input order;
// keys_out (NULL: not wanted; may be keys: the pack / the regroup has consumed the keys before the
// last kernel writes).  Asynchronous on s but for the min/max read-back of the automatic mode.
// kc: the key codec (dsort_keycodec.h; 0 = int64 ascending, the kernels of the int64 entry points):
// min, max and the plan are those of the ENCODED words, whose signed order is the typed keys' order.
int argsort64(dsort_ctx *ctx, const int64_t *keys, int64_t *keys_out, uint32_t *idx_out, size_t n, hipStream_t s,
              int kc) {
    if (n == 0) {
        ctx->stats = fresh_stats();
        ctx->ev_mask = 0;
        ctx->kev_used = 0;
        return DSORT_OK;
    }
    // one bracket around the whole sequence: the arenas are shared by calls on different streams
    int rc = order_begin(ctx, s);
    if (rc) return rc;
    rc = ensure(ctx, ctx->pairs, n * 8, "pair arena");
    if (rc) return rc;
    uint64_t *A = ctx->pairs.as<uint64_t>();
    ctx->a64_clk.start(ctx->ev_ok && ctx->opt.stage_timing);  // (the legs' events, for dsort_argsort64_leg_ms)
    ctx->a64_minmax = false;
    int b = 0, passes = 2;
    int64_t kmin = 0, kmax = 0;
    ctx->a64_clk.mark(s);
    if (!ctx->opt.argsort_wide) {
        if ((rc = minmax(ctx, keys, n, s, &kmin, &kmax, kc))) return rc;
        if ((rc = plan_argsort64(n, kmin, kmax, &b, &passes)))
            return set_err(ctx, DSORT_EHIP, "argsort: the min/max reduction returned min > max");
        ctx->a64_minmax = true;
        ctx->a64_clk.mark(s);
    }
    const unsigned grid = grid_for(((uint64_t)n + 3) / 4);
    int done = 0, src;
    if (passes == 1) {
        if (kc) {
            launch_pack64_keys(kc, false, grid, s, keys, A, (uint64_t)n, (uint64_t)kmin, b, (uint64_t)0);
        } else {
            hipLaunchKernelGGL((pack64_kernel<false>), dim3(grid), dim3(NT), 0, s, keys, A, (uint64_t)n, (uint64_t)kmin,
                               b, (uint64_t)0);
        }
        DSORT_HIP(ctx, hipGetLastError());
        ctx->a64_clk.mark(s);
        // DSORT_ESTAGE (the kill stage was never reached) leaves a valid output: the rest still runs
        src = inner_sort(ctx, A, n, s, &done);
        if (src && src != DSORT_ESTAGE) return src;
        ctx->a64_clk.mark(s);
        if (kc) {
            launch_unpack64_keys(kc, grid, s, A, keys_out, idx_out, (uint64_t)n, (uint64_t)kmin, b);
        } else {
            hipLaunchKernelGGL(unpack64_kernel, dim3(grid), dim3(NT), 0, s, A, keys_out, idx_out, (uint64_t)n,
                               (uint64_t)kmin, b);
        }
        DSORT_HIP(ctx, hipGetLastError());
    } else {
        rc = ensure(ctx, ctx->a64_b, n * 8, "argsort second arena");
        if (rc) return rc;
        uint64_t *B = ctx->a64_b.as<uint64_t>();
        if (kc) {
            launch_pack64_keys(kc, true, grid, s, keys, A, (uint64_t)n, (uint64_t)0, 0, (uint64_t)0);
        } else {
            hipLaunchKernelGGL((pack64_kernel<true>), dim3(grid), dim3(NT), 0, s, keys, A, (uint64_t)n, (uint64_t)0, 0,
                               (uint64_t)0);
        }
        DSORT_HIP(ctx, hipGetLastError());
        ctx->a64_clk.mark(s);
        src = inner_sort(ctx, A, n, s, &done);
        if (src && src != DSORT_ESTAGE) return src;
        ctx->a64_clk.mark(s);
        if (kc) {
            launch_regroup64_keys(kc, grid, s, A, keys, B, (uint64_t)n);
        } else {
            hipLaunchKernelGGL(regroup64_kernel, dim3(grid), dim3(NT), 0, s, A, keys, B, (uint64_t)n);
        }
        DSORT_HIP(ctx, hipGetLastError());
        ctx->a64_clk.mark(s);
        src = inner_sort(ctx, B, n, s, &done);
        if (src && src != DSORT_ESTAGE) return src;
        ctx->a64_clk.mark(s);
        if (kc) {
            launch_final64_keys(kc, grid, s, B, A, keys_out, idx_out, (uint64_t)n);
        } else {
            hipLaunchKernelGGL(final64_kernel, dim3(grid), dim3(NT), 0, s, B, A, keys_out, idx_out, (uint64_t)n);
        }
        DSORT_HIP(ctx, hipGetLastError());
    }
    ctx->a64_clk.mark(s);
    ctx->stats.argsort_passes = passes;
    if ((rc = order_end(ctx, s))) return rc;
    if (src == DSORT_ESTAGE)
        return set_err(ctx, DSORT_ESTAGE,
                       "DSORT_OPT_KILL_AFTER_STAGE = " + std::to_string(ctx->opt.kill_after_pass) + ": this argsort of " +
                           std::to_string(n) + " int64 keys has " + std::to_string(done) + " stages in " +
                           std::to_string(passes) + " sort(s) (kill points 0.." + std::to_string(done - 1) + ")");
    return src;
}

// ------------------------------------------------------------------ across ranks: host ---
// The host rule of the decision (dsort_plan_sample_argsort_i64) and what the call needs besides.
struct SamplePlan {
    uint64_t E = 0, total = 0;  // the end of the global range, the keys of all ranks
    int64_t kmin = 0, kmax = 0;
    int b = 1, passes = 0;
};
static int plan_sample_argsort64(int P, const uint64_t *first, const uint64_t *count, const int64_t *kmin,
                                 const int64_t *kmax, SamplePlan *out) {
    std::vector<uint64_t> lo((size_t)P), hi((size_t)P);
    std::vector<int32_t> own((size_t)P);
    int nr = 0;
    if (dsort_plan_gather_table(P, first, count, lo.data(), hi.data(), own.data(), &nr)) return DSORT_EINVAL;
    SamplePlan p;
    for (int r = 0; r < P; ++r) {
        if (!count[r]) continue;
        if (kmin[r] > kmax[r]) return DSORT_EINVAL;
        p.kmin = !p.total || kmin[r] < p.kmin ? kmin[r] : p.kmin;
        p.kmax = !p.total || kmax[r] > p.kmax ? kmax[r] : p.kmax;
        p.E = first[r] + count[r] > p.E ? first[r] + count[r] : p.E;
        p.total += count[r];
    }
    if (int rc = plan_argsort64(p.E, p.kmin, p.kmax, &p.b, &p.passes)) return rc;
    *out = p;
    return DSORT_OK;
}

static int launched(dsort_ctx *ctx, const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? DSORT_OK : hip_err(ctx, e, what);
}

// dsort_sample_argsort_dev_i64 behind its argument checks (dsort.h has the algorithm).  The call is
// a chain of exchange calls, the LEGS: 0 the decision, 1 the first sample sort, and on the wide
// path 2 the all-gather of the slice lengths, 3 the key gather, 4 the second sample sort, 5 the
// final gather.  Each takes the comm mutex and runs its gates itself, so nothing here holds either
// between two of them; what fails there (an arena, a launch) leaves through exch_leave while legs
// are still ahead, so that the peers meet the failure at their next gate.
static int sample_argsort64(dsort_ctx *ctx, const int64_t *keys, size_t n, uint64_t first, int64_t **keys_out,
                            uint32_t **idx_out, size_t *n_out, void *stream) {
    const hipStream_t s = pick_stream(ctx, stream);
    bool ahead = true;  // legs ahead: the peers wait at a gate
    auto fail = [&](int rc) { return ahead ? exch_leave(ctx, stream, rc) : rc; };
    // DSORT_OPT_TEST_FAIL_LEG: a local failure right before leg k
    auto before_leg = [&](int k) -> int {
        if (ctx->opt.test_fail_leg != k) return DSORT_OK;
        return fail(set_err(ctx, DSORT_EHIP, "injected local failure before leg " + std::to_string(k) +
                                                 " of the int64 sample argsort (DSORT_OPT_TEST_FAIL_LEG)"));
    };
    // The kill options act inside the first inner sample sort only; whatever leaves the call finds
    // them as the caller set them.
    struct KeepOpts {
        dsort_ctx *c;
        const int64_t stage, exch;
        ~KeepOpts() {
            c->opt.kill_after_pass = stage;
            c->opt.kill_in_exchange = exch;
        }
    } keep{ctx, ctx->opt.kill_after_pass, ctx->opt.kill_in_exchange};

    int rc = order_begin(ctx, s);
    if (rc) return fail(rc);
    ctx->s64_clk.start(ctx->ev_ok && ctx->opt.stage_timing);  // (the legs' events, for dsort_sample_argsort64_leg_ms)
    ctx->s64_clk.mark(s);

    // leg 0, the decision: every rank's range, min and max and option, and the host rule on them
    if ((rc = before_leg(0))) return rc;
    const bool forced = ctx->opt.argsort_wide != 0;
    SamplePlan pl;
    int P = 1;
    bool never = false;  // the kill stage lies beyond the first sort's stages
    int stages = 0;
    {
        ExchCall call(ctx, stream, 1);
        if (call.rc) return call.rc;
        P = call.P;
        int64_t kmin = 0, kmax = 0;
        if (n && !forced && (rc = minmax(ctx, keys, n, s, &kmin, &kmax))) return rc;
        const uint64_t mine[5] = {first, (uint64_t)n, (uint64_t)kmin, (uint64_t)kmax, forced ? 1u : 0u};
        std::vector<uint64_t> all((size_t)5 * P);
        rc = allgather_u64(ctx, mine, 5, all.data(), s, call.deadline, "argsort decision all-gather");
        if (rc) return rc;
        call.finished();  // (every rank sees the same table: what leaves below leaves on all of them)
        ahead = false;
        std::vector<uint64_t> f((size_t)P), c((size_t)P);
        std::vector<int64_t> lo((size_t)P), hi((size_t)P);
        for (int r = 0; r < P; ++r) {
            f[r] = all[5 * r], c[r] = all[5 * r + 1];
            lo[r] = forced ? 0 : (int64_t)all[5 * r + 2], hi[r] = forced ? 0 : (int64_t)all[5 * r + 3];
            if (all[5 * r + 4] != all[4])
                return set_err(ctx, DSORT_EINVAL, "sample argsort: the ranks disagree on DSORT_OPT_ARGSORT_WIDE (rank 0 " +
                                                      std::to_string(all[4]) + ", rank " + std::to_string(r) + " " +
                                                      std::to_string(all[5 * r + 4]) + ")");
        }
        if (plan_sample_argsort64(P, f.data(), c.data(), lo.data(), hi.data(), &pl))
            return set_err(ctx, DSORT_EINVAL, "sample argsort: the ranks' key ranges overlap or end beyond 2^32");
        if (forced && pl.total) pl.passes = 2;
        if (pl.passes == 2 && P > 256)
            return set_err(ctx, DSORT_EINVAL, "sample argsort: more than 256 ranks on the two-pass path (the gather's "
                                              "owner table)");
        if (pl.passes == 2 && pl.total >= (1ull << 32))
            return set_err(ctx, DSORT_EINVAL, "sample argsort: 2^32 keys on the two-pass path (a slice is the index "
                                              "array of a gather: fewer than 2^32)");
        if (keep.stage >= 0 && pl.total) {
            BxPlan bp;
            stages = bx_make_plan(ctx->opt, P, call.me, c.data(), 8, bp) ? 3 : sort_stages(ctx->opt, n, 8);
            never = keep.stage >= stages;
        }
    }
    if (pl.total == 0) {  // no rank holds a key: nothing to sort, and no collective is left
        ctx->stats = fresh_stats();
        ctx->ev_mask = 0;
        ctx->kev_used = 0;
        if (keys_out) *keys_out = ctx->s64_k.as<int64_t>();
        *idx_out = ctx->s64_i.as<uint32_t>();
        *n_out = 0;
        return DSORT_OK;
    }
    ahead = true;
    ctx->s64_clk.mark(s);
    const bool wide = pl.passes == 2;
    const unsigned grid = grid_for(((uint64_t)n + 3) / 4);

    // the words of the first (narrow: the only) sort, positions from `first` on
    if ((rc = ensure(ctx, ctx->pairs, (n ? n : 1) * 8, "pair arena"))) return fail(rc);
    uint64_t *A = ctx->pairs.as<uint64_t>();
    if (n) {
        if (wide)
            hipLaunchKernelGGL((pack64_kernel<true>), dim3(grid), dim3(NT), 0, s, keys, A, (uint64_t)n, (uint64_t)0, 0,
                               first);
        else
            hipLaunchKernelGGL((pack64_kernel<false>), dim3(grid), dim3(NT), 0, s, keys, A, (uint64_t)n,
                               (uint64_t)pl.kmin, pl.b, first);
        if ((rc = launched(ctx, "pack64_kernel"))) return fail(rc);
    }
    ctx->s64_clk.mark(s);

    // leg 1.  A kill stage this sort never reaches would make it return early, DSORT_ESTAGE, with
    // the peers in the legs that follow: switched off for it and reported at the end instead.
    if ((rc = before_leg(1))) return rc;
    if (never) ctx->opt.kill_after_pass = -1;
    int64_t *sa = nullptr;
    size_t mA = 0;
    rc = sample_sort_packed(ctx, reinterpret_cast<const int64_t *>(A), n, &sa, &mA, stream);
    ctx->opt.kill_after_pass = -1;  // (and off from here on: the second sort is not a kill point)
    ctx->opt.kill_in_exchange = -1;
    if (rc) return rc;  // (inside a leg: its own guard has told the peers)
    ahead = wide;
    if (mA && (reinterpret_cast<uintptr_t>(sa) & 15))
        return fail(set_err(ctx, DSORT_EHIP, "sample argsort: the sample sort's slice is not 16-byte aligned"));
    ctx->s64_clk.mark(s);

    size_t m = mA;
    const uint64_t *SB = nullptr, *AW = nullptr;
    if (wide) {
        // the slice is saved (the second sort's output takes its place) and split: its low words
        // are the positions of its keys
        if ((rc = ensure(ctx, ctx->s64_sa, (mA ? mA : 1) * 8, "sample argsort saved slice")))
            return fail(rc);
        if ((rc = ensure(ctx, ctx->s64_pos, (mA ? mA : 1) * 4, "sample argsort indices")))
            return fail(rc);
        if ((rc = ensure(ctx, ctx->s64_got, (mA ? mA : 1) * 8, "sample argsort gathered words")))
            return fail(rc);
        uint64_t *SA = ctx->s64_sa.as<uint64_t>();
        uint32_t *pos = ctx->s64_pos.as<uint32_t>();
        uint64_t *got = ctx->s64_got.as<uint64_t>();
        const unsigned gA = grid_for(((uint64_t)mA + 3) / 4);
        if (mA) {
            hipLaunchKernelGGL(split64_kernel, dim3(gA), dim3(NT), 0, s, reinterpret_cast<const uint64_t *>(sa), SA, pos,
                               (uint64_t)mA);
            if ((rc = launched(ctx, "split64_kernel"))) return fail(rc);
        }
        ctx->s64_clk.mark(s);

        // leg 2: every rank's slice length; offA = the rank of this slice's first word in pass-A order
        if ((rc = before_leg(2))) return rc;
        uint64_t offA = 0;
        {
            ExchCall call(ctx, stream, 1);
            if (call.rc) return call.rc;
            const uint64_t mine = mA;
            std::vector<uint64_t> all((size_t)P);
            rc = allgather_u64(ctx, &mine, 1, all.data(), s, call.deadline, "sample argsort slice-length all-gather");
            if (rc) return rc;
            call.finished();
            uint64_t sum = 0;
            for (int r = 0; r < P; ++r) {
                if (r == call.me) offA = sum;
                sum += all[r];
            }
            if (sum != pl.total) {  // (the same on every rank)
                ahead = false;
                return set_err(ctx, DSORT_EHIP, "sample argsort: the slices of the first sort do not add up");
            }
        }

        // leg 3: the whole keys in pass-A order, from wherever they live
        if ((rc = before_leg(3))) return rc;
        rc = dsort_sample_gather_dev(ctx, keys, n, first, pos, mA, got, 8, stream);
        if (rc) return rc;
        ctx->s64_clk.mark(s);

        // the second sort's words: the high halves over the ranks in pass-A order
        if ((rc = ensure(ctx, ctx->pairs, (mA ? mA : 1) * 8, "pair arena"))) return fail(rc);
        uint64_t *B = ctx->pairs.as<uint64_t>();
        if (mA) {
            hipLaunchKernelGGL(regroup_stream64_kernel, dim3(gA), dim3(NT), 0, s, got, B, (uint64_t)mA, (uint32_t)offA);
            if ((rc = launched(ctx, "regroup_stream64_kernel"))) return fail(rc);
        }
        ctx->s64_clk.mark(s);

        // leg 4
        if ((rc = before_leg(4))) return rc;
        int64_t *sb = nullptr;
        size_t mB = 0;
        rc = sample_sort_packed(ctx, reinterpret_cast<const int64_t *>(B), mA, &sb, &mB, stream);
        if (rc) return rc;
        if (mB && (reinterpret_cast<uintptr_t>(sb) & 15))
            return fail(set_err(ctx, DSORT_EHIP, "sample argsort: the sample sort's slice is not 16-byte aligned"));
        ctx->s64_clk.mark(s);
        if ((rc = ensure(ctx, ctx->s64_pos, (mB ? mB : 1) * 4, "sample argsort indices")))
            return fail(rc);
        if ((rc = ensure(ctx, ctx->s64_got, (mB ? mB : 1) * 8, "sample argsort gathered words")))
            return fail(rc);
        pos = ctx->s64_pos.as<uint32_t>();
        got = ctx->s64_got.as<uint64_t>();
        if (mB) {
            hipLaunchKernelGGL(split64_kernel, dim3(grid_for(((uint64_t)mB + 3) / 4)), dim3(NT), 0, s,
                               reinterpret_cast<const uint64_t *>(sb), static_cast<uint64_t *>(nullptr), pos, (uint64_t)mB);
            if ((rc = launched(ctx, "split64_kernel"))) return fail(rc);
        }
        ctx->s64_clk.mark(s);

        // leg 5: every word of the slice gets its pass-A word, which rank offA' + j' of some rank holds
        if ((rc = before_leg(5))) return rc;
        rc = dsort_sample_gather_dev(ctx, SA, mA, offA, pos, mB, got, 8, stream);
        if (rc) return rc;
        ahead = false;
        ctx->s64_clk.mark(s);
        m = mB;
        SB = reinterpret_cast<const uint64_t *>(sb);
        AW = got;
    }

    // this rank's slice into the output arenas
    if (keys_out && (rc = ensure(ctx, ctx->s64_k, (m ? m : 1) * 8, "sample argsort keys"))) return rc;
    if ((rc = ensure(ctx, ctx->s64_i, (m ? m : 1) * 4, "sample argsort positions"))) return rc;
    int64_t *ko = keys_out ? ctx->s64_k.as<int64_t>() : nullptr;
    uint32_t *io = ctx->s64_i.as<uint32_t>();
    if (m) {
        const unsigned g = grid_for(((uint64_t)m + 3) / 4);
        if (wide)
            hipLaunchKernelGGL(final_stream64_kernel, dim3(g), dim3(NT), 0, s, SB, AW, ko, io, (uint64_t)m);
        else
            hipLaunchKernelGGL(unpack64_kernel, dim3(g), dim3(NT), 0, s, reinterpret_cast<const uint64_t *>(sa), ko, io,
                               (uint64_t)m, (uint64_t)pl.kmin, pl.b);
        if ((rc = launched(ctx, "sample argsort unpack"))) return rc;
    }
    ctx->s64_clk.mark(s);
    ctx->stats.argsort_passes = pl.passes;
    if ((rc = order_end(ctx, s))) return rc;
    if (keys_out) *keys_out = ko;
    *idx_out = io;
    *n_out = m;
    if (never)
        return set_err(ctx, DSORT_ESTAGE,
                       "DSORT_OPT_KILL_AFTER_STAGE = " + std::to_string(keep.stage) + ": the first sample sort of this " +
                           "argsort has " + std::to_string(stages) + " stages (kill points 0.." +
                           std::to_string(stages - 1) + "); every leg has run");
    return DSORT_OK;
}

static int check_args(dsort_ctx *ctx, const void *keys, const void *out, size_t n) {
    if ((uint64_t)n > (1ull << 32))
        return set_err(ctx, DSORT_EINVAL, "argsort: more than 2^32 keys (a position must fit 32 bits)");
    if (n && (!keys || !out)) return set_err(ctx, DSORT_EINVAL, "null argument");
    return DSORT_OK;
}

}  // namespace p64
}  // namespace dsort

using namespace dsort;

extern "C" {

int dsort_plan_argsort_i64(size_t n, int64_t key_min, int64_t key_max, int *idx_bits, int *passes) {
    return p64::plan_argsort64(n, key_min, key_max, idx_bits, passes);
}

int dsort_argsort_dev_i64(dsort_ctx *ctx, const int64_t *d_keys, int64_t *d_keys_out, uint32_t *d_idx_out, size_t n,
                          void *stream) {
    if (!ctx) return DSORT_EINVAL;
    if (int rc = p64::check_args(ctx, d_keys, d_idx_out, n)) return rc;
    return p64::argsort64(ctx, d_keys, d_keys_out, d_idx_out, n, pick_stream(ctx, stream));
}

int dsort_sort_records_dev_i64(dsort_ctx *ctx, const int64_t *d_keys, int64_t *d_keys_out, const void *d_src,
                               void *d_dst, size_t n, int elem_bytes, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16)
        return set_err(ctx, DSORT_EINVAL, "record sort: elem_bytes must be 4, 8 or 16");
    if (int rc = p64::check_args(ctx, d_keys, d_dst, n)) return rc;
    if (n && !d_src) return set_err(ctx, DSORT_EINVAL, "null argument");
    hipStream_t s = pick_stream(ctx, stream);
    if (n == 0) return p64::argsort64(ctx, d_keys, d_keys_out, nullptr, 0, s);  // (resets the statistics)
    int rc = order_begin(ctx, s);
    if (rc) return rc;
    rc = ensure(ctx, ctx->a64_idx, n * 4, "record sort indices");
    if (rc) return rc;
    uint32_t *idx = ctx->a64_idx.as<uint32_t>();
    const int src = p64::argsort64(ctx, d_keys, d_keys_out, idx, n, s);
    if (src && src != DSORT_ESTAGE) return src;
    const std::string msg = ctx->err;
    // (the stream as the caller gave it: dsort_gather_dev picks the same one)
    if ((rc = dsort_gather_dev(ctx, d_src, idx, d_dst, n, elem_bytes, stream))) return rc;
    // the gather reads the index arena behind the argsort's bracket: the call ends here
    if ((rc = order_end(ctx, s))) return rc;
    return src ? set_err(ctx, src, msg) : DSORT_OK;
}

int dsort_sample_argsort_dev_i64(dsort_ctx *ctx, const int64_t *d_keys, size_t n_local, uint64_t first,
                                 int64_t **d_keys_out, uint32_t **d_idx_out, size_t *n_out, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    if (first > (1ull << 32) || (uint64_t)n_local > (1ull << 32) - first)
        return set_err(ctx, DSORT_EINVAL,
                       "sample argsort: first + n_local exceeds 2^32 (a global position must fit 32 bits)");
    if (!d_idx_out || !n_out || (n_local && !d_keys)) return set_err(ctx, DSORT_EINVAL, "null argument");
    return p64::sample_argsort64(ctx, d_keys, n_local, first, d_keys_out, d_idx_out, n_out, stream);
}

int dsort_plan_sample_argsort_i64(int nranks, const uint64_t first[], const uint64_t count[], const int64_t key_min[],
                                  const int64_t key_max[], int *idx_bits, int *passes) {
    if (nranks < 1 || !first || !count || !key_min || !key_max) return DSORT_EINVAL;
    p64::SamplePlan pl;
    if (int rc = p64::plan_sample_argsort64(nranks, first, count, key_min, key_max, &pl)) return rc;
    if (idx_bits) *idx_bits = pl.b;
    if (passes) *passes = pl.passes;
    return DSORT_OK;
}

int dsort_argsort_i64(dsort_ctx *ctx, const int64_t *keys, int64_t *keys_out, uint32_t *idx, size_t n) {
    if (!ctx) return DSORT_EINVAL;
    if (int rc = p64::check_args(ctx, keys, idx, n)) return rc;
    if (n == 0) return DSORT_OK;
    int rc = ensure(ctx, ctx->io, n * 8, "staging");
    if (rc) return rc;
    rc = ensure(ctx, ctx->io2, n * 4, "staging 2");
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    int64_t *dk = ctx->io.as<int64_t>();
    uint32_t *di = ctx->io2.as<uint32_t>();
    DSORT_HIP(ctx, hipMemcpyAsync(dk, keys, n * 8, hipMemcpyHostToDevice, s));
    const int src = p64::argsort64(ctx, dk, keys_out ? dk : nullptr, di, n, s);
    if (src && src != DSORT_ESTAGE) return src;
    if (keys_out) DSORT_HIP(ctx, hipMemcpyAsync(keys_out, dk, n * 8, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipMemcpyAsync(idx, di, n * 4, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipStreamSynchronize(s));
    return src;
}

// Not part of the ABI (like dsort_pairs_leg_ms): device time of the last int64 argsort's legs from
// HIP events between them, for scripts/bench_pairs.py --i64.  ms[0] = the min/max reduction with its
// read-back (0 when DSORT_OPT_ARGSORT_WIDE skipped it); one pass: ms[1..3] = pack, sort, unpack;
// two passes: ms[1..5] = pack, sort 1, regroup, sort 2, final.  *legs = the entries written (4 or
// 6; ms must hold 6).  Blocks until that call has finished; DSORT_EINVAL when it recorded none.
int dsort_argsort64_leg_ms(dsort_ctx *ctx, double ms[6], int *legs) {
    if (!ctx || !ms || !legs) return DSORT_EINVAL;
    const LegClock &c = ctx->a64_clk;
    const int first = ctx->a64_minmax ? 0 : 1;  // without the reduction the events start at the pack
    const int nl = c.count() - 1 + first;
    if (!c.count() || (nl != 4 && nl != 6)) return set_err(ctx, DSORT_EINVAL, "no timed int64 argsort on this context");
    int rc = c.wait_last(ctx);
    ms[0] = 0;
    for (int i = first; i < nl && !rc; ++i) rc = c.elapsed(ctx, i - first, i - first + 1, &ms[i]);
    *legs = nl;
    return rc;
}

// The same for the last dsort_sample_argsort_dev_i64 (scripts/bench_pairs.py --sample-i64); the time
// between two events includes the host waits of what lies between them.  One pass, *legs = 4:
// decision (min/max, all-gather), pack, sample sort, unpack.  Two passes, *legs = 10: decision, pack,
// sample sort 1, split, key gather (the slice-length all-gather included), regroup, sample sort 2,
// split, final gather, final.  ms must hold 10.  DSORT_EINVAL when the call recorded none.
int dsort_sample_argsort64_leg_ms(dsort_ctx *ctx, double ms[10], int *legs) {
    if (!ctx || !ms || !legs) return DSORT_EINVAL;
    const LegClock &c = ctx->s64_clk;
    const int nl = c.count() - 1;
    if (nl != 4 && nl != 10) return set_err(ctx, DSORT_EINVAL, "no timed int64 sample argsort on this context");
    int rc = c.wait_last(ctx);
    for (int i = 0; i < nl && !rc; ++i) rc = c.elapsed(ctx, i, i + 1, &ms[i]);
    *legs = nl;
    return rc;
}

}  // extern "C"

namespace dsort {
namespace p64 {

static void launch_minmax_keys(int kc, unsigned grid, hipStream_t s, const int64_t *keys, uint64_t n, int64_t *part) {
    DSORT_KC_SWITCH(kc, hipLaunchKernelGGL((minmax_keys_kernel<KC_>), dim3(grid), dim3(NT), 0, s, keys, n, part));
}

static void launch_pack64_keys(int kc, bool wide, unsigned grid, hipStream_t s, const int64_t *keys, uint64_t *packed,
                               uint64_t n, uint64_t kmin, int b, uint64_t base) {
    if (wide) {
        DSORT_KC_SWITCH(kc, hipLaunchKernelGGL((pack64_keys_kernel<true, KC_>), dim3(grid), dim3(NT), 0, s, keys, packed,
                                               n, kmin, b, base));
    } else {
        DSORT_KC_SWITCH(kc, hipLaunchKernelGGL((pack64_keys_kernel<false, KC_>), dim3(grid), dim3(NT), 0, s, keys,
                                               packed, n, kmin, b, base));
    }
}

static void launch_unpack64_keys(int kc, unsigned grid, hipStream_t s, const uint64_t *packed, int64_t *keys_out,
                                 uint32_t *idx_out, uint64_t n, uint64_t kmin, int b) {
    DSORT_KC_SWITCH(kc, hipLaunchKernelGGL((unpack64_keys_kernel<KC_>), dim3(grid), dim3(NT), 0, s, packed, keys_out,
                                           idx_out, n, kmin, b));
}

static void launch_regroup64_keys(int kc, unsigned grid, hipStream_t s, const uint64_t *A, const int64_t *keys,
                                  uint64_t *B, uint64_t n) {
    DSORT_KC_SWITCH(kc, hipLaunchKernelGGL((regroup64_keys_kernel<KC_>), dim3(grid), dim3(NT), 0, s, A, keys, B, n));
}

static void launch_final64_keys(int kc, unsigned grid, hipStream_t s, const uint64_t *B, const uint64_t *A,
                                int64_t *keys_out, uint32_t *idx_out, uint64_t n) {
    DSORT_KC_SWITCH(kc, hipLaunchKernelGGL((final64_keys_kernel<KC_>), dim3(grid), dim3(NT), 0, s, B, A, keys_out,
                                           idx_out, n));
}

}  // namespace p64
}  // namespace dsort
