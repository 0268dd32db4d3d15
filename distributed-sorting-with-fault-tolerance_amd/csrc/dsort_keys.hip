// dsort_keys.hip -- typed keys and descending order through every sort entry (dsort.h, "Key types
// and order", an ABI 10 addition): float, unsigned and signed keys of 4 and 8 bytes, ascending or
// descending, by the order-preserving codec of dsort_keycodec.h.
//
// Where the codec sits:
//   argsort, pair sort, record sort   fused.  Those paths already stream every key through a pack
//                                     kernel and every output through an unpack kernel
//                                     (dsort_pairs.hip, dsort_pairs64.hip), which take the codec as
//                                     a template parameter: no extra pass over memory.
//   keys-only sort                    encode, the integer sort, decode: the two streaming kernels
//                                     below around sort_device, two extra passes over the keys.
//                                     Fusing the codec into the first-level histogram and scatter
//                                     and the tile sort's store would touch the kernels the metric
//                                     rests on.
//   across ranks                      the local chunk is encoded into an arena of the context, the
//                                     integer sample sort / sample argsort runs on it, and the key
//                                     slice it returns is decoded in place.  No exchange kernel
//                                     changes.
//
// The two kernels are written as pairs_unpack_kernel is: grid-stride, 16 bytes per access typed
// at 4-byte alignment on caller memory (a tensor view at element 1), non-temporal stores, and the
// elements behind the last whole 16 bytes one by one.  HBM bytes per key: each reads W and
// writes W.
#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "dsort_exch.h"
#include "dsort_internal.h"
#include "dsort_keycodec.h"

namespace dsort {
namespace ky {

constexpr int NT = 256;          // threads per workgroup
constexpr unsigned MAXWG = 2048; // workgroups of a launch (256 CUs x 8), the rest by grid stride

// 16 bytes of caller memory: four dwords at dword alignment
typedef uint32_t u4_a4 __attribute__((ext_vector_type(4), aligned(4)));

__device__ __forceinline__ uint64_t join(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// 16 bytes of keys of W bytes through the codec, DEC: back
template <int KC, int W, bool DEC>
__device__ __forceinline__ u4_a4 code16(u4_a4 v) {
    using C = kc::Codec<KC>;
    if (W == 4) {
        if (DEC) return u4_a4{C::dec(v.x), C::dec(v.y), C::dec(v.z), C::dec(v.w)};
        return u4_a4{C::enc(v.x), C::enc(v.y), C::enc(v.z), C::enc(v.w)};
    }
    const uint64_t a = join(v.x, v.y), b = join(v.z, v.w);
    const uint64_t x = DEC ? C::dec(a) : C::enc(a), y = DEC ? C::dec(b) : C::enc(b);
    return u4_a4{(uint32_t)x, (uint32_t)(x >> 32), (uint32_t)y, (uint32_t)(y >> 32)};
}

// out[i] = the codec's word of in[i] (DEC: the key of the word in[i]), n elements of W bytes, both
// arrays as dwords.  out may be in (in place: a lane reads its 16 bytes before it writes them), so
// neither is __restrict__.
template <int KC, int W, bool DEC>
__device__ __forceinline__ void keys_code_body(const uint32_t *in, uint32_t *out, uint64_t n) {
    using C = kc::Codec<KC>;
    constexpr int E = 16 / W;  // elements per lane and step
    constexpr int D = W / 4;   // dwords per element
    const uint64_t groups = n / E;
    const uint64_t stride = (uint64_t)gridDim.x * NT;
    const uint64_t t = (uint64_t)blockIdx.x * NT + threadIdx.x;
    for (uint64_t g = t; g < groups; g += stride) {
        const u4_a4 v = *reinterpret_cast<const u4_a4 *>(in + 4 * g);
        __builtin_nontemporal_store(code16<KC, W, DEC>(v), reinterpret_cast<u4_a4 *>(out + 4 * g));
    }
    const uint64_t i = groups * E + t;  // the n % E last elements, one each
    if (i < n) {
        if (W == 4) {
            out[i] = DEC ? C::dec(in[i]) : C::enc(in[i]);
        } else {
            const uint64_t a = join(in[i * D], in[i * D + 1]);
            const uint64_t x = DEC ? C::dec(a) : C::enc(a);
            out[i * D] = (uint32_t)x;
            out[i * D + 1] = (uint32_t)(x >> 32);
        }
    }
}

template <int KC, int W>
__global__ void __launch_bounds__(NT) keys_encode_kernel(const uint32_t *keys, uint32_t *words, uint64_t n) {
    keys_code_body<KC, W, false>(keys, words, n);
}
template <int KC, int W>
__global__ void __launch_bounds__(NT) keys_decode_kernel(const uint32_t *words, uint32_t *keys, uint64_t n) {
    keys_code_body<KC, W, true>(words, keys, n);
}

static unsigned grid_for(uint64_t lanes) {
    const uint64_t g = (lanes + NT - 1) / NT;
    return (unsigned)(g > MAXWG ? MAXWG : (g ? g : 1));
}

// A key type and flags of the ABI: the codec id and the key's width; false when either is unknown.
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

// words = enc(keys) (dec: keys = dec(words)) on s; n > 0, k.kc != 0
static int code_dev(dsort_ctx *ctx, const void *in, void *out, size_t n, KeySpec k, bool dec, hipStream_t s) {
    const uint32_t *src = static_cast<const uint32_t *>(in);
    uint32_t *dst = static_cast<uint32_t *>(out);
    const unsigned grid = grid_for(((uint64_t)n * k.bytes + 15) / 16);
    if (k.bytes == 4) {
        if (dec) {
            DSORT_KC_SWITCH(k.kc, hipLaunchKernelGGL((keys_decode_kernel<KC_, 4>), dim3(grid), dim3(NT), 0, s, src, dst,
                                                     (uint64_t)n));
        } else {
            DSORT_KC_SWITCH(k.kc, hipLaunchKernelGGL((keys_encode_kernel<KC_, 4>), dim3(grid), dim3(NT), 0, s, src, dst,
                                                     (uint64_t)n));
        }
    } else {
        if (dec) {
            DSORT_KC_SWITCH(k.kc, hipLaunchKernelGGL((keys_decode_kernel<KC_, 8>), dim3(grid), dim3(NT), 0, s, src, dst,
                                                     (uint64_t)n));
        } else {
            DSORT_KC_SWITCH(k.kc, hipLaunchKernelGGL((keys_encode_kernel<KC_, 8>), dim3(grid), dim3(NT), 0, s, src, dst,
                                                     (uint64_t)n));
        }
    }
    DSORT_HIP(ctx, hipGetLastError());
    return DSORT_OK;
}

// The host rule: the loop the kernels run, one element at a time.
template <int KC>
static void code_host_kc(const void *in, void *out, size_t n, int bytes, bool dec) {
    using C = kc::Codec<KC>;
    if (bytes == 4) {
        const uint32_t *a = static_cast<const uint32_t *>(in);
        uint32_t *o = static_cast<uint32_t *>(out);
        for (size_t i = 0; i < n; ++i) o[i] = dec ? C::dec(a[i]) : C::enc(a[i]);
    } else {
        const uint64_t *a = static_cast<const uint64_t *>(in);
        uint64_t *o = static_cast<uint64_t *>(out);
        for (size_t i = 0; i < n; ++i) o[i] = dec ? C::dec(a[i]) : C::enc(a[i]);
    }
}
static int code_host(int key_type, int flags, const void *in, void *out, size_t n, bool dec) {
    KeySpec k;
    if (!parse(key_type, flags, &k) || (n && (!in || !out))) return DSORT_EINVAL;
    if (k.kc == 0) {
        if (in != out) __builtin_memmove(out, in, n * (size_t)k.bytes);
        return DSORT_OK;
    }
    DSORT_KC_SWITCH(k.kc, code_host_kc<KC_>(in, out, n, k.bytes, dec));
    return DSORT_OK;
}

static int check_argsort(dsort_ctx *ctx, const void *keys, const void *out, size_t n) {
    if ((uint64_t)n > (1ull << 32))
        return set_err(ctx, DSORT_EINVAL, "argsort: more than 2^32 keys (a position must fit 32 bits)");
    if (n && (!keys || !out)) return set_err(ctx, DSORT_EINVAL, "null argument");
    return DSORT_OK;
}

// the argsort of either width: keys, keys_out as the integer of the key's width
static int argsort_any(dsort_ctx *ctx, const void *keys, void *keys_out, uint32_t *idx_out, size_t n, KeySpec k,
                       hipStream_t s) {
    if (k.bytes == 4)
        return pr::pairs_sort(ctx, static_cast<const int32_t *>(keys), nullptr, static_cast<int32_t *>(keys_out), idx_out,
                              n, s, k.kc);
    return p64::argsort64(ctx, static_cast<const int64_t *>(keys), static_cast<int64_t *>(keys_out), idx_out, n, s, k.kc);
}

// This rank's chunk, encoded into the context's arena on s (n == 0: the arena alone).  The arena is
// the input of the sample sort that follows, which may still read it for the context's previous
// call on another stream: the caller has opened an order bracket.
static int encode_chunk(dsort_ctx *ctx, const void *d_keys, size_t n, KeySpec k, hipStream_t s) {
    int rc = ensure(ctx, ctx->kenc, (n ? n : 1) * (size_t)k.bytes, "typed-key sample sort words");
    if (rc) return rc;
    return n ? code_dev(ctx, d_keys, ctx->kenc.p, n, k, false, s) : DSORT_OK;
}

}  // namespace ky
}  // namespace dsort

using namespace dsort;

extern "C" {

int dsort_key_encode(int key_type, int flags, const void *keys, void *words, size_t n) {
    return ky::code_host(key_type, flags, keys, words, n, false);
}

int dsort_key_decode(int key_type, int flags, const void *words, void *keys, size_t n) {
    return ky::code_host(key_type, flags, words, keys, n, true);
}

int dsort_sort_dev_keys(dsort_ctx *ctx, void *d_keys, size_t n, int key_type, int flags, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k)) return ky::bad_spec(ctx);
    if (n && !d_keys) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (k.kc == 0)
        return k.bytes == 4 ? dsort_sort_dev_i32(ctx, static_cast<int32_t *>(d_keys), n, stream)
                            : dsort_sort_dev_i64(ctx, static_cast<int64_t *>(d_keys), n, stream);
    hipStream_t s = pick_stream(ctx, stream);
    int rc;
    if (n && (rc = ky::code_dev(ctx, d_keys, d_keys, n, k, false, s))) return rc;
    // DSORT_ESTAGE (the kill stage was never reached) leaves a valid output: the decode still runs
    const int src = k.bytes == 4 ? dsort_sort_dev_i32(ctx, static_cast<int32_t *>(d_keys), n, stream)
                                 : dsort_sort_dev_i64(ctx, static_cast<int64_t *>(d_keys), n, stream);
    if (src && src != DSORT_ESTAGE) return src;
    const std::string msg = ctx->err;
    if (n && (rc = ky::code_dev(ctx, d_keys, d_keys, n, k, true, s))) return rc;
    return src ? set_err(ctx, src, msg) : DSORT_OK;
}

int dsort_sort_dev_copy_keys(dsort_ctx *ctx, const void *d_in, void *d_out, size_t n, int key_type, int flags,
                             void *stream) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k)) return ky::bad_spec(ctx);
    if (n && (!d_in || !d_out)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (k.kc == 0)
        return k.bytes == 4 ? dsort_sort_dev_copy_i32(ctx, static_cast<const int32_t *>(d_in),
                                                      static_cast<int32_t *>(d_out), n, stream)
                            : dsort_sort_dev_copy_i64(ctx, static_cast<const int64_t *>(d_in),
                                                      static_cast<int64_t *>(d_out), n, stream);
    hipStream_t s = pick_stream(ctx, stream);
    int rc;
    // the words go to d_out, which is then sorted and decoded in place: no arena
    if (n && (rc = ky::code_dev(ctx, d_in, d_out, n, k, false, s))) return rc;
    const int src = k.bytes == 4 ? dsort_sort_dev_i32(ctx, static_cast<int32_t *>(d_out), n, stream)
                                 : dsort_sort_dev_i64(ctx, static_cast<int64_t *>(d_out), n, stream);
    if (src && src != DSORT_ESTAGE) return src;
    const std::string msg = ctx->err;
    if (n && (rc = ky::code_dev(ctx, d_out, d_out, n, k, true, s))) return rc;
    return src ? set_err(ctx, src, msg) : DSORT_OK;
}

int dsort_sort_keys(dsort_ctx *ctx, void *host_keys, size_t n, int key_type, int flags) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k)) return ky::bad_spec(ctx);
    if (n && !host_keys) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (k.kc == 0)
        return k.bytes == 4 ? dsort_sort_i32(ctx, static_cast<int32_t *>(host_keys), n)
                            : dsort_sort_i64(ctx, static_cast<int64_t *>(host_keys), n);
    if (n < 2) return DSORT_OK;
    if (n > SIZE_MAX / 8) return set_err(ctx, DSORT_EINVAL, "sort: n * 8 bytes overflow size_t");
    const size_t bytes = n * (size_t)k.bytes;
    int rc = ensure(ctx, ctx->io, bytes, "staging");
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    DSORT_HIP(ctx, hipMemcpyAsync(ctx->io.p, host_keys, bytes, hipMemcpyHostToDevice, s));
    if ((rc = dsort_sort_dev_keys(ctx, ctx->io.p, n, key_type, flags, nullptr))) return rc;
    DSORT_HIP(ctx, hipMemcpyAsync(host_keys, ctx->io.p, bytes, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipStreamSynchronize(s));
    return DSORT_OK;
}

int dsort_argsort_dev_keys(dsort_ctx *ctx, const void *d_keys, void *d_keys_out, uint32_t *d_idx_out, size_t n,
                           int key_type, int flags, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k)) return ky::bad_spec(ctx);
    if (int rc = ky::check_argsort(ctx, d_keys, d_idx_out, n)) return rc;
    return ky::argsort_any(ctx, d_keys, d_keys_out, d_idx_out, n, k, pick_stream(ctx, stream));
}

int dsort_argsort_keys(dsort_ctx *ctx, const void *keys, void *keys_out, uint32_t *idx, size_t n, int key_type,
                       int flags) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k)) return ky::bad_spec(ctx);
    if (int rc = ky::check_argsort(ctx, keys, idx, n)) return rc;
    if (n == 0) return DSORT_OK;
    const size_t bytes = n * (size_t)k.bytes;
    int rc = ensure(ctx, ctx->io, bytes, "staging");
    if (rc) return rc;
    rc = ensure(ctx, ctx->io2, n * 4, "staging 2");
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    uint32_t *di = ctx->io2.as<uint32_t>();
    DSORT_HIP(ctx, hipMemcpyAsync(ctx->io.p, keys, bytes, hipMemcpyHostToDevice, s));
    const int src = ky::argsort_any(ctx, ctx->io.p, keys_out ? ctx->io.p : nullptr, di, n, k, s);
    if (src && src != DSORT_ESTAGE) return src;
    if (keys_out) DSORT_HIP(ctx, hipMemcpyAsync(keys_out, ctx->io.p, bytes, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipMemcpyAsync(idx, di, n * 4, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipStreamSynchronize(s));
    return src;
}

int dsort_sort_pairs_dev_keys(dsort_ctx *ctx, const void *d_keys_in, const uint32_t *d_vals_in, void *d_keys_out,
                              uint32_t *d_vals_out, size_t n, int key_type, int flags, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k)) return ky::bad_spec(ctx);
    if (k.bytes != 4)
        return set_err(ctx, DSORT_EINVAL, "pair sort: 4-byte key types only (an 8-byte key and a value do not fit "
                                          "one 64-bit word: dsort_sort_records_dev_keys)");
    if (n && (!d_keys_in || !d_vals_in || !d_vals_out)) return set_err(ctx, DSORT_EINVAL, "null argument");
    return pr::pairs_sort(ctx, static_cast<const int32_t *>(d_keys_in), d_vals_in, static_cast<int32_t *>(d_keys_out),
                          d_vals_out, n, pick_stream(ctx, stream), k.kc);
}

int dsort_sort_records_dev_keys(dsort_ctx *ctx, const void *d_keys, void *d_keys_out, const void *d_src, void *d_dst,
                                size_t n, int elem_bytes, int key_type, int flags, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k)) return ky::bad_spec(ctx);
    if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16)
        return set_err(ctx, DSORT_EINVAL, "record sort: elem_bytes must be 4, 8 or 16");
    if (int rc = ky::check_argsort(ctx, d_keys, d_dst, n)) return rc;
    if (n && !d_src) return set_err(ctx, DSORT_EINVAL, "null argument");
    hipStream_t s = pick_stream(ctx, stream);
    if (n == 0) return ky::argsort_any(ctx, d_keys, d_keys_out, nullptr, 0, k, s);  // (resets the statistics)
    // as dsort_sort_records_dev_i64: the argsort into an arena of the context, then the gather
    int rc = order_begin(ctx, s);
    if (rc) return rc;
    rc = ensure(ctx, ctx->a64_idx, n * 4, "record sort indices");
    if (rc) return rc;
    uint32_t *idx = ctx->a64_idx.as<uint32_t>();
    const int src = ky::argsort_any(ctx, d_keys, d_keys_out, idx, n, k, s);
    if (src && src != DSORT_ESTAGE) return src;
    const std::string msg = ctx->err;
    if ((rc = dsort_gather_dev(ctx, d_src, idx, d_dst, n, elem_bytes, stream))) return rc;
    // the gather reads the index arena behind the argsort's bracket: the call ends here
    if ((rc = order_end(ctx, s))) return rc;
    return src ? set_err(ctx, src, msg) : DSORT_OK;
}

int dsort_sample_sort_dev_keys(dsort_ctx *ctx, const void *d_keys, size_t n_local, int key_type, int flags,
                               void **d_out, size_t *n_out, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k)) return ky::bad_spec(ctx);
    if (k.kc == 0)
        return k.bytes == 4 ? dsort_sample_sort_dev_i32(ctx, static_cast<const int32_t *>(d_keys), n_local,
                                                        reinterpret_cast<int32_t **>(d_out), n_out, stream)
                            : dsort_sample_sort_dev_i64(ctx, static_cast<const int64_t *>(d_keys), n_local,
                                                        reinterpret_cast<int64_t **>(d_out), n_out, stream);
    if (!d_out || !n_out || (n_local && !d_keys)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (n_local > SIZE_MAX / 8) return set_err(ctx, DSORT_EINVAL, "sample sort: n * 8 bytes overflow size_t");
    hipStream_t s = pick_stream(ctx, stream);
    // a local failure ahead of the collectives leaves through exch_leave: the peers meet it at a gate
    int rc = order_begin(ctx, s);
    if (!rc) rc = ky::encode_chunk(ctx, d_keys, n_local, k, s);
    if (rc) return exch_leave(ctx, stream, rc);
    void *slice = nullptr;
    size_t m = 0;
    rc = k.bytes == 4 ? dsort_sample_sort_dev_i32(ctx, ctx->kenc.as<const int32_t>(), n_local,
                                                  reinterpret_cast<int32_t **>(&slice), &m, stream)
                      : dsort_sample_sort_dev_i64(ctx, ctx->kenc.as<const int64_t>(), n_local,
                                                  reinterpret_cast<int64_t **>(&slice), &m, stream);
    if (rc) return rc;
    // the slice is context-owned and ready after the stream, as it is for the integer call
    if (m && (rc = ky::code_dev(ctx, slice, slice, m, k, true, s))) return rc;
    if ((rc = order_end(ctx, s))) return rc;
    *d_out = slice;
    *n_out = m;
    return DSORT_OK;
}

int dsort_sample_argsort_dev_keys(dsort_ctx *ctx, const void *d_keys, size_t n_local, uint64_t first, int key_type,
                                  int flags, void **d_keys_out, uint32_t **d_idx_out, size_t *n_out, void *stream) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k)) return ky::bad_spec(ctx);
    if (k.kc == 0)
        return k.bytes == 4
                   ? dsort_sample_argsort_dev_i32(ctx, static_cast<const int32_t *>(d_keys), n_local, first,
                                                  reinterpret_cast<int32_t **>(d_keys_out), d_idx_out, n_out, stream)
                   : dsort_sample_argsort_dev_i64(ctx, static_cast<const int64_t *>(d_keys), n_local, first,
                                                  reinterpret_cast<int64_t **>(d_keys_out), d_idx_out, n_out, stream);
    if (first > (1ull << 32) || (uint64_t)n_local > (1ull << 32) - first)
        return set_err(ctx, DSORT_EINVAL,
                       "sample argsort: first + n_local exceeds 2^32 (a global position must fit 32 bits)");
    if (!d_idx_out || !n_out || (n_local && !d_keys)) return set_err(ctx, DSORT_EINVAL, "null argument");
    hipStream_t s = pick_stream(ctx, stream);
    int rc = order_begin(ctx, s);
    if (!rc) rc = ky::encode_chunk(ctx, d_keys, n_local, k, s);
    if (rc) return exch_leave(ctx, stream, rc);
    void *ko = nullptr;
    uint32_t *io = nullptr;
    size_t m = 0;
    // DSORT_ESTAGE of the 8-byte call: every leg has run and the outputs are valid
    const int src =
        k.bytes == 4 ? dsort_sample_argsort_dev_i32(ctx, ctx->kenc.as<const int32_t>(), n_local, first,
                                                    d_keys_out ? reinterpret_cast<int32_t **>(&ko) : nullptr, &io, &m,
                                                    stream)
                     : dsort_sample_argsort_dev_i64(ctx, ctx->kenc.as<const int64_t>(), n_local, first,
                                                    d_keys_out ? reinterpret_cast<int64_t **>(&ko) : nullptr, &io, &m,
                                                    stream);
    if (src && !(src == DSORT_ESTAGE && k.bytes == 8)) return src;
    const std::string msg = ctx->err;
    if (ko && m && (rc = ky::code_dev(ctx, ko, ko, m, k, true, s))) return rc;
    if ((rc = order_end(ctx, s))) return rc;
    if (d_keys_out) *d_keys_out = ko;
    *d_idx_out = io;
    *n_out = m;
    return src ? set_err(ctx, src, msg) : DSORT_OK;
}

// Not part of the ABI (like dsort_pairs_leg_ms): the keys-only path's encode (decode != 0: decode)
// kernel alone, d_in -> d_out (may alias) on `stream`, for scripts/bench_pairs.py --typed.
int dsort_keys_code_dev(dsort_ctx *ctx, const void *d_in, void *d_out, size_t n, int key_type, int flags, int decode,
                        void *stream) {
    if (!ctx) return DSORT_EINVAL;
    ky::KeySpec k;
    if (!ky::parse(key_type, flags, &k) || k.kc == 0) return ky::bad_spec(ctx);
    if (n == 0) return DSORT_OK;
    if (!d_in || !d_out) return set_err(ctx, DSORT_EINVAL, "null argument");
    return ky::code_dev(ctx, d_in, d_out, n, k, decode != 0, pick_stream(ctx, stream));
}

}  // extern "C"
