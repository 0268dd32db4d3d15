// dsort_api.hip -- the C ABI of libdsort (include/dsort.h): contexts and their arenas, host-buffer
// entry points, device utilities (generators, parity checks), sample-sort planning and the
// communicator's set-up and tear-down.  The multi-GPU sample sort itself: dsort_exchange.hip.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <unistd.h>

#include <algorithm>
#include <cmath>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "dsort_exch.h"

#define DSORT_STR2(x) #x
#define DSORT_STR(x) DSORT_STR2(x)
#define DSORT_VERSION_STRING "libdsort 0.1 (gfx950, HIP " DSORT_STR(HIP_VERSION_MAJOR) "." DSORT_STR(HIP_VERSION_MINOR) ")"

namespace dsort {

int set_err(dsort_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->err = msg;
    return code;
}

int hip_err(dsort_ctx *ctx, hipError_t e, const char *what) {
    std::string m = std::string(what) + ": " + hipGetErrorString(e);
    int code = (e == hipErrorOutOfMemory || e == hipErrorMemoryAllocation) ? DSORT_ENOMEM : DSORT_EHIP;
    return set_err(ctx, code, m);
}

int ensure(dsort_ctx *ctx, DevBuf &buf, size_t need, const char *what) {
    if (need <= buf.bytes && buf.p) return DSORT_OK;
    if (buf.p) {
        // the old arena may still be used by queued work on any stream of this device.  Inside the
        // bucket exchange's second level (ctx->poll_waits) the keys are still in flight on the comm
        // stream, which a dead peer never completes: a device-wide synchronize would hang there, so
        // wait for the streams that read the arenas (the sort's and the side stream) with polled
        // waits that see the abort flag and the deadline (the comm stream touches only the
        // partition and receive buffers, which never grow in that window)
        if (ctx->poll_waits) {
            int rc = sync_stream(ctx, ctx->poll_stream, "arena grow (sort stream)");
            if (!rc && ctx->side) rc = sync_stream(ctx, ctx->side, "arena grow (side stream)");
            if (rc) return rc;
        } else {
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) return hip_err(ctx, e, "hipDeviceSynchronize (arena grow)");
        }
        release_dev(ctx, buf);
    }
    size_t sz = need < 256 ? 256 : need;
    hipError_t e = hipMalloc(&buf.p, sz);
    if (e != hipSuccess) {
        buf.p = nullptr;
        return set_err(ctx, DSORT_ENOMEM, std::string("hipMalloc failed for ") + what + " (" +
                                              std::to_string(sz) + " bytes): " + hipGetErrorString(e));
    }
    buf.bytes = sz;
    return DSORT_OK;
}

void release_dev(dsort_ctx *ctx, DevBuf &buf) {
    if (buf.p && ctx->poll_waits) {
        ctx->dev_later.push_back(buf.p);
        ++ctx->deferred_n;
    } else if (buf.p) {
        (void)hipFree(buf.p);
    }
    buf.p = nullptr;
    buf.bytes = 0;
}
void release_host(dsort_ctx *ctx, HostBuf &buf) {
    if (buf.p && ctx->poll_waits) {
        ctx->host_later.push_back(buf.p);
        ++ctx->deferred_n;
    } else if (buf.p) {
        (void)hipHostFree(buf.p);
    }
    buf.p = nullptr;
    buf.bytes = 0;
}
void flush_later(dsort_ctx *ctx) {
    for (void *p : ctx->dev_later) (void)hipFree(p);
    for (void *p : ctx->host_later) (void)hipHostFree(p);
    ctx->dev_later.clear();
    ctx->host_later.clear();
}

// grow-only pinned host buffer
int ensure_host(dsort_ctx *ctx, HostBuf &buf, size_t need) {
    if (need <= buf.bytes && buf.p) return DSORT_OK;
    release_host(ctx, buf);
    if (hipHostMalloc(&buf.p, need, hipHostMallocDefault) != hipSuccess) {
        buf.p = nullptr;
        return set_err(ctx, DSORT_ENOMEM, "hipHostMalloc failed (" + std::to_string(need) + " bytes)");
    }
    buf.bytes = need;
    return DSORT_OK;
}

int LegClock::wait_last(dsort_ctx *ctx) const {
    DSORT_HIP(ctx, hipEventSynchronize(ev[n - 1]));
    return DSORT_OK;
}
int LegClock::elapsed(dsort_ctx *ctx, int a, int b, double *ms) const {
    float f = 0;
    DSORT_HIP(ctx, hipEventElapsedTime(&f, ev[a], ev[b]));
    *ms = f;
    return DSORT_OK;
}

hipStream_t pick_stream(dsort_ctx *ctx, void *stream) {
    if (stream == DSORT_NULL_STREAM) return static_cast<hipStream_t>(nullptr);
    return stream ? static_cast<hipStream_t>(stream) : ctx->stream;
}

// ------------------------------------------------------------------ utility kernels ------
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void gen_uniform_i32_kernel(int32_t *out, uint64_t n, uint64_t seed) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = (int32_t)(uint32_t)(splitmix64(seed + i) >> 32);
}

__global__ void gen_uniform_i64_kernel(int64_t *out, uint64_t n, uint64_t seed) {
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        out[i] = (int64_t)splitmix64(seed + i);
}

// Truncated continuous power law over ranks [1, 2^24], exponent s = 1.2:
// rank = floor((1 + u*((2^24+1)^(1-s) - 1))^(1/(1-s))).  Heavy head (rank 1 ~ 13% of keys).
__global__ void gen_zipf_i64_kernel(int64_t *out, uint64_t n, uint64_t seed) {
    const double s = 1.2, nr = 16777216.0;
    const double e = 1.0 - s;
    const double top = pow(nr + 1.0, e) - 1.0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const double u = (double)(splitmix64(seed + i) >> 11) * 0x1.0p-53;
        double r = floor(pow(1.0 + u * top, 1.0 / e));
        if (r < 1.0) r = 1.0;
        if (r > nr) r = nr;
        out[i] = (int64_t)((uint64_t)r * 0x9E3779B97F4A7C15ull);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) fingerprint_kernel(const T *keys, uint64_t n,
                                                          unsigned long long *acc) {
    uint64_t s = 0, x = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint64_t k = sizeof(T) == 4 ? (uint64_t)(uint32_t)keys[i] : (uint64_t)keys[i];
        s += splitmix64(k);
        x ^= splitmix64(k ^ 0xD1B54A32D192ED03ull);
    }
    __shared__ uint64_t ss[256], sx[256];
    ss[threadIdx.x] = s;
    sx[threadIdx.x] = x;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            ss[threadIdx.x] += ss[threadIdx.x + w];
            sx[threadIdx.x] ^= sx[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        atomicAdd(&acc[0], (unsigned long long)ss[0]);
        atomicXor(&acc[1], (unsigned long long)sx[0]);
    }
}

template <typename T>
__global__ void __launch_bounds__(256) descents_kernel(const T *keys, uint64_t n,
                                                       unsigned long long *acc) {
    unsigned long long c = 0;
    const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x + 1; i < n; i += stride)
        c += keys[i - 1] > keys[i] ? 1 : 0;
    __shared__ unsigned long long sc[256];
    sc[threadIdx.x] = c;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sc[threadIdx.x] += sc[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) atomicAdd(&acc[2], sc[0]);
}

static unsigned grid_for(uint64_t n, int per_block) {
    uint64_t g = (n + per_block - 1) / per_block;
    if (g > 4096) g = 4096;
    if (g == 0) g = 1;
    return (unsigned)g;
}

template <typename T>
int fingerprint_launch(dsort_ctx *ctx, const T *keys, uint64_t n, unsigned long long *acc, hipStream_t s) {
    hipLaunchKernelGGL((fingerprint_kernel<T>), dim3(grid_for(n, 256 * 8)), dim3(256), 0, s, keys, n, acc);
    DSORT_HIP(ctx, hipGetLastError());
    return DSORT_OK;
}
template int fingerprint_launch<int32_t>(dsort_ctx *, const int32_t *, uint64_t, unsigned long long *, hipStream_t);
template int fingerprint_launch<int64_t>(dsort_ctx *, const int64_t *, uint64_t, unsigned long long *, hipStream_t);

template <typename T>
static int fingerprint_t(dsort_ctx *ctx, const T *d, size_t n, uint64_t *sum, uint64_t *xr,
                         uint64_t *desc, bool want_desc) {
    if (!ctx) return DSORT_EINVAL;
    hipStream_t s = ctx->stream;
    DSORT_HIP(ctx, hipMemsetAsync(ctx->red.p, 0, 64, s));
    if (n) {
        auto *red = ctx->red.as<unsigned long long>();
        if (!want_desc) {
            if (int rc = fingerprint_launch<T>(ctx, d, n, red, s)) return rc;
        } else {
            hipLaunchKernelGGL((descents_kernel<T>), dim3(grid_for(n, 256 * 8)), dim3(256), 0, s, d, (uint64_t)n, red);
            DSORT_HIP(ctx, hipGetLastError());
        }
    }
    const uint64_t *h = ctx->red_host.as<uint64_t>();
    DSORT_HIP(ctx, hipMemcpyAsync(ctx->red_host.p, ctx->red.p, 64, hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipStreamSynchronize(s));
    if (sum) *sum = h[0];
    if (xr) *xr = h[1];
    if (desc) *desc = h[2];
    return DSORT_OK;
}

// ------------------------------------------------------------------ host entry points ---
template <typename T>
static int sort_host(dsort_ctx *ctx, T *host, size_t n) {
    if (!ctx || (!host && n)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (n < 2) return DSORT_OK;
    int rc = ensure(ctx, ctx->io, n * sizeof(T), "staging");
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    T *d = ctx->io.as<T>();
    DSORT_HIP(ctx, hipMemcpyAsync(d, host, n * sizeof(T), hipMemcpyHostToDevice, s));
    rc = sort_device<T>(ctx, d, d, n, s, true);
    if (rc) return rc;
    DSORT_HIP(ctx, hipMemcpyAsync(host, d, n * sizeof(T), hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipStreamSynchronize(s));
    return DSORT_OK;
}

template <typename T>
static int merge_host(dsort_ctx *ctx, const T *const runs[], const size_t lens[], int k, T *out) {
    if (!ctx || k < 0 || (k > 0 && (!runs || !lens))) return set_err(ctx, DSORT_EINVAL, "bad argument");
    size_t n = 0;
    for (int j = 0; j < k; ++j) {
        if (lens[j] && !runs[j]) return set_err(ctx, DSORT_EINVAL, "null run");
        n += lens[j];
    }
    if (n == 0) return DSORT_OK;
    if (!out) return set_err(ctx, DSORT_EINVAL, "null output");
    int rc = ensure(ctx, ctx->io, n * sizeof(T), "staging");
    if (rc) return rc;
    rc = ensure(ctx, ctx->io2, n * sizeof(T), "staging 2");
    if (rc) return rc;
    hipStream_t s = ctx->stream;
    T *din = ctx->io.as<T>(), *dout = ctx->io2.as<T>();
    size_t off = 0;
    for (int j = 0; j < k; ++j) {
        if (lens[j])
            DSORT_HIP(ctx, hipMemcpyAsync(din + off, runs[j], lens[j] * sizeof(T),
                                          hipMemcpyHostToDevice, s));
        off += lens[j];
    }
    rc = merge_device<T>(ctx, din, lens, k, dout, s);
    if (rc) return rc;
    DSORT_HIP(ctx, hipMemcpyAsync(out, dout, n * sizeof(T), hipMemcpyDeviceToHost, s));
    DSORT_HIP(ctx, hipStreamSynchronize(s));
    return DSORT_OK;
}

// ------------------------------------------------------------------ planning (host) -----
template <typename T>
static int plan_splitters(int nranks, int s, const T *samples, const uint64_t *idx, T *sv,
                          int32_t *sr, uint64_t *si) {
    if (nranks < 1 || s < 1 || !samples || !idx) return DSORT_EINVAL;
    if (nranks == 1) return DSORT_OK;
    if (!sv || !sr || !si) return DSORT_EINVAL;
    struct S {
        T v;
        int32_t r;
        uint64_t i;
    };
    std::vector<S> all((size_t)nranks * s);
    for (int r = 0; r < nranks; ++r)
        for (int j = 0; j < s; ++j) all[(size_t)r * s + j] = S{samples[(size_t)r * s + j], r, idx[(size_t)r * s + j]};
    std::sort(all.begin(), all.end(), [](const S &a, const S &b) {
        if (a.v != b.v) return a.v < b.v;
        if (a.r != b.r) return a.r < b.r;
        return a.i < b.i;
    });
    // splitter q sits at the q-th P-quantile of the merged sample (PSRS with oversampling s)
    const size_t m = all.size();
    for (int q = 1; q < nranks; ++q) {
        size_t pos = (size_t)q * m / (size_t)nranks;
        if (pos >= m) pos = m - 1;
        sv[q - 1] = all[pos].v;
        sr[q - 1] = all[pos].r;
        si[q - 1] = all[pos].i;
    }
    return DSORT_OK;
}

template <typename T>
static int plan_cuts(const T *sorted, size_t n, int my_rank, int nranks, const T *sv,
                     const int32_t *sr, const uint64_t *si, uint64_t *cuts) {
    if (nranks < 1 || !cuts || (n && !sorted)) return DSORT_EINVAL;
    cuts[0] = 0;
    cuts[nranks] = n;
    for (int q = 0; q + 1 < nranks; ++q) {
        uint64_t pos;
        if (sr[q] == my_rank) {
            pos = si[q] < n ? si[q] : n;
        } else {
            const bool upper = my_rank < sr[q];
            const T *p = upper ? std::upper_bound(sorted, sorted + n, sv[q])
                               : std::lower_bound(sorted, sorted + n, sv[q]);
            pos = (uint64_t)(p - sorted);
        }
        cuts[q + 1] = pos;
    }
    return DSORT_OK;
}

}  // namespace dsort

using namespace dsort;

// ======================================================================== C ABI =========
extern "C" {

const char *dsort_version(void) { return DSORT_VERSION_STRING; }

int dsort_init(dsort_ctx **out, int device) {
    if (!out) return DSORT_EINVAL;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return DSORT_ENODEV;
    if (device < 0 || device >= count) return DSORT_ENODEV;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device) != hipSuccess) return DSORT_ENODEV;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return DSORT_ENODEV;
    dsort_ctx *ctx = new (std::nothrow) dsort_ctx();
    if (!ctx) return DSORT_ENOMEM;
    ctx->device = device;
    if (hipSetDevice(device) != hipSuccess ||
        hipStreamCreateWithFlags(&ctx->stream.h, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return DSORT_EHIP;
    }
    if (ensure(ctx, ctx->red, 64, "reduction accumulators") || ensure_host(ctx, ctx->red_host, 64)) {
        dsort_finalize(ctx);
        return DSORT_ENOMEM;
    }
    ctx->ev_ok = true;
    for (auto &e : ctx->ev)
        if (hipEventCreate(&e.h) != hipSuccess) ctx->ev_ok = false;
    for (auto &e : ctx->kev)
        if (hipEventCreate(&e.h) != hipSuccess) ctx->ev_ok = false;
    ctx->ev_created = ctx->ev_ok;
    *out = ctx;
    return DSORT_OK;
}

int dsort_finalize(dsort_ctx *ctx) {
    if (!ctx) return DSORT_EINVAL;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm) {
        ncclCommAbort(ctx->comm);  // peers may be gone: never wait for them here
        ctx->comm = nullptr;
    }
    ctx->poll_waits = false;
    flush_later(ctx);
    delete ctx;  // (its arenas, events and streams free themselves: dsort_internal.h)
    return DSORT_OK;
}

const char *dsort_last_error(const dsort_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int dsort_set_option(dsort_ctx *ctx, int option, int64_t v) {
    if (!ctx) return DSORT_EINVAL;
    dsort_opts &o = ctx->opt;
    switch (option) {
        case DSORT_OPT_BUCKETS:
            if (v < -1 || v == 1 || v > 1024) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_BUCKETS: -1, 0 or 2..1024");
            o.buckets = v;
            return DSORT_OK;
        case DSORT_OPT_BUCKET_KEYS:
            if (v < 1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_BUCKET_KEYS: >= 1");
            o.bucket_keys = v;
            return DSORT_OK;
        case DSORT_OPT_BUCKET_OVERSAMPLE:
            if (v < 1 || v > 4096) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_BUCKET_OVERSAMPLE: 1..4096");
            o.bucket_os = v;
            return DSORT_OK;
        case DSORT_OPT_MAX_FANIN_LOG2:
            if (v != -1 && (v < 1 || v > kMaxLogF)) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_MAX_FANIN_LOG2: -1 or 1..5");
            o.max_logf = v;
            return DSORT_OK;
        case DSORT_OPT_KILL_AFTER_STAGE:
            if (v < -1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_KILL_AFTER_STAGE: -1 or a stage index");
            o.kill_after_pass = v;
            return DSORT_OK;
        case DSORT_OPT_KILL_IN_EXCHANGE:
            if (v != -1 && v != 1 && v != 2) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_KILL_IN_EXCHANGE: -1, 1 or 2");
            o.kill_in_exchange = v;
            return DSORT_OK;
        case DSORT_OPT_SUB_KEYS:
            if (v < -1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_SUB_KEYS: -1, 0 or >= 1");
            ctx->opt.sub_keys = v;
            return DSORT_OK;
        case DSORT_OPT_SUB_OVERSAMPLE:
            if (v != -1 && (v < 1 || v > 64)) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_SUB_OVERSAMPLE: -1 or 1..64");
            ctx->opt.sub_os = v;
            return DSORT_OK;
        case DSORT_OPT_SUB_GATHER:
            if (v != 0 && v != 1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_SUB_GATHER: 0 or 1");
            ctx->opt.sub_gather = v;
            return DSORT_OK;
        case DSORT_OPT_COMM_TIMEOUT_MS:
            if (v < 0) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_COMM_TIMEOUT_MS: >= 0");
            o.comm_timeout_ms = v;
            return DSORT_OK;
        case DSORT_OPT_TEST_HOLD_EXCHANGE:
            if (v != 0 && v != 1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_TEST_HOLD_EXCHANGE: 0 or 1");
            o.test_hold_exchange = v;
            return DSORT_OK;
        case DSORT_OPT_TEST_FAIL_EXCHANGE:
            if (v < -1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_TEST_FAIL_EXCHANGE: -1 or a collective index");
            o.test_fail_exchange = v;
            return DSORT_OK;
        case DSORT_OPT_STAGE_TIMING:
            if (v != 0 && v != 1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_STAGE_TIMING: 0 or 1");
            o.stage_timing = v;
            ctx->ev_ok = ctx->ev_created && v != 0;
            return DSORT_OK;
        case DSORT_OPT_TEST_TILE_CAP:
            if (v < 0) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_TEST_TILE_CAP: >= 0");
            o.test_tile_cap = v;
            return DSORT_OK;
        case DSORT_OPT_TEST_WAVE_FENCE:
            if (v < 0 || v > 2) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_TEST_WAVE_FENCE: 0, 1 or 2");
            o.test_wave_fence = v;
            return DSORT_OK;
        case DSORT_OPT_ARGSORT_WIDE:
            if (v != 0 && v != 1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_ARGSORT_WIDE: 0 or 1");
            o.argsort_wide = v;
            return DSORT_OK;
        case DSORT_OPT_TEST_FAIL_LEG:
            if (v < -1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_TEST_FAIL_LEG: -1 or a leg index");
            o.test_fail_leg = v;
            return DSORT_OK;
        case DSORT_OPT_TOPK_PATH:
            if (v < -1 || v > 1) return set_err(ctx, DSORT_EINVAL, "DSORT_OPT_TOPK_PATH: -1, 0 or 1");
            o.topk_path = v;
            return DSORT_OK;
        default:
            return set_err(ctx, DSORT_EINVAL, "unknown option " + std::to_string(option));
    }
}

int dsort_get_option(const dsort_ctx *ctx, int option, int64_t *v) {
    if (!ctx || !v) return DSORT_EINVAL;
    const dsort_opts &o = ctx->opt;
    switch (option) {
        case DSORT_OPT_BUCKETS: *v = o.buckets; return DSORT_OK;
        case DSORT_OPT_BUCKET_KEYS: *v = o.bucket_keys; return DSORT_OK;
        case DSORT_OPT_BUCKET_OVERSAMPLE: *v = o.bucket_os; return DSORT_OK;
        case DSORT_OPT_MAX_FANIN_LOG2: *v = o.max_logf; return DSORT_OK;
        case DSORT_OPT_KILL_AFTER_STAGE: *v = o.kill_after_pass; return DSORT_OK;
        case DSORT_OPT_KILL_IN_EXCHANGE: *v = o.kill_in_exchange; return DSORT_OK;
        case DSORT_OPT_COMM_TIMEOUT_MS: *v = o.comm_timeout_ms; return DSORT_OK;
        case DSORT_OPT_TEST_HOLD_EXCHANGE: *v = o.test_hold_exchange; return DSORT_OK;
        case DSORT_OPT_TEST_FAIL_EXCHANGE: *v = o.test_fail_exchange; return DSORT_OK;
        case DSORT_OPT_STAGE_TIMING: *v = o.stage_timing; return DSORT_OK;
        case DSORT_OPT_TEST_TILE_CAP: *v = o.test_tile_cap; return DSORT_OK;
        case DSORT_OPT_TEST_WAVE_FENCE: *v = o.test_wave_fence; return DSORT_OK;
        case DSORT_OPT_SUB_KEYS: *v = o.sub_keys; return DSORT_OK;
        case DSORT_OPT_SUB_OVERSAMPLE: *v = o.sub_os; return DSORT_OK;
        case DSORT_OPT_SUB_GATHER: *v = o.sub_gather; return DSORT_OK;
        case DSORT_OPT_ARGSORT_WIDE: *v = o.argsort_wide; return DSORT_OK;
        case DSORT_OPT_TEST_FAIL_LEG: *v = o.test_fail_leg; return DSORT_OK;
        case DSORT_OPT_TOPK_PATH: *v = o.topk_path; return DSORT_OK;
        default: return DSORT_EINVAL;
    }
}

int dsort_get_stats(const dsort_ctx *cctx, dsort_stats *out) {
    if (!cctx || !out) return DSORT_EINVAL;
    dsort_ctx *ctx = const_cast<dsort_ctx *>(cctx);
    *out = ctx->stats;
    if (!ctx->ev_ok) return DSORT_OK;
    if (hipStreamSynchronize(ctx->last_stream) != hipSuccess) return DSORT_EHIP;
    float ms = 0;
    auto el = [&](StageEv a, StageEv b) -> double {
        if (!(ctx->ev_mask & (1u << a)) || !(ctx->ev_mask & (1u << b))) return 0.0;
        return hipEventElapsedTime(&ms, ctx->ev[a], ctx->ev[b]) == hipSuccess ? (double)ms : 0.0;
    };
    out->merge_kernel_ms = 0;
    out->merge_kernel_launches = 0;
    for (int i = 0; i + 1 < ctx->kev_used; i += 2) {
        if (hipEventQuery(ctx->kev[i + 1]) != hipSuccess) break;
        if (hipEventElapsedTime(&ms, ctx->kev[i], ctx->kev[i + 1]) == hipSuccess) {
            out->merge_kernel_ms += ms;
            out->merge_kernel_launches += 1;
        }
    }
    auto wave0 = [](StageEv e) { return StageEv(e + kWave0Offset); };  // (the bucket exchange's first wave)
    out->block_sort_ms = el(kEvStart, kEvTileSortDone);
    out->merge_ms = el(kEvTileSortDone, kEvLocalDone);
    out->tile_sort_kernel_ms = el(kEvTile0, kEvTile1) + el(wave0(kEvTile0), wave0(kEvTile1));
    out->partition_ms = el(kEvStart, kEvTile0);
    out->bucket_hist_ms = el(kEvHist0, kEvHist1);
    out->bucket_scatter_ms = el(kEvScatter0, kEvScatter1);
    out->sub_partition_ms = el(kEvSub0, kEvSub1) + el(wave0(kEvSub0), wave0(kEvSub1));
    if (ctx->ev_mask & (1u << kEvFinalDone)) {
        out->exchange_ms = el(kEvLocalDone, kEvExchangeDone);
        out->final_merge_ms = el(kEvExchangeDone, kEvFinalDone);
        out->total_ms = el(kEvStart, kEvFinalDone);
        out->alltoall_ms = el(kEvAllToAll0, kEvAllToAll1);
    } else {
        out->total_ms = el(kEvStart, kEvLocalDone);
    }
    return DSORT_OK;
}

int dsort_synchronize(dsort_ctx *ctx) {
    if (!ctx) return DSORT_EINVAL;
    DSORT_HIP(ctx, hipStreamSynchronize(ctx->last_stream));
    DSORT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return DSORT_OK;
}

int dsort_sort_stages(const dsort_ctx *ctx, size_t n, int key_bytes, int *stages) {
    if (!stages || (key_bytes != 4 && key_bytes != 8)) return DSORT_EINVAL;
    static const dsort_opts defaults{};
    *stages = sort_stages(ctx ? ctx->opt : defaults, n, key_bytes);
    return DSORT_OK;
}

int dsort_sample_sort_stages(const dsort_ctx *ctx, size_t n_total, int nranks, int rank, int key_bytes,
                             int *stages) {
    if (!stages || nranks < 1 || rank < 0 || rank >= nranks || (key_bytes != 4 && key_bytes != 8)) return DSORT_EINVAL;
    static const dsort_opts defaults{};
    const dsort_opts &o = ctx ? ctx->opt : defaults;
    std::vector<uint64_t> n_of(nranks);
    for (int r = 0; r < nranks; ++r) n_of[r] = n_total / nranks + ((uint64_t)r < n_total % nranks ? 1 : 0);
    BxPlan pl;
    *stages = bx_make_plan(o, nranks, rank, n_of.data(), key_bytes, pl) ? 3 : sort_stages(o, n_of[rank], key_bytes);
    return DSORT_OK;
}

int dsort_sort_i32(dsort_ctx *ctx, int32_t *keys, size_t n) { return sort_host<int32_t>(ctx, keys, n); }
int dsort_sort_i64(dsort_ctx *ctx, int64_t *keys, size_t n) { return sort_host<int64_t>(ctx, keys, n); }

int dsort_sort_dev_i32(dsort_ctx *ctx, int32_t *d, size_t n, void *stream) {
    if (!ctx || (n && !d)) return set_err(ctx, DSORT_EINVAL, "null argument");
    return sort_device<int32_t>(ctx, d, d, n, pick_stream(ctx, stream), true);
}
int dsort_sort_dev_i64(dsort_ctx *ctx, int64_t *d, size_t n, void *stream) {
    if (!ctx || (n && !d)) return set_err(ctx, DSORT_EINVAL, "null argument");
    return sort_device<int64_t>(ctx, d, d, n, pick_stream(ctx, stream), true);
}
int dsort_sort_dev_copy_i32(dsort_ctx *ctx, const int32_t *in, int32_t *out, size_t n, void *stream) {
    if (!ctx || (n && (!in || !out))) return set_err(ctx, DSORT_EINVAL, "null argument");
    return sort_device<int32_t>(ctx, in, out, n, pick_stream(ctx, stream), true);
}
int dsort_sort_dev_copy_i64(dsort_ctx *ctx, const int64_t *in, int64_t *out, size_t n, void *stream) {
    if (!ctx || (n && (!in || !out))) return set_err(ctx, DSORT_EINVAL, "null argument");
    return sort_device<int64_t>(ctx, in, out, n, pick_stream(ctx, stream), true);
}

int dsort_merge_i32(dsort_ctx *ctx, const int32_t *const runs[], const size_t lens[], int k, int32_t *out) {
    return merge_host<int32_t>(ctx, runs, lens, k, out);
}
int dsort_merge_i64(dsort_ctx *ctx, const int64_t *const runs[], const size_t lens[], int k, int64_t *out) {
    return merge_host<int64_t>(ctx, runs, lens, k, out);
}
int dsort_merge_dev_i32(dsort_ctx *ctx, const int32_t *d_in, const size_t lens[], int k, int32_t *d_out,
                        void *stream) {
    if (!ctx || k < 0 || (k && !lens)) return set_err(ctx, DSORT_EINVAL, "bad argument");
    return merge_device<int32_t>(ctx, d_in, lens, k, d_out, pick_stream(ctx, stream));
}
int dsort_merge_dev_i64(dsort_ctx *ctx, const int64_t *d_in, const size_t lens[], int k, int64_t *d_out,
                        void *stream) {
    if (!ctx || k < 0 || (k && !lens)) return set_err(ctx, DSORT_EINVAL, "bad argument");
    return merge_device<int64_t>(ctx, d_in, lens, k, d_out, pick_stream(ctx, stream));
}

int dsort_comm_unique_id(char id[DSORT_UNIQUE_ID_BYTES]) {
    static_assert(sizeof(ncclUniqueId) == DSORT_UNIQUE_ID_BYTES, "ncclUniqueId size");
    if (!id) return DSORT_EINVAL;
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return DSORT_ECOMM;
    memcpy(id, &u, sizeof(u));
    return DSORT_OK;
}

int dsort_comm_init(dsort_ctx *ctx, int nranks, int rank, const char id[DSORT_UNIQUE_ID_BYTES]) {
    if (!ctx || !id || nranks < 1 || rank < 0 || rank >= nranks) return set_err(ctx, DSORT_EINVAL, "bad argument");
    if (ctx->comm || ctx->has_transport) return set_err(ctx, DSORT_EINVAL, "communicator already initialised");
    DSORT_HIP(ctx, hipSetDevice(ctx->device));
    std::unique_lock<std::mutex> lock(ctx->comm_mu);
    ctx->abort_req.store(0);  // a flag left by the previous communicator's abort
    ncclUniqueId u;
    memcpy(&u, id, sizeof(u));
    ncclComm_t c = nullptr;
    // non-blocking communicator: no RCCL call may block on a dead peer (exch_wait polls instead)
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    ncclResult_t r = ncclCommInitRankConfig(&c, nranks, u, rank, &cfg);
    const double deadline = ctx->opt.comm_timeout_ms > 0 ? tx_now_ms() + (double)ctx->opt.comm_timeout_ms : 0.0;
    while (r == ncclInProgress && c) {
        ncclCommGetAsyncError(c, &r);
        if (r != ncclInProgress) break;
        if (deadline > 0 && tx_now_ms() > deadline) {
            ncclCommAbort(c);
            return set_err(ctx, DSORT_ETIMEOUT, "ncclCommInitRankConfig: peers did not join before the deadline");
        }
        if (ctx->abort_req.load()) {
            ncclCommAbort(c);
            ctx->abort_req.store(0);
            return set_err(ctx, DSORT_ECOMM, "ncclCommInitRankConfig: aborted by dsort_comm_abort");
        }
        usleep(50);
    }
    if (r != ncclSuccess) {
        if (c) ncclCommAbort(c);
        return set_err(ctx, DSORT_ECOMM, std::string("ncclCommInitRankConfig: ") + ncclGetErrorString(r) +
                                             " (RCCL needs one GPU per rank; ranks sharing a GPU use "
                                             "dsort_comm_init_transport)");
    }
    ctx->comm = c;
    ctx->nranks = nranks;
    ctx->rank = rank;
    return DSORT_OK;
}

int dsort_comm_init_transport(dsort_ctx *ctx, int nranks, int rank, const dsort_transport *t) {
    if (!ctx || !t || !t->allgather || !t->alltoallv || nranks < 1 || rank < 0 || rank >= nranks)
        return set_err(ctx, DSORT_EINVAL, "bad argument");
    std::unique_lock<std::mutex> lock(ctx->comm_mu);
    if (ctx->comm || ctx->has_transport) return set_err(ctx, DSORT_EINVAL, "communicator already initialised");
    ctx->abort_req.store(0);  // a flag left by the previous communicator's abort
    ctx->transport = *t;
    ctx->has_transport = true;
    ctx->nranks = nranks;
    ctx->rank = rank;
    return DSORT_OK;
}

int dsort_comm_deadline_ms(const dsort_ctx *ctx, int64_t *remaining_ms) {
    if (!ctx || !remaining_ms) return DSORT_EINVAL;
    *remaining_ms = ctx->tx ? ctx->tx->remaining_ms() : -1;
    return DSORT_OK;
}

int dsort_comm_abort(dsort_ctx *ctx) {
    if (!ctx) return DSORT_EINVAL;
    std::unique_lock<std::mutex> lock(ctx->comm_mu, std::try_to_lock);
    if (!lock.owns_lock()) {  // an exchange is running on another thread: it aborts itself
        ctx->abort_req.store(1);
        return DSORT_OK;
    }
    abort_comm_locked(ctx);
    ctx->abort_req.store(0);
    return DSORT_OK;
}

int dsort_comm_destroy(dsort_ctx *ctx) {
    if (!ctx) return DSORT_EINVAL;
    std::unique_lock<std::mutex> lock(ctx->comm_mu);
    ctx->has_transport = false;
    if (ctx->comm) {
        (void)hipStreamSynchronize(ctx->stream);
        // non-blocking communicator: finalize, wait for it (never longer than the exchange
        // deadline, 10 s without one, or an abort request: a peer that died after its last
        // collective must not hold this rank in shutdown), then destroy -- else abort
        const double limit = ctx->opt.comm_timeout_ms > 0 ? (double)ctx->opt.comm_timeout_ms : 10000.0;
        const double deadline = tx_now_ms() + limit;
        ncclResult_t r = ncclCommFinalize(ctx->comm);
        while (r == ncclInProgress) {
            ncclCommGetAsyncError(ctx->comm, &r);
            if (r != ncclInProgress) break;
            if (ctx->abort_req.load() || tx_now_ms() > deadline) break;
            usleep(50);
        }
        if (r == ncclSuccess) ncclCommDestroy(ctx->comm);
        else ncclCommAbort(ctx->comm);
    }
    ctx->comm = nullptr;
    ctx->nranks = 1;
    ctx->rank = 0;
    return DSORT_OK;
}

int dsort_sample_sort_dev_i32(dsort_ctx *ctx, const int32_t *d, size_t n, int32_t **o, size_t *no, void *st) {
    return sample_sort_entry<int32_t>(ctx, d, n, o, no, st, false);
}
int dsort_sample_sort_dev_i64(dsort_ctx *ctx, const int64_t *d, size_t n, int64_t **o, size_t *no, void *st) {
    return sample_sort_entry<int64_t>(ctx, d, n, o, no, st, false);
}
int dsort_sample_merge_dev_i32(dsort_ctx *ctx, const int32_t *d, size_t n, int32_t **o, size_t *no, void *st) {
    return sample_sort_entry<int32_t>(ctx, d, n, o, no, st, true);
}
int dsort_sample_merge_dev_i64(dsort_ctx *ctx, const int64_t *d, size_t n, int64_t **o, size_t *no, void *st) {
    return sample_sort_entry<int64_t>(ctx, d, n, o, no, st, true);
}

int dsort_plan_sample_positions(size_t n, int s, uint64_t *idx) {
    if (s < 1 || !idx) return DSORT_EINVAL;
    for (int j = 0; j < s; ++j) {
        uint64_t p = n ? (uint64_t)(j + 1) * (uint64_t)n / (uint64_t)(s + 1) : 0;
        if (n && p >= n) p = n - 1;
        idx[j] = p;
    }
    return DSORT_OK;
}

int dsort_plan_splitters_i32(int nranks, int s, const int32_t *samples, const uint64_t *idx,
                             int32_t *sv, int32_t *sr, uint64_t *si) {
    return plan_splitters<int32_t>(nranks, s, samples, idx, sv, sr, si);
}
int dsort_plan_splitters_i64(int nranks, int s, const int64_t *samples, const uint64_t *idx,
                             int64_t *sv, int32_t *sr, uint64_t *si) {
    return plan_splitters<int64_t>(nranks, s, samples, idx, sv, sr, si);
}
int dsort_plan_cuts_i32(const int32_t *sorted, size_t n, int my_rank, int nranks, const int32_t *sv,
                        const int32_t *sr, const uint64_t *si, uint64_t *cuts) {
    return plan_cuts<int32_t>(sorted, n, my_rank, nranks, sv, sr, si, cuts);
}
int dsort_plan_cuts_i64(const int64_t *sorted, size_t n, int my_rank, int nranks, const int64_t *sv,
                        const int32_t *sr, const uint64_t *si, uint64_t *cuts) {
    return plan_cuts<int64_t>(sorted, n, my_rank, nranks, sv, sr, si, cuts);
}

int dsort_gen_uniform_i32(dsort_ctx *ctx, int32_t *d, size_t n, uint64_t seed, uint64_t first, void *stream) {
    if (!ctx || (n && !d)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (!n) return DSORT_OK;
    hipLaunchKernelGGL(gen_uniform_i32_kernel, dim3(grid_for(n, 256 * 4)), dim3(256), 0, pick_stream(ctx, stream), d,
                       (uint64_t)n, seed + first);
    DSORT_HIP(ctx, hipGetLastError());
    return DSORT_OK;
}
int dsort_gen_uniform_i64(dsort_ctx *ctx, int64_t *d, size_t n, uint64_t seed, uint64_t first, void *stream) {
    if (!ctx || (n && !d)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (!n) return DSORT_OK;
    hipLaunchKernelGGL(gen_uniform_i64_kernel, dim3(grid_for(n, 256 * 4)), dim3(256), 0, pick_stream(ctx, stream), d,
                       (uint64_t)n, seed + first);
    DSORT_HIP(ctx, hipGetLastError());
    return DSORT_OK;
}
int dsort_gen_zipf_i64(dsort_ctx *ctx, int64_t *d, size_t n, uint64_t seed, uint64_t first, void *stream) {
    if (!ctx || (n && !d)) return set_err(ctx, DSORT_EINVAL, "null argument");
    if (!n) return DSORT_OK;
    hipLaunchKernelGGL(gen_zipf_i64_kernel, dim3(grid_for(n, 256 * 4)), dim3(256), 0, pick_stream(ctx, stream), d,
                       (uint64_t)n, seed + first);
    DSORT_HIP(ctx, hipGetLastError());
    return DSORT_OK;
}

int dsort_fingerprint_i32(dsort_ctx *ctx, const int32_t *d, size_t n, uint64_t *sum, uint64_t *xr) {
    return fingerprint_t<int32_t>(ctx, d, n, sum, xr, nullptr, false);
}
int dsort_fingerprint_i64(dsort_ctx *ctx, const int64_t *d, size_t n, uint64_t *sum, uint64_t *xr) {
    return fingerprint_t<int64_t>(ctx, d, n, sum, xr, nullptr, false);
}
int dsort_count_descents_i32(dsort_ctx *ctx, const int32_t *d, size_t n, uint64_t *count) {
    return fingerprint_t<int32_t>(ctx, d, n, nullptr, nullptr, count, true);
}
int dsort_count_descents_i64(dsort_ctx *ctx, const int64_t *d, size_t n, uint64_t *count) {
    return fingerprint_t<int64_t>(ctx, d, n, nullptr, nullptr, count, true);
}

int dsort_dev_alloc(dsort_ctx *ctx, void **p, size_t bytes) {
    if (!ctx || !p) return DSORT_EINVAL;
    DSORT_HIP(ctx, hipMalloc(p, bytes ? bytes : 1));
    return DSORT_OK;
}
int dsort_dev_free(dsort_ctx *ctx, void *p) {
    if (!ctx) return DSORT_EINVAL;
    if (p) DSORT_HIP(ctx, hipFree(p));
    return DSORT_OK;
}
int dsort_copy_h2d(dsort_ctx *ctx, void *d, const void *h, size_t bytes) {
    if (!ctx) return DSORT_EINVAL;
    if (bytes) DSORT_HIP(ctx, hipMemcpy(d, h, bytes, hipMemcpyHostToDevice));
    return DSORT_OK;
}
int dsort_copy_d2h(dsort_ctx *ctx, void *h, const void *d, size_t bytes) {
    if (!ctx) return DSORT_EINVAL;
    if (bytes) DSORT_HIP(ctx, hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost));
    return DSORT_OK;
}

int dsort_copy_d2d(dsort_ctx *ctx, void *d, const void *src, size_t bytes) {
    if (!ctx) return DSORT_EINVAL;
    if (bytes) {
        DSORT_HIP(ctx, hipMemcpyAsync(d, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        DSORT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return DSORT_OK;
}
int dsort_host_register(dsort_ctx *ctx, void *host, size_t bytes) {
    if (!ctx || (!host && bytes)) return DSORT_EINVAL;
    if (bytes) DSORT_HIP(ctx, hipHostRegister(host, bytes, hipHostRegisterDefault));
    return DSORT_OK;
}
int dsort_host_unregister(dsort_ctx *ctx, void *host) {
    if (!ctx) return DSORT_EINVAL;
    if (host) DSORT_HIP(ctx, hipHostUnregister(host));
    return DSORT_OK;
}

int dsort_write_text_i32(const char *path, const int32_t *keys, size_t n) {
    if (!path || (n && !keys)) return DSORT_EINVAL;
    FILE *f = fopen(path, "w");
    if (!f) return DSORT_EINVAL;
    std::vector<char> buf(1 << 20);
    size_t o = 0;
    char tmp[16];
    for (size_t i = 0; i < n; ++i) {
        if (o + 13 > buf.size()) {
            if (fwrite(buf.data(), 1, o, f) != o) { fclose(f); return DSORT_EINVAL; }
            o = 0;
        }
        int64_t v = keys[i];
        const bool neg = v < 0;
        uint64_t u = neg ? (uint64_t)(-v) : (uint64_t)v;
        int t = 0;
        do { tmp[t++] = (char)('0' + u % 10); u /= 10; } while (u);
        if (neg) buf[o++] = '-';
        while (t) buf[o++] = tmp[--t];
        buf[o++] = '\n';
    }
    if (o && fwrite(buf.data(), 1, o, f) != o) { fclose(f); return DSORT_EINVAL; }
    return fclose(f) == 0 ? DSORT_OK : DSORT_EINVAL;
}

}  // extern "C"
