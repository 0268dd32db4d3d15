// bkarith_harness.cpp -- TEST HARNESS (not product code): the first level's arithmetic bucket map
// (csrc/dsort_bucket.h: arith_scale, arith_bucket over a BkMap, arith_splitter_key, arith_bucket_full -- the
// very functions the kernels call, which are __host__ __device__) run on the host, for
// tests/test_bkarith_host.py.
//
// For B in {2, 64, 1000, 1024}, spans 2 B (the smallest the rule allows), 2 B + 1, 2^16, 2^31 - 1,
// 2^31 + 12345 and 2^32 - 1, and klo at INT32_MIN, at 0 and with klo + span at INT32_MAX (those that fit
// the key range): the synthetic splitters are built as bucket_slotmap_kernel builds them, composites
// (key, index UINT32_MAX), and over every splitter key and its two neighbours, klo - 1, klo, klo + 1,
// klo + span - 1, klo + span, klo + span + 1 (keys below and above the range where the key range has
// any), INT32_MIN and INT32_MAX:
//   scale      0 < scale < 2^31;
//   range      arith_bucket(key) < B, bucket 0 at and below klo;
//   monotone   arith_bucket never decreases over the sorted keys;
//   splitters  strictly increasing in key; arith_bucket(splitter j) == j and arith_bucket(splitter j + 1)
//              == j + 1 -- but for a splitter capped at INT32_MAX (the last one only), which no key lies
//              above and whose bucket is <= j;
//   lookup     the number of splitters below the composite (key, index), which is what every reader of
//              the splitters computes, == arith_bucket(key) for index in {0, 2^31, UINT32_MAX - 1}.
// Prints the first violations and exits 1; else one line "ok <checks>".
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <vector>

#include "dsort_bucket.h"

namespace {

using namespace dsort::bk;

constexpr int MAXPRINT = 12;
uint64_t g_checks = 0;
int g_fails = 0;

#define CHECK(cond, ...)                         \
    do {                                         \
        ++g_checks;                              \
        if (!(cond)) {                           \
            if (g_fails++ < MAXPRINT) {          \
                printf("VIOLATION %s: ", #cond); \
                printf(__VA_ARGS__);             \
                printf("\n");                    \
            }                                    \
        }                                        \
    } while (0)

void sort_case(int32_t klo, uint32_t span, int B) {
    CHECK(arith_span_ok(span, (uint32_t)B), "span %u B %d", span, B);
    BkMap m{};
    m.ar = 1;
    m.arlo = (uint32_t)klo;
    m.arscale = arith_scale(span, (uint32_t)B);
    CHECK(m.arscale != 0 && m.arscale < 0x80000000u, "scale %u span %u B %d", m.arscale, span, B);
    const int nsp = B - 1;
    std::vector<int64_t> spl(nsp);   // the composites, as the kernel writes them
    std::vector<int32_t> skey(nsp);
    auto f = [&](int64_t key) { return arith_bucket((int32_t)key, m, B); };
    for (int j = 0; j < nsp; ++j) {
        skey[j] = arith_splitter_key(klo, m.arscale, (uint32_t)j);
        spl[j] = Comp<int32_t>::make(skey[j], 0xFFFFFFFFull);
        if (j) CHECK(skey[j - 1] < skey[j] && spl[j - 1] < spl[j], "klo %d span %u B %d: splitters %d, %d = %d, %d", klo, span, B, j - 1, j, skey[j - 1], skey[j]);
        // the splitter before the cap at INT32_MAX, restated
        const int64_t raw = (int64_t)klo + (int64_t)(((((uint64_t)j + 1) << 32) + m.arscale - 1) / m.arscale - 1);
        if (raw <= (int64_t)INT32_MAX) {
            CHECK((int64_t)skey[j] == raw, "klo %d span %u B %d: splitter %d = %d, restated %lld", klo, span, B, j, skey[j], (long long)raw);
            CHECK(f(skey[j]) == j, "klo %d span %u B %d: f(splitter %d = %d) = %d", klo, span, B, j, skey[j], f(skey[j]));
            if (raw < (int64_t)INT32_MAX)
                CHECK(f((int64_t)skey[j] + 1) == j + 1, "klo %d span %u B %d: f(splitter %d + 1) = %d", klo, span, B, j, f((int64_t)skey[j] + 1));
        } else {
            CHECK(skey[j] == INT32_MAX && j == nsp - 1, "klo %d span %u B %d: splitter %d = %d capped", klo, span, B, j, skey[j]);
            CHECK(f(skey[j]) <= j, "klo %d span %u B %d: f(capped splitter %d) = %d", klo, span, B, j, f(skey[j]));
        }
    }
    std::vector<int64_t> keys = {INT32_MIN, INT32_MAX};
    auto add = [&](int64_t k) {
        if (k >= INT32_MIN && k <= INT32_MAX) keys.push_back(k);
    };
    for (int d = -1; d <= 1; ++d) {
        add((int64_t)klo + d);
        add((int64_t)klo + span + d);
        for (int j = 0; j < nsp; ++j) add((int64_t)skey[j] + d);
    }
    std::sort(keys.begin(), keys.end());
    int prev = 0;
    for (const int64_t k : keys) {
        const int j = f(k);
        CHECK(j >= 0 && j < B, "klo %d span %u B %d key %lld: f = %d", klo, span, B, (long long)k, j);
        CHECK(j >= prev, "klo %d span %u B %d key %lld: f = %d after %d", klo, span, B, (long long)k, j, prev);
        if (k <= klo) CHECK(j == 0, "klo %d key %lld: f = %d", klo, (long long)k, j);
        prev = j;
        for (const uint64_t idx : {0ull, 0x80000000ull, 0xFFFFFFFEull}) {
            const int64_t c = Comp<int32_t>::make((int32_t)k, idx);
            const int t = (int)(std::lower_bound(spl.begin(), spl.end(), c) - spl.begin());  // splitters < c
            CHECK(t == j, "klo %d span %u B %d key %lld index %llu: %d splitters below, f %d", klo, span, B, (long long)k, (unsigned long long)idx, t, j);
        }
    }
}

}  // namespace

int main() {
    static_assert(sizeof(BkMap) <= 64, "the map's 64 bytes");
    const int Bs[] = {2, 64, 1000, 1024};
    for (const int B : Bs) {
        const uint64_t spans[] = {2ull * B, 2ull * B + 1, 1ull << 16, (1ull << 31) - 1, (1ull << 31) + 12345, (1ull << 32) - 1};
        for (const uint64_t span : spans) {
            const int64_t klos[] = {INT32_MIN, 0, (int64_t)INT32_MAX - (int64_t)span};
            for (const int64_t klo : klos)
                if (klo >= INT32_MIN && klo + (int64_t)span <= INT32_MAX) sort_case((int32_t)klo, (uint32_t)span, B);
        }
    }
    // the sample bound: 3/2 os
    CHECK(!arith_bucket_full(192, 128) && arith_bucket_full(193, 128), "os 128");
    CHECK(!arith_bucket_full(1, 1) && arith_bucket_full(2, 1), "os 1");
    if (g_fails) {
        printf("%d violations in %llu checks\n", g_fails, (unsigned long long)g_checks);
        return 1;
    }
    printf("ok %llu\n", (unsigned long long)g_checks);
    return 0;
}
