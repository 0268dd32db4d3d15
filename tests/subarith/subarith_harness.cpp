// subarith_harness.cpp -- TEST HARNESS (not product code): the second level's arithmetic sub-bucket map
// (csrc/dsort_sub.h: arith_scale, arith_sub, arith_splitter_key, and slot_of, slot_shift, slot_entry,
// sub_of / sub_pick -- the very functions the kernels call, which are __host__ __device__) run on the
// host, for tests/test_subarith_host.py.
//
//   subarith_harness              the edge buckets: for klo at INT32_MIN, at 0 and with klo + span at
//       INT32_MAX, spans 2 nsub, 2^16, 2^22 - 1, 2^22, 2^31 - 1, 2^31 + 12345 and 2^32 - 1 (those that fit
//       the key range from klo), nsub in {2, 85, 683, 1024}: the synthetic splitters and the slot table
//       are built as sb_splitter_kernel builds them, and over every splitter key and its two neighbours,
//       klo - 1, klo, klo + 1, klo + span - 1, klo + span, klo + span + 1, INT32_MIN and INT32_MAX:
//         range      arith_sub(key) < nsub, sub-bucket 0 at and below klo;
//         monotone   arith_sub never decreases over the sorted keys;
//         splitters  strictly increasing (no two equal); arith_sub(splitter j) <= j and, unless the
//                    splitter is INT32_MAX, arith_sub(splitter j + 1) > j;
//         tables     sub_of(tables, key, pos) == arith_sub(key) for pos in {0, 2^31, UINT32_MAX - 1}.
//       Prints the first violations and exits 1; else one line "ok <checks>".
//   subarith_harness rule NSUB OS FILE   the take / refuse rule of sb_splitter_kernel on the int32 sample
//       keys in FILE (raw, in sampling order: runs of SB_RUN): prints "take" or "refuse".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "dsort_sub.h"

namespace {

using namespace dsort::sb;

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

void bucket(int32_t klo, uint32_t span, uint32_t nsub) {
    const uint32_t scale = arith_scale(span, nsub), sh = slot_shift<int32_t>(span), nspl = nsub - 1;
    CHECK(arith_span_ok(span, nsub), "span %u nsub %u", span, nsub);
    CHECK(scale != 0 && scale < 0x80000000u, "scale %u span %u nsub %u", scale, span, nsub);
    // the tables, as sb_splitter_kernel builds them
    std::vector<Spl<int32_t>> spl(nspl + 1);  // + 1: sub_of reads two entries
    std::vector<uint32_t> sslot(nspl), rng(SB_SLOTS);
    std::vector<int32_t> skey(nspl);
    for (uint32_t j = 0; j < nspl; ++j) {
        spl[j].k = skey[j] = arith_splitter_key(klo, scale, j);
        spl[j].p = UINT32_MAX;
        sslot[j] = slot_of<int32_t>(skey[j], klo, sh);
        if (j) CHECK(skey[j - 1] < skey[j], "klo %d span %u nsub %u: splitters %u, %u = %d, %d", klo, span, nsub, j - 1, j, skey[j - 1], skey[j]);
    }
    for (uint32_t s = 0; s < (uint32_t)SB_SLOTS; ++s) rng[s] = slot_entry<int32_t>(sslot.data(), skey.data(), nspl, s);
    auto f = [&](int64_t key) { return arith_sub((int32_t)key, klo, scale, nsub); };
    std::vector<int64_t> keys = {INT32_MIN, INT32_MAX};
    auto add = [&](int64_t k) {
        if (k >= INT32_MIN && k <= INT32_MAX) keys.push_back(k);
    };
    for (int d = -1; d <= 1; ++d) {
        add((int64_t)klo + d);
        add((int64_t)klo + span + d);
        for (uint32_t j = 0; j < nspl; ++j) add((int64_t)skey[j] + d);
    }
    for (uint32_t j = 0; j < nspl; ++j) {
        CHECK(f(skey[j]) <= j, "klo %d span %u nsub %u: f(splitter %u = %d) = %u", klo, span, nsub, j, skey[j], f(skey[j]));
        if (skey[j] != INT32_MAX)
            CHECK(f((int64_t)skey[j] + 1) > j, "klo %d span %u nsub %u: f(splitter %u + 1) = %u", klo, span, nsub, j, f((int64_t)skey[j] + 1));
    }
    std::sort(keys.begin(), keys.end());
    uint32_t prev = 0;
    for (const int64_t k : keys) {
        const uint32_t j = f(k);
        CHECK(j < nsub, "klo %d span %u nsub %u key %lld: f = %u", klo, span, nsub, (long long)k, j);
        CHECK(j >= prev, "klo %d span %u nsub %u key %lld: f = %u after %u", klo, span, nsub, (long long)k, j, prev);
        if (k <= klo) CHECK(j == 0, "klo %d key %lld: f = %u", klo, (long long)k, j);
        prev = j;
        for (const uint32_t pos : {0u, 0x80000000u, UINT32_MAX - 1}) {
            const int t = sub_of<int32_t>(spl.data(), rng.data(), klo, sh, (int32_t)k, pos);
            CHECK(t == (int)j, "klo %d span %u nsub %u key %lld pos %u: sub_of %d, f %u", klo, span, nsub, (long long)k, pos, t, j);
        }
    }
}

int edges() {
    const uint32_t nsubs[] = {2, 85, 683, 1024};
    for (const uint32_t nsub : nsubs) {
        const uint64_t spans[] = {2ull * nsub, 1ull << 16, (1ull << 22) - 1, 1ull << 22, (1ull << 31) - 1,
                                  (1ull << 31) + 12345, (1ull << 32) - 1};
        for (const uint64_t span : spans) {
            // klo at INT32_MIN, at 0, and with the range's end at INT32_MAX
            const int64_t klos[] = {INT32_MIN, 0, (int64_t)INT32_MAX - (int64_t)span};
            for (const int64_t klo : klos)
                if (klo >= INT32_MIN && klo + (int64_t)span <= INT32_MAX) bucket((int32_t)klo, (uint32_t)span, nsub);
        }
    }
    if (g_fails) {
        printf("%d violations in %llu checks\n", g_fails, (unsigned long long)g_checks);
        return 1;
    }
    printf("ok %llu\n", (unsigned long long)g_checks);
    return 0;
}

// sb_splitter_kernel's rule (arith = -1) over a bucket's samples
int rule(uint32_t nsub, uint32_t os, const char *path) {
    FILE *fp = fopen(path, "rb");
    if (!fp) return 2;
    std::vector<int32_t> sk;
    int32_t buf[4096];
    for (size_t r; (r = fread(buf, 4, 4096, fp)) > 0;) sk.insert(sk.end(), buf, buf + r);
    fclose(fp);
    if (sk.empty() || nsub < 2) return 2;
    // (key, sampling index) order, as the composites' sort gives it; neighbours from one run
    std::vector<uint32_t> idx(sk.size());
    for (uint32_t i = 0; i < idx.size(); ++i) idx[i] = i;
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t x, uint32_t y) { return sk[x] < sk[y]; });
    size_t same = 0;
    const uint32_t run = sk.size() % SB_RUN ? 1u : SB_RUN;
    for (size_t i = 1; run > 1 && i < idx.size(); ++i) same += idx[i] / run == idx[i - 1] / run;
    const uint32_t maxs = 2 * same >= sk.size() ? SB_ARITH_MAXS_RUNS : SB_ARITH_MAXS;
    std::sort(sk.begin(), sk.end());
    const int32_t klo = sk.front();
    const uint32_t span = (uint32_t)sk.back() - (uint32_t)klo;
    bool take = arith_span_ok(span, nsub);
    if (take) {
        const uint32_t scale = arith_scale(span, nsub);
        size_t below = 0;
        for (uint32_t j = 0; j < nsub && take; ++j) {
            const size_t ub = j + 1 < nsub
                                  ? (size_t)(std::upper_bound(sk.begin(), sk.end(), arith_splitter_key(klo, scale, j)) - sk.begin())
                                  : sk.size();
            take = ub - below <= (size_t)maxs * os;
            below = ub;
        }
    }
    printf("%s\n", take ? "take" : "refuse");
    return 0;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 5 && !strcmp(argv[1], "rule")) return rule((uint32_t)atoi(argv[2]), (uint32_t)atoi(argv[3]), argv[4]);
    return edges();
}
