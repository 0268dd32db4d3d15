// slotmap_harness.cpp -- TEST HARNESS (not product code): the slot maps of the first partition level
// (csrc/dsort_bucket.h: log_m, slot_mode, slot_first -- the very functions the kernels call, which are
// __host__ __device__) and of the second (csrc/dsort_sub.h: slot_of), run on the host over the edges of
// the key range, for tests/test_slotmap_host.py.
//
// For both key widths, under the linear map with every shift 0 .. KB - 11 and under the log map, with
// ulo in {0, 1, UMAX, UMAX - 5, 2^(KB-1) - 1, 2^(KB-1) + 1} and NRAND random values of random bit length:
//   bounds    every slot < 2048; log_m is 6 (int32) and 5 (int64); the largest log slot (d = UMAX) < 2048;
//   monotone  the slots of NKEYS sorted keys (random ones, the extremes, -1, 0, 1, the keys around ulo)
//             never decrease;
//   inverse   what build_slots relies on: for every slot i in 1 .. 2047, when slot_first gives u0 the key
//             of u0 has a slot >= i and the key below it a slot < i; when it gives none, the largest
//             key's slot is below i.
// The fixed int32 map is the top 11 bits of the flipped key, and slot_first of the default map gives
// i << 21.  The second level's slot_of is monotone and stays below SB_SLOTS, for klo in {MIN, 0, MAX - 3}
// and every shift 0 .. KB - 10.
//
// Prints the first violations and exits 1; else one line "ok <checks>".
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <limits>
#include <vector>

#include "dsort_bucket.h"
#include "dsort_sub.h"

namespace {

using namespace dsort;
using bk::BK_SLOTB;
using bk::BK_SLOTS;
using bk::BkMap;
using bk::Comp;

constexpr int NRAND = 1000;   // random ulo values per key width
constexpr int NKEYS = 4200;   // keys of a monotone check (>= 4096)
constexpr int MAXPRINT = 12;

uint64_t g_checks = 0;
int g_fails = 0;

uint64_t rnd(uint64_t &x) {  // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

#define CHECK(cond, ...)                                       \
    do {                                                       \
        ++g_checks;                                            \
        if (!(cond)) {                                         \
            if (g_fails++ < MAXPRINT) {                        \
                printf("VIOLATION %s: ", #cond);               \
                printf(__VA_ARGS__);                           \
                printf("\n");                                  \
            }                                                  \
        }                                                      \
    } while (0)

template <typename T> const char *name();
template <> const char *name<int32_t>() { return "int32"; }
template <> const char *name<int64_t>() { return "int64"; }

template <typename T>
T unflip(typename Comp<T>::U u) {
    using U = typename Comp<T>::U;
    return (T)(U)(u ^ ((U)1 << (Comp<T>::KB - 1)));
}

// a value of random bit length 0 .. KB
template <typename T>
typename Comp<T>::U rnd_len(uint64_t &x) {
    using U = typename Comp<T>::U;
    const int len = (int)(rnd(x) % (Comp<T>::KB + 1));
    const uint64_t v = rnd(x);
    return len == 0 ? (U)0 : (U)((v >> (64 - len)) | ((uint64_t)1 << (len - 1)));
}

template <typename T>
BkMap make_map(uint64_t ulo, uint32_t sh, uint32_t mode) {
    BkMap m = {};
    m.ulo = ulo;
    m.sh = sh;
    m.mode = mode;
    return m;
}

template <typename T>
uint32_t slot(const BkMap &m, T key) {
    return bk::slot_at<T, BK_SLOTB, true>(m, key);
}

template <typename T>
void check_map(const BkMap &m, const std::vector<T> &keys) {
    using U = typename Comp<T>::U;
    const T kmax = std::numeric_limits<T>::max();
    // bounds, monotone
    uint32_t prev = 0;
    for (size_t k = 0; k < keys.size(); ++k) {
        const uint32_t s = slot<T>(m, keys[k]);
        CHECK(s < (uint32_t)BK_SLOTS, "%s ulo=%llu sh=%u mode=%u key=%lld slot=%u", name<T>(),
              (unsigned long long)m.ulo, m.sh, m.mode, (long long)keys[k], s);
        CHECK(s >= prev, "%s ulo=%llu sh=%u mode=%u key=%lld slot=%u after slot %u", name<T>(),
              (unsigned long long)m.ulo, m.sh, m.mode, (long long)keys[k], s, prev);
        prev = s;
    }
    // inverse
    const uint32_t top = slot<T>(m, kmax);
    for (uint32_t i = 1; i < (uint32_t)BK_SLOTS; ++i) {
        uint64_t u0 = 0;
        if (bk::slot_first<T, BK_SLOTB>(m, i, u0)) {
            CHECK(u0 <= (uint64_t)(U)~(U)0, "%s ulo=%llu sh=%u mode=%u slot=%u first=%llu beyond the key range",
                  name<T>(), (unsigned long long)m.ulo, m.sh, m.mode, i, (unsigned long long)u0);
            const uint32_t s = slot<T>(m, unflip<T>((U)u0));
            CHECK(s >= i, "%s ulo=%llu sh=%u mode=%u slot=%u first=%llu maps to %u", name<T>(),
                  (unsigned long long)m.ulo, m.sh, m.mode, i, (unsigned long long)u0, s);
            if (u0 > 0) {
                const uint32_t b = slot<T>(m, unflip<T>((U)(u0 - 1)));
                CHECK(b < i, "%s ulo=%llu sh=%u mode=%u slot=%u: key below first=%llu maps to %u", name<T>(),
                      (unsigned long long)m.ulo, m.sh, m.mode, i, (unsigned long long)u0, b);
            }
        } else {
            CHECK(top < i, "%s ulo=%llu sh=%u mode=%u slot=%u has no first key but the largest key maps to %u",
                  name<T>(), (unsigned long long)m.ulo, m.sh, m.mode, i, top);
        }
    }
}

template <typename T>
void check_width(uint64_t seed) {
    using U = typename Comp<T>::U;
    constexpr int KB = Comp<T>::KB;
    const U umax = (U)~(U)0, half = (U)1 << (KB - 1);
    const T kmin = std::numeric_limits<T>::min(), kmax = std::numeric_limits<T>::max();
    uint64_t x = seed;

    CHECK((bk::log_m<T, BK_SLOTB>()) == (KB == 32 ? 6 : 5), "%s log_m = %d", name<T>(), bk::log_m<T, BK_SLOTB>());
    {
        const BkMap m = make_map<T>(0, 0, 1);
        const uint32_t s = slot<T>(m, unflip<T>(umax));
        CHECK(s < (uint32_t)BK_SLOTS, "%s largest log slot %u", name<T>(), s);
    }

    std::vector<U> ulos = {(U)0, (U)1, umax, (U)(umax - 5), (U)(half - 1), (U)(half + 1)};
    for (int r = 0; r < NRAND; ++r) ulos.push_back(rnd_len<T>(x));

    std::vector<T> base = {kmin, (T)(kmin + 1), (T)-1, (T)0, (T)1, (T)(kmax - 1), kmax};
    while ((int)base.size() < NKEYS - 5) {
        // half of them of random bit length above the bottom of the range, half anywhere
        const U u = (rnd(x) & 1) ? rnd_len<T>(x) : (U)rnd(x);
        base.push_back(unflip<T>(u));
    }
    for (const U ulo : ulos) {
        std::vector<T> keys = base;
        for (int d = -2; d <= 2; ++d) keys.push_back(unflip<T>((U)(ulo + (U)d)));  // (wraps at the ends)
        // a few random keys just above ulo, where the log map is finest
        for (int r = 0; r < 64; ++r) {
            const U d = rnd_len<T>(x) >> (rnd(x) % KB);
            if (d <= (U)(umax - ulo)) keys.push_back(unflip<T>((U)(ulo + d)));
        }
        std::sort(keys.begin(), keys.end());
        for (uint32_t sh = 0; sh <= (uint32_t)(KB - BK_SLOTB); ++sh) check_map<T>(make_map<T>(ulo, sh, 0), keys);
        check_map<T>(make_map<T>(ulo, 0, 1), keys);
    }

    // the second level: slot = (max(key - klo, 0) >> sh), capped
    std::vector<T> keys = base;
    std::sort(keys.begin(), keys.end());
    const T klos[3] = {kmin, (T)0, (T)(kmax - 3)};
    for (const T klo : klos)
        for (uint32_t sh = 0; sh <= (uint32_t)(KB - sb::SB_SLOTB); ++sh) {
            uint32_t prev = 0;
            for (const T key : keys) {
                const uint32_t s = sb::slot_of<T>(key, klo, sh);
                CHECK(s < (uint32_t)sb::SB_SLOTS, "sub %s klo=%lld sh=%u key=%lld slot=%u", name<T>(), (long long)klo,
                      sh, (long long)key, s);
                CHECK(s >= prev, "sub %s klo=%lld sh=%u key=%lld slot=%u after slot %u", name<T>(), (long long)klo,
                      sh, (long long)key, s, prev);
                prev = s;
            }
            CHECK(sb::slot_of<T>(klo, klo, sh) == 0, "sub %s klo=%lld sh=%u: klo not in slot 0", name<T>(),
                  (long long)klo, sh);
        }
}

// int32 on the fixed map: the top 11 bits of the flipped key
void check_fixed(uint64_t seed) {
    uint64_t x = seed;
    BkMap m = make_map<int32_t>(0, (uint32_t)(32 - BK_SLOTB), 0);
    // (ADP = false ignores the map: a wild one must change nothing)
    const BkMap wild = make_map<int32_t>(0xDEADBEEFull, 7, 1);
    std::vector<int32_t> keys = {INT32_MIN, INT32_MIN + 1, -1, 0, 1, INT32_MAX - 1, INT32_MAX};
    for (int r = 0; r < 100000; ++r) keys.push_back((int32_t)(uint32_t)rnd(x));
    for (uint32_t i = 0; i < (uint32_t)BK_SLOTS; ++i) {  // both ends of every slot
        keys.push_back(unflip<int32_t>(i << 21));
        keys.push_back(unflip<int32_t>((i << 21) + 0x1FFFFFu));
    }
    for (const int32_t key : keys) {
        const uint32_t want = ((uint32_t)key ^ 0x80000000u) >> 21;
        const uint32_t s0 = bk::slot_mode<int32_t, BK_SLOTB, 0, false>(m, key);
        const uint32_t s1 = bk::slot_mode<int32_t, BK_SLOTB, 1, false>(wild, key);
        const uint32_t s2 = bk::slot_at<int32_t>(wild, key);  // (the default instance of int32 is the fixed one)
        CHECK(s0 == want && s1 == want && s2 == want, "fixed key=%d slots %u %u %u, top bits %u", key, s0, s1, s2, want);
        // (and the adaptive instance of the fixed map's parameters agrees with it)
        const uint32_t s3 = bk::slot_mode<int32_t, BK_SLOTB, 0, true>(m, key);
        CHECK(s3 == want, "adaptive instance of the fixed map: key=%d slot %u, top bits %u", key, s3, want);
    }
    for (uint32_t i = 1; i < (uint32_t)BK_SLOTS; ++i) {
        uint64_t u0 = ~0ull;
        const bool ok = bk::slot_first<int32_t, BK_SLOTB>(m, i, u0);
        CHECK(ok && u0 == (uint64_t)i << 21, "fixed slot_first(%u) = %d, %llu", i, (int)ok, (unsigned long long)u0);
    }
}

}  // namespace

int main() {
    static_assert(bk::log_m<int32_t, BK_SLOTB>() == 6 && bk::log_m<int64_t, BK_SLOTB>() == 5, "log_m");
    check_width<int32_t>(0x5107A932u);
    check_width<int64_t>(0x5107A964u);
    check_fixed(0xF1DEDu);
    if (g_fails) {
        printf("FAILED: %d violations in %llu checks\n", g_fails, (unsigned long long)g_checks);
        return 1;
    }
    printf("ok %llu\n", (unsigned long long)g_checks);
    return 0;
}
