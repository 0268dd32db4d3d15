// bxlayout_harness.cpp -- TEST HARNESS (not product code): the bucket exchange's wave layout
// (csrc/dsort_bxlayout.h, the very function sample_sort_bx lays its waves out with) computed for
// EVERY rank of one synthetic exchange and checked rank against rank, for tests/test_bx_layout.py.
// With the ranks of a test sharing one GPU the RCCL path only ever runs with one rank, so that what
// rank q sends is what rank r expects is otherwise checked nowhere.
//
// The expected figures are computed here from the bucket sizes alone (a pure bucket travels as 0
// keys and counts in full for the output), not taken from the layout.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "dsort_bxlayout.h"

namespace {

uint64_t rnd(uint64_t &x) {  // splitmix64
    x += 0x9E3779B97F4A7C15ull;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

struct Fail {
    std::string msg;
};
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            char b_[256];                                 \
            snprintf(b_, sizeof b_, __VA_ARGS__);         \
            throw Fail{std::string(#cond) + ": " + b_};   \
        }                                                 \
    } while (0)

}  // namespace

extern "C" {

// One exchange over P ranks with Bl buckets each.
//   sizes  0 every bucket of every rank holds 7 keys, 1 skewed (random, some buckets 20 times the
//          others, another draw per rank), 2 skewed and the last rank holds no keys at all
//   pures  0 no pure bucket, 1 about a quarter of them, 2 all but one
//   room   recv_room of every rank: 0 none, 1 ample, 2 exactly what the other ranks send it,
//          3 one key less than that
// Returns 0 when every check holds (else 1 and the first failure in msg); *n_behind / *n_apart
// count the ranks whose pieces land behind their partition / in a receive buffer.
int bxl_check(int P, int Bl, int sizes, int pures, int room, uint64_t seed, char *msg, size_t cap, int *n_behind,
              int *n_apart) {
    const int Bt = P * Bl;
    const size_t row = (size_t)Bt + 1;
    uint64_t x = seed;
    std::vector<uint8_t> pure((size_t)Bt, 0);
    for (int g = 0; g < Bt; ++g) pure[(size_t)g] = pures == 1 ? rnd(x) % 4 == 0 : pures == 2 ? g != Bt / 2 : 0;
    // size[q][g], and every rank's real starts as the exchange all-gathers them
    std::vector<std::vector<uint64_t>> size((size_t)P, std::vector<uint64_t>((size_t)Bt, 7));
    std::vector<uint64_t> hb_all((size_t)P * row, 0), n_local((size_t)P, 0);
    for (int q = 0; q < P; ++q) {
        for (int g = 0; g < Bt; ++g) {
            uint64_t &s = size[(size_t)q][(size_t)g];
            if (sizes >= 1) s = rnd(x) % 50 * (rnd(x) % 3 == 0 ? 20 : 1);
            if (sizes == 2 && q == P - 1) s = 0;
            hb_all[(size_t)q * row + g + 1] = hb_all[(size_t)q * row + g] + s;
        }
        n_local[(size_t)q] = hb_all[(size_t)q * row + Bt];
    }
    auto csize = [&](int q, int g) { return pure[(size_t)g] ? 0 : size[(size_t)q][(size_t)g]; };
    auto cstart = [&](int q, int g) {
        uint64_t o = 0;
        for (int i = 0; i < g; ++i) o += csize(q, i);
        return o;
    };
    const int W = Bl >= 2 ? 2 : 1;
    const int jb[3] = {0, W == 2 ? Bl / 2 : Bl, Bl};
    // keys q ships to r in wave w
    auto ships = [&](int q, int r, int w) {
        uint64_t n = 0;
        for (int j = jb[w]; j < jb[w + 1]; ++j) n += csize(q, r * Bl + j);
        return n;
    };
    try {
        std::vector<dsort::BxLayout> L;
        std::vector<uint64_t> rooms;
        for (int me = 0; me < P; ++me) {
            uint64_t from_others = 0, total = 0;
            for (int q = 0; q < P; ++q) {
                total += n_local[(size_t)q];
                for (int w = 0; w < W; ++w)
                    if (q != me) from_others += ships(q, me, w);
            }
            const uint64_t rr = room == 0 ? 0 : room == 1 ? total : room == 2 ? from_others : from_others ? from_others - 1 : 0;
            rooms.push_back(rr);
            L.push_back(dsort::bx_layout(P, me, Bl, n_local[(size_t)me], rr, hb_all, pure));
        }
        for (int me = 0; me < P; ++me) {
            const dsort::BxLayout &l = L[(size_t)me];
            CHECK(l.W == W && l.jb[0] == jb[0] && l.jb[1] == jb[1] && l.jb[2] == jb[2], "rank %d: waves", me);
            CHECK(l.hc_all.size() == hb_all.size(), "rank %d", me);
            for (int q = 0; q < P; ++q)
                for (int g = 0; g <= Bt; ++g)
                    CHECK(l.hc_all[(size_t)q * row + g] == cstart(q, g), "rank %d: compacted start of rank %d bucket %d", me, q, g);
            uint64_t nrecv = 0, nout = 0, sent = 0, own = 0;
            std::vector<std::pair<uint64_t, uint64_t>> zones;
            for (int q = 0; q < P; ++q) {
                uint64_t from_q = 0;
                for (int w = 0; w < W; ++w) {
                    const size_t k = (size_t)w * P + q;
                    // what q sends to me in wave w is what I expect from q: count and bucket range
                    const dsort::BxLayout &lq = L[(size_t)q];
                    const size_t kq = (size_t)w * P + me;
                    CHECK(lq.scnt[kq] == l.rcnt[k], "wave %d: rank %d sends %llu keys to rank %d, which expects %llu", w, q,
                          (unsigned long long)lq.scnt[kq], me, (unsigned long long)l.rcnt[k]);
                    CHECK(l.rcnt[k] == ships(q, me, w), "wave %d: rank %d expects %llu keys from rank %d", w, me,
                          (unsigned long long)l.rcnt[k], q);
                    CHECK(lq.soff[kq] == cstart(q, me * Bl + jb[w]) &&
                              lq.soff[kq] + lq.scnt[kq] == cstart(q, me * Bl + jb[w + 1]),
                          "wave %d: rank %d's send range to rank %d is not buckets [%d, %d) of its range", w, q, me, jb[w],
                          jb[w + 1]);
                    CHECK(lq.soff[kq] + lq.scnt[kq] <= n_local[(size_t)q], "wave %d: rank %d sends past its keys", w, q);
                    from_q += l.rcnt[k];
                    if (q != me) sent += l.scnt[k];
                    if (l.behind && q == me) {  // read in place
                        CHECK(l.rpos[k] == 0 && l.base[k] == l.soff[k], "wave %d: rank %d's own buckets in place", w, me);
                        continue;
                    }
                    CHECK(l.base[k] == l.rpos[k], "wave %d: rank %d, source %d", w, me, q);
                    if (l.rcnt[k]) zones.push_back({l.rpos[k], l.rpos[k] + l.rcnt[k]});
                }
                CHECK(l.rlen[(size_t)q] == from_q, "rank %d: rlen of source %d", me, q);
                nrecv += from_q;
                if (q == me) own = from_q;
                for (int j = 0; j < Bl; ++j) nout += size[(size_t)q][(size_t)(me * Bl + j)];
            }
            CHECK(l.nrecv == nrecv, "rank %d: nrecv %llu, sum(rlen) %llu", me, (unsigned long long)l.nrecv,
                  (unsigned long long)nrecv);
            CHECK(l.nout == nout, "rank %d: nout %llu, the buckets' real sizes %llu", me, (unsigned long long)l.nout,
                  (unsigned long long)nout);
            CHECK(l.sent == sent, "rank %d: sent", me);
            CHECK(l.behind == (nrecv - own <= rooms[(size_t)me]), "rank %d: behind", me);
            const uint64_t z0 = l.behind ? n_local[(size_t)me] : 0;
            const uint64_t z1 = l.behind ? n_local[(size_t)me] + rooms[(size_t)me] : l.nrecv;
            std::sort(zones.begin(), zones.end());
            for (size_t i = 0; i < zones.size(); ++i) {
                CHECK(zones[i].first >= z0 && zones[i].second <= z1, "rank %d: landing zone [%llu, %llu) outside [%llu, %llu)",
                      me, (unsigned long long)zones[i].first, (unsigned long long)zones[i].second, (unsigned long long)z0,
                      (unsigned long long)z1);
                CHECK(i == 0 || zones[i - 1].second <= zones[i].first, "rank %d: landing zones overlap at %llu", me,
                      (unsigned long long)zones[i].first);
            }
            ++*(l.behind ? n_behind : n_apart);
        }
    } catch (const Fail &f) {
        if (msg && cap) {
            strncpy(msg, f.msg.c_str(), cap - 1);
            msg[cap - 1] = 0;
        }
        return 1;
    }
    return 0;
}

}  // extern "C"
