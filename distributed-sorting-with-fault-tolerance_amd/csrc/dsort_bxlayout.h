// dsort_bxlayout.h -- the wave layout of the bucket exchange (sample_sort_bx, dsort_exchange.hip):
// who sends which keys to whom in which wave, and where they land.  Plain host C++ (no HIP):
// libdsort includes it, and so does the CPU test harness tests/tx/bxlayout_harness.cpp, which
// checks every rank's layout of one exchange against its peers' -- what no test on one GPU sees.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace dsort {

// The exchange in waves of a rank's Bl buckets: two or more buckets, two waves.
inline int bx_waves(int Bl) { return Bl >= 2 ? 2 : 1; }

// Rank `me`'s view of one exchange over P ranks with Bl buckets each (Bt = P * Bl global buckets,
// buckets [q Bl, (q + 1) Bl) belong to rank q).  Arrays "per wave and peer" are indexed [w * P + q].
struct BxLayout {
    // W waves (bx_waves): wave w ships buckets [jb[w], jb[w+1]) of every rank's range.
    int W = 1;
    int jb[3] = {0, 0, 0};
    // Positions in `part` and in the receive buffer follow every rank's compacted starts (a pure
    // bucket -- its keys dropped by the scatter, bx_partition -- of size 0); the output sizes follow
    // the real starts.  hc_all[r * (Bt + 1) + g]: rank r's compacted start of bucket g.
    std::vector<uint64_t> hc_all;
    std::vector<uint64_t> rlen;  // per source: the keys it sends here (compacted), all waves
    uint64_t nrecv = 0;          // their sum: the keys received, this rank's own included
    uint64_t nout = 0;           // keys of this rank's sorted slice (the real sizes)
    uint64_t sent = 0;           // keys this rank ships to other ranks
    // The other ranks' pieces land behind this rank's partitioned keys when they fit (its own buckets
    // are then read in place: no copy); else everything goes to a receive buffer.
    bool behind = false;
    // per wave and source: the keys it sends here (rcnt), where they land (rpos) and the source
    // position of its first key of the wave's first bucket (base; `behind` and the source is this
    // rank: the position in part)
    std::vector<uint64_t> rcnt, rpos, base;
    // per wave and destination: this rank's send range in part, [soff, soff + scnt)
    std::vector<uint64_t> soff, scnt;
};

// hb_all[r * (Bt + 1) + g]: rank r's real start of bucket g; pure[g]: bucket g holds one key value
// only and does not travel; n_local, recv_room: the keys of this rank, and the room behind them.
inline BxLayout bx_layout(int P, int me, int Bl, uint64_t n_local, uint64_t recv_room,
                          const std::vector<uint64_t> &hb_all, const std::vector<uint8_t> &pure) {
    const int Bt = P * Bl;
    const size_t row = (size_t)Bt + 1;
    BxLayout L;
    const int W = L.W = bx_waves(Bl);
    L.jb[1] = W == 2 ? Bl / 2 : Bl;
    L.jb[2] = Bl;
    const int *jb = L.jb;
    L.hc_all.resize(hb_all.size());
    for (int r = 0; r < P; ++r) {
        const uint64_t *h = hb_all.data() + (size_t)r * row;
        uint64_t *c = L.hc_all.data() + (size_t)r * row, run = 0;
        for (int g = 0; g <= Bt; ++g) {
            c[g] = run;
            if (g < Bt && !pure[(size_t)g]) run += h[g + 1] - h[g];
        }
    }
    auto hof = [&](int r) { return L.hc_all.data() + (size_t)r * row; };
    const uint64_t *hme = hof(me);
    L.rlen.assign(P, 0);
    for (int q = 0; q < P; ++q) {
        L.rlen[q] = hof(q)[(size_t)(me + 1) * Bl] - hof(q)[(size_t)me * Bl];
        L.nrecv += L.rlen[q];
        if (q != me) L.sent += hme[(size_t)(q + 1) * Bl] - hme[(size_t)q * Bl];
        const uint64_t *h = hb_all.data() + (size_t)q * row;
        L.nout += h[(size_t)(me + 1) * Bl] - h[(size_t)me * Bl];
    }
    L.behind = L.nrecv - L.rlen[me] <= recv_room;
    const size_t WP = (size_t)W * P;
    L.rcnt.resize(WP), L.rpos.resize(WP), L.base.resize(WP), L.soff.resize(WP), L.scnt.resize(WP);
    uint64_t o = L.behind ? n_local : 0;
    for (int w = 0; w < W; ++w)
        for (int q = 0; q < P; ++q) {
            const size_t k = (size_t)w * P + q;
            L.soff[k] = hme[(size_t)q * Bl + jb[w]];
            L.scnt[k] = hme[(size_t)q * Bl + jb[w + 1]] - L.soff[k];
            L.rcnt[k] = hof(q)[(size_t)me * Bl + jb[w + 1]] - hof(q)[(size_t)me * Bl + jb[w]];
            if (L.behind && q == me) {
                L.base[k] = L.soff[k];
                L.rpos[k] = 0;
                continue;
            }
            L.base[k] = L.rpos[k] = o;
            o += L.rcnt[k];
        }
    return L;
}

}  // namespace dsort
