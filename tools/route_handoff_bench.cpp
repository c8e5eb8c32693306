// Host cost of process_packets' hand-off for one burst, on the CPU (no GPU):
//   lists      yrss_route_lists on the routed lists (ridx, rstart) a route burst
//              kernel wrote: list walks, reads neither q nor filter
//   classified yrss_route_classified, what yrss_route_burst runs after its
//              classification: route classes from q / filter, a stable counting
//              sort into (ridx, rstart), then the same list walks
//   per-packet the former body of yrss_route_burst, kept here as the baseline:
//              the hand-off decided packet by packet from q / filter / qidx /
//              qstart, with its std::vector scratch
// All drive the same callbacks (rings that append into preallocated arrays, a
// clone that hands out addresses, a release that counts), on the same random
// burst: nb_queues 3, queue_id 2, KNI on ("accept"), a tenth of the local
// packets ARP and a fifth KNI.  Reported: ns per packet, median [min-max] over
// the rounds, legs interleaved.
//   g++ -O2 -std=c++17 -I include tools/route_handoff_bench.cpp
//       yastack_amd/csrc/yrss_seg.cpp -o route_handoff_bench && ./route_handoff_bench
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <time.h>

#include <algorithm>
#include <vector>

#include "yrss.h"
#include "../yastack_amd/csrc/yrss_route_internal.h"

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

double now_ns()
{
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e9 + ts.tv_nsec;
}

struct Sink {
    void *ring[YRSS_MAX_QUEUES][4096];
    uint32_t fill[YRSS_MAX_QUEUES];
    uint64_t released, clones;
};

unsigned cb_enqueue(void *user, uint16_t queue, void *const *objs, unsigned n)
{
    Sink *s = (Sink *)user;
    const unsigned k = std::min<unsigned>(n, 4096u - s->fill[queue]);
    memcpy(s->ring[queue] + s->fill[queue], objs, k * sizeof(void *));
    s->fill[queue] += k;
    return k;
}
void *cb_clone(void *user, void *m, uint16_t queue)
{
    Sink *s = (Sink *)user;
    return (void *)((uintptr_t)m + (++s->clones << 32) + queue);
}
void cb_release(void *user, void *) { ((Sink *)user)->released++; }

// yrss_route_burst after classify_staged / finish_burst, as it was before it
// called yrss_route_classified
void per_packet(const int16_t *q, const int8_t *fc, const uint32_t *qidx, const uint32_t *qstart,
                uint32_t nq, uint16_t queue_id, bool kni_enable, bool kni_accept, int kni_primary,
                void *const *mbufs, const yrss_route_ops *ops, void **out_local, void **out_kni,
                yrss_route_result *res)
{
    memset(res, 0, sizeof(*res));
    const bool local_ok = queue_id < nq;
    std::vector<uint32_t> arp;
    if (local_ok)
        for (uint32_t k = qstart[queue_id]; k < qstart[queue_id + 1]; ++k)
            if (fc[qidx[k]] == YRSS_FILTER_ARP)
                arp.push_back(qidx[k]);
    std::vector<void *> clones((size_t)arp.size() * nq, nullptr);
    std::vector<void *> kni_clone(arp.size(), nullptr);
    for (size_t a = 0; a < arp.size(); ++a) {
        void *m = mbufs[arp[a]];
        for (uint16_t j = 0; j < nq; ++j)
            if (j != queue_id)
                clones[a * nq + j] = ops->clone(ops->user, m, j);
        if (kni_enable && kni_primary)
            kni_clone[a] = ops->clone(ops->user, m, 0xFFFFu);
    }
    std::vector<void *> objs;
    for (uint16_t j = 0; j < nq; ++j) {
        if (j == queue_id)
            continue;
        objs.clear();
        uint32_t k = qstart[j];
        const uint32_t e = qstart[j + 1];
        size_t a = 0;
        while (k < e || a < arp.size()) {
            if (a < arp.size() && (k >= e || arp[a] < qidx[k])) {
                if (clones[a * nq + j])
                    objs.push_back(clones[a * nq + j]);
                ++a;
            } else {
                objs.push_back(mbufs[qidx[k++]]);
            }
        }
        unsigned done = objs.empty() ? 0u : ops->enqueue(ops->user, j, objs.data(),
                                                         (unsigned)objs.size());
        if (done > objs.size())
            done = (unsigned)objs.size();
        res->n_ring[j] = done;
        for (size_t r = done; r < objs.size(); ++r) {
            ops->release(ops->user, objs[r]);
            res->n_freed++;
        }
    }
    for (uint32_t k = qstart[nq]; k < qstart[nq + 1]; ++k) {
        ops->release(ops->user, mbufs[qidx[k]]);
        res->n_freed++;
    }
    if (local_ok) {
        size_t a = 0;
        for (uint32_t k = qstart[queue_id]; k < qstart[queue_id + 1]; ++k) {
            const uint32_t i = qidx[k];
            const int f = fc[i];
            if (f == YRSS_FILTER_ARP) {
                if (kni_clone[a])
                    out_kni[res->n_kni++] = kni_clone[a];
                ++a;
                out_local[res->n_local++] = mbufs[i];
                res->n_arp++;
            } else if (f == YRSS_FILTER_TRUNC || f == YRSS_FILTER_LOOP) {
                out_local[res->n_local++] = mbufs[i];
                res->n_unresolved++;
            } else if (kni_enable && ((f == YRSS_FILTER_KNI && kni_accept) ||
                                      (f == YRSS_FILTER_UNKNOWN && !kni_accept))) {
                out_kni[res->n_kni++] = mbufs[i];
            } else {
                out_local[res->n_local++] = mbufs[i];
            }
        }
    }
    (void)q;
}

}  // namespace

int main()
{
    const uint32_t nq = 3, queue_id = 2, rounds = 9;
    static Sink sink;
    const yrss_route_ops ops = {cb_enqueue, cb_clone, cb_release, &sink};
    for (uint32_t n : {32u, 1024u}) {
        std::vector<int16_t> q(n);
        std::vector<int8_t> fc(n);
        std::vector<uint32_t> bkt(n), rbk(n);
        std::vector<void *> mb(n), ol(2 * n), ok(2 * n);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t r = rnd() % 100u;
            q[i] = r < 5 ? 7 : (int16_t)(rnd() % nq);      // 5 % outside the queues
            const uint32_t c = rnd() % 10u;
            fc[i] = c == 0 ? YRSS_FILTER_ARP : c < 3 ? YRSS_FILTER_KNI : YRSS_FILTER_UNKNOWN;
            bkt[i] = q[i] >= 0 && (uint32_t)q[i] < nq ? (uint32_t)q[i] : nq;
            rbk[i] = bkt[i] != queue_id ? bkt[i]
                     : fc[i] == YRSS_FILTER_ARP ? nq + 2
                     : fc[i] == YRSS_FILTER_KNI ? nq + 1 : queue_id;
            mb[i] = (void *)(uintptr_t)(0x1000 + 64 * i);
        }
        auto lists = [&](const std::vector<uint32_t> &b, uint32_t nb, std::vector<uint32_t> &idx,
                         std::vector<uint32_t> &start) {
            idx.clear();
            start.assign(nb + 1, 0);
            for (uint32_t k = 0; k < nb; ++k) {
                start[k] = (uint32_t)idx.size();
                for (uint32_t i = 0; i < n; ++i)
                    if (b[i] == k)
                        idx.push_back(i);
            }
            start[nb] = n;
        };
        std::vector<uint32_t> qidx, qstart, ridx, rstart;
        lists(bkt, nq + 1, qidx, qstart);
        lists(rbk, nq + 3, ridx, rstart);
        const uint32_t reps = n == 32 ? 20000 : 1000;
        std::vector<double> t[3];
        yrss_route_result ra, rb, rc;
        for (uint32_t r = 0; r < rounds; ++r)
            for (int leg : {(int)(r % 3u), (int)((r + 1u) % 3u), (int)((r + 2u) % 3u)}) {
                const double t0 = now_ns();
                for (uint32_t k = 0; k < reps; ++k) {
                    memset(sink.fill, 0, sizeof(sink.fill));
                    if (leg == 0) {
                        if (yrss_route_lists(ridx.data(), rstart.data(), n, nq, queue_id, 1, nullptr,
                                             mb.data(), &ops, ol.data(), ok.data(), &ra))
                            return 1;
                    } else if (leg == 1) {
                        per_packet(q.data(), fc.data(), qidx.data(), qstart.data(), nq, queue_id,
                                   true, true, 1, mb.data(), &ops, ol.data(), ok.data(), &rb);
                    } else {
                        if (yrss_route_classified(q.data(), fc.data(), n, nq, queue_id, 1, 1, 1,
                                                  mb.data(), &ops, ol.data(), ok.data(), &rc))
                            return 1;
                    }
                }
                t[leg].push_back((now_ns() - t0) / reps / n);
            }
        for (const yrss_route_result *o : {&rb, &rc})
            if (ra.n_local != o->n_local || ra.n_kni != o->n_kni || ra.n_freed != o->n_freed ||
                ra.n_arp != o->n_arp || memcmp(ra.n_ring, o->n_ring, sizeof(ra.n_ring))) {
                fprintf(stderr, "the hand-offs disagree\n");
                return 1;
            }
        const char *name[3] = {"yrss_route_lists (routed lists)", "per-packet (q/filter/qidx)     ",
                               "yrss_route_classified (q/filter)"};
        for (int leg = 0; leg < 3; ++leg) {
            std::sort(t[leg].begin(), t[leg].end());
            printf("n %4u  %s  %6.2f ns/pkt median [%.2f-%.2f] over %u rounds of %u bursts\n", n,
                   name[leg], t[leg][t[leg].size() / 2], t[leg].front(), t[leg].back(), rounds,
                   reps);
        }
    }
    return 0;
}
