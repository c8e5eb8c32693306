// Stand-alone host check of yrss_route_lists (yastack_amd/csrc/yrss_seg.cpp),
// meant for a sanitizer build on the CPU; no GPU, no Python:
//   g++ -O1 -g -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I include tools/route_lists_check.cpp yastack_amd/csrc/yrss_seg.cpp
//       -o route_lists_check && ./route_lists_check
// The global-list twin of tools/route_seg_check.cpp.  Every array is
// heap-allocated at exactly the size the contract states (ridx n words, rstart
// nb_queues + 4, filter / objs / out_local / out_kni n), so a read or write
// past it is an AddressSanitizer report.  Valid inputs (random route classes,
// burst sizes from 0 to 4096, 1 / 4 / 61 queues, every queue_id kind, rings
// that fill up, clones that fail) must equal a per-packet restatement of
// process_packets and hand every packet off exactly once; corrupted ones (each
// offset and a stride of index words set to every interesting value, then
// random words) must either give -EINVAL with no callback recorded, or, where
// the arrays stay consistent, again hand every packet off exactly once.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "yrss.h"

namespace {

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 32);
}

// Objects are small integers cast to pointers: packet i is i + 1, the clone of
// packet i for queue j (nq: the KNI clone) is kCloneBase + i * 64 + j.
constexpr uintptr_t kCloneBase = 1u << 24;

struct Recorder {
    uint32_t nq = 0, cap = 0;
    uint64_t calls = 0;
    std::vector<std::vector<uintptr_t>> ring;
    std::vector<uintptr_t> released;
};

bool clone_ok(uintptr_t pkt, uint32_t j) { return (pkt * 7u + j) % 5u != 0u; }

unsigned cb_enqueue(void *user, uint16_t queue, void *const *objs, unsigned n)
{
    Recorder *r = (Recorder *)user;
    r->calls++;
    if (queue >= r->nq) {
        fprintf(stderr, "enqueue to queue %u of %u\n", queue, r->nq);
        abort();
    }
    unsigned k = 0;
    while (k < n && r->ring[queue].size() < r->cap)
        r->ring[queue].push_back((uintptr_t)objs[k++]);
    return k;
}

void *cb_clone(void *user, void *m, uint16_t queue)
{
    Recorder *r = (Recorder *)user;
    r->calls++;
    const uintptr_t i = (uintptr_t)m - 1u;
    const uint32_t j = queue == 0xFFFFu ? r->nq : queue;
    return clone_ok(i, j) ? (void *)(kCloneBase + i * 64u + j) : nullptr;
}

void cb_release(void *user, void *m)
{
    Recorder *r = (Recorder *)user;
    r->calls++;
    r->released.push_back((uintptr_t)m);
}

struct Case {
    uint32_t n, nq, nrb, queue_id;
    std::vector<uint32_t> bkt;           // the route class of every packet
    std::unique_ptr<uint32_t[]> idx;     // exactly n words
    std::unique_ptr<uint32_t[]> off;     // exactly nrb + 1
    std::unique_ptr<int8_t[]> filter;    // exactly n
    std::unique_ptr<void *[]> objs;      // exactly n
};

Case make(uint32_t n, uint32_t nq, uint32_t queue_id)
{
    Case c;
    c.n = n;
    c.nq = nq;
    c.nrb = nq + 3;
    c.queue_id = queue_id;
    c.idx.reset(new uint32_t[n ? n : 1]);
    c.off.reset(new uint32_t[c.nrb + 1]);
    c.filter.reset(new int8_t[n ? n : 1]);
    c.objs.reset(new void *[n ? n : 1]);
    c.bkt.resize(n);
    for (uint32_t i = 0; i < n; ++i) {
        // no local queue: the KNI and ARP classes stay empty; a third of the
        // packets on the lcore's own classes where there is one
        uint32_t b = rnd() % (queue_id < nq ? c.nrb : nq + 1);
        if (queue_id < nq && rnd() % 3u == 0)
            b = rnd() % 3u == 0 ? queue_id : nq + 1 + rnd() % 2u;
        c.bkt[i] = b;
        c.filter[i] = b == queue_id && rnd() % 7u == 0 ? YRSS_FILTER_TRUNC : YRSS_FILTER_UNKNOWN;
        c.objs[i] = (void *)(uintptr_t)(i + 1u);
    }
    uint32_t w = 0;
    for (uint32_t b = 0; b < c.nrb; ++b) {
        c.off[b] = w;
        for (uint32_t i = 0; i < n; ++i)
            if (c.bkt[i] == b)
                c.idx[w++] = i;
    }
    c.off[c.nrb] = w;
    return c;
}

struct Outcome {
    int rc;
    Recorder rec;
    std::vector<uintptr_t> local, kni;
    yrss_route_result res;
};

Outcome run(const Case &c, uint32_t cap, int kni_clone, bool with_filter)
{
    Outcome o;
    o.rec.nq = c.nq;
    o.rec.cap = cap;
    o.rec.ring.resize(c.nq);
    // exactly n slots each
    std::unique_ptr<void *[]> local(new void *[c.n ? c.n : 1]), kni(new void *[c.n ? c.n : 1]);
    const yrss_route_ops ops = {cb_enqueue, cb_clone, cb_release, &o.rec};
    o.rc = yrss_route_lists(c.idx.get(), c.off.get(), c.n, (uint16_t)c.nq, (uint16_t)c.queue_id,
                            kni_clone, with_filter ? c.filter.get() : nullptr, c.objs.get(), &ops,
                            local.get(), kni.get(), &o.res);
    if (o.rc == 0) {
        if (o.res.n_local > c.n || o.res.n_kni > c.n) {
            fprintf(stderr, "n_local %u / n_kni %u beyond n %u\n", o.res.n_local, o.res.n_kni, c.n);
            abort();
        }
        for (uint32_t i = 0; i < o.res.n_local; ++i)
            o.local.push_back((uintptr_t)local[i]);
        for (uint32_t i = 0; i < o.res.n_kni; ++i)
            o.kni.push_back((uintptr_t)kni[i]);
    }
    return o;
}

// every packet object is handed to exactly one place
void check_once(const Case &c, const Outcome &o)
{
    std::vector<uint32_t> seen(c.n, 0);
    auto mark = [&](uintptr_t a) {
        if (a >= 1 && a <= c.n)
            seen[a - 1]++;
        else if (a < kCloneBase) {
            fprintf(stderr, "unknown object %zu\n", (size_t)a);
            abort();
        }
    };
    for (const auto &r : o.rec.ring)
        for (uintptr_t a : r)
            mark(a);
    for (uintptr_t a : o.rec.released)
        mark(a);
    for (uintptr_t a : o.local)
        mark(a);
    for (uintptr_t a : o.kni)
        mark(a);
    for (uint32_t i = 0; i < c.n; ++i)
        if (seen[i] != 1) {
            fprintf(stderr, "packet %u handed off %u times (n %u)\n", i, seen[i], c.n);
            abort();
        }
}

// process_packets one packet at a time over the classes the case was built from
void check_model(const Case &c, const Outcome &o, uint32_t cap, int kni_clone, bool with_filter)
{
    std::vector<std::vector<uintptr_t>> ring(c.nq);
    std::vector<uintptr_t> local, kni;
    uint32_t freed = 0, arp = 0, unresolved = 0;
    for (uint32_t i = 0; i < c.n; ++i) {
        const uint32_t b = c.bkt[i];
        const uintptr_t m = i + 1u;
        if (b == c.nq) {
            freed++;
        } else if (b < c.nq && b != c.queue_id) {
            if (ring[b].size() < cap)
                ring[b].push_back(m);
            else
                freed++;
        } else if (b == c.nq + 2) {
            for (uint32_t j = 0; j < c.nq; ++j) {
                if (j == c.queue_id || !clone_ok(i, j))
                    continue;
                if (ring[j].size() < cap)
                    ring[j].push_back(kCloneBase + i * 64u + j);
                else
                    freed++;
            }
            if (kni_clone && clone_ok(i, c.nq))
                kni.push_back(kCloneBase + i * 64u + c.nq);
            local.push_back(m);
            arp++;
        } else if (b == c.nq + 1) {
            kni.push_back(m);
        } else {
            local.push_back(m);
            if (with_filter && c.filter[i] == YRSS_FILTER_TRUNC)
                unresolved++;
        }
    }
    bool ok = o.rc == 0 && o.rec.ring == ring && o.local == local && o.kni == kni &&
              o.res.n_freed == freed && o.rec.released.size() == freed && o.res.n_arp == arp &&
              o.res.n_unresolved == unresolved;
    for (uint32_t j = 0; ok && j < c.nq; ++j)
        ok = o.res.n_ring[j] == ring[j].size();
    if (!ok) {
        fprintf(stderr, "valid case n %u nq %u queue_id %u cap %u: differs from the model (rc %d)\n",
                c.n, c.nq, c.queue_id, cap, o.rc);
        abort();
    }
}

}  // namespace

int main()
{
    uint64_t valid = 0, refused = 0, consistent = 0;
    const uint32_t sizes[] = {0, 1, 2, 32, 65, 1024, 4096};
    const uint32_t queues[] = {1, 4, YRSS_ROUTE_LISTS_MAX_QUEUES};
    for (uint32_t nq : queues)
        for (uint32_t n : sizes)
            for (uint32_t qsel = 0; qsel < 3; ++qsel) {
                const uint32_t queue_id = qsel == 0 ? 0 : qsel == 1 ? nq - 1 : nq;
                for (uint32_t cap : {1u << 20, 37u}) {
                    Case c = make(n, nq, queue_id);
                    const int kni_clone = (int)(rnd() & 1u);
                    const bool with_filter = rnd() & 1u;
                    Outcome o = run(c, cap, kni_clone, with_filter);
                    check_model(c, o, cap, kni_clone, with_filter);
                    check_once(c, o);
                    valid++;
                }
            }
    // nb_queues beyond the limit, with an offset row sized for the claimed layout
    {
        Case c = make(300, 13, 0);
        const uint32_t nq = YRSS_ROUTE_LISTS_MAX_QUEUES + 1u;
        std::unique_ptr<uint32_t[]> off(new uint32_t[nq + 4]());
        off[nq + 3] = 300;
        Recorder rec;
        rec.nq = nq;
        const yrss_route_ops ops = {cb_enqueue, cb_clone, cb_release, &rec};
        std::unique_ptr<void *[]> l(new void *[300]), k(new void *[300]);
        yrss_route_result res;
        const int rc = yrss_route_lists(c.idx.get(), off.get(), 300, (uint16_t)nq, 0, 1, nullptr,
                                        c.objs.get(), &ops, l.get(), k.get(), &res);
        if (rc != -EINVAL || rec.calls) {
            fprintf(stderr, "nb_queues %u: rc %d, %llu callbacks\n", nq, rc,
                    (unsigned long long)rec.calls);
            abort();
        }
        refused++;
    }
    auto corrupted = [&](Case &c, uint32_t cap) {
        Outcome o = run(c, cap, 1, true);
        if (o.rc == -EINVAL) {
            if (o.rec.calls) {
                fprintf(stderr, "-EINVAL after %llu callbacks\n", (unsigned long long)o.rec.calls);
                abort();
            }
            refused++;
        } else if (o.rc == 0) {
            check_once(c, o);
            consistent++;
        } else {
            fprintf(stderr, "unexpected rc %d\n", o.rc);
            abort();
        }
    };
    const uint32_t offv[] = {0, 1, 149, 150, 299, 300, 301, 4096, 0x77777777u, 0xFFFFFFFFu};
    const uint32_t idxv[] = {0, 1, 150, 299, 300, 301, 0x10000u, 0x80000000u, 0xFFFFFFFFu};
    for (uint32_t queue_id : {0u, 4u}) {
        const uint32_t n = 300, nq = 4;
        Case ref = make(n, nq, queue_id);
        auto copy_of_ref = [&]() {
            Case c = make(n, nq, queue_id);
            memcpy(c.idx.get(), ref.idx.get(), n * sizeof(uint32_t));
            memcpy(c.off.get(), ref.off.get(), (ref.nrb + 1) * sizeof(uint32_t));
            memcpy(c.filter.get(), ref.filter.get(), n);
            c.bkt = ref.bkt;
            return c;
        };
        for (uint32_t e = 0; e <= ref.nrb; ++e)
            for (uint32_t v : offv) {
                Case c = copy_of_ref();
                c.off[e] = v;
                corrupted(c, 1u << 20);
            }
        for (uint32_t e = 0; e < n; e += 7)
            for (uint32_t v : idxv) {
                Case c = copy_of_ref();
                c.idx[e] = v;
                corrupted(c, 37);
            }
        for (uint32_t round = 0; round < 2000; ++round) {
            Case c = make(n, nq, queue_id);
            const uint32_t hits = 1 + rnd() % 4;
            for (uint32_t h = 0; h < hits; ++h) {
                if (rnd() & 1u)
                    c.off[rnd() % (c.nrb + 1)] = rnd() % 320u;
                else
                    c.idx[rnd() % n] = rnd() & 1u ? rnd() % 320u : rnd();
            }
            corrupted(c, 37);
        }
    }
    printf("route_lists_check: %llu valid cases equal the per-packet model, %llu corrupted refused "
           "with -EINVAL before any callback, %llu corrupted but consistent handed off once\n",
           (unsigned long long)valid, (unsigned long long)refused, (unsigned long long)consistent);
    return 0;
}
