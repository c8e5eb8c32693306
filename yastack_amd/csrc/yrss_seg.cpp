// yrss_seg.cpp — the segmented per-queue lists of yrss_dispatch_dev_seg as the
// batch-wide qidx / qstart of yrss_dispatch_dev.  Host-only; no HIP calls.
//
// The reference enqueues burst by burst, in order, into dispatch_ring[port][q]
// (fs/lib/ff_dpdk_if.c:1087-1093 inside the :1674-1683 loop); a consumer of
// the segmented form does the same, segment by segment.  This helper is for
// callers that want the batch-wide list instead (and for the tests): bucket
// b's list is its segments' lists concatenated in segment order.  The input
// arrays come from a device buffer the caller may have mis-sized or not yet
// synchronised, so nothing read from them is used as an index before it is
// checked.  yastack_amd/segments.py is the Python twin.
//
// process_packets' hand-off (ff_dpdk_if.c:1058-1140) is written once, here, as
// walks over route-class lists (route_hand_off), and has three entries.
// yrss_route_seg consumes the routed form of yrss_route_dev_seg (nb_queues + 3
// route buckets a segment), where the parse kernel has already decided every
// packet's class.  yrss_route_lists does the same from the one global routed
// list of a host burst or a route worker's burst (yrss_route_lists_*,
// yrss_worker_start_route).  yrss_route_classified (yrss_route_internal.h, not
// exported) is yrss_route_burst's: that call gets q and filter per packet from
// the GPU, so the classes are sorted out of them here, for any nb_queues.
#include <errno.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <new>

#include "yrss.h"
#include "yrss_route_internal.h"

extern "C" {

int yrss_seg_to_lists(const uint8_t *seg_idx, const uint16_t *seg_off, uint32_t n,
                      uint32_t nbk, uint32_t *out_qidx, uint32_t *out_qstart)
{
    if (nbk < 1 || nbk > YRSS_MAX_QUEUES + 1 || !out_qstart)
        return -EINVAL;
    if (n && (!seg_idx || !seg_off || !out_qidx))
        return -EINVAL;
    const uint32_t nseg = n / YRSS_SEG_PKTS + (n % YRSS_SEG_PKTS ? 1u : 0u);
    // pass 1: every offset row is 0 .. len_s, monotone; bucket totals
    for (uint32_t b = 0; b <= nbk; ++b)
        out_qstart[b] = 0;
    for (uint32_t s = 0; s < nseg; ++s) {
        const uint16_t *o = seg_off + (size_t)s * (nbk + 1u);
        const uint32_t len = n - s * YRSS_SEG_PKTS < YRSS_SEG_PKTS ? n - s * YRSS_SEG_PKTS
                                                                   : (uint32_t)YRSS_SEG_PKTS;
        if (o[0] != 0 || o[nbk] != len)
            return -EINVAL;
        for (uint32_t b = 0; b < nbk; ++b) {
            if (o[b + 1] < o[b])
                return -EINVAL;
            out_qstart[b + 1] += (uint32_t)(o[b + 1] - o[b]);
        }
    }
    for (uint32_t b = 0; b < nbk; ++b)   // counts (at b + 1) -> exclusive starts
        out_qstart[b + 1] += out_qstart[b];
    // pass 2: append segment by segment; out_qstart[b + 1] is bucket b's end,
    // so the cursors are kept apart from it: bucket b writes at start + done
    uint32_t done[YRSS_MAX_QUEUES + 1] = {0};
    for (uint32_t s = 0; s < nseg; ++s) {
        const uint16_t *o = seg_off + (size_t)s * (nbk + 1u);
        const uint8_t *idx = seg_idx + (size_t)s * YRSS_SEG_PKTS;
        const uint32_t len = o[nbk];
        for (uint32_t b = 0; b < nbk; ++b) {
            uint32_t w = out_qstart[b] + done[b];
            for (uint32_t k = o[b]; k < o[b + 1]; ++k) {
                if (idx[k] >= len)
                    return -EINVAL;
                out_qidx[w++] = s * YRSS_SEG_PKTS + idx[k];
            }
            done[b] += (uint32_t)(o[b + 1] - o[b]);
        }
    }
    return 0;
}

// Every offset row 0 .. len_s and monotone, every index byte below len_s and
// (a packet handed off twice would be freed twice) present once in its segment.
static int route_seg_valid(const uint8_t *seg_idx, const uint16_t *seg_off, uint32_t n,
                           uint32_t nq, bool local_ok)
{
    const uint32_t nrb = nq + 3u;
    const uint32_t nseg = n / YRSS_SEG_PKTS + (n % YRSS_SEG_PKTS ? 1u : 0u);
    for (uint32_t s = 0; s < nseg; ++s) {
        const uint16_t *o = seg_off + (size_t)s * (nrb + 1u);
        const uint8_t *idx = seg_idx + (size_t)s * YRSS_SEG_PKTS;
        const uint32_t len = n - s * YRSS_SEG_PKTS < YRSS_SEG_PKTS ? n - s * YRSS_SEG_PKTS
                                                                   : (uint32_t)YRSS_SEG_PKTS;
        if (o[0] != 0 || o[nrb] != len)
            return -EINVAL;
        for (uint32_t b = 0; b < nrb; ++b)
            if (o[b + 1] < o[b])
                return -EINVAL;
        // no local queue: nothing can be KNI or local ARP
        if (!local_ok && o[nq + 1u] != len)
            return -EINVAL;
        uint64_t seen[YRSS_SEG_PKTS / 64] = {0};
        for (uint32_t k = 0; k < len; ++k) {
            const uint32_t i = idx[k];
            if (i >= len || (seen[i >> 6] >> (i & 63u)) & 1u)
                return -EINVAL;
            seen[i >> 6] |= 1ull << (i & 63u);
        }
    }
    return 0;
}

}  // extern "C"

// process_packets' hand-off (ff_dpdk_if.c:1058-1140) over one set of finished
// route lists: idx the packet indices (into m and, offset by first, into
// filter) grouped by route class, o the nq + 4 offsets, already validated.
// Shared by the segments of yrss_route_seg (8-bit indices, 16-bit offsets), the
// one global list of yrss_route_lists and the list yrss_route_classified sorts
// for yrss_route_burst (32-bit both).  Scratch from the
// caller: cl (ARP packets x nq clones), kc (one KNI clone per ARP packet),
// burst (as many objects as one ring can be offered: packets + ARP packets).
template <typename Idx, typename Off>
static void route_hand_off(const Idx *idx, const Off *o, void *const *m, uint32_t first,
                           uint32_t nq, uint16_t queue_id, int kni_clone, const int8_t *filter,
                           const struct yrss_route_ops *ops, void **out_local, void **out_kni,
                           struct yrss_route_result *res, void **cl, void **kc, void **burst)
{
    // ARP kept on this lcore is deep-cloned to every other queue, in packet
    // order, queue order inside a packet, then once more for KNI
    // (ff_dpdk_if.c:1099-1129)
    const Idx *arp = idx + o[nq + 2u];
    const uint32_t na = (uint32_t)(o[nq + 3u] - o[nq + 2u]);
    for (uint32_t a = 0; a < na; ++a) {
        for (uint16_t j = 0; j < nq; ++j)
            cl[(size_t)a * nq + j] = j != queue_id ? ops->clone(ops->user, m[arp[a]], j) : nullptr;
        kc[a] = kni_clone ? ops->clone(ops->user, m[arp[a]], 0xFFFFu) : nullptr;
    }
    // one FIFO burst per ring: bucket j merged by packet index with the
    // clones for j (a failed clone enqueues nothing, :1114-1118)
    for (uint16_t j = 0; j < nq; ++j) {
        if (j == queue_id)
            continue;
        uint32_t k = o[j], nb = 0, a = 0;
        const uint32_t e = o[j + 1];
        while (k < e || a < na) {
            if (a < na && (k >= e || arp[a] < idx[k])) {
                if (cl[(size_t)a * nq + j])
                    burst[nb++] = cl[(size_t)a * nq + j];
                ++a;
            } else {
                burst[nb++] = m[idx[k++]];
            }
        }
        unsigned done = nb ? ops->enqueue(ops->user, j, burst, nb) : 0u;
        if (done > nb)
            done = nb;
        res->n_ring[j] += done;
        for (uint32_t r = done; r < nb; ++r) {      // ring full: free (:1090)
            ops->release(ops->user, burst[r]);
            res->n_freed++;
        }
    }
    // ret < 0 || ret >= nb_queues: freed (:1080-1083)
    for (uint32_t k = o[nq]; k < o[nq + 1u]; ++k) {
        ops->release(ops->user, m[idx[k]]);
        res->n_freed++;
    }
    if (queue_id >= nq)
        return;
    // local input, in packet order: the local bucket and the ARP packets
    uint32_t k = o[queue_id], a = 0;
    const uint32_t e = o[queue_id + 1u];
    while (k < e || a < na) {
        if (a < na && (k >= e || arp[a] < idx[k])) {
            out_local[res->n_local++] = m[arp[a++]];
            res->n_arp++;
        } else {
            const uint32_t i = idx[k++];
            if (filter && (filter[first + i] == YRSS_FILTER_TRUNC ||
                           filter[first + i] == YRSS_FILTER_LOOP))
                res->n_unresolved++;
            out_local[res->n_local++] = m[i];
        }
    }
    // ff_kni_enqueue, in packet order: the KNI bucket and the KNI clones
    k = o[nq + 1u];
    a = 0;
    const uint32_t ek = o[nq + 2u];
    while (k < ek || a < na) {
        if (a < na && (k >= ek || arp[a] < idx[k])) {
            if (kc[a])
                out_kni[res->n_kni++] = kc[a];
            ++a;
        } else {
            out_kni[res->n_kni++] = m[idx[k++]];
        }
    }
}

// The host twin of the parse kernel's route_bucket (yrss.hip): what
// process_packets does with a packet of queue q and filter class fc on the
// lcore whose queue is queue_id, as a class below nq + 3: b < nq the ring of
// queue b, or local delivery where b == queue_id; nq freed; nq + 1 KNI; nq + 2
// ARP on the local queue.  queue_id >= nq: no local queue, classes <= nq only.
static inline uint32_t route_class(int q, int fc, uint32_t nq, uint32_t queue_id, bool kni_enable,
                                   bool kni_accept)
{
    if ((uint32_t)q >= nq)                 // q < 0 included
        return nq;
    if ((uint32_t)q != queue_id)
        return (uint32_t)q;
    if (fc == YRSS_FILTER_ARP)
        return nq + 2u;
    const bool kni = kni_enable && fc == (kni_accept ? YRSS_FILTER_KNI : YRSS_FILTER_UNKNOWN);
    return kni ? nq + 1u : (uint32_t)q;
}

extern "C" {

int yrss_route_classified(const int16_t *q, const int8_t *filter, uint32_t n, uint16_t nb_queues,
                          uint16_t queue_id, int kni_enable, int kni_accept, int kni_primary,
                          void *const *objs, const struct yrss_route_ops *ops, void **out_local,
                          void **out_kni, struct yrss_route_result *res)
{
    if (!ops || !ops->enqueue || !ops->clone || !ops->release || !res)
        return -EINVAL;
    if (nb_queues < 1 || nb_queues > YRSS_MAX_QUEUES)
        return -EINVAL;
    if (n && (!q || !filter || !objs || !out_local || !out_kni))
        return -EINVAL;
    memset(res, 0, sizeof(*res));
    if (n == 0)
        return 0;
    const uint32_t nq = nb_queues, nrb = nq + 3u;
    // stable counting sort by class: counts (at b + 1) -> exclusive starts
    uint32_t rstart[YRSS_MAX_QUEUES + 4] = {0}, cur[YRSS_MAX_QUEUES + 3];
    for (uint32_t i = 0; i < n; ++i)
        rstart[route_class(q[i], filter[i], nq, queue_id, kni_enable, kni_accept) + 1u]++;
    for (uint32_t b = 0; b < nrb; ++b) {
        rstart[b + 1] += rstart[b];
        cur[b] = rstart[b];
    }
    // one allocation: route_hand_off's scratch as yrss_route_lists sizes it (the
    // ARP packets' clones, one ring's burst), then the list
    const size_t na = rstart[nq + 3u] - rstart[nq + 2u];
    void **scratch = (void **)malloc((na * nq + na + n) * sizeof(void *) + n * sizeof(uint32_t));
    if (!scratch)
        return -ENOMEM;
    uint32_t *ridx = (uint32_t *)(scratch + na * nq + na + n);
    for (uint32_t i = 0; i < n; ++i)
        ridx[cur[route_class(q[i], filter[i], nq, queue_id, kni_enable, kni_accept)]++] = i;
    route_hand_off(ridx, rstart, objs, 0u, nq, queue_id, kni_enable && kni_primary, filter, ops,
                   out_local, out_kni, res, scratch, scratch + na * nq, scratch + na * nq + na);
    free(scratch);
    return 0;
}

int yrss_route_seg(const uint8_t *seg_idx, const uint16_t *seg_off, uint32_t n,
                   uint16_t nb_queues, uint16_t queue_id, int kni_clone, const int8_t *filter,
                   void *const *objs, const struct yrss_route_ops *ops, void **out_local,
                   void **out_kni, struct yrss_route_result *res)
{
    if (!ops || !ops->enqueue || !ops->clone || !ops->release || !res)
        return -EINVAL;
    if (nb_queues < 1 || nb_queues > YRSS_ROUTE_SEG_MAX_QUEUES)
        return -EINVAL;
    if (n && (!seg_idx || !seg_off || !objs || !out_local || !out_kni))
        return -EINVAL;
    const uint32_t nq = nb_queues, nrb = nq + 3u;
    const bool local_ok = queue_id < nq;
    memset(res, 0, sizeof(*res));
    if (route_seg_valid(seg_idx, seg_off, n, nq, local_ok))
        return -EINVAL;
    const uint32_t nseg = n / YRSS_SEG_PKTS + (n % YRSS_SEG_PKTS ? 1u : 0u);
    void *cl[YRSS_SEG_PKTS * YRSS_ROUTE_SEG_MAX_QUEUES];
    void *kc[YRSS_SEG_PKTS];
    void *burst[YRSS_SEG_PKTS];
    for (uint32_t s = 0; s < nseg; ++s)
        route_hand_off(seg_idx + (size_t)s * YRSS_SEG_PKTS, seg_off + (size_t)s * (nrb + 1u),
                       objs + (size_t)s * YRSS_SEG_PKTS, s * YRSS_SEG_PKTS, nq, queue_id,
                       kni_clone, filter, ops, out_local, out_kni, res, cl, kc, burst);
    return 0;
}

int yrss_route_lists(const uint32_t *ridx, const uint32_t *rstart, uint32_t n,
                     uint16_t nb_queues, uint16_t queue_id, int kni_primary,
                     const int8_t *filter, void *const *objs, const struct yrss_route_ops *ops,
                     void **out_local, void **out_kni, struct yrss_route_result *res)
{
    if (!ops || !ops->enqueue || !ops->clone || !ops->release || !res || !rstart)
        return -EINVAL;
    if (nb_queues < 1 || nb_queues > YRSS_ROUTE_LISTS_MAX_QUEUES)
        return -EINVAL;
    if (n && (!ridx || !objs || !out_local || !out_kni))
        return -EINVAL;
    const uint32_t nq = nb_queues, nrb = nq + 3u;
    memset(res, 0, sizeof(*res));
    // the offsets 0 .. n and monotone; no local queue: nothing can be KNI or
    // local ARP
    if (rstart[0] != 0 || rstart[nrb] != n)
        return -EINVAL;
    for (uint32_t b = 0; b < nrb; ++b)
        if (rstart[b + 1] < rstart[b])
            return -EINVAL;
    if (queue_id >= nq && rstart[nq + 1u] != n)
        return -EINVAL;
    if (n == 0)
        return 0;
    // scratch: the ARP packets' clones, one ring's burst (at most every
    // packet once, itself or as its clone), and the seen bits of the check
    // that every index is below n and present once (a packet handed off twice
    // would be freed twice)
    const size_t na = rstart[nq + 3u] - rstart[nq + 2u];
    const size_t words = ((size_t)n + 63u) / 64u;
    void **scratch = new (std::nothrow) void *[na * nq + na + n];
    uint64_t *seen = new (std::nothrow) uint64_t[words]();
    int rc = scratch && seen ? 0 : -ENOMEM;
    for (uint32_t k = 0; rc == 0 && k < n; ++k) {
        const uint32_t i = ridx[k];
        if (i >= n || (seen[i >> 6] >> (i & 63u)) & 1u)
            rc = -EINVAL;
        else
            seen[i >> 6] |= 1ull << (i & 63u);
    }
    if (rc == 0)
        route_hand_off(ridx, rstart, objs, 0u, nq, queue_id, kni_primary, filter, ops, out_local,
                       out_kni, res, scratch, scratch + na * nq, scratch + na * nq + na);
    delete[] scratch;
    delete[] seen;
    return rc;
}

}  // extern "C"
