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
#include <errno.h>
#include <stdint.h>

#include "yrss.h"

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

}  // extern "C"
