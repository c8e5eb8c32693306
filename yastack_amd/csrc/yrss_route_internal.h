// yrss_route_internal.h — private to libyrss.so (not installed, not exported):
// the hand-off entry behind yrss_route_burst, defined in yrss_seg.cpp beside
// the one hand-off routine it shares with yrss_route_seg and yrss_route_lists.
#ifndef YRSS_ROUTE_INTERNAL_H
#define YRSS_ROUTE_INTERNAL_H

#include "yrss.h"

#ifdef __cplusplus
extern "C" {
#endif

/* process_packets' hand-off (ff_dpdk_if.c:1058-1140) for n classified packets:
 * q[i] / filter[i] as the parse kernel wrote them, objs[i] the mbuf.  Sorts the
 * packets by route class (stable, so every class keeps packet order) and runs
 * the hand-off of yrss_route_lists on that list; the list is made here, so it
 * is not validated again.  nb_queues 1..YRSS_MAX_QUEUES; queue_id >= nb_queues:
 * no local queue.  out_local / out_kni, res and the callbacks' order as
 * yrss_route_burst documents.  0, -EINVAL, or -ENOMEM before any callback. */
__attribute__((visibility("hidden")))
int yrss_route_classified(const int16_t *q, const int8_t *filter, uint32_t n, uint16_t nb_queues,
                          uint16_t queue_id, int kni_enable, int kni_accept, int kni_primary,
                          void *const *objs, const struct yrss_route_ops *ops, void **out_local,
                          void **out_kni, struct yrss_route_result *res);

#ifdef __cplusplus
}
#endif

#endif
