/*
 * yrss_remote_ext.h — the extended mode (yrss_set_extended in yrss.h: THIS
 * BUILD'S OWN SEMANTICS, NOT fs/lib's) for a yrss_remote client.  Kept apart
 * from yrss_remote.h, whose six calls compute the reference's results and
 * nothing else; defined in the same library (libyrss_remote.so, no HIP).
 */
#ifndef YRSS_REMOTE_EXT_H
#define YRSS_REMOTE_EXT_H

#include "yrss_remote.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The extended mode (YRSS_EXT_* flags) for the helper's context.  The flags
 * are stored in the ring and the helper is replaced by a fresh one, as
 * yrss_remote_restart replaces it; the new helper sets them on its context
 * before it serves its first burst, and its persistent worker follows them
 * (yrss_worker_start_flags, YRSS_WORKER_F_EXTENDED).  Every later
 * yrss_remote_restart keeps them.  flags == 0, the state after
 * yrss_remote_start, is the reference's rules exactly.  -EINVAL on unknown
 * bits; -EBUSY while a submitted ticket has not been polled (it was queued
 * under the old flags); otherwise what yrss_remote_restart returns. */
int yrss_remote_set_extended(yrss_remote *r, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif /* YRSS_REMOTE_EXT_H */
