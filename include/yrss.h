/*
 * yrss.h — C ABI of the MI355X software-RSS engine (parse + Toeplitz hash +
 * per-queue dispatch) that replaces yastack / F-Stack's soft-dispatch path.
 *
 * Reference path being replaced (all paths relative to the yastack tree):
 *   fs/lib/ff_api.h:167-174        dispatch_func_t, ff_regist_packet_dispatcher,
 *                                  toeplitz_dispatch prototypes
 *   fs/lib/ff_dpdk_if.c:1881-1902  toeplitz_hash (bit-serial Toeplitz)
 *   fs/lib/ff_dpdk_if.c:1945-2113  toeplitz_dispatch (L2/L3/L4 parse + queue)
 *   fs/lib/ff_dpdk_if.c:1058-1094  process_packets dispatcher block (drop if
 *                                  ret<0 || ret>=nb_queues, else enqueue to
 *                                  dispatch_ring[port][ret])
 *   fs/lib/ff_dpdk_if.c:1653-1683  main_loop_vm_3 RX burst → per-packet loop
 *
 * The reference calls its dispatcher once per packet on the CPU.  This ABI is
 * burst-shaped instead: the hook sits between rte_eth_rx_burst
 * (ff_dpdk_if.c:1655) and the per-packet loop (:1674), classifies a whole
 * batch on the GPU, and returns per-packet {queue, hash} plus per-queue FIFO
 * index lists (the device-side analogue of dispatch_ring[port][q]).
 *
 * Everything here is plain C: pointers, sizes, ints.  No HIP or torch types
 * appear in signatures; device pointers are `void *`/typed pointers to device
 * memory and HIP streams are passed as `void *` (hipStream_t, NULL = default).
 *
 * Errors: every int-returning call returns 0 on success or a negative errno
 * (-EINVAL bad argument, -ENOMEM allocation failure, -ENODEV no usable GPU,
 * -EIO HIP runtime failure).  This mirrors the reference's only error channel
 * (the sign of the dispatcher's return, ff_api.h:160-163) — there is no errno.
 */
#ifndef YRSS_H
#define YRSS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YRSS_VERSION_STRING "yrss 0.1.0 (gfx950)"

/* ---- constants mirrored from the reference -------------------------------- */

/* Toeplitz key length used by the reference: sizeof(default_rsskey_40bytes),
 * fs/lib/ff_dpdk_if.c:113-119. */
#define YRSS_RSS_KEY_LEN 40

/* Default queue returned for every packet the reference does not hash
 * (`uint16_t default_Q = 2`, ff_dpdk_if.c:1948). */
#define YRSS_DEFAULT_Q 2

/* Queue written for a hashed TCP packet whose L4 ports lie beyond the bytes
 * the caller staged in its header window (only possible when win_stride < 78
 * and data_len > win_stride).  Never produced by yrss_dispatch_burst /
 * yrss_dispatch_frames, which always stage enough bytes (on the reference's
 * rules; see yrss_set_extended for tagged IPv4 with a large IHL).  Such packets
 * land in the drop bucket, like any ret outside [0, nb_queues). */
#define YRSS_Q_TRUNCATED (-2)

/* Widest header window the parse ever needs: with IHL=15 the TCP ports sit at
 * bytes 74..77 (14 + 60 + 4).  A window stride >= 80 never truncates. */
#define YRSS_WIN_FULL 80
/* Minimum window stride: one 64-byte coalesced header block per packet. */
#define YRSS_WIN_MIN 64

/* Largest supported values (queues are buckets of the compaction; q is int16;
 * packet indices stay well inside uint32 arithmetic). */
#define YRSS_MAX_QUEUES 256
#define YRSS_MAX_PROCS 4096
#define YRSS_MAX_BATCH (1u << 31)

/* struct rte_mbuf field offsets for the in-tree DPDK 18.02 (x86_64), measured
 * from dpdk/lib/librte_mbuf/rte_mbuf.h:412-560.  The burst API reads
 * buf_addr/data_off/data_len and may write hash.rss; callers on another DPDK
 * version override them in yrss_config.mbuf. */
#define YRSS_MBUF_OFF_BUF_ADDR 0
#define YRSS_MBUF_OFF_DATA_OFF 16
#define YRSS_MBUF_OFF_DATA_LEN 40
#define YRSS_MBUF_OFF_HASH_RSS 44

struct yrss_mbuf_layout {
    uint16_t off_buf_addr;   /* void *buf_addr                         */
    uint16_t off_data_off;   /* uint16_t data_off                      */
    uint16_t off_data_len;   /* uint16_t data_len (first segment only) */
    uint16_t off_hash_rss;   /* uint32_t hash.rss                      */
};

/* ---- configuration --------------------------------------------------------- */

/* The knobs toeplitz_dispatch / process_packets read:
 *   rss_key            default_rsskey_40bytes           ff_dpdk_if.c:113-119
 *   nb_procs           ff_global_cfg.dpdk.nb_procs      ff_config.c:133 (popcount lcore_mask)
 *   soft_dispatch      ff_global_cfg.dpdk.soft_dispatch ff_config.c:440-441
 *   dispatch_only_core ff_global_cfg.system.dispatch_only_core  ff_config.c:450-451
 *   nb_queues          qconf->nb_queue_list[port]       ff_dpdk_if.c:1063, :420
 */
struct yrss_config {
    uint8_t  rss_key[YRSS_RSS_KEY_LEN];
    uint32_t rss_key_len;          /* 4..40; the reference always uses 40   */
    int32_t  nb_procs;             /* 1..YRSS_MAX_PROCS                     */
    uint16_t nb_queues;            /* 1..YRSS_MAX_QUEUES (drop if q>=this)  */
    uint8_t  soft_dispatch;        /* 0/1                                   */
    uint8_t  dispatch_only_core;   /* 0/1; with soft_dispatch needs nb_procs>=2 */
    int32_t  device;               /* HIP device ordinal for yrss_init      */
    uint32_t max_burst;            /* host-burst staging capacity (packets) */
    struct yrss_mbuf_layout mbuf;  /* rte_mbuf offsets for the burst API    */
};

/* Fill cfg with the reference defaults: the Mellanox key, the shipped
 * fs/config/config.ini (lcore_mask=7 → nb_procs=3, soft_dispatch=1,
 * dispatch_only_core=1), nb_queues=nb_procs, device 0, DPDK 18.02 mbuf. */
void yrss_config_default(struct yrss_config *cfg);

/* Validate without touching the GPU.  Rejects what the reference would divide
 * by zero on (dispatch_only_core && soft_dispatch && nb_procs < 2,
 * ff_dpdk_if.c:2031-2032) and out-of-range sizes.  0 or -EINVAL. */
int yrss_config_validate(const struct yrss_config *cfg);

/* ---- context ------------------------------------------------------------------ */

typedef struct yrss_ctx yrss_ctx;

/* Create a context bound to cfg->device: uploads the key schedule, sizes the
 * compaction workspace, allocates pinned staging for max_burst packets.
 * One context per host thread (the reference's dispatcher is single-threaded,
 * ff_dpdk_if.c:1653). */
int  yrss_init(const struct yrss_config *cfg, yrss_ctx **out);
void yrss_fini(yrss_ctx *ctx);

/* ---- device-resident dispatch (the metric path) ------------------------------ */

/* Classify n packets whose header windows already sit in HBM.
 *   d_win      window i at d_win + i*win_stride holds bytes
 *              [0, min(len_i, win_stride)) of packet i's first segment;
 *              16-byte aligned, win_stride % 16 == 0, win_stride >= 64.
 *   d_len      n x uint16 data_len (rte_pktmbuf_data_len, ff_dpdk_if.c:1076)
 *   d_q        n x int16 queue = toeplitz_dispatch's return
 *   d_hash     n x uint32 Toeplitz hash (0 where the reference does not hash);
 *              may be NULL
 *   d_qidx     n x uint32 packet indices grouped by bucket, FIFO inside each
 *              bucket; may be NULL (then d_qstart is ignored)
 *   d_qstart   nb_queues+2 x uint32: bucket b in [0,nb_queues) holds the
 *              packets dispatched to queue b; bucket nb_queues holds the
 *              packets process_packets frees (ret<0 || ret>=nb_queues,
 *              ff_dpdk_if.c:1080-1083).  Bucket b = d_qidx[d_qstart[b] ..
 *              d_qstart[b+1]).  d_qstart[nb_queues+1] == n.
 *   stream     hipStream_t (NULL = legacy default stream)
 * n <= YRSS_MAX_BATCH.  Asynchronous: returns after enqueueing the kernels.
 * Batches of <= 4096 packets (with nb_queues + 1 <= 64) run as one launch of
 * the one-workgroup burst kernel instead of parse + scan + scatter (same
 * outputs; yrss_timing_* does not count it; yrss_tuning.one_launch turns it off).
 * Dispatches of one context share its compaction workspace: a dispatch on a
 * different stream than the context's previous one waits (on the device) for
 * the work already queued there, so streams may be mixed freely; dispatches
 * on one stream pay nothing for this.  yrss_fini drains the device.
 * Stream lifetime: the context remembers the stream of its last device batch
 * (the switch above, and yrss_status / yrss_fault_info synchronise it), so
 * that stream must stay alive until the context's next dispatch on another
 * stream, its next yrss_status / yrss_fault_info, or yrss_fini. */
int yrss_dispatch_dev(yrss_ctx *ctx, const uint8_t *d_win, uint32_t win_stride,
                      const uint16_t *d_len, uint32_t n, int16_t *d_q,
                      uint32_t *d_hash, uint32_t *d_qidx, uint32_t *d_qstart,
                      void *stream);

/* ---- protocol_filter / KNI ----------------------------- */

/* Per-packet protocol_filter class (fs/lib/ff_dpdk_kni.h:34-38 FilterReturn),
 * computed in the same kernel pass as the hash when requested. */
#define YRSS_FILTER_UNKNOWN (-1)
#define YRSS_FILTER_ARP 1
#define YRSS_FILTER_KNI 2
/* Boundary outcomes the reference cannot produce: the IPIP header walk left
 * the staged window, or hit IHL=0 under IPIP, where ff_kni_proto_filter
 * recurses on the same header forever (ff_dpdk_kni.c:274-275). */
#define YRSS_FILTER_TRUNC (-2)
#define YRSS_FILTER_LOOP (-3)

/* Configure KNI exactly as ff_kni_init/init_kni do (ff_dpdk_if.c:597-606,
 * ff_dpdk_kni.c:99-118,300-331): enable, method "accept"/"reject" (anything
 * else is rejected like ff_config.c:548-553), and comma/range port lists
 * ("80,443,8000-8080") parsed with kni_set_bitmap's rules into the 8 KiB
 * htons-indexed bitmaps.  NULL lists leave a bitmap empty.  On a context with
 * a route worker (yrss_worker_start_route): -EBUSY while a burst is pending,
 * otherwise the worker is halted and relaunched by the next submit. */
int yrss_set_kni(yrss_ctx *ctx, int enable, const char *method,
                 const char *tcp_ports, const char *udp_ports);

/* ---- extended mode: THIS BUILD'S OWN SEMANTICS, NOT fs/lib's ------------------ */

/* toeplitz_dispatch hashes untagged IPv4/TCP and nothing else: every UDP, IPv6
 * or VLAN-tagged packet gets the constant queue 2 (ff_dpdk_if.c:2050-2112).
 * That is the default here too, bit for bit.  The flags below are an opt-in
 * departure from the reference, per context, for deployments that want the
 * flows they carry spread; nothing in fs/lib computes these results, and the
 * hashes are validated against the 82599 datasheet vectors instead
 * (tests/golden/thash_82599.json).  The rules, applied in this order:
 *   YRSS_EXT_VLAN  The frame is classified as if hardware vlan_strip had
 *                  removed its tags: ethertype 0x8100 or 0x88A8 at byte 12
 *                  moves the L3 offset o to 18 (ethertype at byte 16); 0x8100
 *                  there again moves it to 22 (ethertype at byte 20); at most
 *                  two tags.  Every later rule sees the frame without its t
 *                  tags and with len - 4t, the reference's length quirks
 *                  included.  A frame too short to hold the tag(s) and the
 *                  inner ethertype is unhashed (queue 2); ARP / RARP under a
 *                  tag is queue 0.
 *   IPv4           The reference's rule (:1968-2035) on the stripped frame.
 *                  With YRSS_EXT_UDP protocol 17 takes the TCP branch: the
 *                  same checks, the same tuple bytes in the same order
 *                  (:1998-2021), the same hash % d (+1).
 *   YRSS_EXT_IPV6  Ethertype 0x86DD with len - o >= 44 and next-header
 *                  (byte o + 6) 6, or 17 with YRSS_EXT_UDP: the hash is the
 *                  Toeplitz of the 36 bytes src | dst | sport | dport in wire
 *                  order (the 82599 "l3l4" input), the queue as for hashed
 *                  TCP.  No extension-header walk: any other next-header is
 *                  unhashed.  Key bytes past rss_key_len count as zero, as in
 *                  toeplitz_hash (:1896).
 * Everything else is as without flags: queue 2 and hash 0, queue 0 for ARP /
 * RARP.  The window rule is unchanged: ports that end beyond the staged window
 * (o + 4 IHL + 4, or o + 44 for IPv6, > win_stride) give YRSS_Q_TRUNCATED.  At
 * stride 64 that now takes two tags with IPv6 or tags with a large IHL; at
 * YRSS_WIN_FULL (what the host bursts stage) only tagged IPv4 with
 * 4 t + 4 IHL > 62 (IHL 15 under one tag, 14 or 15 under two), which the host
 * bursts can therefore produce under YRSS_EXT_VLAN; QinQ + IPv6 ends at byte 66.
 * The protocol_filter class (filter outputs, route classes, yrss_route_burst)
 * keeps following the reference on the unstripped frame.
 *
 * Honoured by every yrss_dispatch_dev*, yrss_route_dev_seg, the host bursts
 * and frames (zero-copy and routed forms included) and by
 * yrss_toeplitz_dispatch on a context without a worker.  The persistent
 * worker honours them when it was started to:
 * yrss_worker_start_flags(..., YRSS_WORKER_F_EXTENDED) serves every
 * yrss_worker_submit* (and the shim's one-packet bursts) under the flags in
 * force at the submit; in the windows form the caller's stride sets the
 * window rule above.  A worker started by yrss_worker_start or
 * yrss_worker_start_route serves the reference's rules only and says so by
 * refusing: while flags are set those two calls, every yrss_worker_submit* on
 * such a worker and so the shim on its context return -ENOTSUP (the shim -1).
 * The helper process (yrss_remote_set_extended) and the fan-out
 * (yrss_fanout_set_extended) own their contexts and set the flags on them.
 *
 * flags == 0 restores the reference's rules exactly.  -EINVAL on unknown
 * bits; -EBUSY while a YRSS_F_ASYNC or worker burst is pending; a resident
 * worker is halted, and the next submit it serves relaunches it: under the new
 * flags for a YRSS_WORKER_F_EXTENDED worker, after the flags return to 0 for
 * any other.  Tickets continue across the relaunch. */
#define YRSS_EXT_VLAN 0x1u
#define YRSS_EXT_IPV6 0x2u
#define YRSS_EXT_UDP  0x4u
#define YRSS_EXT_ALL  0x7u
int yrss_set_extended(yrss_ctx *ctx, uint32_t flags);

/* ---- redirection table: THIS BUILD'S OWN SEMANTICS, NOT fs/lib's -------------- */

/* toeplitz_dispatch picks a hashed packet's queue as hash % d (+1), d fixed by
 * nb_procs and dispatch_only_core (ff_dpdk_if.c:2031-2034).  That is the
 * default here too, bit for bit.  An RSS redirection table (RETA) is an opt-in
 * departure, per context, for deployments that want to weight, drain or
 * rebalance their lcores without renumbering every flow; nothing in fs/lib
 * computes these results.
 *
 * While a table is set, a hashed packet's queue is table[hash & (size - 1)].
 * "Hashed" means hashed under the rules in force: the reference's with
 * yrss_set_extended flags 0, the extended mode's otherwise.  Nothing else
 * moves: the hash output is the same; an unhashed packet keeps its constant
 * queue (0 for ARP / RARP, YRSS_DEFAULT_Q); a hashed packet whose ports lie
 * beyond the window stays YRSS_Q_TRUNCATED with hash 0; the protocol_filter
 * class still follows the reference on the unstripped frame.  Per-queue lists,
 * segmented lists and route classes follow the new queue.  dispatch_only_core
 * does not constrain the table: an entry may name queue 0, the table being the
 * operator's statement.
 *
 * yrss_set_reta: size is a power of two, 1..YRSS_RETA_MAX, and every entry is
 * < nb_queues of the context; anything else is -EINVAL and the table in force
 * stays as it was.  table == NULL or size == 0 switches the table off and
 * restores hash % d (+1) exactly.  -EBUSY while a YRSS_F_ASYNC or worker burst
 * is pending.  The table is copied (the caller's array is free on return) and
 * holds for every dispatch issued after the call returns, so an lcore rewrites
 * it between two bursts; a device batch still running on a caller's stream may
 * see either table.
 * yrss_get_reta copies the table in force into table[cap] and returns its
 * size, 0 when none is set; -EINVAL when cap is smaller than that size.
 *
 * Honoured by every yrss_dispatch_dev*, yrss_route_dev_seg, the host bursts
 * and frames (zero-copy and routed forms included), yrss_route_burst and by
 * yrss_toeplitz_dispatch on a context without a worker.
 * NOT served yet: the persistent worker, and so the helper process
 * (yrss_remote_*) and the fan-out (yrss_fanout_*), which are built on it and
 * have no table call.  While a table is set yrss_worker_start* and every
 * yrss_worker_submit* return -ENOTSUP, YRSS_WORKER_F_EXTENDED workers
 * included, and the shim on a worker context returns -1; a resident worker is
 * halted by yrss_set_reta as yrss_set_extended halts it, and serves again
 * from the first submit after the table is cleared.  yrss_rss_check_dev and
 * yrss_rss_lport_sweep are unchanged: they model the NIC's RSS over the raw
 * network-order tuple, not this dispatcher's hash, and take their own
 * reta_size.
 *
 * yrss_reta_fill_weighted is pure host code and needs no context: it fills
 * table[size] (a power of two, 1..YRSS_RETA_MAX) with the queue ids
 * 0..nb_queues - 1 in proportion to weights[nb_queues] by smooth weighted
 * round-robin.  Every queue has a running value, 0 at the start; for each
 * slot in order: add each queue's weight to its value, take the queue with
 * the largest value (the lowest index on ties), subtract the sum of all
 * weights from that queue's value, write that queue's id to the slot.  A
 * queue's count is within 1 of size * w / W; weight 0 means the queue never
 * appears; equal weights give table[i] == i % nb_queues.  -EINVAL when every
 * weight is 0, nb_queues is 0 or above YRSS_MAX_QUEUES, or the size is bad. */
#define YRSS_RETA_MAX 512
int yrss_set_reta(yrss_ctx *ctx, const uint16_t *table, uint32_t size);
int yrss_get_reta(yrss_ctx *ctx, uint16_t *table, uint32_t cap);   /* returns size, 0 when off */
int yrss_reta_fill_weighted(uint16_t *table, uint32_t size,
                            const uint32_t *weights, uint32_t nb_queues);

/* Full device batch: yrss_dispatch_dev plus the optional filter output. */
struct yrss_dev_batch {
    const uint8_t *win;       /* as d_win of yrss_dispatch_dev          */
    uint32_t win_stride;
    uint32_t n;
    const uint16_t *len;
    int16_t *q;
    uint32_t *hash;           /* may be NULL                            */
    uint32_t *qidx;           /* may be NULL                            */
    uint32_t *qstart;         /* required with qidx                     */
    int8_t *filter;           /* YRSS_FILTER_* per packet, or NULL      */
};
int yrss_dispatch_dev_ex(yrss_ctx *ctx, const struct yrss_dev_batch *b, void *stream);

/* ---- segmented per-queue lists (the parse kernel's own output) ---------------- */

/* The reference never builds a batch-wide list: process_packets enqueues
 * burst by burst, in order, into dispatch_ring[port][q] (ff_dpdk_if.c:1087-1093
 * inside the :1674-1683 loop).  This form is that contract: the batch is cut
 * into segments of YRSS_SEG_PKTS consecutive packets (segment s = packets
 * [256 s, min(256 s + 256, n)), nseg = ceil(n / 256)), each with its own
 * finished lists over nbk = nb_queues + 1 buckets (the last one holds the
 * packets process_packets frees, :1080-1083, as in yrss_dispatch_dev):
 *   seg_idx   n x uint8.  Bytes [256 s, 256 s + len_s) are the segment-local
 *             indices (0..255) of segment s's packets, grouped by bucket in
 *             bucket order, FIFO inside each bucket.  Packet = 256 s + byte.
 *   seg_off   nseg x (nbk + 1) x uint16, segment-major.  Bucket b of segment
 *             s = seg_idx[256 s + seg_off[s][b] .. 256 s + seg_off[s][b+1]);
 *             seg_off[s][0] == 0, seg_off[s][nbk] == len_s.
 * Walking the segments in order and appending each segment's bucket b to ring
 * b gives bucket b's list of yrss_dispatch_dev, so every queue stays FIFO
 * exactly as with the reference's per-burst rte_ring_enqueue_burst.
 * The parse kernel writes the lists itself, with each segment's q and hash:
 * one launch, no scan or scatter kernel, 1 byte per packet. */
#define YRSS_SEG_PKTS 256
#define YRSS_SEG_MAX_BUCKETS 16
#define YRSS_SEG_MAX_BATCH (1u << 24)

struct yrss_dev_seg_batch {
    const uint8_t *win;       /* as d_win of yrss_dispatch_dev          */
    uint32_t win_stride;
    uint32_t n;
    const uint16_t *len;
    int16_t *q;
    uint32_t *hash;           /* may be NULL                            */
    int8_t *filter;           /* YRSS_FILTER_* per packet, or NULL      */
    uint8_t *seg_idx;         /* n bytes, 16-byte aligned               */
    uint16_t *seg_off;        /* ceil(n / 256) x (nb_queues + 2)        */
};
/* Asynchronous, with the stream and workspace rules of yrss_dispatch_dev (the
 * stream switch waits on the device, -EBUSY while a YRSS_F_ASYNC burst is
 * pending, a resident worker is retired first).  Checked before anything is
 * launched: nb_queues + 1 <= YRSS_SEG_MAX_BUCKETS, else -ENOTSUP;
 * n <= YRSS_SEG_MAX_BATCH and the alignments of yrss_dispatch_dev plus
 * seg_idx (16 bytes) and seg_off (2), else -EINVAL.  Segments are
 * independent, so a larger batch is split at any multiple of 256.  n == 0
 * launches nothing; every n >= 1 runs the parse kernel (no one-launch
 * shortcut).  It leaves the list workspace of yrss_dispatch_dev untouched, so
 * both forms may alternate on one context.  A list slot outside its segment
 * is not stored and sets the fault record (YRSS_FAULT_LIST_RANGE, kernel
 * YRSS_K_PARSE_HASH; yrss_status). */
int yrss_dispatch_dev_seg(yrss_ctx *ctx, const struct yrss_dev_seg_batch *b, void *stream);

/* Host-only: the segmented form as the qidx (n x uint32) / qstart (nbk + 1
 * offsets) of yrss_dispatch_dev.  The arrays are not trusted: every offset
 * row must be monotone from 0 to len_s and every index < len_s, else -EINVAL
 * (nothing outside the arrays' stated sizes is read or written).
 * yastack_amd/segments.py is the Python twin. */
int yrss_seg_to_lists(const uint8_t *seg_idx, const uint16_t *seg_off, uint32_t n,
                      uint32_t nbk, uint32_t *out_qidx, uint32_t *out_qstart);

/* ---- routed segmented lists: process_packets' hand-off classes ---------------- */

/* yrss_dispatch_dev_seg's lists answer "which queue".  process_packets does
 * more with a packet whose queue is the dispatcher lcore's own (queue_id):
 * ARP is cloned to every other ring (ff_dpdk_if.c:1097-1129), the KNI rule
 * hands packets to KNI (:1132-1135), the rest is delivered locally (:1137).
 * This form is the same segmented layout over nrb = nb_queues + 3 route
 * buckets, decided by the parse kernel from the queue and the protocol_filter
 * class it already holds, so the host performs the whole hand-off with list
 * walks (yrss_route_seg) and reads neither q nor filter.  With nq = nb_queues,
 * f the YRSS_FILTER_* class and the context's KNI state (yrss_set_kni):
 *   b < nq, b != queue_id   q == b: for dispatch_ring[port][b] (:1087-1093)
 *   queue_id (if < nq)      local delivery (ff_veth_input): q == queue_id,
 *                           neither ARP nor sent to KNI; YRSS_FILTER_TRUNC /
 *                           YRSS_FILTER_LOOP packets stay here, as in
 *                           yrss_route_burst
 *   nq                      freed: q < 0 || q >= nq (:1080-1083)
 *   nq + 1                  KNI: q == queue_id, KNI on and (f == YRSS_FILTER_KNI
 *                           under "accept" or f == YRSS_FILTER_UNKNOWN under
 *                           "reject")
 *   nq + 2                  ARP on the local queue: q == queue_id,
 *                           f == YRSS_FILTER_ARP, KNI on or off
 * queue_id >= nq is legal: no packet is local, buckets nq + 1 and nq + 2 stay
 * empty.  seg_idx is n x uint8 and seg_off ceil(n / 256) x (nrb + 1) uint16,
 * exactly as in yrss_dispatch_dev_seg with nrb in place of nbk: every bucket
 * FIFO, seg_off[s][0] == 0, seg_off[s][nrb] == len_s. */
#define YRSS_ROUTE_SEG_MAX_QUEUES 13   /* nb_queues + 3 <= YRSS_SEG_MAX_BUCKETS */

struct yrss_dev_route_batch {   /* yrss_dev_seg_batch + queue_id */
    const uint8_t *win;       /* as d_win of yrss_dispatch_dev          */
    uint32_t win_stride;
    uint32_t n;
    const uint16_t *len;
    int16_t *q;
    uint32_t *hash;           /* may be NULL                            */
    int8_t *filter;           /* YRSS_FILTER_* per packet, or NULL      */
    uint8_t *seg_idx;         /* n bytes, 16-byte aligned               */
    uint16_t *seg_off;        /* ceil(n / 256) x (nb_queues + 4)        */
    uint16_t queue_id;        /* the dispatcher lcore's own queue       */
};
/* One launch of the parse kernel, asynchronous, with every rule of
 * yrss_dispatch_dev_seg: stream switch, -EBUSY while a YRSS_F_ASYNC burst is
 * pending, a resident worker retired first, the alignments, n <=
 * YRSS_SEG_MAX_BATCH (else -EINVAL), n == 0 launches nothing, the list
 * workspace of yrss_dispatch_dev untouched, the same guard and fault record,
 * the same timing slot (YRSS_K_PARSE_HASH).  nb_queues >
 * YRSS_ROUTE_SEG_MAX_QUEUES is refused with -ENOTSUP before anything is
 * launched.  The KNI state is the one yrss_set_kni last set, read at the call.
 * q, hash and (when filter is not NULL) filter are written as by
 * yrss_dispatch_dev_seg; the classes are computed whether or not filter is
 * stored. */
int yrss_route_dev_seg(yrss_ctx *ctx, const struct yrss_dev_route_batch *b, void *stream);

struct yrss_route_ops;
struct yrss_route_result;
/* Host-only: process_packets' hand-off from routed segments, segment by
 * segment in order; per segment what yrss_route_burst does for a burst of 256.
 * objs[i] is packet i's mbuf; ops, out_local, out_kni and res are those of
 * yrss_route_burst (below); kni_clone is its "KNI on && kni_primary".
 *   - every ARP-bucket packet, in packet order: ops->clone for each queue
 *     j != queue_id in queue order, then the KNI clone (queue 0xFFFF) when
 *     kni_clone is set
 *   - one ops->enqueue per ring with anything to take: bucket j merged by
 *     packet index with the successful ARP clones for j; the tail the ring
 *     refuses is released (n_freed); n_ring[j] accumulates over the segments
 *   - bucket nq is released (n_freed)
 *   - out_local: the local bucket merged by index with the ARP bucket (n_arp)
 *   - out_kni: the KNI bucket merged by index with the KNI clones
 * n_unresolved counts the local bucket's YRSS_FILTER_TRUNC / YRSS_FILTER_LOOP
 * packets when filter (n x int8, as the kernel wrote it) is given; with
 * filter == NULL it is 0 and those packets are simply part of out_local.
 * The arrays are not trusted: all of them are validated first, by the rules of
 * yrss_seg_to_lists (rows monotone from 0 to len_s, every index < len_s,
 * nb_queues + 3 <= YRSS_SEG_MAX_BUCKETS), and a failure returns -EINVAL before
 * any callback is invoked.  out_local and out_kni need room for n each (a packet
 * adds itself or its one KNI clone to out_kni, never both). */
int yrss_route_seg(const uint8_t *seg_idx, const uint16_t *seg_off, uint32_t n,
                   uint16_t nb_queues, uint16_t queue_id, int kni_clone,
                   const int8_t *filter, void *const *objs,
                   const struct yrss_route_ops *ops, void **out_local, void **out_kni,
                   struct yrss_route_result *res);

/* ---- routed global lists: the same classes for one-workgroup bursts ----------- */

/* The host bursts (one launch of the one-workgroup burst kernel, n <= 4096) and
 * the persistent worker build global lists, not segments: 32-bit packet
 * indices and one offset row.  Their routed form is
 *   ridx     n x uint32 packet indices grouped by route class, FIFO inside
 *   rstart   nb_queues + 4 x uint32 offsets: class b = ridx[rstart[b] ..
 *            rstart[b+1]), rstart[0] == 0, rstart[nb_queues + 3] == n
 * with the classes numbered exactly as in yrss_route_dev_seg above.  One lane
 * holds one class, so nb_queues + 3 <= 64. */
#define YRSS_ROUTE_LISTS_MAX_QUEUES 61

/* Synchronous: a host gather and ONE launch, like yrss_dispatch_burst /
 * yrss_dispatch_frames (flags: YRSS_F_WRITE_RSS; YRSS_F_ASYNC is refused with
 * -EINVAL).  out_hash and out_filter may be NULL (the classes are computed
 * either way); out_q, out_ridx and out_rstart are required.  n == 0 zeroes the
 * nb_queues + 4 offsets.  -ENOTSUP, before anything is launched, for n > 4096
 * or nb_queues > YRSS_ROUTE_LISTS_MAX_QUEUES: larger batches belong to
 * yrss_route_dev_seg.  The KNI state is the one yrss_set_kni last set. */
int yrss_route_lists_burst(yrss_ctx *ctx, void *const *mbufs, uint32_t n, uint16_t queue_id,
                           int16_t *out_q, uint32_t *out_hash, int8_t *out_filter,
                           uint32_t *out_ridx, uint32_t *out_rstart, uint32_t flags);
int yrss_route_lists_frames(yrss_ctx *ctx, const uint8_t *const *data, const uint16_t *len,
                            uint32_t n, uint16_t queue_id, int16_t *out_q, uint32_t *out_hash,
                            int8_t *out_filter, uint32_t *out_ridx, uint32_t *out_rstart);

/* Host-only: process_packets' hand-off from routed global lists; the twin of
 * yrss_route_seg for one burst, with its arguments, callbacks and results
 * (kni_primary is its kni_clone: pass "KNI on && kni_primary").  The same
 * hand-off routine as yrss_route_burst, which sorts these classes on the host
 * from q and filter where this call is given them by the kernel: list walks,
 * ARP clones in packet order (queue order inside a packet, then the KNI
 * clone), one enqueue per ring merged by index with the successful clones,
 * release of the refused tail and of the freed class, out_local = local class
 * merged with the ARP class, out_kni = KNI class merged with the KNI clones.
 * n_unresolved is 0 without filter.  Validated before the first callback, a
 * failure returning -EINVAL with no callback made: the offsets monotone from 0
 * to n, every index < n and present exactly once, the KNI and ARP classes empty
 * when queue_id >= nb_queues, nb_queues <= YRSS_ROUTE_LISTS_MAX_QUEUES. */
int yrss_route_lists(const uint32_t *ridx, const uint32_t *rstart, uint32_t n,
                     uint16_t nb_queues, uint16_t queue_id, int kni_primary,
                     const int8_t *filter, void *const *objs,
                     const struct yrss_route_ops *ops, void **out_local, void **out_kni,
                     struct yrss_route_result *res);

/* ---- host-resident dispatch (the drop-in burst hook) ------------------------ */

/* Classify a burst of DPDK mbufs straight off rte_eth_rx_burst.
 *   mbufs      n x `struct rte_mbuf *` (read per cfg->mbuf offsets)
 *   out_q      n x int16 host array (required)
 *   out_hash   n x uint32 host array or NULL
 *   out_qidx / out_qstart  host arrays as in yrss_dispatch_dev, or NULL
 *   flags      YRSS_F_WRITE_RSS: also store each hash into mbuf hash.rss
 * Gathers min(data_len, 64 or 80) header bytes into pinned memory.  Bursts of
 * up to 4096 packets (with nb_queues + 1 <= 64) run as ONE kernel launch that
 * reads the pinned windows and writes the pinned results in place; larger ones
 * copy to the GPU, run the batch kernels and copy back.  Synchronous unless
 * flags has YRSS_F_ASYNC. */
#define YRSS_F_WRITE_RSS 0x1u
/* Return once the burst is queued on the context's stream; the outputs (and the
 * hash.rss write-back) are valid after yrss_wait(ctx) returns 0.  Everything
 * the call reads in place (the mbufs, registered pointer/length arrays) and
 * the output arrays must stay untouched until then.  One burst in flight per
 * context: another host-resident call (or yrss_dispatch_dev*) returns -EBUSY
 * until yrss_wait.  Pipeline bursts over several contexts (one per slot). */
#define YRSS_F_ASYNC 0x2u
int yrss_dispatch_burst(yrss_ctx *ctx, void *const *mbufs, uint32_t n,
                        int16_t *out_q, uint32_t *out_hash, uint32_t *out_qidx,
                        uint32_t *out_qstart, uint32_t flags);

/* Zero-copy variant: the mbufs (headers and data) live in host memory that was
 * registered with yrss_register_host_memory (e.g. the DPDK mbuf pool's
 * memzones).  Only the mbuf pointer array crosses PCIe host->device; a gfx950
 * kernel reads each mbuf's buf_addr/data_off/data_len and the header window
 * straight from host memory, and with YRSS_F_WRITE_RSS writes hash.rss back
 * into the mbuf itself.  The dispatcher core does no per-packet work.
 * Returns -EFAULT if a mbuf or its data lies outside every registered range
 * (checked on the GPU; results are then not written).  Synchronous unless
 * flags has YRSS_F_ASYNC. */
int yrss_dispatch_burst_zc(yrss_ctx *ctx, void *const *mbufs, uint32_t n, int16_t *out_q,
                           uint32_t *out_hash, uint32_t *out_qidx, uint32_t *out_qstart,
                           uint32_t flags);

/* Zero-copy frames: (data pointer, data_len) pairs the host already holds —
 * e.g. read from the cache-hot mbuf headers right after rte_eth_rx_burst — so
 * the GPU reads only the header windows from registered host memory (one
 * 64-byte PCIe read per packet).  Synchronous.
 *
 * For both zero-copy calls, pointer/length arrays and output arrays that lie
 * in registered memory are read and written in place (no staging copies). */
int yrss_dispatch_frames_zc(yrss_ctx *ctx, const uint8_t *const *data, const uint16_t *len,
                            uint32_t n, int16_t *out_q, uint32_t *out_hash,
                            uint32_t *out_qidx, uint32_t *out_qstart);
/* Same, with flags (YRSS_F_ASYNC). */
int yrss_dispatch_frames_zc_ex(yrss_ctx *ctx, const uint8_t *const *data, const uint16_t *len,
                               uint32_t n, int16_t *out_q, uint32_t *out_hash,
                               uint32_t *out_qidx, uint32_t *out_qstart, uint32_t flags);

/* Complete the burst queued with YRSS_F_ASYNC: 0 (outputs valid), or the error
 * the synchronous call would have returned (-EFAULT, -EIO, ...).  0 when
 * nothing is in flight. */
int yrss_wait(yrss_ctx *ctx);

/* Register / unregister a host range (hipHostRegister, mapped) for the
 * zero-copy path; up to 16 ranges per context.  Unregistering returns -EBUSY
 * while a persistent-worker burst of the context is pending (not yet polled):
 * it may still read mbufs or write outputs in that range. */
#define YRSS_MAX_HOST_RANGES 16
int yrss_register_host_memory(yrss_ctx *ctx, void *base, size_t len);
int yrss_unregister_host_memory(yrss_ctx *ctx, void *base);

/* Same, for frames given as (data pointer, data_len) pairs. */
int yrss_dispatch_frames(yrss_ctx *ctx, const uint8_t *const *data,
                         const uint16_t *len, uint32_t n, int16_t *out_q,
                         uint32_t *out_hash, uint32_t *out_qidx,
                         uint32_t *out_qstart);

/* ---- per-packet registration ------------------------------ */

/* The reference's per-packet hook, unchanged:
 *   typedef int (*dispatch_func_t)(void *data, uint16_t len, uint16_t queue_id,
 *                                  uint16_t nb_queues);            fs/lib/ff_api.h:167
 *   ff_regist_packet_dispatcher(yrss_toeplitz_dispatch);           fs/lib/ff_api.h:170
 * yrss_toeplitz_dispatch has toeplitz_dispatch's signature and return values
 * (fs/lib/ff_dpdk_if.c:1945-2113): the target queue, default_Q (2) for unhashed
 * packets, -1 on error (no context set, a failed GPU call), which F-Stack
 * answers by freeing the mbuf (ff_dpdk_if.c:1080-1083).  queue_id and
 * nb_queues are unused, as in the reference.  dispatch_func_t carries no
 * context, so yrss_set_dispatch_ctx names the one to use (NULL clears it;
 * yrss_fini clears it for its own context).  Every call is a one-packet GPU
 * burst with its own launch and synchronisation (10.8 µs per call measured);
 * if the context has a resident worker (yrss_worker_start), the call is a
 * one-packet worker burst instead, no HIP call (9.3 µs; the window is copied
 * into a slot the context registers on first use; the shim then shares that
 * worker's ring, so submit nothing else to the context while shim calls run:
 * a slot still holding an unpolled ticket makes the call return -1).  A
 * drop-in for registration, not the fast path — use the burst hook or the
 * worker.
 * Calls from several threads (soft_dispatch=0 runs the dispatcher on every
 * lcore, ff_dpdk_if.c:1653) are serialised by one process-wide mutex.  Give the
 * shim a context of its own: while that context has a YRSS_F_ASYNC burst
 * pending the call returns -1, and F-Stack frees the mbuf. */
int yrss_set_dispatch_ctx(yrss_ctx *ctx);
int yrss_toeplitz_dispatch(void *data, uint16_t len, uint16_t queue_id, uint16_t nb_queues);

/* ---- burst routing: process_packets' hand-off --------- */

/* Caller-side plumbing, so the routing drives real DPDK objects:
 *   enqueue  rte_ring_enqueue_burst(dispatch_ring[port][queue], objs, n) —
 *            returns how many of objs (a prefix) were enqueued
 *   clone    pktmbuf_deep_clone(m, pool of queue) (ff_dpdk_if.c:1009-1056);
 *            NULL when the pool is exhausted
 *   release  rte_pktmbuf_free(m) */
struct yrss_route_ops {
    unsigned (*enqueue)(void *user, uint16_t queue, void *const *objs, unsigned n);
    void *(*clone)(void *user, void *mbuf, uint16_t queue);
    void (*release)(void *user, void *mbuf);
    void *user;
};

struct yrss_route_result {
    uint32_t n_local;         /* out_local[]: ff_veth_input on this lcore, in order */
    uint32_t n_kni;           /* out_kni[]: ff_kni_enqueue, in order                */
    uint32_t n_freed;         /* bad queue, ring full or failed clone enqueue       */
    uint32_t n_arp;           /* ARP packets kept local (and cloned)               */
    uint32_t n_unresolved;    /* YRSS_FILTER_TRUNC/LOOP packets, left in out_local */
    uint32_t n_ring[YRSS_MAX_QUEUES];   /* objects enqueued per queue ring        */
};

/* process_packets(port, queue_id, mbufs, n, ctx, pkts_from_ring=0) with the
 * dispatcher registered (ff_dpdk_if.c:1058-1140), for a whole burst: classify
 * on the GPU (queue + protocol_filter), sort the packets by route class on the
 * host (any nb_queues) and run the list hand-off of yrss_route_lists, whose
 * outcome is, packet by packet in order,
 *   ret < 0 || ret >= nb_queues        -> release (:1080-1083)
 *   ret != queue_id                    -> ring[ret], FIFO; release if full (:1087-1093)
 *   local, FILTER_ARP                  -> clone to every other queue's ring, a KNI
 *                                         clone if KNI is on and kni_primary, and
 *                                         local input (:1097-1129)
 *   local, KNI accept/reject rule      -> out_kni (:1132-1135)
 *   local, otherwise                   -> out_local (:1137)
 * Ring order equals the reference's one-at-a-time enqueue order.  out_local and
 * out_kni need room for n (+ n ARP clones for out_kni). */
int yrss_route_burst(yrss_ctx *ctx, void *const *mbufs, uint32_t n, uint16_t queue_id,
                     int kni_primary, const struct yrss_route_ops *ops, void **out_local,
                     void **out_kni, struct yrss_route_result *res);

/* ---- connect-side RSS check ----------------------------- */

/* One ff_rss_check call (fs/lib/ff_dpdk_if.c:1904-1940): addresses and ports
 * exactly as the caller stores them (network byte order, in_pcb.c:1155-1156
 * passes faddr, laddr, fport, lport). */
struct yrss_rss_tuple {
    uint32_t saddr;
    uint32_t daddr;
    uint16_t sport;
    uint16_t dport;
};

/* For n tuples in HBM: d_ok[i] = ff_rss_check(...) (1 when nb_queues <= 1, else
 * ((hash & (reta_size - 1)) % nb_queues) == queueid), d_hash[i] (may be NULL)
 * the Toeplitz hash of the 12 raw tuple bytes.  Asynchronous. */
int yrss_rss_check_dev(yrss_ctx *ctx, const struct yrss_rss_tuple *d_tuples, uint32_t n,
                       uint16_t nb_queues, uint16_t reta_size, uint16_t queueid,
                       uint8_t *d_ok, uint32_t *d_hash, void *stream);

/* The whole ephemeral-port search of in_pcbconnect_setup (in_pcb.c:1131-1170)
 * in one launch: bit (p & 31) of bitmap[p >> 5] is ff_rss_check(faddr, laddr,
 * fport, p) for every stored (network-order) lport value p in 0..65535.
 * bitmap is 2048 host words.  Synchronous.  It runs through the host-burst
 * staging, so while a YRSS_F_ASYNC burst is pending it returns -EBUSY, with
 * bitmap untouched, until yrss_wait. */
int yrss_rss_lport_sweep(yrss_ctx *ctx, uint32_t faddr, uint32_t laddr, uint16_t fport,
                         uint16_t nb_queues, uint16_t reta_size, uint16_t queueid,
                         uint32_t *bitmap);

/* ---- multi-GPU sharding ------------------------------------------ */

/* One yrss_ctx and one stream per GPU; each classifies a contiguous shard of the
 * batch with no collective.  yrss_shard_range gives shard `rank` of `world`
 * (balanced: the first n_total % world shards get one packet more).
 * yrss_merge_queue_lists concatenates the shards' per-queue lists in shard
 * order, which keeps every queue FIFO over the whole batch, as the reference's
 * rte_ring does (fs/lib/ff_dpdk_if.c:1087-1093): nbk = nb_queues + 1 buckets;
 * shard s holds qidx[s] (shard-local indices) and qstart[s] (nbk + 1 offsets)
 * and starts at global packet first[s]; out_qidx gets global indices (64-bit:
 * a node's batch can exceed 2^32 packets), out_qstart nbk + 1 offsets.
 * Host-only.  yastack_amd/shard.py is the Python twin. */
int yrss_shard_range(uint64_t n_total, uint32_t world, uint32_t rank, uint64_t *first,
                     uint64_t *count);
int yrss_merge_queue_lists(uint32_t nshards, uint32_t nbk, const uint64_t *first,
                           const uint32_t *const *qidx, const uint32_t *const *qstart,
                           uint64_t *out_qidx, uint64_t *out_qstart);

/* ---- pcap capture I/O ----------------------------------- */

/* ff_enable_pcap + ff_dump_packets (fs/lib/ff_dpdk_pcap.c:49-102) for a burst:
 * append == 0 creates the file with the reference's 24-byte header (magic
 * 0xA1B2C3D4, v2.4, snaplen 65535, LINKTYPE_ETHERNET); every frame gets a
 * 16-byte record {sec, usec, caplen = len, len} and its bytes.  ts_* may be
 * NULL (zeros).  Host file I/O only. */
int yrss_pcap_write(const char *path, int append, const uint8_t *const *data,
                    const uint32_t *len, uint32_t n, const uint32_t *ts_sec,
                    const uint32_t *ts_usec);

/* Replay: records [first, first+max) of an Ethernet pcap (either byte order,
 * usec or nsec magic) into header windows of `stride` bytes (>= 64) plus
 * data_len = min(caplen, 65535) — each record is one single-segment mbuf —
 * and, if non-NULL, the wire length.  Returns the number of records read, or
 * -errno.  max == 0 returns the capture's record count. */
int yrss_pcap_read(const char *path, uint64_t first, uint32_t max, uint8_t *win,
                   uint32_t stride, uint16_t *len, uint32_t *wire_len);

/* ---- synthetic traffic (bench / parity inputs; see yrss_synth.h) ------------- */

struct yrss_synth_params;
/* Write header windows + data_len of packets [first, first+n) of a synthetic
 * stream directly into HBM.  Bit-identical to yrss_synth_window() on the host. */
int yrss_synth_dev(yrss_ctx *ctx, const struct yrss_synth_params *p,
                   uint64_t first, uint32_t n, uint8_t *d_win,
                   uint32_t win_stride, uint16_t *d_len, void *stream);

/* ---- timing hook (bench) ------------------------------------------------------- */

/* kernel_mask bit k (YRSS_K_*) brackets every launch of kernel k by
 * yrss_dispatch_dev with hipEvents on the launch stream (0 disables; enabling
 * resets the totals).  yrss_timing_read synchronises the pending events and
 * returns the summed milliseconds and launch count for one kernel. */
#define YRSS_K_PARSE_HASH 0
#define YRSS_K_SCAN       1
#define YRSS_K_SCATTER    2
#define YRSS_K_COUNT      3
/* Kernel ids that appear only in fault records (not timed). */
#define YRSS_K_BURST      8   /* yrss_burst_small: one-launch bursts / batches */
#define YRSS_K_WORKER     9   /* yrss_burst_worker */
int yrss_timing_enable(yrss_ctx *ctx, int kernel_mask);
int yrss_timing_read(yrss_ctx *ctx, int kernel, double *total_ms,
                     uint32_t *launches);
/* The q-quantile (0.5: median) of kernel k's per-launch
 * durations since yrss_timing_enable, in ms; -ENODATA before any launch. */
int yrss_timing_quantile(yrss_ctx *ctx, int kernel, double q, double *ms);

/* ---- persistent burst worker ------------------------------------------------------ */

/* Small bursts with no kernel launch and no stream synchronisation per burst:
 * a persistent gfx950 kernel (nblocks workgroups, one CU each) polls a ring of
 * nslots slots in host-coherent pinned memory.  Submit copies the mbuf pointer
 * array into a slot and publishes it; the kernel reads the mbufs (which must
 * lie in memory registered with yrss_register_host_memory) over PCIe and
 * classifies them like yrss_dispatch_burst_zc.  Output arrays that lie in
 * registered memory are written in place; others are written into the slot
 * and copied to the caller's arrays by the poll.  Up to nslots bursts are in
 * flight; every ticket must be polled before its slot is reused (submit
 * returns -EBUSY otherwise).  The kernel leaves after YRSS_WORKER_IDLE_MS
 * (default 50) without a submit or YRSS_WORKER_LIFE_MS (default 1000) in total
 * and is relaunched transparently by the next submit or poll (also by a
 * wait = 0 poll); registering or unregistering host memory restarts it.
 * nslots is a multiple of nblocks; nb_queues + 1 <= 64.  Submits and polls of
 * one context come from one thread at a time (the dispatcher lcore). */
#define YRSS_WORKER_MAX_BURST 1024
#define YRSS_WORKER_MAX_BLOCKS 128
#define YRSS_WORKER_MAX_SLOTS 4096
int yrss_worker_start(yrss_ctx *ctx, uint32_t nslots, uint32_t nblocks);
/* The same worker in route mode, for the lcore whose queue is queue_id
 * (queue_id >= nb_queues is legal: nothing is local): the three submit calls
 * keep their signatures, out_q and out_hash are unchanged, and out_qidx /
 * out_qstart receive the ROUTED lists of yrss_route_lists_burst: packet indices
 * grouped by route class, FIFO inside a class, and nb_queues + 4 offsets
 * (n == 0 zeroes them), for yrss_route_lists to hand off.  YRSS_F_WRITE_RSS,
 * the frames form and the windows form work as in the plain worker; there is
 * no per-packet filter output.  Same arguments and limits as
 * yrss_worker_start; -ENOTSUP when nb_queues > YRSS_ROUTE_LISTS_MAX_QUEUES.
 * The KNI state is the context's when the kernel is launched: yrss_set_kni on
 * a context with a route worker returns -EBUSY while a burst is pending, and
 * otherwise halts the kernel, so the next submit relaunches it with the new
 * state (as registering host memory does). */
int yrss_worker_start_route(yrss_ctx *ctx, uint32_t nslots, uint32_t nblocks, uint16_t queue_id);
/* The worker with its options spelled out: flags 0 is yrss_worker_start,
 * YRSS_WORKER_F_ROUTE is yrss_worker_start_route (queue_id is read only then).
 * YRSS_WORKER_F_EXTENDED makes the worker follow yrss_set_extended: it starts
 * whatever the context's flags are, and each launch of its kernel serves the
 * flags the context holds then (the extended kernel, with 4.5 KiB more LDS for
 * its nibble tables, while any flag is set; with flags 0 the very kernel of
 * yrss_worker_start[_route]).  yrss_set_extended halts it as it halts any
 * worker; its next submit relaunches it.  In route mode the lists follow the
 * extended q, and the filter class the reference on the unstripped frame.
 * -EINVAL on unknown bits; otherwise as the two calls above. */
#define YRSS_WORKER_F_ROUTE    0x1u   /* as yrss_worker_start_route (queue_id is read) */
#define YRSS_WORKER_F_EXTENDED 0x2u   /* the worker follows yrss_set_extended */
int yrss_worker_start_flags(yrss_ctx *ctx, uint32_t nslots, uint32_t nblocks,
                            uint32_t flags, uint16_t queue_id);
/* Queue one burst (n <= YRSS_WORKER_MAX_BURST; flags: YRSS_F_WRITE_RSS);
 * *ticket identifies it for yrss_worker_poll.  The output arrays must stay
 * valid until the ticket is polled. */
int yrss_worker_submit(yrss_ctx *ctx, void *const *mbufs, uint32_t n, int16_t *out_q,
                       uint32_t *out_hash, uint32_t *out_qidx, uint32_t *out_qstart,
                       uint32_t flags, uint64_t *ticket);
/* Same for (data pointer, data_len) pairs the host already holds, like
 * yrss_dispatch_frames_zc: the GPU reads only the windows (in registered
 * memory). */
int yrss_worker_submit_frames(yrss_ctx *ctx, const uint8_t *const *data, const uint16_t *len,
                              uint32_t n, int16_t *out_q, uint32_t *out_hash,
                              uint32_t *out_qidx, uint32_t *out_qstart, uint64_t *ticket);
/* Same for windows the caller has copied, contiguously, into registered
 * memory: window i at win + i * stride holds the first min(len[i], stride)
 * bytes of packet i's first segment (stride >= 64, a multiple of 16; 80 never
 * truncates).  The GPU reads the burst as one stretch of host memory, with no
 * per-packet pointer reads: the dispatcher lcore's copy of each window (cache
 * hot after rte_eth_rx_burst) replaces the GPU's dependent PCIe reads of the
 * pointer array and then each scattered window.  -EFAULT if the windows are
 * not in registered memory. */
int yrss_worker_submit_windows(yrss_ctx *ctx, const uint8_t *win, uint32_t stride,
                               const uint16_t *len, uint32_t n, int16_t *out_q,
                               uint32_t *out_hash, uint32_t *out_qidx, uint32_t *out_qstart,
                               uint64_t *ticket);
/* 0: the burst is done and its outputs in place; -EAGAIN: not yet (wait = 0);
 * -EFAULT: a mbuf or its data lies outside every registered range;
 * -ETIMEDOUT: waited 10 s (a burst takes microseconds: the GPU is hung).  The
 * context is then marked hung: yrss_fini neither waits for the device nor
 * frees memory a still-running kernel may write (it is left to process exit). */
int yrss_worker_poll(yrss_ctx *ctx, uint64_t ticket, int wait);
/* Stop the kernel and free the ring (also done by yrss_fini). */
int yrss_worker_stop(yrss_ctx *ctx);

/* ---- host bursts fanned out over several GPUs ------------------- */

/* The reference's soft dispatch is ONE lcore feeding every dispatch ring
 * (fs/lib/ff_dpdk_if.c:1653-1683).  A fan-out keeps that single dispatcher
 * thread and spreads its consecutive bursts round-robin over nctx contexts,
 * each with its own persistent worker (yrss_worker_*) on its own device and
 * PCIe link: burst g (tickets 1, 2, ...) goes to context (g - 1) % nctx.
 * yrss_fanout_next returns tickets in submission order as they complete, so
 * handing each burst's per-queue lists to the rings in that order keeps every
 * queue FIFO over the whole stream, as rte_ring does (:1087-1093).  devices may
 * repeat (several contexts on one GPU).  Host memory is registered with every
 * context.  Submit and next come from one thread (the dispatcher lcore); each
 * context holds up to nslots bursts, and a ticket must be returned by
 * yrss_fanout_next before its context's slot is reused (submit: -EBUSY). */
#define YRSS_FANOUT_MAX_CTX 64
typedef struct yrss_fanout yrss_fanout;
int yrss_fanout_init(const struct yrss_config *cfg, const int *devices, uint32_t nctx,
                     uint32_t nslots, uint32_t nblocks, yrss_fanout **out);
int yrss_fanout_fini(yrss_fanout *f);
uint32_t yrss_fanout_size(yrss_fanout *f);
/* yrss_set_extended on every context of the fan-out (their workers are started
 * with YRSS_WORKER_F_EXTENDED).  -EINVAL on unknown bits; -EBUSY while a ticket
 * is outstanding (submitted and not yet returned by yrss_fanout_next); if a
 * context refuses, those already changed are set back and its error returned. */
int yrss_fanout_set_extended(yrss_fanout *f, uint32_t flags);
int yrss_fanout_register_host_memory(yrss_fanout *f, void *base, size_t len);
int yrss_fanout_unregister_host_memory(yrss_fanout *f, void *base);
/* As yrss_worker_submit / yrss_worker_submit_frames; *ticket is the fan-out's. */
int yrss_fanout_submit(yrss_fanout *f, void *const *mbufs, uint32_t n, int16_t *out_q,
                       uint32_t *out_hash, uint32_t *out_qidx, uint32_t *out_qstart,
                       uint32_t flags, uint64_t *ticket);
int yrss_fanout_submit_frames(yrss_fanout *f, const uint8_t *const *data, const uint16_t *len,
                              uint32_t n, int16_t *out_q, uint32_t *out_hash,
                              uint32_t *out_qidx, uint32_t *out_qstart, uint64_t *ticket);
/* The oldest ticket not yet returned, once its burst is done: 0 with *ticket
 * set (-EFAULT also sets it: the burst is consumed, a pointer was outside every
 * registered range); -EAGAIN: still running (wait = 0); -ENOENT: nothing
 * outstanding; other errors as yrss_worker_poll. */
int yrss_fanout_next(yrss_fanout *f, int wait, uint64_t *ticket);
/* Host-only: the context serving fan-out ticket `ticket`, and its ticket there. */
int yrss_fanout_route(uint64_t ticket, uint32_t nctx, uint32_t *ctx, uint64_t *ctx_ticket);

/* ---- device-side status ----------------------------------------------------------- */

/* Every index the per-queue lists are built from (count slots, stage slots,
 * list slots) is bounds-checked on the GPU.  A check that fails stores nothing
 * and sets the context's fault record (first fault wins): that batch's
 * qidx/qstart are invalid; q and hash are not affected.  Codes: */
#define YRSS_FAULT_NONE           0
#define YRSS_FAULT_SCAN_TIMEOUT   1   /* scan look-back did not resolve: where = bucket row  */
#define YRSS_FAULT_LIST_RANGE     2   /* list slot >= n: where = packet, value = slot        */
#define YRSS_FAULT_COUNT_MISMATCH 3   /* a span's histogram differs from the parse counts:
                                         where = span, value = bucket                        */
#define YRSS_FAULT_COUNT_SLOT     4   /* parse count slot beyond LDS: where = wave, value = slot */
#define YRSS_FAULT_STAGE          5   /* scatter stage slot out of range: where = packet     */
#define YRSS_FAULT_LINE_CAPACITY  6   /* a line-scatter kernel launched for more buckets than
                                         its per-bucket arrays hold (the host refuses such a
                                         plan with -EINVAL; the kernel checks again at entry
                                         and leaves): where = buckets, value = its capacity */
struct yrss_fault {
    uint32_t code;     /* YRSS_FAULT_*                                   */
    uint32_t kernel;   /* YRSS_K_* of the kernel whose guard fired       */
    uint32_t where;
    uint32_t value;
};

/* Synchronises the context's own streams (its internal one and the stream of
 * its last device batch, not the whole device) and reports (then clears) the
 * fault record: 0 = no guard fired since the last call, -EIO = one did (the
 * record is printed to stderr).  The host-synchronous entry points check it
 * themselves and return -EIO.  A persistent-worker burst carries its own
 * record: yrss_worker_poll returns -EIO for exactly the burst whose guard
 * fired (other bursts in flight are unaffected) and copies the record here
 * when this one is empty.  The reference has no equivalent: its per-packet
 * rte_ring_enqueue cannot fail this way (ff_dpdk_if.c:1087-1093). */
int yrss_status(yrss_ctx *ctx);
/* Same, copying the record (code 0 = none) instead of printing it. */
int yrss_fault_info(yrss_ctx *ctx, struct yrss_fault *out);

/* ---- layout overrides (tests and measurements) ------------------------------------ */

/* Every field 0 (scatter_xcd -1) is the built-in default; results never
 * depend on these, only the work layout does. */
struct yrss_tuning {
    uint32_t chunk_tiles;    /* parse chunk in 64-packet tiles, power of two (default 4
                                up to 16 buckets, 8 to 128, 16 beyond; larger when a
                                wave's count slots run out)                          */
    uint32_t span_tiles;     /* line-scatter span in tiles, power of two (default 128
                                up to 128 buckets, 256 beyond)                       */
    uint32_t parse_blocks;   /* parse grid (default one workgroup per CU)            */
    uint32_t one_launch;     /* batches <= 4096 packets in one launch: 0 host bursts
                                and device batches, 1 host bursts only, 2 never      */
    int32_t  scatter_xcd;    /* XCD-contiguous scatter ranges: -1 default (on), 0, 1 */
    uint32_t scan_kernel;    /* per-chunk list prefixes: 0 default (up to 16 buckets
                                inside the line scatter, no scan kernel), 1 always
                                the scan kernel                                      */
};
int yrss_set_tuning(yrss_ctx *ctx, const struct yrss_tuning *t);

/* ---- introspection --------------------------------------------------------------- */

const char *yrss_version(void);
/* Kernel-name string as it appears in rocprof traces, for kernel id k. */
const char *yrss_kernel_name(int kernel);
/* Number of workgroups the parse+hash kernel will use for n packets. */
uint32_t yrss_grid_for(yrss_ctx *ctx, uint32_t n);

#ifdef __cplusplus
}
#endif
#endif /* YRSS_H */
