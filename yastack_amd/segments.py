"""The segmented per-queue list form of ``yrss_dispatch_dev_seg`` on the host.

A batch of n packets is cut into segments of ``abi.SEG_PKTS`` = 256 consecutive
packets, each with its own finished lists over nbk = nb_queues + 1 buckets (the
last one holds the packets process_packets frees, fs/lib/ff_dpdk_if.c:1080-1083):

* ``seg_idx``  n x uint8: bytes [256 s, 256 s + len_s) are segment s's
  segment-local packet indices grouped by bucket, FIFO inside each bucket
* ``seg_off``  nseg x (nbk + 1) uint16 offsets into those bytes

Appending each segment's bucket b to ring b, segment after segment, is the
reference's per-burst enqueue into dispatch_ring[port][q] (:1087-1093 inside the
:1674-1683 loop).  :func:`from_q` builds the form from a per-packet queue array
(the tests' expected value, from the oracle's q); :func:`to_lists` is the numpy
twin of the C helper ``yrss_seg_to_lists``; :func:`to_lists_c` calls that helper.

The routed form of ``yrss_route_dev_seg`` is the same layout over nrb =
nb_queues + 3 route buckets (:func:`route_buckets`: what process_packets,
:1058-1140, does with the packet on the lcore whose queue is ``queue_id``);
:func:`route_from` builds it from per-packet q and filter-class arrays;
:func:`route_lists_from` gives the same classes as one global list (32-bit
packet indices, one offset row), the form of the one-workgroup bursts.
"""
from __future__ import annotations

import errno

import numpy as np

from . import abi

SEG = abi.SEG_PKTS


def nseg_for(n: int) -> int:
    return -(-int(n) // SEG)


def buckets_of(q: np.ndarray, nb_queues: int) -> np.ndarray:
    """Bucket of every packet: its queue, or nb_queues where process_packets
    frees it (ret < 0 || ret >= nb_queues)."""
    q = np.asarray(q).astype(np.int64)
    return np.where((q >= 0) & (q < nb_queues), q, nb_queues)


def from_buckets(bkt: np.ndarray, nb: int):
    """(seg_idx uint8[n], seg_off uint16[nseg, nb + 1]) of a per-packet bucket
    array with values in [0, nb)."""
    bkt = np.asarray(bkt).astype(np.int64).reshape(-1)
    n = int(bkt.size)
    if n and (bkt.min() < 0 or bkt.max() >= nb):
        raise ValueError("bucket out of range")
    nseg = nseg_for(n)
    seg_idx = np.empty(n, np.uint8)
    seg_off = np.zeros((nseg, nb + 1), np.uint16)
    for s in range(nseg):
        b = bkt[s * SEG:(s + 1) * SEG]
        # a stable sort by bucket keeps packet order inside each bucket
        seg_idx[s * SEG:s * SEG + b.size] = np.argsort(b, kind="stable")
        seg_off[s, 1:] = np.cumsum(np.bincount(b, minlength=nb))
    return seg_idx, seg_off


def from_q(q: np.ndarray, nb_queues: int):
    """(seg_idx uint8[n], seg_off uint16[nseg, nb_queues + 2]) of a q array."""
    return from_buckets(buckets_of(q, nb_queues), nb_queues + 1)


def route_buckets(q: np.ndarray, fclass: np.ndarray, nb_queues: int, queue_id: int,
                  kni_enable: bool, kni_accept: bool) -> np.ndarray:
    """Route bucket of every packet (``yrss_route_dev_seg``), nq = nb_queues:
    b < nq, b != queue_id the ring of queue b; queue_id local delivery (with
    the TRUNC / LOOP classes); nq freed; nq + 1 KNI; nq + 2 ARP on the local
    queue.  queue_id >= nq: no packet is local."""
    q = np.asarray(q).astype(np.int64)
    f = np.asarray(fclass).astype(np.int64)
    nq = int(nb_queues)
    bkt = np.where((q >= 0) & (q < nq), q, nq)
    local = bkt == queue_id if queue_id < nq else np.zeros(q.shape, bool)
    arp = local & (f == abi.FILTER_ARP)
    want = abi.FILTER_KNI if kni_accept else abi.FILTER_UNKNOWN
    kni = local & ~arp & bool(kni_enable) & (f == want)
    bkt = np.where(kni, nq + 1, bkt)
    return np.where(arp, nq + 2, bkt)


def route_from(q: np.ndarray, fclass: np.ndarray, nb_queues: int, queue_id: int,
               kni_enable: bool, kni_accept: bool):
    """(seg_idx uint8[n], seg_off uint16[nseg, nb_queues + 4]): the routed
    segmented lists of per-packet q and filter-class arrays."""
    return from_buckets(route_buckets(q, fclass, nb_queues, queue_id, kni_enable, kni_accept),
                        nb_queues + 3)


def route_lists_from(q: np.ndarray, fclass: np.ndarray, nb_queues: int, queue_id: int,
                     kni_enable: bool, kni_accept: bool):
    """(ridx uint32[n], rstart uint32[nb_queues + 4]): the routed global lists
    of a one-workgroup burst (``yrss_route_lists_burst`` / ``_frames``, the
    route worker), a stable sort by :func:`route_buckets`."""
    bkt = route_buckets(q, fclass, nb_queues, queue_id, kni_enable, kni_accept).reshape(-1)
    nrb = int(nb_queues) + 3
    ridx = np.argsort(bkt, kind="stable").astype(np.uint32)
    rstart = np.zeros(nrb + 1, np.uint32)
    rstart[1:] = np.cumsum(np.bincount(bkt, minlength=nrb))
    return ridx, rstart


def to_lists(seg_idx: np.ndarray, seg_off: np.ndarray, n: int, nbk: int):
    """(qidx uint32[n], qstart uint32[nbk + 1]) as ``yrss_dispatch_dev`` gives
    them.  Raises ValueError on what ``yrss_seg_to_lists`` answers with -EINVAL:
    an offset row that is not monotone from 0 to len_s, an index >= len_s."""
    n = int(n)
    nseg = nseg_for(n)
    seg_idx = np.asarray(seg_idx).reshape(-1).view(np.uint8)
    off = np.asarray(seg_off).reshape(-1).view(np.uint16)
    if seg_idx.size < n or off.size < nseg * (nbk + 1):
        raise ValueError("arrays shorter than the batch")
    off = off[:nseg * (nbk + 1)].reshape(nseg, nbk + 1).astype(np.int64)
    lens = np.minimum(SEG, n - SEG * np.arange(nseg, dtype=np.int64))
    if nseg and (np.any(off[:, 0] != 0) or np.any(off[:, nbk] != lens) or
                 np.any(np.diff(off, axis=1) < 0)):
        raise ValueError("bad segment offsets")
    idx = seg_idx[:n].astype(np.int64)
    seg_of = np.arange(n, dtype=np.int64) // SEG
    if n and np.any(idx >= lens[seg_of]):
        raise ValueError("segment index out of range")
    # position k of segment s lies in bucket b iff off[s][b] <= k < off[s][b+1]
    pos = np.arange(n, dtype=np.int64) - seg_of * SEG
    bkt = np.zeros(n, np.int64)
    for b in range(1, nbk):
        bkt += pos >= off[seg_of, b]
    order = np.argsort(bkt, kind="stable")     # bucket-major, segment order inside
    qidx = (seg_of * SEG + idx)[order].astype(np.uint32)
    qstart = np.zeros(nbk + 1, np.uint32)
    qstart[1:] = np.cumsum(np.bincount(bkt, minlength=nbk)[:nbk])
    return qidx, qstart


def to_lists_c(seg_idx: np.ndarray, seg_off: np.ndarray, n: int, nbk: int):
    """The same through the C helper ``yrss_seg_to_lists`` of libyrss.so."""
    seg_idx = np.ascontiguousarray(np.asarray(seg_idx).reshape(-1).view(np.uint8))
    off = np.ascontiguousarray(np.asarray(seg_off).reshape(-1).view(np.uint16))
    if seg_idx.size < n or off.size < nseg_for(n) * (nbk + 1):
        raise ValueError("arrays shorter than the batch")
    qidx = np.empty(max(int(n), 1), np.uint32)
    qstart = np.empty(nbk + 1, np.uint32)
    rc = abi.load().yrss_seg_to_lists(seg_idx.ctypes.data, off.ctypes.data, int(n), int(nbk),
                                      qidx.ctypes.data, qstart.ctypes.data)
    if rc == -errno.EINVAL:
        raise ValueError("yrss_seg_to_lists: bad segment arrays")
    abi.check(rc, "yrss_seg_to_lists")
    return qidx[:int(n)], qstart
