"""Host-side mirror of yastack's dispatch interface over the HIP engine.

Reference interface (fs/lib/ff_api.h:146-176, fs/lib/ff_dpdk_if.c):

* ``toeplitz_dispatch(data, len, queue_id, nb_queues) -> int`` — per packet.
  Here: :meth:`SoftRss.dispatch_frames` / :meth:`SoftRss.dispatch_burst`
  return the same per-packet ints for a whole burst, computed on the GPU.
* ``process_packets``' dispatcher block (ff_dpdk_if.c:1078-1094) — drop
  ``ret < 0 || ret >= nb_queues``, else enqueue to ``dispatch_ring[port][ret]``.
  Here: the per-queue FIFO index lists of :class:`DispatchResult`.
* ``ff_global_cfg`` knobs (nb_procs, soft_dispatch, dispatch_only_core) and the
  port's nb_queues: the :class:`SoftRss` constructor, or
  :meth:`SoftRss.from_ff_config` for an fs/lib INI file.

Device memory and streams come from PyTorch (plumbing only); every byte of
parse/hash/compaction runs in the HIP kernels of libyrss.so.
"""
from __future__ import annotations

import ctypes
import errno
from dataclasses import dataclass

import numpy as np

from . import abi


@dataclass
class DispatchResult:
    """Per-packet queue/hash plus per-queue FIFO index lists.

    ``q[i]``      toeplitz_dispatch's return for packet i (int16)
    ``hash[i]``   Toeplitz hash (0 where the reference does not hash)
    ``qidx``      packet indices grouped by bucket, FIFO inside a bucket
    ``qstart``    nb_queues+2 offsets; bucket nb_queues = packets the
                  reference frees (ret < 0 or ret >= nb_queues)
    """

    q: object
    hash: object
    qidx: object = None
    qstart: object = None
    filter: object = None     # protocol_filter class per packet (abi.FILTER_*)

    def queue(self, b: int):
        """Indices dispatched to queue b (b == nb_queues: dropped)."""
        s = self.qstart
        return self.qidx[int(s[b]):int(s[b + 1])]


@dataclass
class SegResult:
    """Per-packet queue/hash plus the segmented per-queue lists
    (``yrss_dispatch_dev_seg``): the batch in segments of ``abi.SEG_PKTS``
    consecutive packets, each with its own finished lists.

    ``seg_idx``   n x uint8: bytes [256 s, 256 s + len_s) are segment s's
                  segment-local packet indices, grouped by bucket, FIFO inside
    ``seg_off``   nseg x (nb_queues + 2) uint16 offsets into those bytes

    From ``yrss_route_dev_seg`` the buckets are the nb_queues + 3 route classes
    (``segments.route_buckets``) and a ``seg_off`` row has nb_queues + 4 entries.
    """

    q: object
    hash: object
    filter: object
    seg_idx: object
    seg_off: object
    n: int = 0

    def segment(self, s: int, b: int):
        """Segment-local indices of segment s dispatched to queue b (b ==
        nb_queues: dropped); packet number = 256 * s + index."""
        o = self.seg_off[s]
        base = s * abi.SEG_PKTS
        return self.seg_idx[base + int(o[b]):base + int(o[b + 1])]


def _check_sizes(n, stride, win, lens, out, required=(), optional=()):
    """The C ABI takes raw device pointers and cannot see the buffers' sizes: a
    batch larger than its buffers would fault the GPU.  Refuse it here.  Beside
    win, lens, q and the optional hash and filter a form has rows of its own,
    (name, buffer, bytes): ``required`` ones, and ``optional`` ones that are
    checked where the buffer is given."""
    def nbytes(t):
        return 0 if t is None else int(t.numel()) * int(t.element_size())
    if n < 0:
        raise ValueError("negative batch size")
    if n == 0:
        return
    # the kernel may read any byte below the stride of a window (rare header walks)
    need = [("win", win, n * stride), ("lens", lens, 2 * n), ("q", out.q, 2 * n), *required]
    need += [row for row in (("hash", out.hash, 4 * n), *optional, ("filter", out.filter, n))
             if row[1] is not None]
    for name, t, b in need:
        if nbytes(t) < b:
            raise ValueError(f"{name} holds {nbytes(t)} bytes, the batch of {n} needs {b}")


def _check_dev_sizes(n, stride, win, lens, out, nb_queues):
    """_check_sizes for the global lists' buffers."""
    _check_sizes(n, stride, win, lens, out, optional=(
        ("qidx", out.qidx, 4 * n), ("qstart", out.qstart, 4 * (nb_queues + 2))))


def _check_seg_sizes(n, stride, win, lens, out, nb_queues, nbk=None):
    """_check_sizes for the segmented form's buffers (nbk buckets a segment:
    nb_queues + 1, or the routed form's nb_queues + 3)."""
    nbk = nb_queues + 1 if nbk is None else nbk
    nseg = -(-n // abi.SEG_PKTS)
    _check_sizes(n, stride, win, lens, out, required=(
        ("seg_idx", out.seg_idx, n), ("seg_off", out.seg_off, 2 * nseg * (nbk + 1))))


def _ptr(t) -> int | None:
    if t is None:
        return None
    if isinstance(t, np.ndarray):
        return t.ctypes.data
    return t.data_ptr()


def _host_out(n, noff, want_hash=True, compact=True, want_filter=False):
    """The host output arrays of one burst, (q, hash, qidx, qstart, filter): n
    entries each (one at least) and noff offsets, None where not wanted.  The
    routed forms always have their lists (compact) and may have the filter."""
    m = max(n, 1)
    return (np.empty(m, np.int16),
            np.empty(m, np.uint32) if want_hash else None,
            np.empty(m, np.uint32) if compact else None,
            np.empty(noff, np.uint32) if compact else None,
            np.empty(m, np.int8) if want_filter else None)


def _host_result(n, out) -> DispatchResult:
    """_host_out's arrays, the per-packet ones cut to the burst's n."""
    q, h, qi, _, f = (None if a is None else a[:n] for a in out)
    return DispatchResult(q, h, qi, out[3], f)   # (the offsets are whole)


def _frame_ptrs(frames):
    """A list of frames (bytes) as the C calls take it: (the data pointers, the
    lengths, the buffers the pointers point into, to be kept until the call
    has returned)."""
    sizes = [len(f) for f in frames]
    if any(size > 65535 for size in sizes):
        raise ValueError("frame longer than 65535 bytes")
    bufs = [np.frombuffer(bytes(f), dtype=np.uint8) if len(f) else np.zeros(1, np.uint8)
            for f in frames]
    ptrs = np.array([b.ctypes.data for b in bufs], dtype=np.uint64)
    return ptrs, np.array(sizes, dtype=np.uint16), bufs


def _flat(a, dtype):
    """A host array as the flat contiguous one of dtype that a C hand-off
    reads (None stays None)."""
    return None if a is None else np.ascontiguousarray(np.asarray(a).reshape(-1)).view(dtype)


def reta_weighted(weights, size: int = 128, lib_path: str | None = None):
    """A redirection table of ``size`` entries over the queues
    ``0..len(weights) - 1`` in proportion to ``weights`` (smooth weighted
    round-robin, ``yrss_reta_fill_weighted``; pure host code).  Weight 0 keeps
    a queue out; equal weights give ``table[i] == i % len(weights)``."""
    w = np.asarray(weights)
    if w.ndim != 1 or np.any(w < 0) or np.any(w > 0xFFFFFFFF):
        raise ValueError("weights are a flat list of 32-bit unsigned numbers")
    w = np.ascontiguousarray(w, dtype=np.uint32)
    t = np.zeros(max(int(size), 1), np.uint16)
    abi.check(abi.load(lib_path).yrss_reta_fill_weighted(t.ctypes.data, int(size), w.ctypes.data,
                                                          int(w.size)),
              "yrss_reta_fill_weighted")
    return t


class SoftRss:
    """One engine context on one GPU (``yrss_ctx``)."""

    def __init__(self, nb_procs: int = 3, nb_queues: int | None = None,
                 soft_dispatch: int = 1, dispatch_only_core: int = 1,
                 rss_key: bytes | None = None, device: int = 0,
                 max_burst: int = 1 << 16, lib_path: str | None = None):
        self._lib = abi.load(lib_path)
        cfg = abi.Config()
        self._lib.yrss_config_default(ctypes.byref(cfg))
        if rss_key is not None:
            if not 4 <= len(rss_key) <= abi.RSS_KEY_LEN:
                raise ValueError("rss_key must be 4..40 bytes")
            ctypes.memmove(cfg.rss_key, bytes(rss_key), len(rss_key))
            cfg.rss_key_len = len(rss_key)
        cfg.nb_procs = nb_procs
        cfg.nb_queues = nb_procs if nb_queues is None else nb_queues
        cfg.soft_dispatch = soft_dispatch
        cfg.dispatch_only_core = dispatch_only_core
        cfg.device = device
        cfg.max_burst = max_burst
        self.cfg = cfg
        self.nb_queues = int(cfg.nb_queues)
        self.device = device
        ctx = ctypes.c_void_p()
        abi.check(self._lib.yrss_init(ctypes.byref(cfg), ctypes.byref(ctx)), "yrss_init")
        self._ctx = ctx
        self._kni_enable = False

    @classmethod
    def from_ff_config(cls, path: str, port: int = 0, device: int = 0, **kw) -> "SoftRss":
        from .ffconfig import load_ff_config

        fc = load_ff_config(path)
        eng = cls(nb_procs=fc.nb_procs, nb_queues=fc.nb_queues[port],
                  soft_dispatch=fc.soft_dispatch,
                  dispatch_only_core=fc.dispatch_only_core, device=device, **kw)
        if fc.kni_enable:
            # init_kni (ff_dpdk_if.c:598-606) behind enable_kni (:921-923)
            eng.set_kni(True, fc.kni_method, fc.kni_tcp_port, fc.kni_udp_port)
        return eng

    # -- lifetime ---------------------------------------------------------
    def close(self) -> None:
        if getattr(self, "_ctx", None) and self._ctx.value:
            # a device guard that fired and was never read (yrss_status /
            # fault_info) is logged before the context goes (abi.FAULT_LOG);
            # a context that already timed out on the GPU is not waited for
            # again (yrss_fault_info drains the context's streams)
            f = abi.Fault()
            if not getattr(self, "_hung", False) and \
                    self._lib.yrss_fault_info(self._ctx, ctypes.byref(f)) == 0 and f.code:
                abi.FAULT_LOG.append((int(f.code), int(f.kernel), int(f.where), int(f.value)))
            self._lib.yrss_fini(self._ctx)
            self._ctx = ctypes.c_void_p()

    def _ck(self, rc: int, what: str) -> None:
        if rc == -errno.ETIMEDOUT:
            self._hung = True     # close() does not wait on this context again
        abi.check(rc, what)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    # -- torch plumbing ------------------------------------------------------
    def _torch(self):
        import torch

        return torch

    def _stream(self, stream):
        torch = self._torch()
        if stream is None:
            stream = torch.cuda.current_stream(self.device)
        return ctypes.c_void_p(stream.cuda_stream)

    # -- KNI / protocol_filter ------------------------------------------------
    def set_kni(self, enable: bool, method: str | None = "reject", tcp_ports: str | None = None,
                udp_ports: str | None = None) -> None:
        """ff_kni_init/init_kni: enable, method accept|reject, port lists."""
        enc = (lambda x: None if x is None else x.encode())
        abi.check(self._lib.yrss_set_kni(self._ctx, 1 if enable else 0, enc(method),
                                         enc(tcp_ports), enc(udp_ports)), "yrss_set_kni")
        self._kni_enable = bool(enable)

    # -- extended mode (this build's own semantics, not fs/lib's) -----------
    def set_extended(self, vlan: bool = False, ipv6: bool = False, udp: bool = False) -> None:
        """Opt into hashing what ``toeplitz_dispatch`` leaves on queue 2
        (``yrss_set_extended``): ``vlan`` classifies a frame as if its one or
        two VLAN tags had been stripped, ``ipv6`` hashes IPv6 TCP over the 36
        wire-order tuple bytes, ``udp`` lets UDP take the TCP branch.  All
        False restores the reference's rules exactly.  A persistent worker
        started with ``extended=True`` follows the flags; any other refuses
        bursts (ENOTSUP) while a flag is set."""
        flags = (abi.EXT_VLAN if vlan else 0) | (abi.EXT_IPV6 if ipv6 else 0) | \
            (abi.EXT_UDP if udp else 0)
        abi.check(self._lib.yrss_set_extended(self._ctx, flags), "yrss_set_extended")
        self.ext_flags = flags

    # -- redirection table (this build's own semantics as well) --------------
    def set_reta(self, table=None) -> None:
        """Queue of a hashed packet from a redirection table
        (``yrss_set_reta``): ``table[hash & (len(table) - 1)]`` in place of
        ``hash % d (+1)``; a power of two of entries, 1..``abi.RETA_MAX``, each
        below ``nb_queues``.  ``None`` (or an empty table) restores the
        reference's rule exactly.  Unhashed and truncated packets keep their
        queues.  The persistent worker does not follow a table: its starts and
        submits are refused (ENOTSUP) while one is set."""
        if table is None or len(table) == 0:
            rc = self._lib.yrss_set_reta(self._ctx, None, 0)
        else:
            t = np.asarray(table)
            if t.ndim != 1 or np.any(t < 0) or np.any(t > 0xFFFF):
                raise ValueError("a redirection table is a flat list of queue ids")
            t = np.ascontiguousarray(t, dtype=np.uint16)
            rc = self._lib.yrss_set_reta(self._ctx, t.ctypes.data, int(t.size))
        abi.check(rc, "yrss_set_reta")

    def get_reta(self):
        """The table in force (uint16 array), ``None`` when none is set
        (``yrss_get_reta``)."""
        t = np.zeros(abi.RETA_MAX, np.uint16)
        size = self._lib.yrss_get_reta(self._ctx, t.ctypes.data, abi.RETA_MAX)
        abi.check(size, "yrss_get_reta")
        return t[:size].copy() if size else None

    # -- device-resident path ---------------------------------------------
    def dispatch_dev(self, win, lens, stride: int, n: int | None = None, *,
                     out=None, want_hash: bool = True, compact: bool = True,
                     want_filter: bool = False, stream=None) -> DispatchResult:
        """Classify n packets resident in HBM (``yrss_dispatch_dev_ex``)."""
        n = int(lens.numel()) if n is None else n
        dev = lens.device
        if out is None:
            out = self.alloc_out(n, dev, want_hash, compact, want_filter)
        _check_dev_sizes(n, stride, win, lens, out, self.nb_queues)
        b = abi.DevBatch(_ptr(win), stride, n, _ptr(lens), _ptr(out.q), _ptr(out.hash),
                         _ptr(out.qidx), _ptr(out.qstart), _ptr(out.filter))
        rc = self._lib.yrss_dispatch_dev_ex(self._ctx, ctypes.byref(b), self._stream(stream))
        abi.check(rc, "yrss_dispatch_dev_ex")
        return out

    def dispatch_dev_seg(self, win, lens, stride: int, n: int | None = None, *, out=None,
                         want_hash: bool = True, want_filter: bool = False,
                         stream=None) -> SegResult:
        """Classify n packets resident in HBM and return the per-queue lists in
        segments of 256 packets, written by the parse kernel itself
        (``yrss_dispatch_dev_seg``: one launch; nb_queues + 1 <= 16, n <= 2^24)."""
        n = int(lens.numel()) if n is None else n
        if out is None:
            out = self.alloc_seg_out(n, lens.device, want_hash, want_filter)
        _check_seg_sizes(n, stride, win, lens, out, self.nb_queues)
        b = abi.DevSegBatch(_ptr(win), stride, n, _ptr(lens), _ptr(out.q), _ptr(out.hash),
                            _ptr(out.filter), _ptr(out.seg_idx), _ptr(out.seg_off))
        rc = self._lib.yrss_dispatch_dev_seg(self._ctx, ctypes.byref(b), self._stream(stream))
        abi.check(rc, "yrss_dispatch_dev_seg")
        out.n = n
        return out

    def alloc_seg_out(self, n: int, dev, want_hash=True, want_filter=False) -> SegResult:
        return self._alloc_seg(n, dev, want_hash, want_filter, self.nb_queues + 2)

    def _alloc_seg(self, n, dev, want_hash, want_filter, noff) -> SegResult:
        torch = self._torch()
        nseg = max(-(-n // abi.SEG_PKTS), 1)
        q = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
        h = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if want_hash else None
        f = torch.empty(max(n, 1), dtype=torch.int8, device=dev) if want_filter else None
        si = torch.empty(max(n, 1), dtype=torch.uint8, device=dev)
        so = torch.empty((nseg, noff), dtype=torch.int16, device=dev)
        return SegResult(q, h, f, si, so, n)

    def route_dev_seg(self, win, lens, stride: int, queue_id: int, n: int | None = None, *,
                      out=None, want_hash: bool = True, want_filter: bool = False,
                      stream=None) -> SegResult:
        """Classify n packets resident in HBM into process_packets' hand-off
        classes for the lcore whose queue is ``queue_id`` and return them as
        segmented lists over nb_queues + 3 route buckets (``yrss_route_dev_seg``:
        one launch; nb_queues <= 13, n <= 2^24; the KNI state is that of the
        last :meth:`set_kni`).  :meth:`route_seg` performs the hand-off."""
        n = int(lens.numel()) if n is None else n
        if out is None:
            out = self.alloc_route_out(n, lens.device, want_hash, want_filter)
        _check_seg_sizes(n, stride, win, lens, out, self.nb_queues, self.nb_queues + 3)
        b = abi.DevRouteBatch(_ptr(win), stride, n, _ptr(lens), _ptr(out.q), _ptr(out.hash),
                              _ptr(out.filter), _ptr(out.seg_idx), _ptr(out.seg_off), queue_id)
        rc = self._lib.yrss_route_dev_seg(self._ctx, ctypes.byref(b), self._stream(stream))
        abi.check(rc, "yrss_route_dev_seg")
        out.n = n
        return out

    def alloc_route_out(self, n: int, dev, want_hash=True, want_filter=False) -> SegResult:
        """Output buffers of :meth:`route_dev_seg`: those of the segmented form
        with nb_queues + 4 offsets a segment."""
        return self._alloc_seg(n, dev, want_hash, want_filter, self.nb_queues + 4)

    def alloc_out(self, n: int, dev, want_hash=True, compact=True,
                  want_filter=False) -> DispatchResult:
        torch = self._torch()
        q = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
        h = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if want_hash else None
        qi = torch.empty(max(n, 1), dtype=torch.int32, device=dev) if compact else None
        qs = torch.empty(self.nb_queues + 2, dtype=torch.int32, device=dev) if compact else None
        f = torch.empty(max(n, 1), dtype=torch.int8, device=dev) if want_filter else None
        return DispatchResult(q, h, qi, qs, f)

    def synth(self, profile: int, n: int, first: int = 0, seed: int = 0x9E3779B97F4A7C15,
              nflows: int = 1 << 20, stride: int = abi.WIN_MIN, stream=None):
        """Synthetic header windows + data_len written straight into HBM."""
        torch = self._torch()
        dev = torch.device("cuda", self.device)
        win = torch.empty(max(n, 1) * stride, dtype=torch.uint8, device=dev)
        lens = torch.empty(max(n, 1), dtype=torch.int16, device=dev)
        p = abi.SynthParams(seed & 0xFFFFFFFFFFFFFFFF, profile, nflows)
        rc = self._lib.yrss_synth_dev(self._ctx, ctypes.byref(p), first, n, _ptr(win), stride,
                                      _ptr(lens), self._stream(stream))
        abi.check(rc, "yrss_synth_dev")
        return win, lens[:n] if n else lens[:0]

    # -- host-resident paths (synchronous) ----------------------------------
    def dispatch_frames(self, frames, want_hash=True, compact=True) -> DispatchResult:
        """Classify a list of frames (bytes) — one toeplitz_dispatch per frame."""
        n = len(frames)
        ptrs, lens, _bufs = _frame_ptrs(frames)
        out = _host_out(n, self.nb_queues + 2, want_hash, compact)
        rc = self._lib.yrss_dispatch_frames(self._ctx, _ptr(ptrs), _ptr(lens), n,
                                            *map(_ptr, out[:4]))
        abi.check(rc, "yrss_dispatch_frames")
        return _host_result(n, out)

    def dispatch_burst(self, mbuf_ptrs: np.ndarray, want_hash=True, compact=True,
                       write_rss=False, async_=False) -> DispatchResult:
        """Classify a burst of ``struct rte_mbuf *`` (uint64 addresses).

        ``async_=True`` (YRSS_F_ASYNC) returns once the burst is queued; the
        result's arrays are valid after :meth:`wait`."""
        return self._burst("yrss_dispatch_burst", mbuf_ptrs, want_hash, compact, write_rss,
                           async_)

    def _burst(self, name, mbuf_ptrs, want_hash, compact, write_rss, async_) -> DispatchResult:
        """dispatch_burst / dispatch_burst_zc: the C call ``name`` on the burst."""
        mb = np.ascontiguousarray(mbuf_ptrs, dtype=np.uint64)
        n = int(mb.size)
        out = _host_out(n, self.nb_queues + 2, want_hash, compact)
        flags = (abi.F_WRITE_RSS if write_rss else 0) | (abi.F_ASYNC if async_ else 0)
        rc = getattr(self._lib, name)(self._ctx, _ptr(mb), n, *map(_ptr, out[:4]), flags)
        abi.check(rc, name)
        self._inflight = mb if async_ else None   # keep the pointer array alive
        return _host_result(n, out)

    def wait(self) -> None:
        """Complete the burst queued with ``async_=True`` (``yrss_wait``)."""
        rc = self._lib.yrss_wait(self._ctx)
        self._inflight = None
        self._ck(rc, "yrss_wait")

    # -- persistent burst worker ------------------------------------------------
    def worker_start(self, nslots: int = 16, nblocks: int = 4,
                     route_queue_id: int | None = None, extended: bool = False) -> None:
        """Start the persistent small-burst worker (``yrss_worker_start``).
        With ``route_queue_id`` (``yrss_worker_start_route``, nb_queues <= 61)
        every burst's ``qidx`` / ``qstart`` are the routed lists for the lcore
        whose queue that is: packet indices grouped by route class
        (``segments.route_buckets``) and nb_queues + 4 offsets, under the KNI
        state of the last :meth:`set_kni`; :meth:`route_lists` hands them off.
        ``extended`` (``yrss_worker_start_flags``, ``WORKER_F_EXTENDED``): the
        worker follows :meth:`set_extended` instead of refusing bursts while
        a flag is set."""
        if extended:
            flags = abi.WORKER_F_EXTENDED | (0 if route_queue_id is None else abi.WORKER_F_ROUTE)
            abi.check(self._lib.yrss_worker_start_flags(self._ctx, nslots, nblocks, flags,
                                                        route_queue_id or 0),
                      "yrss_worker_start_flags")
        elif route_queue_id is None:
            abi.check(self._lib.yrss_worker_start(self._ctx, nslots, nblocks),
                      "yrss_worker_start")
        else:
            abi.check(self._lib.yrss_worker_start_route(self._ctx, nslots, nblocks,
                                                        route_queue_id),
                      "yrss_worker_start_route")
        self._wk = {}
        self._wk_offsets = self.nb_queues + (2 if route_queue_id is None else 4)

    def worker_submit(self, mbuf_ptrs: np.ndarray, want_hash=True, compact=True,
                      write_rss=False) -> int:
        """Queue one burst of ``struct rte_mbuf *`` (registered memory); returns
        its ticket.  :meth:`worker_poll` returns the DispatchResult."""
        mb = np.ascontiguousarray(mbuf_ptrs, dtype=np.uint64)
        n = int(mb.size)
        flags = abi.F_WRITE_RSS if write_rss else 0
        return self._worker_queue(
            "yrss_worker_submit", n, want_hash, compact,
            lambda outs, t: self._lib.yrss_worker_submit(self._ctx, _ptr(mb), n, *outs, flags, t))

    def _worker_queue(self, name, n, want_hash, compact, call) -> int:
        """The three worker submits: ``call(outs, ticket)`` makes the C call
        ``name`` with the burst's four output pointers and the ticket to fill;
        the DispatchResult waits under its ticket for :meth:`worker_poll`."""
        out = _host_out(n, self._wk_offsets, want_hash, compact)
        t = ctypes.c_uint64()
        abi.check(call([_ptr(a) for a in out[:4]], ctypes.byref(t)), name)
        self._wk[t.value] = _host_result(n, out)
        return t.value

    def worker_submit_frames(self, data_ptrs: np.ndarray, lens: np.ndarray, want_hash=True,
                             compact=True) -> int:
        """Queue one burst of (frame data pointer, data_len) pairs in registered
        memory (``yrss_worker_submit_frames``); returns its ticket."""
        dp = np.ascontiguousarray(data_ptrs, dtype=np.uint64)
        ln = np.ascontiguousarray(lens, dtype=np.uint16)
        n = int(dp.size)
        if ln.size != n:
            raise ValueError("data_ptrs and lens differ in length")
        return self._worker_queue(
            "yrss_worker_submit_frames", n, want_hash, compact,
            lambda outs, t: self._lib.yrss_worker_submit_frames(self._ctx, _ptr(dp), _ptr(ln), n,
                                                                *outs, t))

    def worker_submit_windows(self, win: np.ndarray, stride: int, lens: np.ndarray,
                              want_hash=True, compact=True) -> int:
        """Queue one burst of contiguous windows (window i at win[i * stride:])
        that lie in registered memory (``yrss_worker_submit_windows``)."""
        ln = np.ascontiguousarray(lens, dtype=np.uint16)
        n = int(ln.size)
        return self._worker_queue(
            "yrss_worker_submit_windows", n, want_hash, compact,
            lambda outs, t: self._lib.yrss_worker_submit_windows(self._ctx, _ptr(win), stride,
                                                                 _ptr(ln), n, *outs, t))

    def toeplitz_dispatch(self, frame: bytes, queue_id: int = 0) -> int:
        """The per-packet registration shim (``yrss_toeplitz_dispatch``) on this
        context: ``toeplitz_dispatch``'s return value for one frame, computed on
        the GPU.  One launch per call: for compatibility, not speed."""
        abi.check(self._lib.yrss_set_dispatch_ctx(self._ctx), "yrss_set_dispatch_ctx")
        buf = ctypes.create_string_buffer(bytes(frame), len(frame))
        return int(self._lib.yrss_toeplitz_dispatch(ctypes.cast(buf, ctypes.c_void_p),
                                                    len(frame), queue_id, self.nb_queues))

    def worker_poll(self, ticket: int, wait: bool = True):
        """The burst's DispatchResult, or None while it is pending (wait=False)."""
        rc = self._lib.yrss_worker_poll(self._ctx, ticket, 1 if wait else 0)
        if rc == -11:   # -EAGAIN
            return None
        res = self._wk.pop(ticket, None)
        self._ck(rc, "yrss_worker_poll")
        return res

    def worker_stop(self) -> None:
        abi.check(self._lib.yrss_worker_stop(self._ctx), "yrss_worker_stop")
        self._wk = {}

    def register_host_memory(self, base: int, nbytes: int) -> None:
        abi.check(self._lib.yrss_register_host_memory(self._ctx, base, nbytes),
                  "yrss_register_host_memory")

    def unregister_host_memory(self, base: int) -> None:
        abi.check(self._lib.yrss_unregister_host_memory(self._ctx, base),
                  "yrss_unregister_host_memory")

    def dispatch_burst_zc(self, mbuf_ptrs: np.ndarray, want_hash=True, compact=True,
                          write_rss=False, async_=False) -> DispatchResult:
        """Zero-copy burst: mbufs in registered host memory are read by the GPU.
        ``async_`` as in :meth:`dispatch_burst`."""
        return self._burst("yrss_dispatch_burst_zc", mbuf_ptrs, want_hash, compact, write_rss,
                           async_)

    def route_burst(self, mbuf_ptrs: np.ndarray, queue_id: int, enqueue, clone, release,
                    kni_primary: bool = True):
        """process_packets' hand-off for a burst (``yrss_route_burst``).

        ``enqueue(queue, [mbuf addr...]) -> n_enqueued``, ``clone(mbuf, queue)
        -> addr or 0``, ``release(mbuf)`` are called back from C.  Returns
        (local list, kni list, RouteResult)."""
        mb = np.ascontiguousarray(mbuf_ptrs, dtype=np.uint64)
        n = int(mb.size)
        return self._hand_off(
            "yrss_route_burst", n, 2 * n, enqueue, clone, release,
            lambda ops, local, kni, res: self._lib.yrss_route_burst(
                self._ctx, _ptr(mb), n, queue_id, 1 if kni_primary else 0, ops, local, kni, res))

    @staticmethod
    def _hand_off(name, n, kni_size, enqueue, clone, release, call):
        """The callback shim of the three hand-off calls: ``call(ops, local,
        kni, res)`` makes the C call ``name`` with the RouteOps built from the
        Python callbacks (the thunks live until it returns), a local list of n
        and a KNI list of ``kni_size`` addresses."""
        def _enq(user, queue, ptrs, cnt):
            return int(enqueue(int(queue), [int(ptrs[i] or 0) for i in range(cnt)]))

        def _clone(user, m, queue):
            return int(clone(int(m or 0), int(queue)) or 0)

        def _rel(user, m):
            release(int(m or 0))

        ops = abi.RouteOps(abi.ENQUEUE_FN(_enq), abi.CLONE_FN(_clone), abi.RELEASE_FN(_rel), None)
        local = np.zeros(max(n, 1), np.uint64)
        kni = np.zeros(max(kni_size, 1), np.uint64)
        res = abi.RouteResult()
        abi.check(call(ctypes.byref(ops), _ptr(local), _ptr(kni), ctypes.byref(res)), name)
        return local[:res.n_local].tolist(), kni[:res.n_kni].tolist(), res

    def route_lists_frames(self, frames, queue_id: int, want_hash=True,
                           want_filter=True) -> DispatchResult:
        """Classify a list of frames (bytes) into process_packets' hand-off
        classes for the lcore whose queue is ``queue_id``, in one launch
        (``yrss_route_lists_frames``: n <= 4096, nb_queues <= 61).  The
        result's ``qidx`` / ``qstart`` are the routed lists: packet indices
        grouped by route class and nb_queues + 4 offsets."""
        n = len(frames)
        ptrs, lens, _bufs = _frame_ptrs(frames)
        out = _host_out(n, self.nb_queues + 4, want_hash, want_filter=want_filter)
        q, h, ri, rs, f = map(_ptr, out)
        rc = self._lib.yrss_route_lists_frames(self._ctx, _ptr(ptrs), _ptr(lens), n, queue_id,
                                               q, h, f, ri, rs)
        self._ck(rc, "yrss_route_lists_frames")
        return _host_result(n, out)

    def route_lists_burst(self, mbuf_ptrs: np.ndarray, queue_id: int, want_hash=True,
                          want_filter=True, write_rss=False) -> DispatchResult:
        """The same for a burst of ``struct rte_mbuf *`` (uint64 addresses;
        ``yrss_route_lists_burst``)."""
        mb = np.ascontiguousarray(mbuf_ptrs, dtype=np.uint64)
        n = int(mb.size)
        out = _host_out(n, self.nb_queues + 4, want_hash, want_filter=want_filter)
        q, h, ri, rs, f = map(_ptr, out)
        rc = self._lib.yrss_route_lists_burst(self._ctx, _ptr(mb), n, queue_id, q, h, f, ri, rs,
                                              abi.F_WRITE_RSS if write_rss else 0)
        self._ck(rc, "yrss_route_lists_burst")
        return _host_result(n, out)

    def route_lists(self, result_or_arrays, objs, queue_id: int, enqueue, clone, release,
                    kni_primary: bool = True):
        """process_packets' hand-off from routed global lists
        (``yrss_route_lists``), mirroring :meth:`route_seg`:
        ``result_or_arrays`` is the DispatchResult of :meth:`route_lists_frames`
        / :meth:`route_lists_burst` / a route worker's poll, or host arrays
        ``(ridx, rstart)`` / ``(ridx, rstart, filter)``; ``objs`` the mbuf
        addresses, ``queue_id`` the one the lists were built for.  Returns
        (local list, kni list, RouteResult)."""
        if isinstance(result_or_arrays, DispatchResult):
            ridx, rstart, filt = (result_or_arrays.qidx, result_or_arrays.qstart,
                                  result_or_arrays.filter)
        else:
            ridx, rstart, *rest = result_or_arrays
            filt = rest[0] if rest else None
        ridx, rstart, filt = _flat(ridx, np.uint32), _flat(rstart, np.uint32), _flat(filt, np.int8)
        mb = np.ascontiguousarray(objs, dtype=np.uint64)
        n = int(mb.size)
        # the C call sees raw pointers only: the sizes are checked here
        if ridx.size < n or rstart.size < self.nb_queues + 4 or \
                (filt is not None and filt.size < n):
            raise ValueError("arrays shorter than the burst")

        kni_clone = 1 if self._kni_enable and kni_primary else 0
        return self._hand_off(
            "yrss_route_lists", n, n, enqueue, clone, release,
            lambda ops, local, kni, res: self._lib.yrss_route_lists(
                _ptr(ridx), _ptr(rstart), n, self.nb_queues, queue_id, kni_clone, _ptr(filt),
                _ptr(mb), ops, local, kni, res))

    def route_seg(self, result_or_arrays, objs, queue_id: int, enqueue, clone, release,
                  kni_primary: bool = True):
        """process_packets' hand-off from routed segments (``yrss_route_seg``),
        mirroring :meth:`route_burst`: ``result_or_arrays`` is the SegResult of
        :meth:`route_dev_seg` (copied to the host here; synchronise its stream
        first) or host arrays ``(seg_idx, seg_off, n)`` / ``(seg_idx, seg_off,
        n, filter)``; ``objs`` the n mbuf addresses, ``queue_id`` the one the
        lists were built for.  Returns (local list, kni list, RouteResult)."""
        if isinstance(result_or_arrays, SegResult):
            r = result_or_arrays
            n = int(r.n)
            host = (lambda t: None if t is None else t.cpu().numpy())
            seg_idx, seg_off, filt = host(r.seg_idx), host(r.seg_off), host(r.filter)
        else:
            seg_idx, seg_off, n, *rest = result_or_arrays
            filt = rest[0] if rest else None
            n = int(n)
        nseg = -(-n // abi.SEG_PKTS)
        seg_idx, seg_off, filt = (_flat(seg_idx, np.uint8), _flat(seg_off, np.uint16),
                                  _flat(filt, np.int8))
        mb = np.ascontiguousarray(objs, dtype=np.uint64)
        # the C call sees raw pointers only: the sizes are checked here
        if seg_idx.size < n or seg_off.size < nseg * (self.nb_queues + 4) or mb.size < n or \
                (filt is not None and filt.size < n):
            raise ValueError("arrays shorter than the batch")

        kni_clone = 1 if self._kni_enable and kni_primary else 0
        return self._hand_off(
            "yrss_route_seg", n, n, enqueue, clone, release,
            lambda ops, local, kni, res: self._lib.yrss_route_seg(
                _ptr(seg_idx), _ptr(seg_off), n, self.nb_queues, queue_id, kni_clone, _ptr(filt),
                _ptr(mb), ops, local, kni, res))

    # -- connect-side RSS check (ff_rss_check) -------------------------------
    def rss_check_dev(self, tuples, nb_queues: int, reta_size: int, queueid: int, stream=None):
        """ff_rss_check for n raw 12-byte tuples on the device (uint8 tensor n*12).
        Returns (ok uint8 tensor, hash int32 tensor)."""
        torch = self._torch()
        n = int(tuples.numel()) // 12
        ok = torch.empty(max(n, 1), dtype=torch.uint8, device=tuples.device)
        h = torch.empty(max(n, 1), dtype=torch.int32, device=tuples.device)
        abi.check(self._lib.yrss_rss_check_dev(self._ctx, _ptr(tuples), n, nb_queues, reta_size,
                                               queueid, _ptr(ok), _ptr(h), self._stream(stream)),
                  "yrss_rss_check_dev")
        return ok[:n], h[:n]

    def rss_lport_sweep(self, faddr: int, laddr: int, fport: int, nb_queues: int,
                        reta_size: int, queueid: int) -> np.ndarray:
        """Bitmap (2048 uint32) of every stored lport value accepted by ff_rss_check."""
        bm = np.zeros(2048, np.uint32)
        abi.check(self._lib.yrss_rss_lport_sweep(self._ctx, faddr, laddr, fport, nb_queues,
                                                 reta_size, queueid, _ptr(bm)),
                  "yrss_rss_lport_sweep")
        return bm

    # -- timing hook --------------------------------------------------------
    def timing_enable(self, mask: int = 1 << abi.K_PARSE_HASH) -> None:
        """Bracket every launch of kernel k (bit k of mask, abi.K_*) with HIP
        events on its own dispatch packet; 0 disables."""
        abi.check(self._lib.yrss_timing_enable(self._ctx, int(mask)), "yrss_timing_enable")

    def timing_read(self, kernel: int) -> tuple[float, int]:
        ms = ctypes.c_double()
        cnt = ctypes.c_uint32()
        abi.check(self._lib.yrss_timing_read(self._ctx, kernel, ctypes.byref(ms),
                                             ctypes.byref(cnt)), "yrss_timing_read")
        return ms.value, cnt.value

    def timing_quantile(self, kernel: int, q: float = 0.5) -> float:
        """q-quantile of kernel's per-launch durations (ms) since timing_enable."""
        ms = ctypes.c_double()
        abi.check(self._lib.yrss_timing_quantile(self._ctx, kernel, q, ctypes.byref(ms)),
                  "yrss_timing_quantile")
        return ms.value

    def status(self) -> int:
        """Synchronise and return (then clear) the device-side fault state:
        0, or -EIO if a list guard fired (yrss_status; details: fault_info)."""
        return int(self._lib.yrss_status(self._ctx))

    def fault_info(self):
        """Synchronise and return (then clear) the fault record as
        (code, kernel, where, value); code 0 (abi.FAULT_NONE) = no guard fired."""
        f = abi.Fault()
        abi.check(self._lib.yrss_fault_info(self._ctx, ctypes.byref(f)), "yrss_fault_info")
        return (int(f.code), int(f.kernel), int(f.where), int(f.value))

    def set_tuning(self, chunk_tiles: int = 0, span_tiles: int = 0, parse_blocks: int = 0,
                   one_launch: int = 0, scatter_xcd: int = -1, scan_kernel: int = 0) -> None:
        """Layout overrides for tests and measurements (yrss_set_tuning); the
        results never depend on them."""
        t = abi.Tuning(chunk_tiles, span_tiles, parse_blocks, one_launch, scatter_xcd, scan_kernel)
        abi.check(self._lib.yrss_set_tuning(self._ctx, ctypes.byref(t)), "yrss_set_tuning")

    def grid_for(self, n: int) -> int:
        return int(self._lib.yrss_grid_for(self._ctx, n))


class FanOut:
    """One dispatcher thread's host bursts spread round-robin over several
    contexts / GPUs (``yrss_fanout_*``), returned in submission order by
    :meth:`next` so per-queue FIFO holds over the whole stream."""

    def __init__(self, devices, nb_procs: int = 3, nb_queues: int | None = None,
                 soft_dispatch: int = 1, dispatch_only_core: int = 1, nslots: int = 16,
                 nblocks: int = 4):
        self._lib = abi.load()
        cfg = abi.default_config()
        cfg.nb_procs = nb_procs
        cfg.nb_queues = nb_procs if nb_queues is None else nb_queues
        cfg.soft_dispatch = soft_dispatch
        cfg.dispatch_only_core = dispatch_only_core
        self.nb_queues = int(cfg.nb_queues)
        devs = (ctypes.c_int * len(devices))(*devices)
        f = ctypes.c_void_p()
        abi.check(self._lib.yrss_fanout_init(ctypes.byref(cfg), devs, len(devices), nslots,
                                             nblocks, ctypes.byref(f)), "yrss_fanout_init")
        self._f = f
        self._res = {}

    def close(self) -> None:
        if getattr(self, "_f", None) and self._f.value:
            rc = self._lib.yrss_fanout_fini(self._f)
            self._f = ctypes.c_void_p()
            abi.check(rc, "yrss_fanout_fini")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def register_host_memory(self, base: int, nbytes: int) -> None:
        abi.check(self._lib.yrss_fanout_register_host_memory(self._f, base, nbytes),
                  "yrss_fanout_register_host_memory")

    def unregister_host_memory(self, base: int) -> None:
        abi.check(self._lib.yrss_fanout_unregister_host_memory(self._f, base),
                  "yrss_fanout_unregister_host_memory")

    def set_extended(self, vlan: bool = False, ipv6: bool = False, udp: bool = False) -> None:
        """:meth:`SoftRss.set_extended` on every context
        (``yrss_fanout_set_extended``); EBUSY while a ticket is outstanding."""
        flags = (abi.EXT_VLAN if vlan else 0) | (abi.EXT_IPV6 if ipv6 else 0) | \
            (abi.EXT_UDP if udp else 0)
        abi.check(self._lib.yrss_fanout_set_extended(self._f, flags), "yrss_fanout_set_extended")
        self.ext_flags = flags

    def _queue(self, name, n, call) -> int:
        """As SoftRss._worker_queue: ``call(outs, ticket)`` makes the C call ``name``."""
        out = _host_out(n, self.nb_queues + 2)
        t = ctypes.c_uint64()
        abi.check(call([_ptr(a) for a in out[:4]], ctypes.byref(t)), name)
        self._res[t.value] = _host_result(n, out)
        return t.value

    def submit(self, mbuf_ptrs: np.ndarray) -> int:
        mb = np.ascontiguousarray(mbuf_ptrs, dtype=np.uint64)
        n = int(mb.size)
        return self._queue("yrss_fanout_submit", n, lambda outs, t: self._lib.yrss_fanout_submit(
            self._f, _ptr(mb), n, *outs, 0, t))

    def submit_frames(self, data_ptrs: np.ndarray, lens: np.ndarray) -> int:
        dp = np.ascontiguousarray(data_ptrs, dtype=np.uint64)
        ln = np.ascontiguousarray(lens, dtype=np.uint16)
        n = int(dp.size)
        return self._queue(
            "yrss_fanout_submit_frames", n,
            lambda outs, t: self._lib.yrss_fanout_submit_frames(self._f, _ptr(dp), _ptr(ln), n,
                                                                *outs, t))

    def next(self, wait: bool = True):
        """(ticket, DispatchResult) of the oldest outstanding burst once done;
        None while it runs (wait=False) or when nothing is outstanding."""
        t = ctypes.c_uint64()
        rc = self._lib.yrss_fanout_next(self._f, 1 if wait else 0, ctypes.byref(t))
        if rc in (-11, -2):   # -EAGAIN, -ENOENT
            return None
        res = self._res.pop(t.value, None) if rc in (0, -14) else None
        abi.check(rc, "yrss_fanout_next")
        return t.value, res
