"""Shared by the routed-segment tests (test_route_segments.py on the CPU,
test_gpu_route_segments.py on the GPU): the input stream, the oracle's q and
filter class for it (computed once per shape), the callback model of
yrss_route_burst's tests, and a ctypes driver of yrss_route_seg."""
import ctypes
import functools

import numpy as np

from oracle import oracle
from yastack_amd import abi

STRIDE = 80
TCP_PORTS, UDP_PORTS = "0-30000", "20000-65535"
# (enable, method): KNI off, accept, reject
KNI_MODES = {"off": (False, "reject"), "accept": (True, "accept"), "reject": (True, "reject")}
CONFIGS = [(6, 4, 1, 0), (3, 3, 1, 1), (13, 13, 1, 0)]
OBJ_BASE = 0x100000


def clone_ok(i, j):
    """Some clones fail (the pool is exhausted)."""
    return (i * 7 + j) % 5 != 0


@functools.lru_cache(maxsize=None)
def stream(n, stride=STRIDE):
    """oracle.synth(SYN_FUZZ, n, 5): (win uint8[n * stride], lens uint16[n]), read-only."""
    win, lens = oracle.synth(abi.SYN_FUZZ, n, 5, stride=stride)
    win.setflags(write=False)
    lens.setflags(write=False)
    return win, lens


@functools.lru_cache(maxsize=None)
def oracle_qh(cfg, n, stride=STRIDE):
    win, lens = stream(n, stride)
    q, h = oracle.dispatch_windows(win, stride, lens, oracle.cfg(*cfg))
    q.setflags(write=False)
    h.setflags(write=False)
    return q, h


@functools.lru_cache(maxsize=None)
def oracle_filter(enable, n, stride=STRIDE):
    win, lens = stream(n, stride)
    f = oracle.filter_windows(win, stride, lens, enable, oracle.kni_bitmap(TCP_PORTS),
                              oracle.kni_bitmap(UDP_PORTS))
    f.setflags(write=False)
    return f


def class_counts(q, f, nq, queue_id, enable, accept):
    """Sizes of the classes a routed test may claim to cover, from the oracle."""
    q = np.asarray(q).astype(np.int64)
    f = np.asarray(f).astype(np.int64)
    local = (q == queue_id) & (queue_id < nq)
    arp = local & (f == abi.FILTER_ARP)
    kni = local & bool(enable) & (f == (abi.FILTER_KNI if accept else abi.FILTER_UNKNOWN))
    return {"arp": int(arp.sum()), "kni": int(kni.sum()),
            "freed": int(((q < 0) | (q >= nq)).sum()),
            "unresolved": int((local & ((f == abi.FILTER_TRUNC) | (f == abi.FILTER_LOOP))).sum())}


class Rings:
    """Callback side of the route calls: bounded FIFO rings + clone pool."""

    def __init__(self, addr_to_idx, capacity, clone_ok):
        self.addr_to_idx = addr_to_idx
        self.free = list(capacity)
        self.rings = {j: [] for j in range(len(capacity))}
        self.clone_ok = clone_ok
        self.clones = {}
        self.next_clone = 0x7F0000000000
        self.released = []
        self.calls = 0

    def obj(self, a):
        return self.clones[a] if a in self.clones else ("pkt", self.addr_to_idx[a])

    def enqueue(self, queue, objs):
        self.calls += 1
        k = min(self.free[queue], len(objs))
        self.rings[queue] += [self.obj(a) for a in objs[:k]]
        self.free[queue] -= k
        return k

    def clone(self, m, queue):
        self.calls += 1
        i = self.addr_to_idx[m]
        if not self.clone_ok(i, queue):
            return 0
        self.next_clone += 64
        self.clones[self.next_clone] = ("clone", i, queue)
        return self.next_clone

    def release(self, m):
        self.calls += 1
        self.released.append(self.obj(m))


def fake_objs(n):
    """n distinct mbuf addresses and the map back to packet indices."""
    ptrs = OBJ_BASE + 64 * np.arange(n, dtype=np.uint64)
    return ptrs, {int(a): i for i, a in enumerate(ptrs)}


def route_seg_c(seg_idx, seg_off, n, nq, queue_id, kni_clone, filt, ptrs, cb):
    """yrss_route_seg through ctypes callbacks into cb (a Rings).
    Returns (rc, local objects, kni objects, RouteResult)."""
    def _enq(user, queue, objs, cnt):
        return int(cb.enqueue(int(queue), [int(objs[i] or 0) for i in range(cnt)]))

    def _clone(user, m, queue):
        return int(cb.clone(int(m or 0), int(queue)) or 0)

    def _rel(user, m):
        cb.release(int(m or 0))

    ops = abi.RouteOps(abi.ENQUEUE_FN(_enq), abi.CLONE_FN(_clone), abi.RELEASE_FN(_rel), None)
    seg_idx = np.ascontiguousarray(seg_idx, np.uint8)
    seg_off = np.ascontiguousarray(seg_off, np.uint16)
    ptrs = np.ascontiguousarray(ptrs, np.uint64)
    local = np.zeros(max(n, 1), np.uint64)
    kni = np.zeros(max(n, 1), np.uint64)
    res = abi.RouteResult()
    fp = None if filt is None else np.ascontiguousarray(filt, np.int8)
    rc = abi.load().yrss_route_seg(seg_idx.ctypes.data, seg_off.ctypes.data, n, nq, queue_id,
                                   1 if kni_clone else 0, None if fp is None else fp.ctypes.data,
                                   ptrs.ctypes.data, ctypes.byref(ops), local.ctypes.data,
                                   kni.ctypes.data, ctypes.byref(res))
    return (rc, [cb.obj(int(a)) for a in local[:res.n_local]],
            [cb.obj(int(a)) for a in kni[:res.n_kni]], res)


def assert_matches_model(cb, local, kni, res, q, f, nq, queue_id, enable, accept, cap,
                         with_filter=True):
    """The callbacks' record, out_local, out_kni and the counters against
    oracle.process_packets_route (one packet at a time over the whole batch)."""
    rings_ref, local_ref, kni_ref, freed_ref = oracle.process_packets_route(
        q, f, nq, queue_id, enable, accept, True, [cap] * nq, clone_ok)
    assert cb.rings == rings_ref
    assert local == local_ref
    assert kni == kni_ref
    assert sorted(cb.released) == sorted(freed_ref)
    assert res.n_freed == len(freed_ref)
    assert res.n_local == len(local_ref) and res.n_kni == len(kni_ref)
    assert res.n_arp == sum(1 for o in local_ref if f[o[1]] == abi.FILTER_ARP)
    unresolved = sum(1 for o in local_ref if f[o[1]] in (abi.FILTER_TRUNC, abi.FILTER_LOOP))
    assert res.n_unresolved == (unresolved if with_filter else 0)
    assert [res.n_ring[j] for j in range(nq)] == [len(rings_ref[j]) for j in range(nq)]
    return rings_ref, local_ref, kni_ref, freed_ref
