"""Shared by the routed-global-list tests (test_route_lists.py on the CPU,
test_gpu_route_bursts.py on the GPU): a ctypes driver of yrss_route_lists over
route_helpers.Rings, and the expected lists of a burst from the oracle."""
import ctypes

import numpy as np

import route_helpers as rh
from yastack_amd import abi, segments


def route_lists_c(ridx, rstart, n, nq, queue_id, kni_clone, filt, ptrs, cb):
    """yrss_route_lists through ctypes callbacks into cb (a Rings).
    Returns (rc, local objects, kni objects, RouteResult)."""
    def _enq(user, queue, objs, cnt):
        return int(cb.enqueue(int(queue), [int(objs[i] or 0) for i in range(cnt)]))

    def _clone(user, m, queue):
        return int(cb.clone(int(m or 0), int(queue)) or 0)

    def _rel(user, m):
        cb.release(int(m or 0))

    ops = abi.RouteOps(abi.ENQUEUE_FN(_enq), abi.CLONE_FN(_clone), abi.RELEASE_FN(_rel), None)
    ridx = np.ascontiguousarray(ridx, np.uint32)
    rstart = np.ascontiguousarray(rstart, np.uint32)
    ptrs = np.ascontiguousarray(ptrs, np.uint64)
    local = np.zeros(max(n, 1), np.uint64)
    kni = np.zeros(max(n, 1), np.uint64)
    res = abi.RouteResult()
    fp = None if filt is None else np.ascontiguousarray(filt, np.int8)
    rc = abi.load().yrss_route_lists(ridx.ctypes.data, rstart.ctypes.data, n, nq, queue_id,
                                     1 if kni_clone else 0, None if fp is None else fp.ctypes.data,
                                     ptrs.ctypes.data, ctypes.byref(ops), local.ctypes.data,
                                     kni.ctypes.data, ctypes.byref(res))
    return (rc, [cb.obj(int(a)) for a in local[:res.n_local]],
            [cb.obj(int(a)) for a in kni[:res.n_kni]], res)


def inputs(cfg, kni, n):
    """(q, filter class, enable, accept) of route_helpers.stream(n) from the oracle."""
    enable, method = rh.KNI_MODES[kni]
    q, _ = rh.oracle_qh(cfg, n)
    return q, rh.oracle_filter(enable, n), enable, method == "accept"


def expected(q, f, nq, queue_id, enable, accept):
    return segments.route_lists_from(q, f, nq, queue_id, enable, accept)
