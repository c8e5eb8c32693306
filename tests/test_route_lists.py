"""Routed global lists on the host (no GPU): segments.route_lists_from (the
numpy twin of the route burst kernels' lists) and the C consumer
yrss_route_lists against oracle.process_packets_route, the refusal of
corrupted arrays before any callback, and the header and the Python binding in
agreement.

Input: route_helpers.stream (oracle.synth SYN_FUZZ from packet 5, stride 80),
KNI ports "0-30000" / "20000-65535"; each test asserts, from the oracle, that
what it claims to cover is there."""
import ctypes
import errno
import re
import subprocess

import numpy as np
import pytest

import route_helpers as rh
import route_lists_helpers as rl
from yastack_amd import abi, segments

SIZES = [0, 1, 2, 65, 1024]
QSEL = ["0", "nq-1", "nq"]


def _queue_id(qsel, nq):
    return {"0": 0, "nq-1": nq - 1, "nq": nq}[qsel]


def _inputs(cfg, kni, n):
    if n == 0:
        enable, method = rh.KNI_MODES[kni]
        return np.zeros(0, np.int16), np.zeros(0, np.int8), enable, method == "accept"
    return rl.inputs(cfg, kni, n)


@pytest.mark.parametrize("cap", [10**6, 40])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kni", list(rh.KNI_MODES))
@pytest.mark.parametrize("qsel", QSEL)
@pytest.mark.parametrize("cfg", rh.CONFIGS)
def test_route_lists_vs_process_packets(oracle_mod, cfg, qsel, kni, n, cap):
    nq = cfg[1]
    queue_id = _queue_id(qsel, nq)
    q, f, enable, accept = _inputs(cfg, kni, n)
    cnt = rh.class_counts(q, f, nq, queue_id, enable, accept)
    if n == 1024:
        assert (cnt["arp"] > 0) == (queue_id == 0)
        assert (cnt["freed"] > 0) == (nq < cfg[0])
        if queue_id == 2:
            assert (cnt["kni"] > 0) == enable
        if queue_id == nq:
            assert cnt["kni"] == 0 and cnt["arp"] == 0
    ptrs, addr_to_idx = rh.fake_objs(n)
    cb = rh.Rings(addr_to_idx, [cap] * nq, rh.clone_ok)
    ridx, rstart = segments.route_lists_from(q, f, nq, queue_id, enable, accept)
    assert ridx.dtype == np.uint32 and ridx.shape == (n,)
    assert rstart.dtype == np.uint32 and rstart.shape == (nq + 4,)
    rc, local, kni_list, res = rl.route_lists_c(ridx, rstart, n, nq, queue_id, enable, f, ptrs, cb)
    assert rc == 0
    _, _, _, freed_ref = rh.assert_matches_model(cb, local, kni_list, res, q, f, nq, queue_id,
                                                 enable, accept, cap)
    if n == 1024 and queue_id == 0:
        arp = np.nonzero((q == 0) & (f == abi.FILTER_ARP))[0]
        assert any(not rh.clone_ok(int(i), j) for i in arp for j in range(1, nq)), "failed clones"
    if n == 1024 and cap == 40 and nq <= 4:
        assert len(freed_ref) > cnt["freed"], "ring-full frees"


def test_route_lists_without_filter_counts_nothing_unresolved(oracle_mod):
    cfg, n, queue_id = (6, 4, 1, 0), 3000, 2
    q, f, enable, accept = _inputs(cfg, "accept", n)
    assert rh.class_counts(q, f, 4, queue_id, enable, accept)["unresolved"] > 0
    ptrs, addr_to_idx = rh.fake_objs(n)
    ridx, rstart = segments.route_lists_from(q, f, 4, queue_id, enable, accept)
    for filt in (f, None):
        cb = rh.Rings(addr_to_idx, [300] * 4, rh.clone_ok)
        rc, local, kni_list, res = rl.route_lists_c(ridx, rstart, n, 4, queue_id, enable, filt,
                                                    ptrs, cb)
        assert rc == 0
        rh.assert_matches_model(cb, local, kni_list, res, q, f, 4, queue_id, enable, accept, 300,
                                with_filter=filt is not None)


@pytest.mark.parametrize("kni", list(rh.KNI_MODES))
@pytest.mark.parametrize("qsel", QSEL)
@pytest.mark.parametrize("cfg", rh.CONFIGS)
def test_twin_is_the_stable_sort_by_route_bucket(oracle_mod, cfg, qsel, kni):
    nq, n = cfg[1], 1024
    queue_id = _queue_id(qsel, nq)
    q, f, enable, accept = _inputs(cfg, kni, n)
    bkt = segments.route_buckets(q, f, nq, queue_id, enable, accept)
    ridx, rstart = segments.route_lists_from(q, f, nq, queue_id, enable, accept)
    assert rstart[0] == 0 and rstart[nq + 3] == n
    assert np.array_equal(rstart[1:], np.cumsum(np.bincount(bkt, minlength=nq + 3)))
    for b in range(nq + 3):
        assert np.array_equal(ridx[rstart[b]:rstart[b + 1]], np.nonzero(bkt == b)[0])
    # one segment's worth: the segmented twin holds the same lists
    si, so = segments.route_from(q[:256], f[:256], nq, queue_id, enable, accept)
    r2, s2 = segments.route_lists_from(q[:256], f[:256], nq, queue_id, enable, accept)
    assert np.array_equal(si.astype(np.uint32), r2) and np.array_equal(so[0].astype(np.uint32), s2)


CORRUPTIONS = ["duplicate", "missing", "non_monotone", "first_offset", "last_offset", "index",
               "index_2_31", "nb_queues_62", "kni_without_local_queue", "arp_without_local_queue"]


@pytest.mark.parametrize("case", CORRUPTIONS)
def test_corrupted_arrays_are_refused_before_any_callback(oracle_mod, case):
    """The corruption sits at the end of the arrays: a consumer that validated
    as it went would already have called back for what comes before it."""
    cfg, n, queue_id, nq = (6, 4, 1, 0), 700, 0, 4
    q, f, enable, accept = _inputs(cfg, "accept", n)
    cnt = rh.class_counts(q, f, nq, queue_id, enable, accept)
    assert cnt["arp"] > 0 and cnt["freed"] > 0 and cnt["kni"] > 0
    ridx, rstart = segments.route_lists_from(q, f, nq, queue_id, enable, accept)
    assert rstart[nq + 3] > rstart[nq + 2] > rstart[nq + 1]
    nq_arg, qid_arg = nq, queue_id
    if case == "duplicate":
        ridx[n - 1] = ridx[n - 2]
    elif case == "missing":
        ridx[n - 1] = ridx[0]           # the last ARP packet is gone, another one twice
    elif case == "non_monotone":
        rstart[nq + 1], rstart[nq + 2] = rstart[nq + 2], rstart[nq + 1]
    elif case == "first_offset":
        rstart[0] = 1
    elif case == "last_offset":
        rstart[nq + 3] = n - 1
    elif case == "index":
        ridx[n - 1] = n
    elif case == "index_2_31":
        ridx[n - 1] = 0x80000000 | int(ridx[n - 1])
    elif case == "nb_queues_62":
        nq_arg = 62
        rstart = np.zeros(66, np.uint32)    # sized for the claimed layout
        rstart[1:] = n
    elif case == "kni_without_local_queue":
        qid_arg = nq                        # no local queue, but the KNI class is not empty
        rstart[nq + 2] = n                  # (the ARP class emptied into it: only KNI offends)
    else:
        qid_arg = nq
        rstart[nq + 1] = rstart[nq + 2]     # KNI class emptied into the freed one
    ptrs, addr_to_idx = rh.fake_objs(n)
    cb = rh.Rings(addr_to_idx, [10**6] * 64, rh.clone_ok)
    rc, local, kni_list, res = rl.route_lists_c(ridx, rstart, n, nq_arg, qid_arg, enable, f, ptrs,
                                                cb)
    assert rc == -errno.EINVAL
    assert cb.calls == 0 and not cb.released and not any(cb.rings.values())
    assert res.n_local == 0 and res.n_kni == 0 and res.n_freed == 0


def test_route_lists_refuses_bad_arguments(oracle_mod):
    n, nq = 300, 4
    q, f, enable, accept = _inputs((6, 4, 1, 0), "accept", n)
    ridx, rstart = segments.route_lists_from(q, f, nq, 0, enable, accept)
    ptrs, _ = rh.fake_objs(n)
    ops = abi.RouteOps(abi.ENQUEUE_FN(lambda *a: 0), abi.CLONE_FN(lambda *a: 0),
                       abi.RELEASE_FN(lambda *a: None), None)
    out = np.zeros(n, np.uint64)
    res = abi.RouteResult()
    args = [ridx.ctypes.data, rstart.ctypes.data, n, nq, 0, 1, None, ptrs.ctypes.data,
            ctypes.byref(ops), out.ctypes.data, out.ctypes.data, ctypes.byref(res)]
    lib = abi.load()
    for k, bad in ((0, None), (1, None), (3, 0), (7, None), (8, None), (9, None), (10, None),
                   (11, None)):
        a = list(args)
        a[k] = bad
        assert lib.yrss_route_lists(*a) == -errno.EINVAL, k
    # an empty burst needs only its (zero) offsets and calls nothing
    zero = np.zeros(nq + 4, np.uint32)
    a = list(args)
    a[0] = a[7] = a[9] = a[10] = None
    a[1] = zero.ctypes.data
    a[2] = 0
    assert lib.yrss_route_lists(*a) == 0 and res.n_local == 0


def test_header_constants_and_exports():
    text = abi.HEADER_PATH.read_text()
    assert int(re.search(r"#define YRSS_ROUTE_LISTS_MAX_QUEUES (\d+)", text).group(1)) == \
        abi.ROUTE_LISTS_MAX_QUEUES == 64 - 3 == 61
    new = {"yrss_worker_start_route", "yrss_route_lists_burst", "yrss_route_lists_frames",
           "yrss_route_lists"}
    assert new <= set(abi.header_functions())
    for path in (abi.LIB_PATH, abi.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True,
                             text=True, check=True).stdout
        assert new <= set(re.findall(r"\bT (yrss_\w+)", out)), path
    # the prototypes, argument by argument
    for name in sorted(new):
        proto = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
        assert len(proto.split(",")) == len(abi._PROTOS[name][1]), name
    # the worker's slot header keeps its one line: no filter address was added
    src = (abi.REPO_DIR / "yastack_amd" / "csrc" / "yrss.hip").read_text()
    assert "static_assert(sizeof(WorkerSlot) == 64" in src
    assert 'case YRSS_K_WORKER: return "yrss_burst_worker";' in src
