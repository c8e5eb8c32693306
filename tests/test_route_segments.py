"""Routed segmented lists on the host (no GPU): segments.route_buckets /
route_from (the numpy twin of the parse kernel's route classes) and the C
consumer yrss_route_seg against oracle.process_packets_route, the refusal of
corrupted arrays before any callback, from_q unchanged, and the header and the
Python binding in agreement.

Input: oracle.synth(SYN_FUZZ, n, 5, stride=80), KNI ports "0-30000" /
"20000-65535".  On config (6,4,1,0) it holds ARP on queue 0 (191 of 3000),
packets outside the queues (293), and on queue 2 the KNI classes (274 / 1651)
and TRUNC/LOOP packets (6); each test asserts, from the oracle, that what it
claims to cover is there."""
import ctypes
import errno
import re
import subprocess

import numpy as np
import pytest

import route_helpers as rh
from yastack_amd import abi, segments

SIZES = [1, 255, 256, 257, 3000]


def _inputs(cfg, kni, n):
    enable, method = rh.KNI_MODES[kni]
    q, _ = rh.oracle_qh(cfg, n)
    return q, rh.oracle_filter(enable, n), enable, method == "accept"


@pytest.mark.parametrize("cap", [10**6, 300])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kni", list(rh.KNI_MODES))
@pytest.mark.parametrize("qsel", [0, 2, "nq"])
@pytest.mark.parametrize("cfg", rh.CONFIGS)
def test_route_seg_vs_process_packets(oracle_mod, cfg, qsel, kni, n, cap):
    nq = cfg[1]
    queue_id = nq if qsel == "nq" else qsel
    q, f, enable, accept = _inputs(cfg, kni, n)
    # what this case covers, from the oracle
    cnt = rh.class_counts(q, f, nq, queue_id, enable, accept)
    if n >= 255:
        assert (cnt["arp"] > 0) == (queue_id == 0)
        assert (cnt["freed"] > 0) == (nq < cfg[0])
        if queue_id == 2:
            assert (cnt["kni"] > 0) == enable
        if queue_id == nq:
            assert cnt["kni"] == 0 and cnt["arp"] == 0
    ptrs, addr_to_idx = rh.fake_objs(n)
    cb = rh.Rings(addr_to_idx, [cap] * nq, rh.clone_ok)
    si, so = segments.route_from(q, f, nq, queue_id, enable, accept)
    assert si.dtype == np.uint8 and si.shape == (n,)
    assert so.dtype == np.uint16 and so.shape == (segments.nseg_for(n), nq + 4)
    rc, local, kni_list, res = rh.route_seg_c(si, so, n, nq, queue_id, enable, f, ptrs, cb)
    assert rc == 0
    _, _, _, freed_ref = rh.assert_matches_model(cb, local, kni_list, res, q, f, nq, queue_id,
                                                 enable, accept, cap)
    if n == 3000 and queue_id == 0:
        arp = np.nonzero((q == 0) & (f == abi.FILTER_ARP))[0]
        assert any(not rh.clone_ok(int(i), j) for i in arp for j in range(1, nq)), "failed clones"
    if n == 3000 and cap == 300 and nq <= 4:
        assert len(freed_ref) > cnt["freed"], "ring-full frees"
    if n == 3000 and queue_id == 2 and enable:
        assert cnt["unresolved"] > 0 and res.n_unresolved == cnt["unresolved"]


def test_route_seg_without_filter_counts_nothing_unresolved(oracle_mod):
    cfg, n, queue_id = (6, 4, 1, 0), 3000, 2
    q, f, enable, accept = _inputs(cfg, "accept", n)
    assert rh.class_counts(q, f, 4, queue_id, enable, accept)["unresolved"] > 0
    ptrs, addr_to_idx = rh.fake_objs(n)
    cb = rh.Rings(addr_to_idx, [300] * 4, rh.clone_ok)
    si, so = segments.route_from(q, f, 4, queue_id, enable, accept)
    rc, local, kni_list, res = rh.route_seg_c(si, so, n, 4, queue_id, enable, None, ptrs, cb)
    assert rc == 0
    rh.assert_matches_model(cb, local, kni_list, res, q, f, 4, queue_id, enable, accept, 300,
                            with_filter=False)


@pytest.mark.parametrize("kni", list(rh.KNI_MODES))
@pytest.mark.parametrize("qsel", [0, 2, "nq"])
@pytest.mark.parametrize("cfg", rh.CONFIGS)
def test_every_segment_is_the_stable_sort_of_its_slice(oracle_mod, cfg, qsel, kni):
    nq, n = cfg[1], 3000
    queue_id = nq if qsel == "nq" else qsel
    q, f, enable, accept = _inputs(cfg, kni, n)
    bkt = segments.route_buckets(q, f, nq, queue_id, enable, accept)
    assert bkt.shape == (n,) and bkt.min() >= 0 and bkt.max() < nq + 3
    # the class table, restated per packet
    for i in range(n):
        qi, fi = int(q[i]), int(f[i])
        if qi < 0 or qi >= nq:
            want = nq
        elif qi != queue_id:
            want = qi
        elif fi == abi.FILTER_ARP:
            want = nq + 2
        elif enable and ((fi == abi.FILTER_KNI and accept) or
                         (fi == abi.FILTER_UNKNOWN and not accept)):
            want = nq + 1
        else:
            want = queue_id
        assert bkt[i] == want, i
    si, so = segments.route_from(q, f, nq, queue_id, enable, accept)
    for s in range(segments.nseg_for(n)):
        b = bkt[s * 256:(s + 1) * 256]
        assert so[s, 0] == 0 and so[s, nq + 3] == b.size
        assert np.array_equal(so[s, 1:], np.cumsum(np.bincount(b, minlength=nq + 3)))
        assert np.array_equal(si[s * 256:s * 256 + b.size], np.argsort(b, kind="stable"))


CORRUPTIONS = ["non_monotone", "first_offset", "last_offset", "index", "duplicate",
               "nb_queues_14", "kni_without_local_queue"]


@pytest.mark.parametrize("case", CORRUPTIONS)
def test_corrupted_arrays_are_refused_before_any_callback(oracle_mod, case):
    """The corruption sits in the last segment: a consumer that validated as it
    went would already have called back for the segments before it."""
    cfg, n, queue_id = (6, 4, 1, 0), 700, 0
    nq = 4
    q, f, enable, accept = _inputs(cfg, "accept", n)
    cnt = rh.class_counts(q[:512], f[:512], nq, queue_id, enable, accept)
    assert cnt["arp"] > 0 and cnt["freed"] > 0     # segments 0 and 1 alone need callbacks
    si, so = segments.route_from(q, f, nq, queue_id, enable, accept)
    last = segments.nseg_for(n) - 1
    len_s = n - 256 * last
    nq_arg, qid_arg = nq, queue_id
    if case == "non_monotone":
        so[last, 2] = so[last, 1] + 300
        so[last, 3] = so[last, 1]
    elif case == "first_offset":
        so[last, 0] = 1
    elif case == "last_offset":
        so[last, nq + 3] = len_s + 1
    elif case == "index":
        si[256 * last] = len_s
    elif case == "duplicate":
        si[256 * last + 1] = si[256 * last]
    elif case == "nb_queues_14":
        nq_arg = 14
        so = np.zeros((segments.nseg_for(n), 18), np.uint16)   # sized for the claimed layout
    else:
        qid_arg = nq      # no local queue, but the ARP / KNI buckets are not empty
        assert so[last, nq + 3] > so[last, nq + 1]
    ptrs, addr_to_idx = rh.fake_objs(n)
    cb = rh.Rings(addr_to_idx, [10**6] * 16, rh.clone_ok)
    rc, local, kni_list, res = rh.route_seg_c(si, so, n, nq_arg, qid_arg, enable, f, ptrs, cb)
    assert rc == -errno.EINVAL
    assert cb.calls == 0 and not cb.released and not any(cb.rings.values())
    assert res.n_local == 0 and res.n_kni == 0 and res.n_freed == 0


def test_route_seg_refuses_bad_arguments(oracle_mod):
    n, nq = 300, 4
    q, f, enable, accept = _inputs((6, 4, 1, 0), "accept", n)
    si, so = segments.route_from(q, f, nq, 0, enable, accept)
    ptrs, _ = rh.fake_objs(n)
    ops = abi.RouteOps(abi.ENQUEUE_FN(lambda *a: 0), abi.CLONE_FN(lambda *a: 0),
                       abi.RELEASE_FN(lambda *a: None), None)
    out = np.zeros(n, np.uint64)
    res = abi.RouteResult()
    args = [si.ctypes.data, so.ctypes.data, n, nq, 0, 1, None, ptrs.ctypes.data,
            ctypes.byref(ops), out.ctypes.data, out.ctypes.data, ctypes.byref(res)]
    lib = abi.load()
    for k, bad in ((0, None), (1, None), (3, 0), (7, None), (8, None), (9, None), (10, None),
                   (11, None)):
        a = list(args)
        a[k] = bad
        assert lib.yrss_route_seg(*a) == -errno.EINVAL, k
    # an empty batch needs no arrays and calls nothing
    a = list(args)
    a[0] = a[1] = a[7] = a[9] = a[10] = None
    a[2] = 0
    assert lib.yrss_route_seg(*a) == 0 and res.n_local == 0


@pytest.mark.parametrize("cfg", [(3, 3, 1, 1), (15, 15, 1, 0), (5, 2, 0, 1)])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 4097])
def test_from_q_is_unchanged(oracle_mod, cfg, n):
    """from_q, now through from_buckets, against the oracle's process_burst
    segment by segment (what it returned before)."""
    nq = cfg[1]
    win, lens = oracle_mod.synth(abi.SYN_FUZZ, n, first=11)
    q, _ = oracle_mod.dispatch_windows(win, 64, lens, oracle_mod.cfg(*cfg))
    si, so = segments.from_q(q, nq)
    assert si.dtype == np.uint8 and si.shape == (n,)
    assert so.dtype == np.uint16 and so.shape == (segments.nseg_for(n), nq + 2)
    for s in range(segments.nseg_for(n)):
        sl = q[s * 256:(s + 1) * 256]
        li, ls = oracle_mod.process_burst(sl, nq)
        assert np.array_equal(so[s].astype(np.uint32), ls)
        assert np.array_equal(si[s * 256:s * 256 + sl.size].astype(np.uint32), li)
    b = segments.buckets_of(q, nq)
    for a, c in zip(segments.from_buckets(b, nq + 1), (si, so)):
        assert np.array_equal(a, c)
    with pytest.raises(ValueError):
        segments.from_buckets(np.array([0, nq + 1]), nq + 1)


def test_header_constants_layout_and_exports():
    text = abi.HEADER_PATH.read_text()
    assert int(re.search(r"#define YRSS_ROUTE_SEG_MAX_QUEUES (\d+)", text).group(1)) == \
        abi.ROUTE_SEG_MAX_QUEUES == abi.SEG_MAX_BUCKETS - 3 == 13
    names = abi.header_functions()
    assert "yrss_route_dev_seg" in names and "yrss_route_seg" in names
    for path in (abi.LIB_PATH, abi.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True,
                             text=True, check=True).stdout
        exported = set(re.findall(r"\bT (yrss_\w+)", out))
        assert {"yrss_route_dev_seg", "yrss_route_seg"} <= exported, path
    # struct yrss_dev_route_batch: yrss_dev_seg_batch, then queue_id (padded to 8)
    assert ctypes.sizeof(abi.DevRouteBatch) == ctypes.sizeof(abi.DevSegBatch) + 8
    assert abi.DevRouteBatch.queue_id.offset == ctypes.sizeof(abi.DevSegBatch)
    body = re.search(r"struct yrss_dev_route_batch \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+);", body) == [f for f, *_ in abi.DevRouteBatch._fields_]
    seg = re.search(r"struct yrss_dev_seg_batch \{(.*?)\};", text, re.S).group(1)
    seg = re.sub(r"/\*.*?\*/", "", seg, flags=re.S)
    strip = (lambda t: re.sub(r"\s+", " ", t).strip())
    assert strip(body).startswith(strip(seg)), "the seg batch's fields, then queue_id"
    # yrss_route_seg's prototype, argument by argument
    proto = re.search(r"int yrss_route_seg\((.*?)\);", text, re.S).group(1)
    assert len(proto.split(",")) == len(abi._PROTOS["yrss_route_seg"][1]) == 12


def test_route_dev_seg_refuses_short_buffers():
    """SoftRss.route_dev_seg sizes seg_off for nb_queues + 4 offsets a segment."""
    from yastack_amd import dispatch

    class T:
        def __init__(self, nbytes):
            self.nb = nbytes

        def numel(self):
            return self.nb

        def element_size(self):
            return 1

    n, nq = 300, 3
    good = dict(q=T(2 * n), hash=T(4 * n), filter=T(n), seg_idx=T(n), seg_off=T(2 * 2 * (nq + 4)))
    dispatch._check_seg_sizes(n, 80, T(80 * n), T(2 * n), dispatch.SegResult(**good), nq, nq + 3)
    bad = dict(good, seg_off=T(2 * 2 * (nq + 4) - 1))
    with pytest.raises(ValueError, match="seg_off"):
        dispatch._check_seg_sizes(n, 80, T(80 * n), T(2 * n), dispatch.SegResult(**bad), nq,
                                  nq + 3)
