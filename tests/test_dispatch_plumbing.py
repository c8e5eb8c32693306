"""What every host entry of dispatch.py hands to C and returns, pinned against a
fake library (no libyrss call, no GPU): the output arrays' dtypes, their
lengths max(n, 1) sliced to n, the number of offsets (nb_queues + 2, or
nb_queues + 4 for the routed forms and the route worker) and None for the
outputs not asked for."""
import ctypes
import itertools

import numpy as np
import pytest

from yastack_amd import abi
from yastack_amd.dispatch import DispatchResult, FanOut, SoftRss

NQ = 5
SIZES = (0, 1, 33)


class FakeLib:
    """Records every call; a trailing ticket argument gets the next ticket."""

    def __init__(self):
        self.calls = []
        self.ticket = 0
        self.seen = {}     # what the frames-to-pointers arrays held during the call

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            if name in ("yrss_dispatch_frames", "yrss_route_lists_frames"):
                n = args[3]
                ptrs = (ctypes.c_uint64 * n).from_address(args[1]) if n else []
                lens = (ctypes.c_uint16 * n).from_address(args[2]) if n else []
                self.seen[name] = [ctypes.string_at(p, l) for p, l in zip(ptrs, lens)]
            if name.startswith(("yrss_worker_submit", "yrss_fanout_submit")):
                self.ticket += 1
                args[-1]._obj.value = self.ticket
            if name == "yrss_fanout_next":
                args[-1]._obj.value = self.ticket
            return 0
        return call


def _engine():
    eng = SoftRss.__new__(SoftRss)
    eng._lib = FakeLib()
    eng._ctx = ctypes.c_void_p(0x1000)
    eng.nb_queues = NQ
    eng._hung = True      # close() then makes no yrss_fault_info call
    return eng


def _fanout():
    fo = FanOut.__new__(FanOut)
    fo._lib = FakeLib()
    fo._f = ctypes.c_void_p(0x2000)
    fo.nb_queues = NQ
    fo._res = {}
    return fo


def _mbufs(n):
    return np.arange(1, n + 1, dtype=np.uint64) * 4096


def _frames(n):
    # an empty frame too: it is handed over as a pointer to one byte, length 0
    return [bytes([i & 255]) * ((i * 7) % 90) for i in range(n)]


def _check_array(arr, ptr, n, dtype):
    """arr is the first n of an array of max(n, 1) whose address went to C."""
    assert isinstance(arr, np.ndarray) and arr.dtype == np.dtype(dtype)
    assert arr.shape == (n,)
    assert arr.base is not None and arr.base.shape == (max(n, 1),)
    assert arr.base.dtype == np.dtype(dtype) and arr.base.ctypes.data == ptr


def _check_offsets(arr, ptr, noff):
    assert isinstance(arr, np.ndarray) and arr.dtype == np.uint32
    assert arr.shape == (noff,) and arr.ctypes.data == ptr


def _check_compact(res, outs, n, noff, want_hash, compact):
    """outs: the (q, hash, qidx, qstart) arguments of the C call."""
    assert isinstance(res, DispatchResult) and res.filter is None
    _check_array(res.q, outs[0], n, np.int16)
    if want_hash:
        _check_array(res.hash, outs[1], n, np.uint32)
    else:
        assert res.hash is None and outs[1] is None
    if compact:
        _check_array(res.qidx, outs[2], n, np.uint32)
        _check_offsets(res.qstart, outs[3], noff)
    else:
        assert res.qidx is None and res.qstart is None
        assert outs[2] is None and outs[3] is None


def _check_routed(res, outs, n, want_hash, want_filter):
    """outs: the (q, hash, filter, ridx, rstart) arguments of the C call."""
    assert isinstance(res, DispatchResult)
    _check_array(res.q, outs[0], n, np.int16)
    if want_hash:
        _check_array(res.hash, outs[1], n, np.uint32)
    else:
        assert res.hash is None and outs[1] is None
    if want_filter:
        _check_array(res.filter, outs[2], n, np.int8)
    else:
        assert res.filter is None and outs[2] is None
    _check_array(res.qidx, outs[3], n, np.uint32)
    _check_offsets(res.qstart, outs[4], NQ + 4)


FLAGS = list(itertools.product((True, False), (True, False)))


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("want_hash,compact", FLAGS)
def test_dispatch_frames(n, want_hash, compact):
    eng = _engine()
    frames = _frames(n)
    res = eng.dispatch_frames(frames, want_hash=want_hash, compact=compact)
    (name, a), = eng._lib.calls
    assert name == "yrss_dispatch_frames" and a[0] is eng._ctx and a[3] == n and len(a) == 8
    assert eng._lib.seen[name] == frames
    _check_compact(res, a[4:8], n, NQ + 2, want_hash, compact)


@pytest.mark.parametrize("entry", ["dispatch_frames", "route_lists_frames"])
def test_a_frame_longer_than_65535_bytes_is_refused(entry):
    eng = _engine()
    frames = [b"\x00" * 60, b"\x00" * 65536]
    # (the uint16 conversion itself refuses the length where numpy checks it)
    with pytest.raises((ValueError, OverflowError)):
        if entry == "dispatch_frames":
            eng.dispatch_frames(frames)
        else:
            eng.route_lists_frames(frames, 0)
    assert eng._lib.calls == []
    frames[1] = b"\x00" * 65535
    (eng.dispatch_frames(frames) if entry == "dispatch_frames"
     else eng.route_lists_frames(frames, 0))
    assert len(eng._lib.calls) == 1


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("want_hash,compact", FLAGS)
@pytest.mark.parametrize("entry", ["dispatch_burst", "dispatch_burst_zc"])
def test_dispatch_burst(entry, n, want_hash, compact):
    eng = _engine()
    mb = _mbufs(n)
    res = getattr(eng, entry)(mb, want_hash=want_hash, compact=compact, write_rss=True,
                              async_=True)
    (name, a), = eng._lib.calls
    assert name == "yrss_" + entry and a[0] is eng._ctx and len(a) == 8
    assert a[1] == mb.ctypes.data and a[2] == n
    assert a[7] == abi.F_WRITE_RSS | abi.F_ASYNC
    assert eng._inflight is mb        # the pointer array lives until wait()
    _check_compact(res, a[3:7], n, NQ + 2, want_hash, compact)
    getattr(eng, entry)(mb)
    assert eng._lib.calls[-1][1][7] == 0 and eng._inflight is None


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("want_hash,compact", FLAGS)
@pytest.mark.parametrize("route_queue_id", [None, 2])
@pytest.mark.parametrize("entry", ["worker_submit", "worker_submit_frames",
                                   "worker_submit_windows"])
def test_worker_submit(entry, route_queue_id, n, want_hash, compact):
    eng = _engine()
    eng.worker_start(8, 4, route_queue_id=route_queue_id)
    (name, a), = eng._lib.calls
    if route_queue_id is None:
        assert name == "yrss_worker_start" and a[1:] == (8, 4)
    else:
        assert name == "yrss_worker_start_route" and a[1:] == (8, 4, 2)
    noff = NQ + (2 if route_queue_id is None else 4)
    mb = _mbufs(n)
    lens = np.full(n, 60, np.uint16)
    if entry == "worker_submit":
        t = eng.worker_submit(mb, want_hash=want_hash, compact=compact, write_rss=True)
        name, a = eng._lib.calls[-1]
        assert len(a) == 9 and a[1] == mb.ctypes.data and a[2] == n
        assert a[7] == abi.F_WRITE_RSS
        outs = a[3:7]
    elif entry == "worker_submit_frames":
        t = eng.worker_submit_frames(mb, lens, want_hash=want_hash, compact=compact)
        name, a = eng._lib.calls[-1]
        assert len(a) == 9 and a[1] == mb.ctypes.data and a[2] == lens.ctypes.data
        assert a[3] == n
        outs = a[4:8]
    else:
        win = np.zeros(max(n, 1) * 64, np.uint8)
        t = eng.worker_submit_windows(win, 64, lens, want_hash=want_hash, compact=compact)
        name, a = eng._lib.calls[-1]
        assert len(a) == 10 and a[1] == win.ctypes.data and a[2] == 64
        assert a[3] == lens.ctypes.data and a[4] == n
        outs = a[5:9]
    assert name == "yrss_" + entry and a[0] is eng._ctx and t == 1
    res = eng.worker_poll(t)
    assert eng._lib.calls[-1] == ("yrss_worker_poll", (eng._ctx, 1, 1))
    _check_compact(res, outs, n, noff, want_hash, compact)
    assert eng.worker_poll(t) is None      # handed out once


def test_worker_submit_frames_refuses_arrays_of_different_length():
    eng = _engine()
    eng.worker_start()
    with pytest.raises(ValueError):
        eng.worker_submit_frames(_mbufs(3), np.zeros(2, np.uint16))
    assert len(eng._lib.calls) == 1


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("want_hash,want_filter", FLAGS)
def test_route_lists_frames(n, want_hash, want_filter):
    eng = _engine()
    frames = _frames(n)
    res = eng.route_lists_frames(frames, 3, want_hash=want_hash, want_filter=want_filter)
    (name, a), = eng._lib.calls
    assert name == "yrss_route_lists_frames" and a[0] is eng._ctx and len(a) == 10
    assert a[3] == n and a[4] == 3
    assert eng._lib.seen[name] == frames
    _check_routed(res, a[5:10], n, want_hash, want_filter)


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("want_hash,want_filter", FLAGS)
def test_route_lists_burst(n, want_hash, want_filter):
    eng = _engine()
    mb = _mbufs(n)
    res = eng.route_lists_burst(mb, 3, want_hash=want_hash, want_filter=want_filter,
                                write_rss=True)
    (name, a), = eng._lib.calls
    assert name == "yrss_route_lists_burst" and a[0] is eng._ctx and len(a) == 10
    assert a[1] == mb.ctypes.data and a[2] == n and a[3] == 3 and a[9] == abi.F_WRITE_RSS
    _check_routed(res, a[4:9], n, want_hash, want_filter)
    eng.route_lists_burst(mb, 3)
    assert eng._lib.calls[-1][1][9] == 0


def test_route_lists_defaults_ask_for_hash_and_filter():
    eng = _engine()
    res = eng.route_lists_burst(_mbufs(4), 0)
    assert res.hash is not None and res.filter is not None
    res = eng.route_lists_frames(_frames(4), 0)
    assert res.hash is not None and res.filter is not None


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("entry", ["submit", "submit_frames"])
def test_fanout_submit(entry, n):
    fo = _fanout()
    mb = _mbufs(n)
    lens = np.full(n, 60, np.uint16)
    if entry == "submit":
        t = fo.submit(mb)
        (name, a), = fo._lib.calls
        assert name == "yrss_fanout_submit" and len(a) == 9
        assert a[1] == mb.ctypes.data and a[2] == n and a[7] == 0
        outs = a[3:7]
    else:
        t = fo.submit_frames(mb, lens)
        (name, a), = fo._lib.calls
        assert name == "yrss_fanout_submit_frames" and len(a) == 9
        assert a[1] == mb.ctypes.data and a[2] == lens.ctypes.data and a[3] == n
        outs = a[4:8]
    assert a[0] is fo._f and t == 1
    got = fo.next()
    assert got[0] == 1
    _check_compact(got[1], outs, n, NQ + 2, True, True)
