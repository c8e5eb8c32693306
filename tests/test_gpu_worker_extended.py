"""GPU parity of the extended mode on the persistent worker
(yrss_worker_start_flags with YRSS_WORKER_F_EXTENDED) against tests/ext_model.py:
q, hash and both list arrays of every burst, in the three submit forms, in
route mode, across flag changes on one worker, and through the shim.

Every case asserts that what it expects under its flags differs from what the
same packets give under flags 0.  The contract of a worker started the old
way (refusing while flags are set) is test_gpu_extended.py's.
"""
import errno
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ext_model as xm  # noqa: E402
import route_lists_helpers as rl  # noqa: E402
from yastack_amd import SoftRss, abi  # noqa: E402

from gpu_checks import _gpu  # noqa: E402,F401
from hostbufs import Arena, assert_same, check_lists, fake_mbufs, frames_of  # noqa: E402

V, V6, U = abi.EXT_VLAN, abi.EXT_IPV6, abi.EXT_UDP
ALL = V | V6 | U
CFGS = ((3, 3, 1, 1), (8, 8, 1, 0))     # nb_procs 3 with dispatch_only_core, 8 without
HEADROOM = 128
NSLOTS, NBLOCKS = 4, 2
MIX = -1                                # _pool: three streams interleaved


def _set(eng, flags):
    eng.set_extended(vlan=bool(flags & V), ipv6=bool(flags & V6), udp=bool(flags & U))
    assert eng.ext_flags == flags


def _no_fault(eng):
    fault = eng.fault_info()
    assert fault[0] == abi.FAULT_NONE, f"device guard fired: {fault}"


def _differs(a, b):
    return any(not np.array_equal(x, y) for x, y in zip(a, b))


@functools.lru_cache(maxsize=None)
def _sweep(stride):
    return xm.sweep_batch(stride)


@functools.lru_cache(maxsize=None)
def _sweep_model(stride, flags):
    win, lens = _sweep(stride)
    return xm.classify_windows(win, stride, lens, flags, CFGS[1])


@functools.lru_cache(maxsize=None)
def _pool(profile, n=1024):
    """The stream's first n packets as frames in an rte_mbuf pool: (frames,
    pool memory, mbuf pointers, frame data pointers, data_len, pool row stride)."""
    if profile == MIX:
        # SYN_FUZZ has neither tags nor IPv6: UDP4, VLAN6_TCP and FUZZ packets
        # in turn, so that every flag changes something
        parts = [_pool(p, n // 3)[0] for p in (abi.SYN_UDP4, abi.SYN_VLAN6_TCP, abi.SYN_FUZZ)]
        frames = [f for trio in zip(*parts) for f in trio]
    else:
        w, ln = xm.stream(profile, n, 80)
        frames = frames_of(w, ln)
    mem, ptrs, stride = fake_mbufs(frames, headroom=HEADROOM)
    data = (ptrs + np.uint64(128 + HEADROOM)).astype(np.uint64)
    lens = np.array([len(f) for f in frames], np.uint16)
    return frames, mem, ptrs, data, lens, stride


@functools.lru_cache(maxsize=None)
def _frames_model(profile, flags, cfg, n=1024):
    """The model's (q, hash) per frame at the 80 bytes the worker's gather stages."""
    frames = _pool(profile, n)[0]
    want = [xm.classify(f, len(f), flags, cfg, stride=80) for f in frames]
    return (np.array([x for x, _ in want], np.int16), np.array([y for _, y in want], np.uint32))


# ---- boundary sweep, windows form ----------------------------------------------------

@pytest.mark.parametrize("stride", [64, 80])
@pytest.mark.parametrize("flags", xm.ALL_FLAG_SETS)
def test_boundary_sweep_windows(flags, stride):
    """Every data_len 0..90 of every frame kind, in bursts of at most 1024
    through yrss_worker_submit_windows: the caller's stride sets the window
    rule (IHL 12 and 15 at stride 64 under any flags; at 80 only tags with
    IHL 15, so only under YRSS_EXT_VLAN)."""
    cfg = CFGS[1]
    nq = cfg[1]
    win, lens = _sweep(stride)
    n = int(lens.size)
    q_ref, h_ref = _sweep_model(stride, flags)
    q0, h0 = _sweep_model(stride, 0)
    assert (flags != 0) == _differs((q_ref, h_ref), (q0, h0))
    trunc = np.count_nonzero(q_ref == abi.Q_TRUNCATED)
    assert (trunc > 0) == (stride == 64 or bool(flags & V)), trunc
    arena = Arena(win.size)
    arena.mem[:win.size] = win
    bursts = [(lo, min(lo + 1024, n)) for lo in range(0, n, 1024)]
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        _set(eng, flags)
        eng.register_host_memory(arena.mem.ctypes.data, arena.mem.nbytes)
        eng.worker_start(NSLOTS, NBLOCKS, extended=True)
        for first in range(0, len(bursts), NSLOTS):
            flight = [(eng.worker_submit_windows(arena.mem[lo * stride:], stride, lens[lo:hi]),
                       lo, hi) for lo, hi in bursts[first:first + NSLOTS]]
            for t, lo, hi in flight:
                check_lists(eng.worker_poll(t), q_ref[lo:hi], h_ref[lo:hi],
                            *xm.lists(q_ref[lo:hi], nq))
        _no_fault(eng)
        eng.worker_stop()
        eng.unregister_host_memory(arena.mem.ctypes.data)


# ---- burst sizes, mbuf and frames forms -------------------------------------------------

SIZES = (0, 1, 63, 64, 65, 1023, 1024)   # 63 / 64 / 65 straddle a tile; 1024: a tile per wave
STREAMS = ((abi.SYN_UDP4, U), (abi.SYN_VLAN6_TCP, V | V6), (abi.SYN_FUZZ, ALL))


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("profile,flags", STREAMS)
def test_burst_sizes(profile, flags, cfg):
    """Each size through the mbuf form with YRSS_F_WRITE_RSS (hash.rss of the
    burst's mbufs is the model's hash, of no other) and the frames form."""
    nq = cfg[1]
    frames, mem, ptrs, data, lens, stride = _pool(profile)
    q, h = _frames_model(profile, flags, cfg)
    q0, h0 = _frames_model(profile, 0, cfg)
    rows = mem.reshape(-1, stride)
    rows[:, 44:48] = 0
    lo = int(np.flatnonzero((q != q0) | (h != h0))[0])
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        _set(eng, flags)
        eng.register_host_memory(mem.ctypes.data, mem.nbytes)
        eng.worker_start(NSLOTS, NBLOCKS, extended=True)
        for n in SIZES:
            if n == 0:
                for t in (eng.worker_submit(ptrs[:0]), eng.worker_submit_frames(data[:0], lens[:0])):
                    r = eng.worker_poll(t)
                    assert r.q.size == 0
                    assert_same("qstart of an empty burst", r.qstart[:nq + 2], 0)
                continue
            # the burst starts at the stream's first packet that the flags change
            # (SYN_FUZZ opens with plain TCP), or as near to it as n allows: an
            # empty burst has nothing to differ in, every other size must
            s = slice(min(lo, 1024 - n), min(lo, 1024 - n) + n)
            assert _differs((q[s], h[s]), (q0[s], h0[s])), n
            qi, qs = xm.lists(q[s], nq)
            t1 = eng.worker_submit(ptrs[s], write_rss=True)
            t2 = eng.worker_submit_frames(data[s], lens[s])
            check_lists(eng.worker_poll(t1), q[s], h[s], qi, qs)
            check_lists(eng.worker_poll(t2), q[s], h[s], qi, qs)
            rss = rows[:, 44:48].copy().view(np.uint32).ravel()
            assert_same("hash.rss of the burst", rss[s], h[s])
            assert_same("hash.rss before the burst", rss[:s.start], 0)
            assert_same("hash.rss past the burst", rss[s.stop:], 0)
            rows[:, 44:48] = 0
        _no_fault(eng)
        eng.worker_stop()
        eng.unregister_host_memory(mem.ctypes.data)


# ---- route mode --------------------------------------------------------------------------

ROUTE_CFG = {3: (3, 3, 1, 0), 61: (61, 61, 1, 0)}
KNI = ("accept", "0-32767", "1000-40000,53,123")   # wide: both streams have KNI packets


@pytest.mark.parametrize("nq,lq,kni", [(3, 1, True), (3, 2, False), (61, 2, True)])
@pytest.mark.parametrize("profile,flags", [(abi.SYN_FUZZ, ALL), (abi.SYN_UDP4, U)])
def test_route_mode(oracle_mod, profile, flags, nq, lq, kni):
    """YRSS_WORKER_F_ROUTE | YRSS_WORKER_F_EXTENDED: the routed lists are
    route_lists_helpers' model fed with the extended q and the reference's
    filter class of the unstripped frame.  61 queues: the LDS maximum."""
    cfg = ROUTE_CFG[nq]
    n = 300
    frames, mem, ptrs, data, lens, _ = _pool(profile)
    q, h = _frames_model(profile, flags, cfg)
    q0, _ = _frames_model(profile, 0, cfg)
    q, h, q0 = q[:n], h[:n], q0[:n]
    w80 = np.frombuffer(b"".join(f[:80].ljust(80, b"\0") for f in frames[:n]), np.uint8)
    f_ref = oracle_mod.filter_windows(w80, 80, lens[:n], kni, oracle_mod.kni_bitmap(KNI[1]),
                                      oracle_mod.kni_bitmap(KNI[2]))
    assert (np.count_nonzero(f_ref == abi.FILTER_KNI) > 0) == kni
    ri, rs = rl.expected(q, f_ref, nq, lq, kni, True)
    ri0, rs0 = rl.expected(q0, f_ref, nq, lq, kni, True)
    assert _differs((q, ri, rs), (q0, ri0, rs0))
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        _set(eng, flags)
        eng.set_kni(kni, *KNI)
        eng.register_host_memory(mem.ctypes.data, mem.nbytes)
        eng.worker_start(NSLOTS, NBLOCKS, route_queue_id=lq, extended=True)
        t1 = eng.worker_submit_frames(data[:n], lens[:n])
        t2 = eng.worker_submit(ptrs[:n])
        for t in (t1, t2):
            r = eng.worker_poll(t)
            assert_same("q", r.q, q)
            assert_same("hash", r.hash, h)
            assert_same("rstart", r.qstart[:nq + 4], rs)
            assert_same("ridx", r.qidx, ri)
        _no_fault(eng)
        eng.worker_stop()
        eng.unregister_host_memory(mem.ctypes.data)


# ---- flag changes on one worker --------------------------------------------------------------

def test_flag_changes_on_one_worker():
    """0, U, 0, V | V6, ALL on one worker: every change halts it and the next
    submit relaunches it under the new flags, the plain kernel for flags 0;
    tickets run on; -EBUSY while a burst is pending."""
    cfg = CFGS[1]
    nq, n = cfg[1], 201
    frames, mem, ptrs, data, lens, _ = _pool(MIX, 201)
    q0, h0 = _frames_model(MIX, 0, cfg, 201)
    seen = []
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        lib, ctx = eng._lib, eng._ctx
        assert lib.yrss_worker_start_flags(ctx, NSLOTS, NBLOCKS, 4, 0) == -errno.EINVAL
        assert lib.yrss_worker_start_flags(ctx, NSLOTS, NBLOCKS, 0xFFFFFFFF, 0) == -errno.EINVAL
        eng.register_host_memory(mem.ctypes.data, mem.nbytes)
        eng.worker_start(NSLOTS, NBLOCKS, extended=True)
        want_ticket = 1
        for flags in (0, U, 0, V | V6, ALL):
            _set(eng, flags)
            q, h = _frames_model(MIX, flags, cfg, 201)
            assert (flags != 0) == _differs((q, h), (q0, h0))
            assert all(_differs((q, h), s) for f, s in seen if f != flags)
            seen.append((flags, (q, h)))
            for form in ("frames", "mbufs"):
                t = (eng.worker_submit_frames(data[:n], lens[:n]) if form == "frames"
                     else eng.worker_submit(ptrs[:n]))
                assert t == want_ticket
                want_ticket += 1
                for other in (U, 0, ALL):
                    assert lib.yrss_set_extended(ctx, other) == -errno.EBUSY
                check_lists(eng.worker_poll(t), q, h, *xm.lists(q, nq))
        _no_fault(eng)
        eng.worker_stop()
        eng.unregister_host_memory(mem.ctypes.data)


# ---- off means off ----------------------------------------------------------------------------

def test_off_means_off(oracle_mod):
    """With flags 0 a YRSS_WORKER_F_EXTENDED worker gives the oracle's answers
    on SYN_FUZZ at n = 1024, as a plain worker does, before and after a spell
    under every flag."""
    cfg = CFGS[0]
    nq, n = cfg[1], 1024
    frames, mem, ptrs, data, lens, _ = _pool(abi.SYN_FUZZ)
    c = oracle_mod.cfg(*cfg)
    want = [oracle_mod.toeplitz_dispatch(f, len(f), c) for f in frames]
    q0 = np.array([x for x, _ in want], np.int16)
    h0 = np.array([y for _, y in want], np.uint32)
    q1, h1 = _frames_model(abi.SYN_FUZZ, ALL, cfg)
    assert _differs((q1, h1), (q0, h0))
    lists0 = xm.lists(q0, nq)
    with SoftRss(*cfg, device=0, max_burst=0) as ext, SoftRss(*cfg, device=0, max_burst=0) as pl:
        for eng in (ext, pl):
            eng.register_host_memory(mem.ctypes.data, mem.nbytes)
        ext.worker_start(NSLOTS, NBLOCKS, extended=True)
        pl.worker_start(NSLOTS, NBLOCKS)
        for eng in (ext, pl):
            check_lists(eng.worker_poll(eng.worker_submit(ptrs[:n])), q0, h0, *lists0)
        _set(ext, ALL)
        check_lists(ext.worker_poll(ext.worker_submit_frames(data[:n], lens[:n])), q1, h1,
                    *xm.lists(q1, nq))
        _set(ext, 0)
        check_lists(ext.worker_poll(ext.worker_submit_frames(data[:n], lens[:n])), q0, h0, *lists0)
        for eng in (ext, pl):
            _no_fault(eng)
            eng.worker_stop()
            eng.unregister_host_memory(mem.ctypes.data)


# ---- the registration shim ---------------------------------------------------------------------

def test_shim_on_an_extended_worker_context():
    """yrss_toeplitz_dispatch on a YRSS_WORKER_F_EXTENDED worker context: its
    one-packet worker bursts follow the flags."""
    cfg = CFGS[1]
    frames = _pool(abi.SYN_UDP4)[0][:8]
    q1, _ = _frames_model(abi.SYN_UDP4, U, cfg)
    want = q1[:8].tolist()
    assert len(set(want)) > 3 and want != [2] * 8
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.worker_start(NSLOTS, NBLOCKS, extended=True)
        _set(eng, U)
        assert [eng.toeplitz_dispatch(f) for f in frames] == want
        _set(eng, 0)
        assert [eng.toeplitz_dispatch(f) for f in frames] == [2] * 8
        _no_fault(eng)
        eng.worker_stop()
