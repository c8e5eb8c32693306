"""GPU parity of the redirection table (yrss_set_reta) against
tests/reta_model.py: q, hash and every list form in full, and an empty fault
record.

The table is this build's own semantics.  What ties it to the reference is the
first test: an equal-weights table over 8 queues is hash % 8, so every served
form must return what the same context returned before the table was set (and
that is the first GPU run of the extended kernels with no flag set).  Every
other case asserts that what it expects under its table differs from what the
same packets give without one.
"""
import ctypes
import errno
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ext_model as xm  # noqa: E402
import reta_model as rm  # noqa: E402
from yastack_amd import SoftRss, abi, segments  # noqa: E402
from yastack_amd.dispatch import reta_weighted  # noqa: E402

from gpu_checks import SEG_KNI, dev, first_mismatch_qh, to_np, upload  # noqa: E402,F401
from hostbufs import assert_same, check_lists, fake_mbufs, frames_of  # noqa: E402

V, V6, U = abi.EXT_VLAN, abi.EXT_IPV6, abi.EXT_UDP
CFGS = ((3, 3, 1, 1), (8, 8, 1, 0))     # nb_procs 3 with dispatch_only_core, 8 without
CFG61 = (61, 61, 1, 0)
W103 = (1, 0, 3)                        # queue 1 drained, queue 2 three times queue 0
HEADROOM = 128


def _engine(cfg, flags=0, table=None, **kw):
    eng = SoftRss(*cfg, device=0, max_burst=0, **kw)
    eng.set_extended(vlan=bool(flags & V), ipv6=bool(flags & V6), udp=bool(flags & U))
    if table is not None:
        eng.set_reta(table)
        assert_same("get_reta", eng.get_reta(), table)
    return eng


def _no_fault(eng):
    fault = eng.fault_info()
    assert fault[0] == abi.FAULT_NONE, f"device guard fired: {fault}"


def _moved(q, q0, hashed):
    """The expectation is not the table-free one, and only hashed packets moved."""
    assert not np.array_equal(q, q0), "the table changes nothing here: a vacuous case"
    assert_same("unhashed and truncated packets", q[~hashed], q0[~hashed])


def _check_global(eng, win, lens, stride, n, q_ref, h_ref, nq):
    """yrss_dispatch_dev: q, hash, qidx, qstart."""
    res = eng.dispatch_dev(win, lens, stride, n)
    torch.cuda.synchronize()
    _no_fault(eng)
    first_mismatch_qh(to_np(res.q[:n], np.int16), to_np(res.hash[:n], np.uint32), q_ref, h_ref)
    qi, qs = rm.lists(q_ref, nq)
    assert_same("qstart", to_np(res.qstart, np.uint32), qs)
    assert_same("qidx", to_np(res.qidx[:n], np.uint32), qi)
    return qs


def _check_seg(eng, win, lens, stride, n, q_ref, h_ref, nq):
    """yrss_dispatch_dev_seg: q, hash, seg_idx, seg_off."""
    res = eng.dispatch_dev_seg(win, lens, stride, n)
    torch.cuda.synchronize()
    _no_fault(eng)
    first_mismatch_qh(to_np(res.q[:n], np.int16), to_np(res.hash[:n], np.uint32), q_ref, h_ref)
    si, so = rm.seg_lists(q_ref, nq)
    assert_same("seg_off", to_np(res.seg_off, np.uint16), so)
    assert_same("seg_idx", res.seg_idx[:n].cpu().numpy(), si)


def _filter_ref(oracle_mod, w_h, stride, l_h):
    """The protocol_filter class: the reference's, on the unstripped frame."""
    return oracle_mod.filter_windows(w_h, stride, l_h, True, oracle_mod.kni_bitmap(SEG_KNI[1]),
                                     oracle_mod.kni_bitmap(SEG_KNI[2]))


def _check_route_seg(eng, oracle_mod, win, lens, w_h, l_h, stride, n, q_ref, h_ref, nq, lq):
    """yrss_route_dev_seg under KNI SEG_KNI: q, hash, filter, the routed lists."""
    res = eng.route_dev_seg(win, lens, stride, lq, n, want_filter=True)
    torch.cuda.synchronize()
    _no_fault(eng)
    first_mismatch_qh(to_np(res.q[:n], np.int16), to_np(res.hash[:n], np.uint32), q_ref, h_ref)
    f_ref = _filter_ref(oracle_mod, w_h, stride, l_h)
    assert_same("filter", res.filter[:n].cpu().numpy(), f_ref)
    si, so = segments.route_from(q_ref, f_ref, nq, lq, True, True)
    assert_same("routed seg_off", to_np(res.seg_off, np.uint16), so)
    assert_same("routed seg_idx", res.seg_idx[:n].cpu().numpy(), si)


# ---- an equal table is the reference ------------------------------------------------------

def _host(r):
    arrays = (r.q, r.hash, r.qidx, r.qstart, r.filter)
    return tuple(np.array(a) for a in arrays if a is not None)


def _every_served_form(eng, win, lens, n, frames, pool, ptrs):
    """What every served form returns for the batch (device forms: n windows of
    64 bytes; host forms: the first frames), by name."""
    out = {}

    def dev_res(res, *extra):
        torch.cuda.synchronize()
        _no_fault(eng)
        return tuple(t.cpu().numpy() for t in (res.q[:n], res.hash[:n], *extra))
    for name, tune in (("dev", {}), ("dev scan_kernel", {"scan_kernel": 1}),
                       ("dev grid only", {"one_launch": 2})):
        eng.set_tuning(**tune)
        r = eng.dispatch_dev(win, lens, 64, n)
        out[name] = dev_res(r, r.qidx[:n], r.qstart)
    eng.set_tuning()
    r = eng.dispatch_dev(win, lens, 64, 4096)           # the one-launch kernel
    out["dev one launch"] = dev_res(r, r.qidx[:4096], r.qstart)
    r = eng.dispatch_dev(win, lens, 64, n, want_filter=True)
    out["dev filter"] = dev_res(r, r.qidx[:n], r.qstart, r.filter[:n])
    r = eng.dispatch_dev_seg(win, lens, 64, n)
    out["seg"] = dev_res(r, r.seg_idx[:n], r.seg_off)
    r = eng.route_dev_seg(win, lens, 64, 1, n, want_filter=True)
    out["route seg"] = dev_res(r, r.seg_idx[:n], r.seg_off, r.filter[:n])
    # host forms: one launch (300 frames) and the staged batch (all of them)
    out["frames"] = _host(eng.dispatch_frames(frames[:300]))
    out["frames staged"] = _host(eng.dispatch_frames(frames))
    out["burst"] = _host(eng.dispatch_burst(ptrs[:300]))
    out["burst zc"] = _host(eng.dispatch_burst_zc(ptrs[:300]))
    data = (ptrs[:300] + np.uint64(128 + HEADROOM)).astype(np.uint64)
    ln = np.array([len(f) for f in frames[:300]], np.uint16)
    q, h = np.empty(300, np.int16), np.empty(300, np.uint32)
    qi, qs = np.empty(300, np.uint32), np.empty(eng.nb_queues + 2, np.uint32)
    rc = eng._lib.yrss_dispatch_frames_zc(eng._ctx, data.ctypes.data, ln.ctypes.data, 300,
                                          q.ctypes.data, h.ctypes.data, qi.ctypes.data,
                                          qs.ctypes.data)
    assert rc == 0, rc
    out["frames zc"] = (q, h, qi, qs)
    out["route lists frames"] = _host(eng.route_lists_frames(frames[:300], 1))
    out["route lists burst"] = _host(eng.route_lists_burst(ptrs[:300], 1))
    log = []

    def enqueue(queue, objs):
        log.append((queue, tuple(objs)))
        return len(objs)
    local, kni, res = eng.route_burst(ptrs[:64], 1, enqueue, lambda m, queue: 0, lambda m: None)
    out["route burst"] = (np.array(local, np.uint64), np.array(kni, np.uint64),
                          np.array([res.n_local, res.n_kni, res.n_freed, res.n_arp,
                                    res.n_unresolved, *res.n_ring]),
                          np.array([x for queue, objs in log for x in (queue, *objs)], np.uint64))
    out["shim"] = (np.array([eng.toeplitz_dispatch(f) for f in frames[:8]]),)
    _no_fault(eng)
    return out


@pytest.mark.parametrize("profile", [abi.SYN_FUZZ, abi.SYN_TCP4])
def test_equal_table_equals_reference(dev, oracle_mod, profile):
    """(8, 8, 1, 0), flags 0, 128 entries of i % 8: every served form returns
    what the same context returned before the table was set, at n = 4097."""
    cfg, n = rm.CFG_A, 4097
    w_h, l_h = xm.stream(profile, n, 64)
    q0, h, hashed = rm.stream_model(profile, n, 64, 0, cfg)
    q_ref, h_ref = oracle_mod.dispatch_windows(w_h, 64, l_h, oracle_mod.cfg(*cfg))
    table = reta_weighted([1] * 8, 128)
    assert np.array_equal(rm.apply(table, q0, h, hashed), q_ref) and np.array_equal(h, h_ref)
    # not vacuous: the batch has hashed packets, and another table would show
    assert np.count_nonzero(hashed) > 1000
    assert not np.array_equal(rm.apply(np.zeros(128, np.uint16), q0, h, hashed), q_ref)
    frames = frames_of(*xm.stream(profile, n, 80))
    pool, ptrs, _ = fake_mbufs(frames[:300], headroom=HEADROOM)
    win, lens = upload(w_h, l_h)
    with _engine(cfg) as eng:
        eng.set_kni(True, *SEG_KNI)
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        before = _every_served_form(eng, win, lens, n, frames, pool, ptrs)
        assert_same("q before", before["dev"][0], q_ref)
        assert_same("hash before", before["dev"][1].view(np.uint32), h_ref)
        eng.set_reta(table)
        after = _every_served_form(eng, win, lens, n, frames, pool, ptrs)
        assert before.keys() == after.keys() and len(before) == 16
        for name in before:
            assert len(before[name]) == len(after[name])
            for k, (a, b) in enumerate(zip(before[name], after[name])):
                assert_same(f"{name}[{k}] with the equal table", b, a)
        eng.unregister_host_memory(pool.ctypes.data)


# ---- boundary sweep -----------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _sweep(stride):
    return xm.sweep_batch(stride)


@functools.lru_cache(maxsize=None)
def _sweep_model(stride, flags, cfg):
    win, lens = _sweep(stride)
    return rm.classify_windows(win, stride, lens, flags, cfg)


SWEEP_TABLES = {
    "w103-1": (CFGS[0], lambda: reta_weighted(W103, 1)),
    "w103-2": (CFGS[0], lambda: reta_weighted(W103, 2)),
    "w103-512": (CFGS[0], lambda: reta_weighted(W103, 512)),
    "q61-512": (CFG61, lambda: reta_weighted([1] * 61, 512)),
}


@pytest.mark.parametrize("stride", [64, 80])
@pytest.mark.parametrize("flags", [0, abi.EXT_ALL])
@pytest.mark.parametrize("case", SWEEP_TABLES)
def test_boundary_sweep(dev, case, flags, stride):
    """Every data_len 0..90 of every frame kind (ext_model.sweep_batch) under a
    table of size 1, 2 or 512 with weights (1, 0, 3) on nb_procs 3 with
    dispatch_only_core, and under 512 entries of 61 distinct queues: the grid
    kernel (global and segmented lists) and, in two pieces, the one-launch
    kernel.  Truncated and unhashed packets keep their queues.  (61 queues are
    more than the segmented form takes: that one has the global lists only.)"""
    cfg, make = SWEEP_TABLES[case]
    table = make()
    nq = cfg[1]
    if case == "q61-512":
        assert len(set(table.tolist())) == 61
    win, lens = _sweep(stride)
    n = int(lens.size)
    q0, h_ref, hashed = _sweep_model(stride, flags, cfg)
    q_ref = rm.apply(table, q0, h_ref, hashed)
    _moved(q_ref, q0, hashed)
    trunc = q0 == abi.Q_TRUNCATED
    assert (np.count_nonzero(trunc) > 0) == (stride == 64 or bool(flags & V))
    assert_same("truncated stay truncated", q_ref[trunc], abi.Q_TRUNCATED)
    assert set(q_ref[~hashed & ~trunc].tolist()) == {0, abi.DEFAULT_Q}
    w_d, l_d = upload(win, lens)
    with _engine(cfg, flags, table) as eng:
        eng.set_tuning(one_launch=2)
        _check_global(eng, w_d, l_d, stride, n, q_ref, h_ref, nq)
        eng.set_tuning()
        _check_global(eng, w_d, l_d, stride, n, q_ref, h_ref, nq)
        if nq + 1 <= abi.SEG_MAX_BUCKETS:
            _check_seg(eng, w_d, l_d, stride, n, q_ref, h_ref, nq)
        for lo, hi in ((0, 4096), (4096, n)):
            _check_global(eng, w_d[lo * stride:], l_d[lo:hi], stride, hi - lo, q_ref[lo:hi],
                          h_ref[lo:hi], nq)


# ---- streams ------------------------------------------------------------------------------

STREAMS = ((abi.SYN_TCP4, 0), (abi.SYN_IMIX, 0), (abi.SYN_UDP4, U), (abi.SYN_VLAN6_TCP, V | V6))


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("profile,flags", STREAMS)
def test_streams(dev, oracle_mod, profile, flags, cfg):
    """Synthetic streams at n = 64 and 4096 (the one-launch kernel), 4097 and
    20000 (the grid kernels) under a (1, 0, 3) table of 128 entries through
    every list form: queue 1 gets no hashed packet, queues 0 and 2 get some
    (test_reta_model.py confirms it for these seeds)."""
    nq, lq = cfg[1], 1
    table = reta_weighted(W103, 128)
    for n in (64, 4096, 4097, 20000):
        w_h, l_h = xm.stream(profile, n, 64)
        q0, h_ref, hashed = rm.stream_model(profile, n, 64, flags, cfg)
        q_ref = rm.apply(table, q0, h_ref, hashed)
        _moved(q_ref, q0, hashed)
        with _engine(cfg, flags, table) as eng:
            win, lens = eng.synth(profile, n, stride=64)
            assert_same("synth windows", win[:n * 64].cpu().numpy(), w_h)
            qs = _check_global(eng, win, lens, 64, n, q_ref, h_ref, nq)
            counts = np.diff(qs.astype(np.int64))[:nq]
            assert counts[0] > 0 and counts[2] > 0, counts
            assert counts[1] == np.count_nonzero(~hashed & (q0 == 1)), counts
            eng.set_tuning(scan_kernel=1)
            _check_global(eng, win, lens, 64, n, q_ref, h_ref, nq)
            eng.set_tuning()
            _check_seg(eng, win, lens, 64, n, q_ref, h_ref, nq)
            eng.set_kni(True, *SEG_KNI)
            _check_route_seg(eng, oracle_mod, win, lens, w_h, l_h, 64, n, q_ref, h_ref, nq, lq)
            if n == 20000:
                continue
            # The host forms stage 80 bytes of every frame once one is longer
            # than 64 (frames_of: the window and a zero tail): the model per frame.
            frames = frames_of(w_h, l_h, stride=64)
            f0, fh, fhashed = rm.classify_frames(frames, flags, cfg, stride=80)
            fq = rm.apply(table, f0, fh, fhashed)
            _moved(fq, f0, fhashed)
            r = eng.dispatch_frames(frames)      # one launch; the staged batch at 4097
            _no_fault(eng)
            check_lists(r, fq, fh, *rm.lists(fq, nq))
            if n <= 4096:
                # the one-launch routed burst
                w80 = np.frombuffer(b"".join(f[:80].ljust(80, b"\0") for f in frames), np.uint8)
                f_ref = _filter_ref(oracle_mod, w80, 80, np.array([len(f) for f in frames],
                                                                  np.uint16))
                r = eng.route_lists_frames(frames, lq)
                _no_fault(eng)
                assert_same("routed burst q", r.q, fq)
                assert_same("routed burst hash", r.hash, fh)
                assert_same("routed burst filter", r.filter, f_ref)
                ri, rs = segments.route_lists_from(fq, f_ref, nq, lq, True, True)
                assert_same("rstart", r.qstart, rs)
                assert_same("ridx", r.qidx, ri)


# ---- contract -----------------------------------------------------------------------------

def test_set_get_and_rewrite(dev):
    """-EINVAL leaves the table in force untouched; yrss_get_reta round-trips;
    off means off; a table rewritten between two dispatches holds for the
    second; -EBUSY while a YRSS_F_ASYNC burst is pending."""
    cfg, n, stride = CFGS[0], 5000, 64
    nq = cfg[1]
    w_h, l_h = xm.stream(abi.SYN_IMIX, n, stride)
    q0, h_ref, hashed = rm.stream_model(abi.SYN_IMIX, n, stride, 0, cfg)
    t_a, t_b = reta_weighted(W103, 128), reta_weighted((3, 1, 0), 16)
    q_a, q_b = rm.apply(t_a, q0, h_ref, hashed), rm.apply(t_b, q0, h_ref, hashed)
    _moved(q_a, q0, hashed)
    _moved(q_b, q0, hashed)
    assert not np.array_equal(q_a, q_b)
    win, lens = upload(w_h, l_h)
    frames = frames_of(*xm.stream(abi.SYN_IMIX, 64, 80))
    pool, ptrs, _ = fake_mbufs(frames, headroom=HEADROOM)
    with _engine(cfg) as eng:
        lib, ctx = eng._lib, eng._ctx
        assert eng.get_reta() is None
        _check_global(eng, win, lens, stride, n, q0, h_ref, nq)
        eng.set_reta(t_a)
        assert_same("get_reta", eng.get_reta(), t_a)
        _check_global(eng, win, lens, stride, n, q_a, h_ref, nq)
        # refused tables: a size that is no power of two, one too large, an
        # entry that is no queue of the context
        bad = np.zeros(1024, np.uint16)
        for size in (3, 1024):
            assert lib.yrss_set_reta(ctx, bad.ctypes.data, size) == -errno.EINVAL
        bad[5] = nq
        assert lib.yrss_set_reta(ctx, bad.ctypes.data, 8) == -errno.EINVAL
        small = np.zeros(64, np.uint16)
        assert lib.yrss_get_reta(ctx, small.ctypes.data, 64) == -errno.EINVAL   # cap < 128
        assert_same("get_reta after the refusals", eng.get_reta(), t_a)
        _check_global(eng, win, lens, stride, n, q_a, h_ref, nq)
        _check_seg(eng, win, lens, stride, n, q_a, h_ref, nq)
        # rewritten between two dispatches
        eng.set_reta(t_b)
        assert_same("get_reta", eng.get_reta(), t_b)
        _check_global(eng, win, lens, stride, n, q_b, h_ref, nq)
        _check_global(eng, win, lens, stride, 4096, q_b[:4096], h_ref[:4096], nq)
        # off means off, by either spelling, and on again
        for off in (lambda: eng.set_reta(None),
                    lambda: abi.check(lib.yrss_set_reta(ctx, t_a.ctypes.data, 0), "size 0")):
            off()
            assert eng.get_reta() is None
            assert lib.yrss_get_reta(ctx, None, 0) == 0
            _check_global(eng, win, lens, stride, n, q0, h_ref, nq)
            _check_seg(eng, win, lens, stride, n, q0, h_ref, nq)
            _check_global(eng, win, lens, stride, 4096, q0[:4096], h_ref[:4096], nq)
            eng.set_reta(t_a)
            _check_global(eng, win, lens, stride, 4096, q_a[:4096], h_ref[:4096], nq)
        # a burst in flight was queued under the table in force
        f0, fh, fhashed = rm.classify_frames(frames, 0, cfg, stride=80)
        fq_a, fq_b = rm.apply(t_a, f0, fh, fhashed), rm.apply(t_b, f0, fh, fhashed)
        assert not np.array_equal(fq_a, fq_b) and not np.array_equal(fq_a, f0)
        r = eng.dispatch_burst(ptrs, async_=True)
        assert lib.yrss_set_reta(ctx, t_b.ctypes.data, 16) == -errno.EBUSY
        assert lib.yrss_set_reta(ctx, None, 0) == -errno.EBUSY
        eng.wait()
        check_lists(r, fq_a, fh, *rm.lists(fq_a, nq))
        assert_same("get_reta after -EBUSY", eng.get_reta(), t_a)
        eng.set_reta(t_b)
        check_lists(eng.dispatch_burst(ptrs), fq_b, fh, *rm.lists(fq_b, nq))
        _no_fault(eng)


@pytest.mark.parametrize("extended", [False, True])
def test_worker_and_shim_contract(dev, extended):
    """No worker kernel follows a table: with one set, a worker started either
    way refuses start and submit with -ENOTSUP (the shim on its context: -1)
    and serves again once it is cleared; yrss_set_reta halts a resident worker
    and returns -EBUSY while one of its bursts is pending.  The shim on a
    context without a worker follows the table."""
    cfg = CFGS[1]
    nq = cfg[1]
    flags = U if extended else 0
    w_h, l_h = xm.stream(abi.SYN_UDP4 if extended else abi.SYN_TCP4, 64, 80)
    frames = frames_of(w_h, l_h)
    pool, ptrs, _ = fake_mbufs(frames, headroom=HEADROOM)
    q0, h0, hashed = rm.classify_frames(frames, flags, cfg, stride=80)
    table = reta_weighted(W103, 128)
    q1 = rm.apply(table, q0, h0, hashed)
    _moved(q1, q0, hashed)
    assert np.all(hashed) and q0[:8].tolist() != q1[:8].tolist()
    with _engine(cfg, flags) as eng:
        lib, ctx = eng._lib, eng._ctx
        # the shim without a worker: one-packet launches under the table
        eng.set_reta(table)
        assert [eng.toeplitz_dispatch(f) for f in frames[:8]] == q1[:8].tolist()
        assert lib.yrss_worker_start(ctx, 4, 2) == -errno.ENOTSUP
        assert lib.yrss_worker_start_route(ctx, 4, 2, 1) == -errno.ENOTSUP
        for wf in (0, abi.WORKER_F_ROUTE, abi.WORKER_F_EXTENDED,
                   abi.WORKER_F_EXTENDED | abi.WORKER_F_ROUTE):
            assert lib.yrss_worker_start_flags(ctx, 4, 2, wf, 1) == -errno.ENOTSUP
        eng.set_reta(None)
        assert [eng.toeplitz_dispatch(f) for f in frames[:8]] == q0[:8].tolist()
        # a worker context
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(4, 2, extended=extended)
        t = eng.worker_submit(ptrs)
        assert lib.yrss_set_reta(ctx, table.ctypes.data, 128) == -errno.EBUSY   # a burst is pending
        check_lists(eng.worker_poll(t), q0, h0, *rm.lists(q0, nq))
        assert eng.get_reta() is None
        eng.set_reta(table)                                       # halts the worker
        with pytest.raises(abi.YrssError) as e:
            eng.worker_submit(ptrs)
        assert e.value.errno == errno.ENOTSUP
        tk = ctypes.c_uint64()
        data = (ptrs + np.uint64(128 + HEADROOM)).astype(np.uint64)
        ln = np.array([len(f) for f in frames], np.uint16)
        o = [np.empty(64, np.int16), np.empty(64, np.uint32), np.empty(64, np.uint32),
             np.empty(nq + 2, np.uint32)]
        assert lib.yrss_worker_submit_frames(ctx, data.ctypes.data, ln.ctypes.data, 64,
                                             *(a.ctypes.data for a in o),
                                             ctypes.byref(tk)) == -errno.ENOTSUP
        assert lib.yrss_worker_submit_windows(ctx, pool.ctypes.data, 80, ln.ctypes.data, 64,
                                              *(a.ctypes.data for a in o),
                                              ctypes.byref(tk)) == -errno.ENOTSUP
        assert eng.toeplitz_dispatch(frames[0]) == -1
        # the launch paths of the same context follow the table meanwhile
        check_lists(eng.dispatch_burst(ptrs), q1, h0, *rm.lists(q1, nq))
        eng.set_reta(None)
        t = eng.worker_submit(ptrs)                               # relaunched
        check_lists(eng.worker_poll(t), q0, h0, *rm.lists(q0, nq))
        assert eng.toeplitz_dispatch(frames[0]) == int(q0[0])
        _no_fault(eng)
        eng.worker_stop()
        eng.unregister_host_memory(pool.ctypes.data)
