"""Routed lists of the one-workgroup bursts (GPU): yrss_route_lists_burst /
yrss_route_lists_frames (one launch of the route burst kernel) and the
persistent worker in route mode (yrss_worker_start_route).

Every case is bit-exact against the oracle's q / hash / filter class and the
numpy twin's (ridx, rstart) = segments.route_lists_from of them; every output
array is allocated longer than needed, pre-filled, and checked untouched past
its end; every test ends with yrss_fault_info clean.  Input: the first POOL
packets of route_helpers.stream (oracle.synth SYN_FUZZ from packet 5), laid out
once as an rte_mbuf pool; a burst is a slice of it.  data_len is capped at
2048 (one mbuf segment), and the oracle sees the capped lengths."""
import errno
import functools

import numpy as np
import pytest

import route_helpers as rh
import route_lists_helpers as rl

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from frames import ethertype_frame, ipip_frame, ipv4_frame  # noqa: E402
from gpu_checks import _gpu  # noqa: E402,F401
from hostbufs import PAD, Arena, Out, fake_mbufs, mbuf_pool, submit  # noqa: E402
from yastack_amd import SoftRss, abi, segments  # noqa: E402

POOL = 4200
# nb_queues -> (nb_procs, nb_queues, soft_dispatch, dispatch_only_core); the route
# bucket counts are 4, 6, 16, 17 (one more ballot bit in peer_mask) and 64 (the cap)
CFG = {1: (4, 1, 1, 0), 3: (3, 3, 1, 0), 13: (13, 13, 1, 0), 14: (14, 14, 1, 0),
       61: (61, 61, 1, 0)}


@functools.lru_cache(maxsize=None)
def _kni_bitmaps():
    from oracle import oracle
    return oracle.kni_bitmap(rh.TCP_PORTS), oracle.kni_bitmap(rh.UDP_PORTS)


@functools.lru_cache(maxsize=None)
def _full(cfg, enable):
    from oracle import oracle
    win, lens = mbuf_pool(POOL)[:2]
    q, h = oracle.dispatch_windows(win, 80, lens, oracle.cfg(*cfg))
    return q, h, oracle.filter_windows(win, 80, lens, enable, *_kni_bitmaps())


def expect(cfg, enable, lo, n, stride=None):
    """The oracle's (q, hash, filter class) of pool packets [lo, lo + n) as a
    burst.  stride None: the host gather's rule (64-byte windows when every
    frame of the burst fits, else 80); the worker's gather always stages 80."""
    from oracle import oracle
    win, lens = mbuf_pool(POOL)[:2]
    if stride is None:
        stride = 64 if n and int(lens[lo:lo + n].max()) <= 64 else 80
    if stride == 80 or n == 0:
        return tuple(a[lo:lo + n] for a in _full(cfg, enable))
    w = np.ascontiguousarray(win.reshape(-1, 80)[lo:lo + n, :stride]).reshape(-1)
    ln = np.ascontiguousarray(lens[lo:lo + n])
    q, h = oracle.dispatch_windows(w, stride, ln, oracle.cfg(*cfg))
    return q, h, oracle.filter_windows(w, stride, ln, enable, *_kni_bitmaps())


def one_launch(eng, form, lo, n, queue_id, want_hash=True, want_filter=True, flags=0):
    _, lens, _, _, ptrs, data = mbuf_pool(POOL)
    o = Out(n, eng.nb_queues, want_hash, want_filter)
    if form == "mbufs":
        rc = eng._lib.yrss_route_lists_burst(eng._ctx, ptrs[lo:].ctypes.data, n, queue_id,
                                             o.p(o.q), o.p(o.h), o.p(o.f), o.p(o.ri), o.p(o.rs),
                                             flags)
    else:
        rc = eng._lib.yrss_route_lists_frames(eng._ctx, data[lo:].ctypes.data,
                                              lens[lo:].ctypes.data, n, queue_id, o.p(o.q),
                                              o.p(o.h), o.p(o.f), o.p(o.ri), o.p(o.rs))
    return rc, o


def lo_for(n, k=37):
    return (k * n) % (POOL - n + 1)


# ---- one-launch path -------------------------------------------------------------


@pytest.mark.parametrize("kni", list(rh.KNI_MODES))
@pytest.mark.parametrize("nq", sorted(CFG))
def test_one_launch_routes(oracle_mod, nq, kni):
    """n on both sides of a tile and of a wave's second and fourth tile (wave w
    owns tiles w, w + 16, ...), every bucket count, every queue_id kind, both
    forms, out_hash / out_filter null and non-null."""
    cfg = CFG[nq]
    enable, method = rh.KNI_MODES[kni]
    accept = method == "accept"
    if nq == 3:    # what the matrix covers, from the oracle
        q, _, f = _full(cfg, enable)
        assert rh.class_counts(q, f, nq, 0, enable, accept)["arp"] > 0
        assert (rh.class_counts(q, f, nq, 2, enable, accept)["kni"] > 0) == enable
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(enable, method, rh.TCP_PORTS, rh.UDP_PORTS)
        k = 0
        for n in (1, 63, 64, 65, 1023, 1025, 4096):
            lo = lo_for(n)
            q, h, f = expect(cfg, enable, lo, n)
            for queue_id in sorted({0, nq - 1, nq}):
                for form in ("mbufs", "frames"):
                    rc, o = one_launch(eng, form, lo, n, queue_id, want_hash=bool(k // 2 & 1),
                                       want_filter=bool(k // 4 & 1))
                    assert rc == 0, (n, queue_id, form, rc)
                    o.check(q, h, f, queue_id, enable, accept)
                    k += 1
        assert eng.fault_info()[0] == abi.FAULT_NONE


def test_one_launch_write_rss_and_empty_burst(oracle_mod):
    cfg, nq, n, lo = CFG[3], 3, 300, 100
    mem, ptrs = mbuf_pool(POOL).mem, mbuf_pool(POOL).ptrs
    stride = int(ptrs[1] - ptrs[0])
    rows = mem.reshape(-1, stride)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(True, "accept", rh.TCP_PORTS, rh.UDP_PORTS)
        q, h, f = expect(cfg, True, lo, n)
        rows[:, 44:48] = 0
        rc, o = one_launch(eng, "mbufs", lo, n, 0, flags=abi.F_WRITE_RSS)
        assert rc == 0
        o.check(q, h, f, 0, True, True)
        rss = rows[:, 44:48].copy().view(np.uint32).ravel()
        assert np.array_equal(rss[lo:lo + n], h) and not rss[:lo].any() and not rss[lo + n:].any()
        rows[:, 44:48] = 0
        # n == 0 zeroes nb_queues + 4 offsets and nothing else
        for form in ("mbufs", "frames"):
            rc, o = one_launch(eng, form, 0, 0, 0)
            assert rc == 0
            assert np.all(o.rs[:nq + 4] == 0) and np.all(o.rs[nq + 4:] == 0x77777777)
            assert np.all(o.q == 0x5A5A) and np.all(o.ri == 0xEEEEEEEE)
        # through the Python entry points
        r = eng.route_lists_burst(ptrs[lo:lo + n], 2)
        ri_ref, rs_ref = segments.route_lists_from(q, f, nq, 2, True, True)
        assert np.array_equal(r.qidx, ri_ref) and np.array_equal(r.qstart, rs_ref)
        assert np.array_equal(r.q, q) and np.array_equal(r.hash, h) and np.array_equal(r.filter, f)
        assert eng.fault_info()[0] == abi.FAULT_NONE


def test_refusals_before_any_launch(oracle_mod):
    with SoftRss(*CFG[3], device=0, max_burst=0) as eng:
        for form in ("mbufs", "frames"):
            rc, o = one_launch(eng, form, 0, 4097, 0)
            assert rc == -errno.ENOTSUP and o.untouched()
        rc, o = one_launch(eng, "mbufs", 0, 64, 0, flags=abi.F_ASYNC)
        assert rc == -errno.EINVAL and o.untouched()
        assert eng.fault_info()[0] == abi.FAULT_NONE
    with SoftRss(62, 62, 1, 0, device=0, max_burst=0) as eng:    # 65 route classes
        for form in ("mbufs", "frames"):
            rc, o = one_launch(eng, form, 0, 64, 0)
            assert rc == -errno.ENOTSUP and o.untouched()
        assert eng._lib.yrss_worker_start_route(eng._ctx, 8, 2, 0) == -errno.ENOTSUP
        eng.worker_start(8, 2)              # 63 buckets: the plain worker still starts
        eng.worker_stop()
        assert eng.fault_info()[0] == abi.FAULT_NONE


# ---- directed bursts ---------------------------------------------------------------


def _windows(frames, stride):
    w = np.zeros((len(frames), stride), np.uint8)
    for i, f in enumerate(frames):
        b = np.frombuffer(f[:stride], np.uint8)
        w[i, :b.size] = b
    return w.reshape(-1), np.array([len(f) for f in frames], np.uint16)


def _expect_frames(oracle_mod, frames, cfg, enable, tcp, udp, stride=None):
    if stride is None:
        stride = 64 if max(len(f) for f in frames) <= 64 else 80
    w, ln = _windows(frames, stride)
    q, h = oracle_mod.dispatch_windows(w, stride, ln, oracle_mod.cfg(*cfg))
    f = oracle_mod.filter_windows(w, stride, ln, enable, oracle_mod.kni_bitmap(tcp),
                                  oracle_mod.kni_bitmap(udp))
    return q, h, f


ARP = ethertype_frame(0x0806, 64)[:64]


def _udp(i, length=64, dport=9999):
    return ipv4_frame("10.1.0.%d" % (i % 250 + 1), 1000 + i, "10.2.0.1", dport, proto=17,
                      length=length)[:length]


DIRECTED = {
    # name: (frames, queue_id, kni mode, tcp ports, udp ports, class of every packet)
    "all_arp_local": ([ARP] * 130, 0, "accept", "80", "53", lambda i, n, nq: nq + 2),
    "all_udp_kni_reject": ([_udp(i) for i in range(130)], 2, "reject", "80", "53",
                           lambda i, n, nq: nq + 1),
    "foreign_first_and_last": ([ARP] + [_udp(i) for i in range(127)] + [ARP], 2, "off", None,
                               None, lambda i, n, nq: 0 if i in (0, n - 1) else 2),
    # (port 53 is on the list: FILTER_KNI, which "reject" keeps local)
    "foreign_first_and_last_kni": ([ARP] + [_udp(i, 90, 53 if i % 3 == 0 else 9999)
                                            for i in range(63)] + [ARP], 2, "reject", "80", "53",
                                   lambda i, n, nq: 0 if i in (0, n - 1) else
                                   (2 if (i - 1) % 3 == 0 else nq + 1)),
}


@pytest.mark.parametrize("name", sorted(DIRECTED))
def test_directed_bursts(oracle_mod, name):
    frames, queue_id, kni, tcp, udp, want_class = DIRECTED[name]
    cfg, nq, n = CFG[3], 3, len(DIRECTED[name][0])
    enable, method = rh.KNI_MODES[kni]
    accept = method == "accept"
    q, h, f = _expect_frames(oracle_mod, frames, cfg, enable, tcp, udp)
    bkt = segments.route_buckets(q, f, nq, queue_id, enable, accept)
    assert [int(b) for b in bkt] == [want_class(i, n, nq) for i in range(n)]
    mem, ptrs, _ = fake_mbufs(frames, headroom=128)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(enable, method, tcp, udp)
        ri_ref, rs_ref = segments.route_lists_from(q, f, nq, queue_id, enable, accept)
        for r in (eng.route_lists_frames(frames, queue_id),
                  eng.route_lists_burst(ptrs, queue_id)):
            assert np.array_equal(r.q, q) and np.array_equal(r.hash, h)
            assert np.array_equal(r.filter, f)
            assert np.array_equal(r.qstart, rs_ref) and np.array_equal(r.qidx, ri_ref)
        assert eng.fault_info()[0] == abi.FAULT_NONE


def test_unresolved_filter_classes_stay_local(oracle_mod):
    """YRSS_FILTER_LOOP (inner IHL 0 under IPIP) and YRSS_FILTER_TRUNC (the
    header walk leaves the 80 staged bytes) on the local queue are local
    delivery, never KNI, under accept and under reject."""
    cfg, nq, queue_id = CFG[3], 3, 2
    loop = ipip_frame(0, 4, 0, length=100)
    trunc = ipip_frame(5, 6, 80, outer_ihl=15, length=140)
    frames = ([loop, trunc, _udp(1, 100)] * 23)[:67]
    for kni in ("accept", "reject"):
        enable, method = rh.KNI_MODES[kni]
        q, h, f = _expect_frames(oracle_mod, frames, cfg, True, "80", "53")
        assert f[0] == abi.FILTER_LOOP and f[1] == abi.FILTER_TRUNC and np.all(q == 2)
        bkt = segments.route_buckets(q, f, nq, queue_id, True, method == "accept")
        assert np.all(bkt[0::3] == queue_id) and np.all(bkt[1::3] == queue_id)
        assert np.all(bkt[2::3] == (nq + 1 if kni == "reject" else queue_id))
        with SoftRss(*cfg, device=0, max_burst=0) as eng:
            eng.set_kni(True, method, "80", "53")
            r = eng.route_lists_frames(frames, queue_id)
            ri_ref, rs_ref = segments.route_lists_from(q, f, nq, queue_id, True, method == "accept")
            assert np.array_equal(r.filter, f) and np.array_equal(r.q, q)
            assert np.array_equal(r.qstart, rs_ref) and np.array_equal(r.qidx, ri_ref)
            assert eng.fault_info()[0] == abi.FAULT_NONE


# ---- the worker in route mode ----------------------------------------------------

BURSTS = [1, 32, 0, 63, 64, 65, 1000, 1024]


def _registered_windows():
    win = mbuf_pool(POOL).win
    a = Arena(win.size)
    a.mem[:win.size] = win
    return a


@pytest.mark.parametrize("nslots,nblocks,nq,queue_id", [
    (8, 2, 3, 0), (4, 1, 3, 2), (4, 1, 3, 3), (8, 2, 61, 2), (4, 1, 61, 0), (8, 2, 61, 61)])
def test_route_worker_bursts(oracle_mod, nslots, nblocks, nq, queue_id):
    """Every burst size twice round the ring (slots are reused), the three
    submit forms, YRSS_F_WRITE_RSS on the mbufs form, outputs in registered
    memory and in slot staging, hash wanted and not."""
    cfg = CFG[nq]
    _, lens, _, mem, ptrs, data = mbuf_pool(POOL)
    src = (lens, ptrs, data)
    rows = mem.reshape(-1, int(ptrs[1] - ptrs[0]))
    rows[:, 44:48] = 0
    sizes = BURSTS * 2 if nslots == 8 else BURSTS + BURSTS[:nslots]
    assert len(sizes) >= 2 * nslots
    wreg = _registered_windows()
    arena = Arena(len(sizes) * (1024 + PAD + nq + 4 + PAD) * 12)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(True, "accept", rh.TCP_PORTS, rh.UDP_PORTS)
        for a in (mem, wreg.mem, arena.mem):
            eng.register_host_memory(a.ctypes.data, a.nbytes)
        eng.worker_start(nslots, nblocks, route_queue_id=queue_id)
        wb = []
        for first in range(0, len(sizes), nslots):
            flight = []
            for k in range(first, min(first + nslots, len(sizes))):
                n = sizes[k]
                lo = lo_for(n, 41 + k)
                form = ("mbufs", "frames", "windows")[k % 3]
                o = Out(n, nq, want_hash=k % 4 != 3, want_filter=False,
                        arena=arena if k % 2 else None)
                write_rss = form == "mbufs" and k % 2 == 0
                flight.append((submit(eng, form, lo, n, o, src, wreg, write_rss=write_rss), lo, n,
                               o))
                if write_rss:
                    wb.append((lo, n))
            for t, lo, n, o in flight:
                assert eng._lib.yrss_worker_poll(eng._ctx, t, 1) == 0
                q, h, f = expect(cfg, True, lo, n, stride=80)
                o.check(q, h, f, queue_id, True, True)
        rss = rows[:, 44:48].copy().view(np.uint32).ravel()
        h_all = _full(cfg, True)[1]
        hit = np.zeros(POOL, bool)
        for lo, n in wb:
            hit[lo:lo + n] = True
        assert hit.any() and np.array_equal(rss[hit], h_all[hit]) and not rss[~hit].any()
        rows[:, 44:48] = 0
        eng.worker_stop()
        for a in (mem, wreg.mem, arena.mem):
            eng.unregister_host_memory(a.ctypes.data)
        assert eng.fault_info()[0] == abi.FAULT_NONE


def test_route_worker_truncated_window_is_freed(oracle_mod):
    """Windows form at stride 64: a hashed TCP frame whose ports lie beyond the
    window is YRSS_Q_TRUNCATED, the freed class, among local and ring packets."""
    cfg, nq, queue_id, stride = CFG[3], 3, 2, 64
    cut = ipv4_frame("10.0.0.1", 1, "10.0.0.2", 2, ihl=15, length=120)
    tcp = ipv4_frame("10.0.0.3", 7, "10.0.0.4", 8, length=64)[:64]
    frames = ([cut, _udp(3), tcp, ARP] * 20)[:77]
    w, ln = _windows(frames, stride)
    q, h, f = _expect_frames(oracle_mod, frames, cfg, True, "80", "53", stride=stride)
    assert q[0] == abi.Q_TRUNCATED and q[1] == 2 and q[3] == 0
    bkt = segments.route_buckets(q, f, nq, queue_id, True, False)
    assert np.all(bkt[0::4] == nq) and np.all(bkt[1::4] == nq + 1)
    a = Arena(w.size)
    a.mem[:w.size] = w
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(True, "reject", "80", "53")
        eng.register_host_memory(a.mem.ctypes.data, a.mem.nbytes)
        eng.worker_start(4, 1, route_queue_id=queue_id)
        r = eng.worker_poll(eng.worker_submit_windows(a.mem, stride, ln))
        ri_ref, rs_ref = segments.route_lists_from(q, f, nq, queue_id, True, False)
        assert np.array_equal(r.q, q) and np.array_equal(r.hash, h)
        assert np.array_equal(r.qstart, rs_ref) and np.array_equal(r.qidx, ri_ref)
        eng.worker_stop()
        eng.unregister_host_memory(a.mem.ctypes.data)
        assert eng.fault_info()[0] == abi.FAULT_NONE


def test_set_kni_on_a_route_worker_and_a_plain_worker_alongside(oracle_mod):
    """yrss_set_kni between bursts changes the classes of the next burst (the
    kernel is relaunched with the new state) and returns -EBUSY while a burst
    is pending; a plain worker on a second context keeps giving the global
    per-queue lists."""
    cfg, nq, queue_id, n = CFG[3], 3, 2, 500
    _, lens, _, mem, ptrs, data = mbuf_pool(POOL)
    lists = []
    with SoftRss(*cfg, device=0, max_burst=0) as eng, \
            SoftRss(*cfg, device=0, max_burst=0) as plain:
        for e in (eng, plain):
            e.register_host_memory(mem.ctypes.data, mem.nbytes)
        eng.worker_start(4, 1, route_queue_id=queue_id)
        plain.worker_start(4, 2)
        for k, kni in enumerate(("accept", "reject", "off", "accept")):
            enable, method = rh.KNI_MODES[kni]
            eng.set_kni(enable, method, rh.TCP_PORTS, rh.UDP_PORTS)
            lo = lo_for(n, 50)
            o = Out(n, nq, want_filter=False)
            t = submit(eng, "mbufs", lo, n, o, (lens, ptrs, data))
            tp = plain.worker_submit(ptrs[lo:lo + n])
            if k == 1:      # a burst is pending: the state it runs under stays
                rc = eng._lib.yrss_set_kni(eng._ctx, 0, b"reject", None, None)
                assert rc == -errno.EBUSY
            assert eng._lib.yrss_worker_poll(eng._ctx, t, 1) == 0
            q, h, f = expect(cfg, enable, lo, n, stride=80)
            o.check(q, h, f, queue_id, enable, method == "accept")
            lists.append(o.rs[:nq + 4].copy())
            r = plain.worker_poll(tp)
            qi_ref, qs_ref = oracle_mod.process_burst(q, nq)
            assert np.array_equal(r.q, q) and np.array_equal(r.hash, h)
            assert np.array_equal(r.qidx, qi_ref) and np.array_equal(r.qstart, qs_ref)
        assert not np.array_equal(lists[0], lists[1]) and not np.array_equal(lists[1], lists[2])
        assert np.array_equal(lists[0], lists[3])
        for e in (eng, plain):
            e.worker_stop()
            e.unregister_host_memory(mem.ctypes.data)
            assert e.fault_info()[0] == abi.FAULT_NONE


# ---- end to end ----------------------------------------------------------------------


@pytest.mark.parametrize("queue_id", [0, 2])
def test_end_to_end_hand_off(oracle_mod, queue_id):
    """A worker burst and a one-launch burst through route_lists with rings of
    limited capacity and failing clones: the per-packet model's result, ring
    order the reference's one-at-a-time order."""
    cfg, nq = (6, 4, 1, 0), 4
    mem, ptrs = mbuf_pool(POOL).mem, mbuf_pool(POOL).ptrs
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(True, "accept", rh.TCP_PORTS, rh.UDP_PORTS)
        eng.register_host_memory(mem.ctypes.data, mem.nbytes)
        eng.worker_start(4, 1, route_queue_id=queue_id)
        for path, n, cap in (("worker", 1000, 100), ("one_launch", 3000, 300)):
            lo = lo_for(n, 3)
            q, _, f = expect(cfg, True, lo, n, stride=80)
            cnt = rh.class_counts(q, f, nq, queue_id, True, True)
            assert cnt["freed"] > 0 and cnt["kni"] > 0 and (cnt["arp"] > 0) == (queue_id == 0)
            if path == "worker":
                r = eng.worker_poll(eng.worker_submit(ptrs[lo:lo + n]))
            else:
                r = eng.route_lists_burst(ptrs[lo:lo + n], queue_id)
            objs, addr_to_idx = rh.fake_objs(n)
            for with_filter in ((True, False) if path == "one_launch" else (False,)):
                cb = rh.Rings(addr_to_idx, [cap] * nq, rh.clone_ok)
                arrays = (r.qidx, r.qstart, r.filter) if with_filter else (r.qidx, r.qstart)
                local, kni_list, rr = eng.route_lists(arrays, objs, queue_id, cb.enqueue, cb.clone,
                                                      cb.release)
                _, _, _, freed_ref = rh.assert_matches_model(
                    cb, [cb.obj(a) for a in local], [cb.obj(a) for a in kni_list], rr, q, f, nq,
                    queue_id, True, True, cap, with_filter=with_filter)
                assert len(freed_ref) > cnt["freed"], "ring-full frees"
        eng.worker_stop()
        eng.unregister_host_memory(mem.ctypes.data)
        assert eng.fault_info()[0] == abi.FAULT_NONE
