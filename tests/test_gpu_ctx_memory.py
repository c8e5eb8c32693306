"""The memory a context owns (GPU): the burst staging regrown on one context,
workers of different shapes started and stopped on one context, and the count
of live buffers (yrss_debug_live_buffers of libyrss_test.so) over both.

Input: the first POOL packets of route_helpers.stream, laid out once as an
rte_mbuf pool (data_len capped at 2048, one mbuf segment); a burst is a slice
of it.  Every output is bit-exact against the oracle.

No host entry point hands the filter class back above 4096 packets, so the
5000-packet burst's filter is checked through the only staged call that asks
for it there, yrss_route_burst: its hand-off against the per-packet model of
the oracle's q and filter class (route_helpers.assert_matches_model)."""
import functools

import numpy as np
import pytest

import route_helpers as rh

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_checks import _gpu  # noqa: E402,F401
from hostbufs import Out, check_lists, mbuf_pool, submit  # noqa: E402
from yastack_amd import SoftRss, abi, segments  # noqa: E402

POOL = 5000
CFG, NQ = (8, 8, 1, 0), 8
# first allocation at the 1024 floor, a regrow, a regrow past the one-launch
# limit (4096: the multi-launch path on the device twins), the one-launch path
# on the mapped views after both
STAGED = (32, 1500, 5000, 32)
ZC = 1500


@functools.lru_cache(maxsize=None)
def expect(lo, n, stride=None):
    """The oracle's (q, hash, filter class, qidx, qstart) of pool packets
    [lo, lo + n) as one burst under KNI accept.  stride None: the host gather's
    rule (64-byte windows when every frame of the burst fits, else 80)."""
    from oracle import oracle
    win, lens = mbuf_pool(POOL)[:2]
    if stride is None:
        stride = 64 if int(lens[lo:lo + n].max()) <= 64 else 80
    w = np.ascontiguousarray(win.reshape(-1, 80)[lo:lo + n, :stride]).reshape(-1)
    ln = np.ascontiguousarray(lens[lo:lo + n])
    q, h = oracle.dispatch_windows(w, stride, ln, oracle.cfg(*CFG))
    f = oracle.filter_windows(w, stride, ln, True, oracle.kni_bitmap(rh.TCP_PORTS),
                              oracle.kni_bitmap(rh.UDP_PORTS))
    return (q, h, f, *oracle.process_burst(q, NQ))


def _lo(n, k):
    return (k * 37) % (POOL - n + 1)


def _engine(lib_path=None):
    eng = SoftRss(*CFG, device=0, max_burst=0, lib_path=lib_path)
    eng.set_kni(True, "accept", rh.TCP_PORTS, rh.UDP_PORTS)
    return eng


def staged_bursts(eng, after=lambda: None):
    """The staged bursts of STAGED and the zero-copy one on eng, each checked;
    after() runs once each burst size is done."""
    frames, mem, ptrs = mbuf_pool(POOL).frames, mbuf_pool(POOL).mem, mbuf_pool(POOL).ptrs
    queue_id = 2
    for k, n in enumerate(STAGED):
        lo = _lo(n, k)
        q, h, f, qi, qs = expect(lo, n)
        check_lists(eng.dispatch_frames(frames[lo:lo + n]), q, h, qi, qs)
        if n <= 4096:
            r = eng.route_lists_frames(frames[lo:lo + n], queue_id)
            ri, rs = segments.route_lists_from(q, f, NQ, queue_id, True, True)
            assert np.array_equal(r.filter, f)
            assert np.array_equal(r.q, q) and np.array_equal(r.hash, h)
            assert np.array_equal(r.qidx, ri) and np.array_equal(r.qstart, rs)
        else:
            cap = 400
            cb = rh.Rings({int(a): i for i, a in enumerate(ptrs[lo:lo + n])}, [cap] * NQ,
                          rh.clone_ok)
            local, kni, res = eng.route_burst(ptrs[lo:lo + n], queue_id, cb.enqueue, cb.clone,
                                              cb.release)
            assert rh.class_counts(q, f, NQ, queue_id, True, True)["kni"] > 0
            freed = rh.assert_matches_model(cb, [cb.obj(a) for a in local],
                                            [cb.obj(a) for a in kni], res, q, f, NQ, queue_id,
                                            True, True, cap)[3]
            assert freed, "ring-full frees"
        after()
    eng.register_host_memory(mem.ctypes.data, mem.nbytes)
    lo = _lo(ZC, 5)
    q, h, _, qi, qs = expect(lo, ZC, 80)    # (the device gather always stages 80)
    check_lists(eng.dispatch_burst_zc(ptrs[lo:lo + ZC]), q, h, qi, qs)
    eng.unregister_host_memory(mem.ctypes.data)
    assert eng.fault_info()[0] == abi.FAULT_NONE
    after()


# (nslots, nblocks, route queue or None, bursts)
WORKERS = ((8, 4, None, 3), (16, 2, 2, 3), (8, 4, None, 1))


def worker_rounds(eng, around=lambda start_stop: start_stop()):
    """A plain worker, a route worker and a plain one again on eng, 32-packet
    bursts, each checked; around(f) runs f, one worker's start to its stop."""
    _, lens, _, mem, ptrs, data = mbuf_pool(POOL)
    eng.register_host_memory(mem.ctypes.data, mem.nbytes)
    k = 0
    for nslots, nblocks, queue_id, bursts in WORKERS:
        def start_stop():
            nonlocal k
            eng.worker_start(nslots, nblocks, route_queue_id=queue_id)
            for _ in range(bursts):
                lo, k = _lo(32, 11 + k), k + 1
                q, h, f, qi, qs = expect(lo, 32, 80)    # (the worker's gather stages 80)
                if queue_id is None:
                    check_lists(eng.worker_poll(eng.worker_submit(ptrs[lo:lo + 32])), q, h, qi, qs)
                else:
                    o = Out(32, NQ, want_filter=False)
                    t = submit(eng, "mbufs", lo, 32, o, (lens, ptrs, data))
                    assert eng._lib.yrss_worker_poll(eng._ctx, t, 1) == 0
                    o.check(q, h, f, queue_id, True, True)
            eng.worker_stop()
        around(start_stop)
    eng.unregister_host_memory(mem.ctypes.data)
    assert eng.fault_info()[0] == abi.FAULT_NONE


def test_staging_regrowth(oracle_mod):
    with _engine() as eng:
        staged_bursts(eng)


def test_worker_restart_on_one_context(oracle_mod):
    with _engine() as eng:
        worker_rounds(eng)


def test_live_buffers(oracle_mod):
    """The ranks' workspace is one more buffer from the first multi-launch
    batch with lists on: a device batch of POOL packets allocates it before the
    first staged burst, so the staged bursts' counts show the staging alone."""
    path = str(abi.TEST_LIB_PATH)
    live = abi.load(path).yrss_debug_live_buffers
    assert live() == 0
    with _engine(path) as eng:
        win, lens = eng.synth(abi.SYN_FUZZ, POOL, stride=80)
        eng.dispatch_dev(win, lens, 80)
        torch.cuda.synchronize()
        counts = []
        staged_bursts(eng, lambda: counts.append(live()))
        assert len(counts) == len(STAGED) + 1 and counts[0] > 0
        assert counts == [counts[0]] * len(counts), counts

        def around(start_stop):
            before = live()
            start_stop()
            assert live() == before
        worker_rounds(eng, around)
        own = live()
        with _engine(path) as other:
            assert live() > own
            staged_bursts(other)
            other.worker_start(8, 4)
        assert live() == own    # (close stops the worker and frees the staging)
    assert live() == 0
