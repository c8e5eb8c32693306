"""GPU parity of the extended mode behind the fan-out
(yrss_fanout_set_extended) and the helper process (yrss_remote_set_extended)
against tests/ext_model.py.  Both own their contexts and start their workers
with YRSS_WORKER_F_EXTENDED; with flags 0 they give the oracle's answers."""
import errno
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ext_model as xm  # noqa: E402
from yastack_amd import abi  # noqa: E402
from yastack_amd.dispatch import FanOut  # noqa: E402
from yastack_amd.remote import RemoteRss  # noqa: E402

from gpu_checks import _gpu  # noqa: E402,F401
from hostbufs import check_lists, expect_lists, fake_mbufs, frames_of  # noqa: E402

U = abi.EXT_UDP
CFG = (8, 8, 1, 0)
BURST, NBURSTS = 65, 6


@functools.lru_cache(maxsize=None)
def _udp4():
    """NBURSTS bursts of BURST UDP4 frames: (frames, model q and hash under
    YRSS_EXT_UDP at the 80 bytes both paths stage)."""
    w, ln = xm.stream(abi.SYN_UDP4, BURST * NBURSTS, 80)
    frames = frames_of(w, ln)
    want = [xm.classify(f, len(f), U, CFG, stride=80) for f in frames]
    return (frames, np.array([x for x, _ in want], np.int16),
            np.array([y for _, y in want], np.uint32))


def _burst(k):
    return slice(k * BURST, (k + 1) * BURST)


def test_fanout_extended(oracle_mod):
    """Two contexts on device 0: six bursts under YRSS_EXT_UDP come back in
    ticket order and equal the model; -EBUSY while a ticket is outstanding;
    flags 0 again gives the oracle's answers."""
    frames, q1, h1 = _udp4()
    q0, h0, _, _ = expect_lists(oracle_mod, frames, CFG)
    assert np.all(q0 == 2) and not h0.any() and np.all(h1 != 0) and len(set(q1.tolist())) > 3
    pool, ptrs, _ = fake_mbufs(frames)
    data = (ptrs + np.uint64(128 + 128)).astype(np.uint64)
    lens = np.array([len(f) for f in frames], np.uint16)
    with FanOut([0, 0], *CFG, nslots=4, nblocks=2) as fo:
        lib = fo._lib
        assert lib.yrss_fanout_set_extended(fo._f, 8) == -errno.EINVAL
        fo.register_host_memory(pool.ctypes.data, pool.nbytes)
        for flags, q, h in ((U, q1, h1), (0, q0, h0)):
            fo.set_extended(udp=bool(flags))
            assert fo.ext_flags == flags
            first = None
            for k in range(NBURSTS):
                s = _burst(k)
                t = fo.submit_frames(data[s], lens[s]) if k % 2 else fo.submit(ptrs[s])
                first = t if first is None else first
                assert t == first + k
                assert lib.yrss_fanout_set_extended(fo._f, flags ^ U) == -errno.EBUSY
            for k in range(NBURSTS):
                # bursts k.. are still outstanding, whatever was handed back
                assert lib.yrss_fanout_set_extended(fo._f, 0) == -errno.EBUSY
                t, r = fo.next()
                assert t == first + k
                s = _burst(k)
                check_lists(r, q[s], h[s], *xm.lists(q[s], CFG[1]))
            assert fo.next(wait=False) is None
        fo.unregister_host_memory(pool.ctypes.data)


def _cfg():
    c = abi.default_config()
    c.nb_procs, c.nb_queues, c.soft_dispatch, c.dispatch_only_core = CFG
    c.device = 0
    return c


def test_remote_extended(oracle_mod):
    """Three helper starts: flags 0 (the oracle's answers), set_extended
    (the model's), restart with a ticket queued (the republished burst and a
    fresh one still equal the model: the flags are the ring's, not the
    helper's)."""
    frames, q1, h1 = _udp4()
    q0, h0, _, _ = expect_lists(oracle_mod, frames, CFG)
    assert np.all(q0 == 2) and np.all(h1 != 0)

    def run(r, k, q, h):
        t = r.submit(frames[_burst(k)])
        return t, (q[_burst(k)], h[_burst(k)])

    def done(r, t, want):
        rc, q, h, qi, qs = r.poll(t)
        assert rc == 0, rc
        qi_ref, qs_ref = xm.lists(want[0], CFG[1])
        assert np.array_equal(q, want[0]) and np.array_equal(h, want[1])
        assert np.array_equal(qi, qi_ref) and np.array_equal(qs[:qs_ref.size], qs_ref)

    with RemoteRss(_cfg(), nslots=4, max_burst=128, nblocks=2, timeout_ms=20000) as r:
        done(r, *run(r, 0, q0, h0))
        pid = r.pid
        r.set_extended(udp=True)
        assert r.pid != pid
        done(r, *run(r, 1, q1, h1))
        queued = run(r, 2, q1, h1)
        assert r._lib.yrss_remote_set_extended(r._r, 0) == -errno.EBUSY
        r.restart()
        done(r, *queued)
        done(r, *run(r, 3, q1, h1))
