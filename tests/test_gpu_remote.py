"""The helper-process engine on the GPU (include/yrss_remote.h): bursts
copied into the shared ring come back bit-exact against the oracle
(toeplitz_dispatch, fs/lib/ff_dpdk_if.c:1945-2113, and the process_packets
FIFO lists, :1058-1094); killing the helper with bursts in flight makes the
poll return -EPIPE, and a restarted helper (a fresh GPU context) completes
every queued burst, still bit-exact."""
import errno
import os
import signal

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from yastack_amd import abi  # noqa: E402
from yastack_amd.remote import RemoteRss  # noqa: E402

from hostbufs import expect_lists, synth_frames  # noqa: E402


def _cfg(npr, nq, soft, only):
    c = abi.default_config()
    c.nb_procs, c.nb_queues, c.soft_dispatch, c.dispatch_only_core = npr, nq, soft, only
    c.device = 0
    return c


def _check(oracle_mod, frames, cfg, res):
    rc, q, h, qi, qs = res
    assert rc == 0
    qr, hr, qir, qsr = expect_lists(oracle_mod, frames, cfg)
    assert np.array_equal(q, qr) and np.array_equal(h, hr)
    assert np.array_equal(qi, qir) and np.array_equal(qs[: qsr.size], qsr)


@pytest.mark.parametrize("cfg", [(3, 3, 1, 1), (8, 8, 1, 0)])
def test_remote_bursts_bit_exact(oracle_mod, cfg):
    frames = synth_frames(oracle_mod, 2000, 31 + cfg[0])
    sizes = [32, 1, 1024, 300, 0, 643]
    with RemoteRss(_cfg(*cfg), nslots=8, max_burst=1024, nblocks=4, timeout_ms=20000) as r:
        off, tk = 0, []
        for n in sizes:
            tk.append((r.submit(frames[off:off + n]), off, n))
            off += n
        for t, o, n in tk:
            _check(oracle_mod, frames[o:o + n], cfg, r.poll(t))


def test_remote_helper_killed_then_restarted(oracle_mod):
    cfg = (5, 4, 1, 1)
    frames = synth_frames(oracle_mod, 640, 77)
    with RemoteRss(_cfg(*cfg), nslots=16, max_burst=64, nblocks=4, timeout_ms=20000) as r:
        first = r.submit(frames[:64])
        _check(oracle_mod, frames[:64], cfg, r.poll(first))
        tk = [(r.submit(frames[64 * k:64 * k + 64]), 64 * k) for k in range(1, 10)]
        pid = r.pid
        os.kill(pid, signal.SIGKILL)
        rc = r.poll(tk[-1][0])[0]
        # the helper may have finished some bursts before it died; a burst it
        # did not finish is reported, not waited on
        assert rc in (0, -errno.EPIPE)
        if rc == 0:
            tk = tk[:-1]
        r.restart()
        assert r.pid != pid
        for t, o in tk:
            res = r.poll(t)
            if res[0] == -errno.EINVAL:      # already collected above
                continue
            _check(oracle_mod, frames[o:o + 64], cfg, res)
        t = r.submit(frames[:64])
        _check(oracle_mod, frames[:64], cfg, r.poll(t))
