"""GPU parity of the persistent burst worker (yrss_worker_*): bursts handed
to a resident gfx950 kernel through a ring in host-coherent memory, checked
against the oracle; relaunch after an idle exit; fault and limit reporting.
"""
import ctypes
import time

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from yastack_amd import SoftRss, abi  # noqa: E402

from gpu_checks import dev  # noqa: E402,F401
from hostbufs import check_lists, expect_lists, fake_mbufs, synth_frames  # noqa: E402


@pytest.mark.parametrize("nslots,nblocks", [(16, 4), (8, 1), (32, 8)])
def test_worker_bursts_vs_oracle(dev, oracle_mod, nslots, nblocks):
    cfg = (5, 4, 1, 1)
    rng = np.random.default_rng(nslots * 100 + nblocks)
    sizes = [1, 32, 1024, 0, 33, 64, 1000, 7] + list(rng.integers(1, 1025, 30))
    total = int(sum(sizes))
    frames = synth_frames(oracle_mod, total, 4000 + nslots)
    pool, ptrs, stride = fake_mbufs(frames, headroom=129)
    q_all, h_all, _, _ = expect_lists(oracle_mod, frames, cfg)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(nslots, nblocks)
        tickets, offs, off = [], [], 0
        for i, n in enumerate(sizes):
            if len(tickets) - len(offs) >= 0 and i >= nslots:   # keep <= nslots in flight
                _verify(eng, oracle_mod, tickets, offs, sizes, q_all, h_all, cfg)
            tickets.append(eng.worker_submit(ptrs[off:off + n], write_rss=(i % 3 == 0)))
            offs.append(off)
            off += n
        while len(offs) > 0 and tickets:
            _verify(eng, oracle_mod, tickets, offs, sizes, q_all, h_all, cfg)
        rss = pool.reshape(-1, stride)[:, 44:48].copy().view(np.uint32).ravel()
        off = 0
        for i, n in enumerate(sizes):
            if i % 3 == 0 and n:
                assert np.array_equal(rss[off:off + n], h_all[off:off + n])
            off += n
        eng.worker_stop()
        eng.unregister_host_memory(pool.ctypes.data)


def _verify(eng, oracle_mod, tickets, offs, sizes, q_all, h_all, cfg):
    t = tickets.pop(0)
    off = offs.pop(0)
    n = sizes[t - 1]
    r = eng.worker_poll(t)
    q = q_all[off:off + n]
    qi, qs = oracle_mod.process_burst(q, cfg[1])
    check_lists(r, q, h_all[off:off + n], qi, qs)


def test_worker_idle_exit_and_relaunch(dev, oracle_mod, monkeypatch):
    monkeypatch.setenv("YRSS_WORKER_IDLE_MS", "5")
    monkeypatch.setenv("YRSS_WORKER_LIFE_MS", "200")
    cfg = (3, 3, 1, 1)
    frames = synth_frames(oracle_mod, 600, 9)
    pool, ptrs, _ = fake_mbufs(frames)
    q, h, _, _ = expect_lists(oracle_mod, frames, cfg)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(4, 2)
        for k in range(6):
            lo = 100 * k
            t = eng.worker_submit(ptrs[lo:lo + 100])
            r = eng.worker_poll(t)
            qi, qs = oracle_mod.process_burst(q[lo:lo + 100], 3)
            check_lists(r, q[lo:lo + 100], h[lo:lo + 100], qi, qs)
            time.sleep(0.03 if k % 2 == 0 else 0.25)   # past the idle / lifetime limits
        # registering more memory restarts the worker with the new range table
        extra = synth_frames(oracle_mod, 50, 10)
        pool2, ptrs2, _ = fake_mbufs(extra)
        eng.register_host_memory(pool2.ctypes.data, pool2.nbytes)
        q2, h2, qi2, qs2 = expect_lists(oracle_mod, extra, cfg)
        check_lists(eng.worker_poll(eng.worker_submit(ptrs2)), q2, h2, qi2, qs2)
        eng.worker_stop()
        eng.unregister_host_memory(pool2.ctypes.data)
        eng.unregister_host_memory(pool.ctypes.data)


def test_worker_errors(dev, oracle_mod):
    cfg = (3, 3, 1, 1)
    frames = synth_frames(oracle_mod, 1100, 12)
    pool, ptrs, _ = fake_mbufs(frames)
    lib = abi.load()
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        assert lib.yrss_worker_start(eng._ctx, 6, 4) == -22          # nslots % nblocks
        assert lib.yrss_worker_start(eng._ctx, 256, 256) == -22       # too many blocks
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(2, 1)
        with pytest.raises(abi.YrssError):
            eng.worker_submit(ptrs[:1025])                            # > 1024 packets
        bad = ptrs[:50].copy()
        bad[7] = np.uint64(pool.ctypes.data + pool.nbytes + 8192)
        tb = eng.worker_submit(bad)
        t2 = eng.worker_submit(ptrs[:20])
        with pytest.raises(abi.YrssError):
            eng.worker_submit(ptrs[:5])                               # both slots unpolled
        with pytest.raises(abi.YrssError):
            eng.worker_poll(tb)                                       # -EFAULT
        q, h, qi, qs = expect_lists(oracle_mod, frames[:20], cfg)
        check_lists(eng.worker_poll(t2), q, h, qi, qs)
        eng.worker_stop()
        eng.unregister_host_memory(pool.ctypes.data)


def test_worker_frames(dev, oracle_mod):
    """yrss_worker_submit_frames: (data, data_len) pairs; the GPU reads only
    the windows."""
    cfg = (8, 8, 1, 0)
    sizes = [32, 1, 1024, 500, 0, 77]
    frames = synth_frames(oracle_mod, sum(sizes), 55)
    pool, ptrs, _ = fake_mbufs(frames, headroom=130)
    data = (ptrs + np.uint64(128 + 130)).astype(np.uint64)
    flen = np.array([len(f) for f in frames], np.uint16)
    q_all, h_all, _, _ = expect_lists(oracle_mod, frames, cfg)
    lib = abi.load()
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(8, 2)
        off = 0
        for n in sizes:
            q = np.empty(max(n, 1), np.int16)
            h = np.empty(max(n, 1), np.uint32)
            qi = np.empty(max(n, 1), np.uint32)
            qs = np.empty(cfg[1] + 2, np.uint32)
            t = ctypes.c_uint64()
            rc = lib.yrss_worker_submit_frames(eng._ctx, data[off:].ctypes.data,
                                               flen[off:].ctypes.data, n, q.ctypes.data,
                                               h.ctypes.data, qi.ctypes.data, qs.ctypes.data,
                                               ctypes.byref(t))
            assert rc == 0
            assert lib.yrss_worker_poll(eng._ctx, t.value, 1) == 0
            qr = q_all[off:off + n]
            qi_ref, qs_ref = oracle_mod.process_burst(qr, cfg[1])
            assert np.array_equal(q[:n], qr) and np.array_equal(h[:n], h_all[off:off + n])
            assert np.array_equal(qi[:n], qi_ref) and np.array_equal(qs[: qs_ref.size], qs_ref)
            off += n
        eng.worker_stop()
        eng.unregister_host_memory(pool.ctypes.data)


@pytest.mark.parametrize("stride", [80, 96, 128])
def test_worker_windows(dev, oracle_mod, stride):
    """yrss_worker_submit_windows: the caller copied each packet's first
    min(len, 80) bytes into registered staging (window i at i * stride); the
    GPU reads only the staging, bit-identical to the frames form."""
    cfg = (8, 8, 1, 0)
    sizes = [32, 1, 1024, 500, 0, 77, 1000]
    frames = synth_frames(oracle_mod, sum(sizes), 56 + stride)
    q_all, h_all, _, _ = expect_lists(oracle_mod, frames, cfg)
    lens = np.array([len(f) for f in frames], np.uint16)
    raw = np.zeros(len(frames) * stride + 128, np.uint8)
    win = raw[(-raw.ctypes.data) % 64:]                      # 64-byte aligned staging
    for i, f in enumerate(frames):
        w = bytes(f[:80])
        win[i * stride:i * stride + len(w)] = np.frombuffer(w, np.uint8)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(raw.ctypes.data, raw.nbytes)
        eng.worker_start(8, 2)
        off = 0
        for n in sizes:
            view = win[off * stride:]
            t = eng.worker_submit_windows(view, stride, lens[off:off + n])
            r = eng.worker_poll(t)
            qr = q_all[off:off + n]
            qi_ref, qs_ref = oracle_mod.process_burst(qr, cfg[1])
            check_lists(r, qr, h_all[off:off + n], qi_ref, qs_ref)
            off += n
        with pytest.raises(abi.YrssError):
            eng.worker_submit_windows(win, 0, lens[:4])       # stride below a window
        eng.worker_stop()
        eng.unregister_host_memory(raw.ctypes.data)


def test_worker_low_rate_no_stall(dev, oracle_mod, monkeypatch):
    """Fewer than B bursts per idle period: idle is judged over the whole
    ring, so no workgroup leaves while the others keep serving (its tickets
    would wait for the rest of the launch to go idle)."""
    monkeypatch.setenv("YRSS_WORKER_IDLE_MS", "20")
    cfg = (4, 4, 1, 1)
    nb, per, nburst = 8, 16, 40
    frames = synth_frames(oracle_mod, per * nburst, 77)
    pool, ptrs, _ = fake_mbufs(frames)
    q, h, _, _ = expect_lists(oracle_mod, frames, cfg)
    lat = []
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(nb, nb)
        for k in range(nburst):
            lo = per * k
            t = eng.worker_submit(ptrs[lo:lo + per])
            t0 = time.perf_counter()
            r = eng.worker_poll(t)
            lat.append(time.perf_counter() - t0)
            qi, qs = oracle_mod.process_burst(q[lo:lo + per], cfg[1])
            check_lists(r, q[lo:lo + per], h[lo:lo + per], qi, qs)
            time.sleep(0.005)        # each workgroup sees a burst every ~40 ms
        eng.worker_stop()
        eng.unregister_host_memory(pool.ctypes.data)
    # the first burst includes the launch; a stranded ticket would wait for the
    # rest of the launch to idle out (up to 20 ms); a served one takes ~20 us
    assert max(lat[1:]) < 0.010, sorted(lat)[-5:]


def test_worker_relaunch_nonblocking_poll(dev, oracle_mod, monkeypatch):
    """After the launch left, a poller that never blocks (wait=0) still gets
    the burst served: the poll relaunches."""
    monkeypatch.setenv("YRSS_WORKER_IDLE_MS", "2")
    cfg = (3, 3, 1, 1)
    frames = synth_frames(oracle_mod, 64, 78)
    pool, ptrs, _ = fake_mbufs(frames)
    q, h, qi, qs = expect_lists(oracle_mod, frames[:32], cfg)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(4, 4)
        for _ in range(3):
            t = eng.worker_submit(ptrs[:32])
            r, deadline = None, time.time() + 5.0
            while r is None and time.time() < deadline:
                r = eng.worker_poll(t, wait=False)
            assert r is not None
            check_lists(r, q, h, qi, qs)
            time.sleep(0.02)         # past the idle limit: every workgroup leaves
        eng.worker_stop()
        eng.unregister_host_memory(pool.ctypes.data)


def test_worker_then_device_batch(dev, oracle_mod, monkeypatch):
    """A device-resident batch on the same context retires the resident worker
    first (its CUs would otherwise stall the batch's grid until the worker
    idles out); tickets published before it are served after it."""
    monkeypatch.setenv("YRSS_WORKER_IDLE_MS", "3000")
    monkeypatch.setenv("YRSS_WORKER_LIFE_MS", "3000")
    cfg = (3, 3, 1, 1)
    frames = synth_frames(oracle_mod, 256, 91)
    pool, ptrs, _ = fake_mbufs(frames)
    q, h, _, _ = expect_lists(oracle_mod, frames, cfg)
    n = 1 << 20
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(128, 64)
        t_a = eng.worker_submit(ptrs[:128])
        assert eng.worker_poll(t_a) is not None          # the worker is resident now
        t_b = eng.worker_submit(ptrs[128:256])
        win, lens = eng.synth(2, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = eng.dispatch_dev(win, lens, 64, n)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert dt < 0.5, dt                               # not held up for the 3 s idle limit
        w_h = win[: 4096 * 64].cpu().numpy()
        l_h = lens[:4096].cpu().numpy().view(np.uint16)
        q_ref, h_ref = oracle_mod.dispatch_windows(w_h, 64, l_h, oracle_mod.cfg(*cfg))
        assert np.array_equal(res.q[:4096].cpu().numpy().view(np.int16), q_ref)
        assert np.array_equal(res.hash[:4096].cpu().numpy().view(np.uint32), h_ref)
        r = eng.worker_poll(t_b)                          # relaunched by the poll
        qi, qs = oracle_mod.process_burst(q[128:256], cfg[1])
        check_lists(r, q[128:256], h[128:256], qi, qs)
        eng.worker_stop()
        eng.unregister_host_memory(pool.ctypes.data)


def test_worker_direct_outputs(dev, oracle_mod):
    """Output arrays inside registered host memory are written by the GPU in
    place (the poll copies nothing); arrays outside go through the slot's
    staging; both match the oracle, also mixed within one burst.  A registered
    range a pending burst may touch cannot be unregistered (-EBUSY)."""
    cfg = (5, 4, 1, 1)
    sizes = [32, 1024, 7, 500, 32, 1]
    frames = synth_frames(oracle_mod, sum(sizes), 66)
    pool, ptrs, _ = fake_mbufs(frames)
    q_all, h_all, _, _ = expect_lists(oracle_mod, frames, cfg)
    lib = abi.load()
    arena = np.zeros(1 << 20, np.uint8)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.register_host_memory(arena.ctypes.data, arena.nbytes)
        eng.worker_start(8, 2)
        off, pend = 0, []
        nonlocal_pos = [0]
        for i, n in enumerate(sizes):
            m = max(n, 1)
            # even bursts: every output in the registered arena; odd: q and
            # qstart there, hash and qidx in plain (unregistered) arrays
            def take(nbytes, dtype):
                nonlocal_pos[0] = (nonlocal_pos[0] + 63) & ~63
                a = arena[nonlocal_pos[0]:nonlocal_pos[0] + nbytes].view(dtype)
                nonlocal_pos[0] += nbytes
                return a
            q = take(2 * m, np.int16)
            qs = take(4 * (cfg[1] + 2), np.uint32)
            if i % 2 == 0:
                h = take(4 * m, np.uint32)
                qi = take(4 * m, np.uint32)
            else:
                h = np.zeros(m, np.uint32)
                qi = np.zeros(m, np.uint32)
            t = ctypes.c_uint64()
            mb = np.ascontiguousarray(ptrs[off:off + n])
            assert lib.yrss_worker_submit(eng._ctx, mb.ctypes.data, n, q.ctypes.data,
                                          h.ctypes.data, qi.ctypes.data, qs.ctypes.data, 0,
                                          ctypes.byref(t)) == 0
            pend.append((t.value, off, n, q, h, qi, qs))
            off += n
        assert lib.yrss_unregister_host_memory(eng._ctx, arena.ctypes.data) == -16   # EBUSY
        for t, o, n, q, h, qi, qs in pend:
            assert lib.yrss_worker_poll(eng._ctx, t, 1) == 0
            qr = q_all[o:o + n]
            qi_ref, qs_ref = oracle_mod.process_burst(qr, cfg[1])
            assert np.array_equal(q[:n], qr) and np.array_equal(h[:n], h_all[o:o + n])
            assert np.array_equal(qi[:n], qi_ref)
            assert np.array_equal(qs[: qs_ref.size], qs_ref)
        eng.worker_stop()
        eng.unregister_host_memory(arena.ctypes.data)
        eng.unregister_host_memory(pool.ctypes.data)


@pytest.mark.parametrize("registered", [True, False])
def test_worker_per_slot_outputs(dev, oracle_mod, registered):
    """F-Stack's pattern: one fixed set of output arrays per ring slot, reused
    burst after burst (the workgroups then keep the slot's output addresses and
    skip reading them).  Sizes vary, so stale addresses or counts would show."""
    cfg = (6, 5, 1, 1)
    nslots, nblocks = 8, 2
    rng = np.random.default_rng(5)
    sizes = [int(x) for x in rng.integers(1, 300, 48)]
    frames = synth_frames(oracle_mod, sum(sizes), 88)
    pool, ptrs, _ = fake_mbufs(frames)
    q_all, h_all, _, _ = expect_lists(oracle_mod, frames, cfg)
    lib = abi.load()
    arena = np.zeros(nslots * 4096, np.uint8)
    outs = []
    for k in range(nslots):
        base = arena[k * 4096:(k + 1) * 4096]
        if registered:
            outs.append((base[0:600].view(np.int16), base[640:1840].view(np.uint32),
                         base[1856:3056].view(np.uint32), base[3072:3072 + 4 * 8].view(np.uint32)))
        else:
            outs.append((np.zeros(300, np.int16), np.zeros(300, np.uint32),
                         np.zeros(300, np.uint32), np.zeros(8, np.uint32)))
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.register_host_memory(arena.ctypes.data, arena.nbytes)
        eng.worker_start(nslots, nblocks)
        off, pend = 0, []
        for i, n in enumerate(sizes):
            if len(pend) == nslots:
                _check_slot(lib, eng, oracle_mod, pend.pop(0), q_all, h_all, cfg)
            q, h, qi, qs = outs[i % nslots]
            t = ctypes.c_uint64()
            mb = np.ascontiguousarray(ptrs[off:off + n])
            assert lib.yrss_worker_submit(eng._ctx, mb.ctypes.data, n, q.ctypes.data,
                                          h.ctypes.data, qi.ctypes.data, qs.ctypes.data, 0,
                                          ctypes.byref(t)) == 0
            pend.append((t.value, off, n, outs[i % nslots]))
            off += n
        while pend:
            _check_slot(lib, eng, oracle_mod, pend.pop(0), q_all, h_all, cfg)
        eng.worker_stop()
        eng.unregister_host_memory(arena.ctypes.data)
        eng.unregister_host_memory(pool.ctypes.data)


def _check_slot(lib, eng, oracle_mod, item, q_all, h_all, cfg):
    t, o, n, (q, h, qi, qs) = item
    assert lib.yrss_worker_poll(eng._ctx, t, 1) == 0
    qr = q_all[o:o + n]
    qi_ref, qs_ref = oracle_mod.process_burst(qr, cfg[1])
    assert np.array_equal(q[:n], qr) and np.array_equal(h[:n], h_all[o:o + n]), t
    assert np.array_equal(qi[:n], qi_ref) and np.array_equal(qs[: qs_ref.size], qs_ref), t


# ---- a full-grid batch from another context or process beside a resident
# worker: the chip is shared (the batch's workgroups take the CUs the worker
# leaves free), the batch never waits for the worker's idle or lifetime exit.
# A device-wide yield (worker leaves on a shared epoch, relaunch gated) was
# built and measured: no gain for the batch, a slower next burst
# (profiles/r02_v4_worker_yield_ab.log); it is not in the build. ----

def _batch_ms(eng, win, lens, n, reps=3, filt=False):
    """Wall time of one 2^24-packet device batch (dispatch + synchronize)."""
    best = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.dispatch_dev(win, lens, 64, n, want_filter=filt)
        torch.cuda.synchronize()
        best.append((time.perf_counter() - t0) * 1e3)
    return min(best)


def test_device_batch_beside_other_contexts_worker(dev, oracle_mod, monkeypatch):
    """Context A's worker (idle exit 8 s, lifetime 10 s) holds 128 CUs; context
    B's 2^24-packet batch (KNI-filter parse kernel, the largest LDS footprint)
    finishes within a few ms, not after the worker's 8 s idle exit, and A's
    bursts before and after are bit-exact."""
    monkeypatch.setenv("YRSS_WORKER_IDLE_MS", "8000")
    monkeypatch.setenv("YRSS_WORKER_LIFE_MS", "10000")
    cfg = (3, 3, 1, 1)
    frames = synth_frames(oracle_mod, 256, 21)
    pool, ptrs, _ = fake_mbufs(frames)
    q, h, _, _ = expect_lists(oracle_mod, frames, cfg)
    n = 1 << 24
    with SoftRss(*cfg, device=0, max_burst=0) as b_eng, \
            SoftRss(*cfg, device=0, max_burst=0) as a_eng:
        win, lens = b_eng.synth(abi.SYN_UDP4, n)
        b_eng.set_kni(True, "reject", "80,443", "53")
        b_eng.dispatch_dev(win, lens, 64, n, want_filter=True)
        solo = _batch_ms(b_eng, win, lens, n, filt=True)
        a_eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        a_eng.worker_start(512, 128)
        r = a_eng.worker_poll(a_eng.worker_submit(ptrs[:128]))   # resident now
        check_lists(r, q[:128], h[:128], *oracle_mod.process_burst(q[:128], 3))
        shared = _batch_ms(b_eng, win, lens, n, reps=1, filt=True)
        assert shared < solo + 5.0, (solo, shared)
        r = a_eng.worker_poll(a_eng.worker_submit(ptrs[128:256]))
        check_lists(r, q[128:], h[128:], *oracle_mod.process_burst(q[128:], 3))
        a_eng.worker_stop()
        a_eng.unregister_host_memory(pool.ctypes.data)


_CHILD = r"""
import os, sys, time
sys.path[:0] = [sys.argv[1], os.path.join(sys.argv[1], "tests")]
os.environ["YRSS_WORKER_IDLE_MS"] = "8000"
os.environ["YRSS_WORKER_LIFE_MS"] = "10000"
import numpy as np
from oracle import oracle
from yastack_amd import SoftRss
from hostbufs import check_lists, expect_lists, fake_mbufs, synth_frames
frames = synth_frames(oracle, 128, 33)
pool, ptrs, _ = fake_mbufs(frames)
q, h, _, _ = expect_lists(oracle, frames, (3, 3, 1, 1))
with SoftRss(3, 3, 1, 1, device=0, max_burst=0) as eng:
    eng.register_host_memory(pool.ctypes.data, pool.nbytes)
    eng.worker_start(512, 128)
    check_lists(eng.worker_poll(eng.worker_submit(ptrs[:64])), q[:64], h[:64],
                *oracle.process_burst(q[:64], 3))
    print("ready", flush=True)
    sys.stdin.readline()
    check_lists(eng.worker_poll(eng.worker_submit(ptrs[64:])), q[64:], h[64:],
                *oracle.process_burst(q[64:], 3))
    eng.worker_stop()
    eng.unregister_host_memory(pool.ctypes.data)
print("ok", flush=True)
"""


def test_device_batch_beside_other_process_worker(dev):
    """The same with the worker in another process."""
    import subprocess
    import sys
    from pathlib import Path

    root = str(Path(__file__).resolve().parent.parent)
    n = 1 << 24
    with SoftRss(3, 3, 1, 1, device=0, max_burst=0) as eng:
        win, lens = eng.synth(abi.SYN_UDP4, n)
        eng.dispatch_dev(win, lens, 64, n)
        solo = _batch_ms(eng, win, lens, n)
        p = subprocess.Popen([sys.executable, "-c", _CHILD, root], stdin=subprocess.PIPE,
                             stdout=subprocess.PIPE, text=True)
        try:
            assert p.stdout.readline().strip() == "ready"
            shared = _batch_ms(eng, win, lens, n, reps=1)
            p.stdin.write("go\n")
            p.stdin.flush()
            assert p.stdout.readline().strip() == "ok"
            assert p.wait(timeout=60) == 0
        finally:
            if p.poll() is None:
                p.kill()
        assert shared < solo + 5.0, (solo, shared)


def test_worker_guard_fault_is_per_burst(dev, oracle_mod):
    """A list guard that fires in one worker burst fails that burst alone
    (-EIO), with several bursts of other workgroups in flight at once; the
    record names it and the bursts around it stay bit-exact (ADVICE r03:
    the context-wide record used to be taken by whichever poll came first).
    Driven through libyrss_test.so's yrss_debug_worker_inject (the shipping
    library has no injection path)."""
    import errno

    cfg = (8, 8, 1, 0)
    nb, per = 12, 40
    frames = synth_frames(oracle_mod, nb * per, 77)
    pool, ptrs, _ = fake_mbufs(frames)
    q_all, h_all, _, _ = expect_lists(oracle_mod, frames, cfg)
    with SoftRss(*cfg, device=0, max_burst=0, lib_path=str(abi.TEST_LIB_PATH)) as eng:
        assert eng._lib.yrss_debug_worker_inject(eng._ctx, 5) == 0   # ticket 5 fires a guard
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(16, 4)
        tickets = [eng.worker_submit(ptrs[i * per:(i + 1) * per]) for i in range(nb)]
        for i, t in enumerate(tickets):
            q = q_all[i * per:(i + 1) * per]
            if t == 5:
                with pytest.raises(abi.YrssError) as ei:
                    eng.worker_poll(t)
                assert ei.value.errno == errno.EIO
                continue
            r = eng.worker_poll(t)
            qi, qs = oracle_mod.process_burst(q, cfg[1])
            check_lists(r, q, h_all[i * per:(i + 1) * per], qi, qs)
        code, kernel, where, value = eng.fault_info()
        assert (code, kernel, where, value) == (abi.FAULT_LIST_RANGE, abi.K_WORKER, 5, 0xdead)
        assert eng.fault_info()[0] == abi.FAULT_NONE
        # later bursts are unaffected
        t = eng.worker_submit(ptrs[:per])
        qi, qs = oracle_mod.process_burst(q_all[:per], cfg[1])
        check_lists(eng.worker_poll(t), q_all[:per], h_all[:per], qi, qs)
        eng.worker_stop()
        eng.unregister_host_memory(pool.ctypes.data)
