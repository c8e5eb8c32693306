"""GPU parity of the parse kernels at hashes chosen for the modulo, and under
short RSS keys.

The parse kernel computes hash % d as a mask where d is a power of two and as
a reciprocal multiplication (fastmod) elsewhere (yrss.hip, process_tile).  The
values that break either (0, d - 1, d, the largest multiple of d below 2^32
and its neighbours, 2^32 - 1) essentially never occur in synthetic traffic,
so the frames here are solved for them (rss_tuples.py).  Every expectation is
computed twice: in Python integers from the target hash, and by the oracle.
"""
import numpy as np
import pytest

from frames import ethertype_frame, ipv4_frame
from rss_tuples import edge_hashes, solve_tuple, tcp_frame_for_tuple, window_rank

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from yastack_amd import SoftRss, abi  # noqa: E402

from gpu_checks import dev, to_np  # noqa: E402,F401

KEY2 = bytes(range(7, 47))
N_DIRECTED = 300


def _targets(d):
    """edge_hashes(d); for a small d also every remainder class at both ends of
    the range, so that each queue of the modulo receives a packet."""
    hs = set(edge_hashes(d))
    if d <= 10:
        m = (2**32 - 1) // d * d
        hs |= set(range(d)) | {v for v in range(m - d, m + d) if v < 2**32}
    return sorted(hs)


def _directed_burst(oracle_mod, d, ihl=5, length=64, n=N_DIRECTED):
    """n frames: TCP frames whose hashes walk _targets(d), with a UDP frame and
    an ARP frame in every 50 (queues 2 and 0, unhashed).  Returns (frames, the
    target hash of each or None)."""
    targets = _targets(d)
    rng = np.random.default_rng(d * 16 + ihl)
    tcp = []
    for h in targets:
        base = bytes(rng.integers(0, 256, 12, dtype=np.uint8))
        tcp.append(tcp_frame_for_tuple(solve_tuple(oracle_mod.MLX_KEY, 40, h, base=base),
                                       ihl=ihl, length=length))
    assert len(tcp) < n - n // 25
    frames, hs, k = [], [], 0
    for i in range(n):
        if i % 50 == 7:
            frames.append(ipv4_frame("10.1.2.3", 53, "10.3.2.1", 5353, proto=17, ihl=ihl,
                                     length=length))
            hs.append(None)
        elif i % 50 == 31:
            frames.append(ethertype_frame(0x0806, length=length))
            hs.append(None)
        else:
            frames.append(tcp[k % len(tcp)])
            hs.append(targets[k % len(tcp)])
            k += 1
    return frames, hs


def _py_lists(q, nq):
    """process_packets' per-queue FIFO lists in plain Python."""
    buckets = [[] for _ in range(nq + 1)]
    for i, v in enumerate(q):
        buckets[v if 0 <= v < nq else nq].append(i)
    qstart = [0]
    for b in buckets:
        qstart.append(qstart[-1] + len(b))
    return np.array([i for b in buckets for i in b], np.uint32), np.array(qstart, np.uint32)


def _expectation(oracle_mod, frames, hs, length, stride, cfg_tuple, d, key=None):
    """(q, hash, qidx, qstart) from Python integers, checked against the oracle's
    account of the same windows; also that the input holds what it aims at."""
    npr, nq, soft, only = cfg_tuple
    n = len(frames)
    w = np.stack([np.frombuffer(f[:stride], np.uint8) for f in frames])
    l_h = np.full(n, length, np.uint16)
    c = oracle_mod.cfg(npr, nq, soft, only) if key is None else \
        oracle_mod.cfg(npr, nq, soft, only, key=key)
    q_ref, h_ref = oracle_mod.dispatch_windows(w.reshape(-1), stride, l_h, c)
    one = [oracle_mod.toeplitz_dispatch(f, length, c) for f in frames]     # bit-serial engine
    q_py = np.array([2 if h is None else h % d + only for h in hs], np.int16)
    q_py[[i for i, f in enumerate(frames) if f[12:14] == b"\x08\x06"]] = 0
    h_py = np.array([0 if h is None else h for h in hs], np.uint32)
    assert np.array_equal(q_ref, q_py) and np.array_equal(h_ref, h_py)
    assert [x for x, _ in one] == q_py.tolist() and [y for _, y in one] == h_py.tolist()
    qi_ref, qs_ref = oracle_mod.process_burst(q_ref, nq)
    qi_py, qs_py = _py_lists(q_py.tolist(), nq)
    assert np.array_equal(qi_ref, qi_py) and np.array_equal(qs_ref, qs_py)
    # the edges are in the input: every target hash, nothing truncated, the
    # unhashed queues 2 and 0, and the remainder classes the modulo can get wrong
    hashed = [h for h in hs if h is not None]
    assert set(hashed) == set(_targets(d)) and not np.any(q_ref == abi.Q_TRUNCATED)
    assert sum(h is None for h in hs) == 2 * (n // 50)
    assert np.any((q_ref == 2) & (h_ref == 0)) and np.any((q_ref == 0) & (h_ref == 0))
    rem = {h % d for h in hashed}
    assert {0, 1 % d, d - 1} <= rem
    if d <= 10:
        assert rem == set(range(d))
    return w, l_h, (q_py, h_py, qi_py, qs_py)


def _dev_result(eng, w, l_h, stride):
    n = l_h.size
    win = torch.from_numpy(w.reshape(-1).copy()).cuda()
    lens = torch.from_numpy(l_h.view(np.int16).copy()).cuda()
    res = eng.dispatch_dev(win, lens, stride, n)
    torch.cuda.synchronize()
    assert eng.status() == 0
    return (to_np(res.q[:n], np.int16), to_np(res.hash[:n], np.uint32),
            to_np(res.qidx[:n], np.uint32), to_np(res.qstart, np.uint32))


def _same(got, want, what):
    for name, g, w in zip(("q", "hash", "qidx", "qstart"), got, want):
        g = np.asarray(g)
        bad = np.nonzero(g != w)[0]
        assert bad.size == 0, f"{what}: {name} differs at {bad[:5]}: {g[bad[:5]]} vs {w[bad[:5]]}"


@pytest.mark.parametrize("nb_procs,only", [(3, 1), (4, 1), (6, 0), (7, 0), (8, 0), (10, 1),
                                           (255, 0), (258, 1), (4095, 0), (4096, 0), (4096, 1)])
def test_directed_modulo(dev, oracle_mod, nb_procs, only):
    """hash % (nb_procs - dispatch_only_core) at the ends of its range: the mask
    (d a power of two) and fastmod (every other d), in the one-launch kernel,
    in the grid parse kernel + scatter, and through the host frames call."""
    d = nb_procs - only
    cfg_tuple = (nb_procs, min(nb_procs, 256), 1, only)
    assert window_rank(oracle_mod.MLX_KEY, 40) == 32
    frames, hs = _directed_burst(oracle_mod, d)
    w, l_h, want = _expectation(oracle_mod, frames, hs, 64, 64, cfg_tuple, d)
    for one_launch in (0, 2):       # one launch where nb_queues allows it / never
        with SoftRss(*cfg_tuple, device=0, max_burst=0) as eng:
            eng.set_tuning(one_launch=one_launch)
            _same(_dev_result(eng, w, l_h, 64), want, f"dispatch_dev one_launch={one_launch}")
            if one_launch == 0:
                r = eng.dispatch_frames([f[:64] for f in frames])
                _same((r.q, r.hash, r.qidx, r.qstart), want, "dispatch_frames")
                assert eng.status() == 0


@pytest.mark.parametrize("ihl", [12, 15])
def test_directed_modulo_ihl_tail(dev, oracle_mod, ihl):
    """IHL >= 12: the ports lie past byte 64 and are fetched by the rare global
    load.  The same directed hashes for d = 7, 100-byte frames in 80-byte
    windows: every TCP packet is hashed and nothing is truncated."""
    cfg_tuple, d = (7, 7, 1, 0), 7
    frames, hs = _directed_burst(oracle_mod, d, ihl=ihl, length=100)
    assert all(len(f) == 100 for f in frames)
    w, l_h, want = _expectation(oracle_mod, frames, hs, 100, 80, cfg_tuple, d)
    assert np.count_nonzero(want[1]) >= sum(h not in (None, 0) for h in hs) > 200
    for one_launch in (0, 2):
        with SoftRss(*cfg_tuple, device=0, max_burst=0) as eng:
            eng.set_tuning(one_launch=one_launch)
            _same(_dev_result(eng, w, l_h, 80), want, f"ihl {ihl} one_launch={one_launch}")


@pytest.mark.parametrize("kl", [4, 5, 15, 16, 39])
def test_short_keys_parse_kernels(dev, oracle_mod, kl):
    """rss_key_len below 40 through both parse kernels: key bits past the
    length are zero.  A tuple consumes key bytes 0..15, so 16 and 39 hash as
    40 does and anything shorter does not."""
    cfg_tuple, stride = (8, 8, 1, 0), 80
    key = KEY2[:kl]
    c = oracle_mod.cfg(*cfg_tuple, key=key)
    c_full = oracle_mod.cfg(*cfg_tuple, key=KEY2)
    for one_launch, cut in ((2, None), (0, 3000)):
        with SoftRss(*cfg_tuple, rss_key=key, device=0, max_burst=0) as eng:
            assert eng.cfg.rss_key_len == kl
            eng.set_tuning(one_launch=one_launch)
            for profile, n in ((abi.SYN_TCP4, 10000), (abi.SYN_FUZZ, 5000)):
                win, lens = eng.synth(profile, n, stride=stride)
                n = n if cut is None else cut
                res = eng.dispatch_dev(win, lens, stride, n)
                torch.cuda.synchronize()
                assert eng.status() == 0
                w_h = win[: n * stride].cpu().numpy()
                l_h = to_np(lens[:n], np.uint16)
                q_ref, h_ref = oracle_mod.dispatch_windows(w_h, stride, l_h, c)
                _, h_full = oracle_mod.dispatch_windows(w_h, stride, l_h, c_full)
                hashed = h_full != 0
                assert hashed.sum() > n // 4
                if kl >= 16:
                    assert np.array_equal(h_ref, h_full)
                else:
                    assert (h_ref[hashed] != h_full[hashed]).mean() > 0.9   # (15/16 at 15)
                qi_ref, qs_ref = oracle_mod.process_burst(q_ref, cfg_tuple[1])
                got = (to_np(res.q[:n], np.int16), to_np(res.hash[:n], np.uint32),
                       to_np(res.qidx[:n], np.uint32), to_np(res.qstart, np.uint32))
                _same(got, (q_ref, h_ref, qi_ref, qs_ref),
                      f"key length {kl} profile {profile} one_launch={one_launch}")
