"""GPU parity: the HIP path (through the C ABI) against the oracle, bit-exact.

Every test here runs on a real MI355X (`-m gpu`).  Inputs are generated on the
device by yrss_synth_dev and on the host by the oracle from the same header
(include/yrss_synth.h); both sides are compared packet by packet: queue, hash,
per-queue FIFO lists.  Full BASELINE sizes (2^24 packets) are compared in full
— the C oracle finishes them in about a second.
"""
import ctypes
import json

import numpy as np
import pytest

from frames import ethertype_frame, ipv4_frame

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_checks import dev, run_and_compare, to_np  # noqa: E402,F401
from hostbufs import fake_mbufs, synth_frames  # noqa: E402
from yastack_amd import SoftRss, abi  # noqa: E402

CONFIGS = [
    (3, 3, 1, 1),     # fs/config/config.ini: lcore_mask=7, dispatch_only_core=1
    (8, 8, 1, 0),
    (1, 1, 1, 0),     # every hashed packet → q 0; q=2 packets dropped
    (5, 2, 0, 1),     # soft_dispatch=0: dispatch_only_core ignored; nb_queues < nb_procs
    (4096, 256, 1, 1),
    (2, 3, 1, 1),     # nb_procs-1 == 1: hash % 1
]


@pytest.mark.parametrize("cfg_tuple", CONFIGS)
@pytest.mark.parametrize("profile", range(7))
def test_profiles_configs(dev, oracle_mod, cfg_tuple, profile):
    npr, nq, soft, only = cfg_tuple
    with SoftRss(npr, nq, soft, only, device=0, max_burst=0) as eng:
        run_and_compare(eng, oracle_mod, cfg_tuple, profile, 70001, 80, first=12345)


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 255, 257, 1023, 4097, 100003])
def test_ragged_sizes(dev, oracle_mod, n):
    with SoftRss(8, 8, 1, 0, device=0, max_burst=0) as eng:
        run_and_compare(eng, oracle_mod, (8, 8, 1, 0), abi.SYN_FUZZ, n, 80)
        run_and_compare(eng, oracle_mod, (8, 8, 1, 0), abi.SYN_TCP4, n, 64)


def test_empty_batch(dev):
    with SoftRss(3, device=0, max_burst=0) as eng:
        win = torch.zeros(64, dtype=torch.uint8, device=dev)
        lens = torch.zeros(1, dtype=torch.int16, device=dev)
        out = eng.alloc_out(0, dev)
        out.qstart.fill_(-1)
        eng.dispatch_dev(win, lens, 64, 0, out=out)
        torch.cuda.synchronize()
        assert out.qstart.cpu().tolist() == [0] * 5
        r = eng.dispatch_frames([])
        assert r.q.size == 0 and list(r.qstart) == [0] * 5


@pytest.mark.parametrize("stride", [64, 80, 96, 128, 2176])
def test_strides(dev, oracle_mod, stride):
    with SoftRss(8, 8, 1, 0, device=0, max_burst=0) as eng:
        for profile in (abi.SYN_FUZZ, abi.SYN_IMIX, abi.SYN_JUMBO_TCP4):
            run_and_compare(eng, oracle_mod, (8, 8, 1, 0), profile, 20000, stride)


def test_truncated_window_flagged(dev, oracle_mod):
    # stride 64 cannot hold ports of IHL>=12 packets longer than 64 bytes
    frames, lens = [], []
    for ihl in range(5, 16):
        for L in (64, 70, 80, 1500):
            frames.append(ipv4_frame("10.0.0.1", 12345, "10.0.0.2", 80, ihl=ihl, length=L))
            lens.append(L)
    n = len(frames)
    w = np.zeros((n, 64), np.uint8)
    for i, f in enumerate(frames):
        w[i] = np.frombuffer(f[:64], np.uint8)
    l_h = np.array(lens, np.uint16)
    c = oracle_mod.cfg(8, 8, 1, 0)
    q_ref, h_ref = oracle_mod.dispatch_windows(w.reshape(-1), 64, l_h, c)
    assert (q_ref == abi.Q_TRUNCATED).sum() > 0
    with SoftRss(8, 8, 1, 0, device=0, max_burst=0) as eng:
        win = torch.from_numpy(w.reshape(-1)).to(dev)
        lt = torch.from_numpy(l_h.view(np.int16)).to(dev)
        res = eng.dispatch_dev(win, lt, 64, n)
        torch.cuda.synchronize()
        assert np.array_equal(to_np(res.q[:n], np.int16), q_ref)
        assert np.array_equal(to_np(res.hash[:n], np.uint32), h_ref)
        # the host API stages 80-byte windows when needed, so never truncates
        r = eng.dispatch_frames([f[:L] for f, L in zip(frames, lens)])
        full = [oracle_mod.toeplitz_dispatch(f, L, c) for f, L in zip(frames, lens)]
        assert list(r.q) == [q for q, _ in full]
        assert list(r.hash) == [h for _, h in full]


def test_survey_kat_on_gpu(dev, golden_dir):
    g = json.loads((golden_dir / "survey_kat.json").read_text())
    for cname, (npr, nq, soft, only) in g["configs"].items():
        with SoftRss(npr, nq, soft, only, device=0) as eng:
            cases = [c for c in g["cases"] if cname in c["expect"]]
            frames = [bytes.fromhex(c["frame"])[: c["len"]] for c in cases]
            r = eng.dispatch_frames(frames)
            for c, q, h in zip(cases, r.q, r.hash):
                assert q == c["expect"][cname], (c["name"], cname)
                if cname == "np8" and "hash" in c["expect"]:
                    assert h == c["expect"]["hash"], c["name"]


@pytest.mark.parametrize("name", ["udp4_1flow", "udp4", "imix", "vlan6_tcp", "jumbo_tcp4",
                                  "tcp4", "fuzz"])
def test_golden_fixtures_on_gpu(dev, golden_dir, name):
    d = np.load(golden_dir / f"synth_{name}.npz")
    seed, profile, nflows, stride = (int(x) for x in d["meta"])
    n = d["len"].size
    for cname, (npr, nq, soft, only) in {"np8": (8, 8, 1, 0), "ini": (3, 3, 1, 1)}.items():
        with SoftRss(npr, nq, soft, only, device=0, max_burst=0) as eng:
            win, lens = eng.synth(profile, n, 0, seed, nflows, stride)
            assert np.array_equal(win.cpu().numpy().reshape(n, stride), d["win"])
            res = eng.dispatch_dev(win, lens, stride, n)
            torch.cuda.synchronize()
            assert np.array_equal(to_np(res.q[:n], np.int16), d[f"q_{cname}"])
            assert np.array_equal(to_np(res.hash[:n], np.uint32), d[f"hash_{cname}"])
            assert np.array_equal(to_np(res.qidx[:n], np.uint32), d[f"qidx_{cname}"])
            assert np.array_equal(to_np(res.qstart, np.uint32), d[f"qstart_{cname}"])


def test_edge_frames_host_api(dev, oracle_mod):
    base = ("10.0.0.1", 12345, "10.0.0.2", 80)
    frames, lens = [], []
    for L in list(range(0, 82)) + [1500, 2048, 65535]:
        for ihl in (0, 1, 4, 5, 6, 11, 12, 15):
            f = ipv4_frame(*base, ihl=ihl, length=max(L, 80), pad_to=80)
            frames.append(f)
            lens.append(L)
    for et in (0x0806, 0x8035, 0x86DD, 0x8100, 0x88A8, 0x88F7, 0x8809, 0x6558, 0x88CC, 0x1234):
        frames.append(ethertype_frame(et))
        lens.append(64)
    for proto in (17, 4, 1, 0, 255):
        frames.append(ipv4_frame(*base, proto=proto))
        lens.append(64)
    c = oracle_mod.cfg(8, 8, 1, 0)
    want = [oracle_mod.toeplitz_dispatch(f, L, c) for f, L in zip(frames, lens)]
    with SoftRss(8, 8, 1, 0, device=0) as eng:
        # frames API gets exactly len bytes (padded buffers beyond len are not read)
        bufs = [f if L > len(f) else f[:L] for f, L in zip(frames, lens)]
        big = [f + bytes(L - len(f)) if L > len(f) else f for f, L in zip(bufs, lens)]
        r = eng.dispatch_frames(big)
        assert list(r.q) == [q for q, _ in want]
        assert list(r.hash) == [h for _, h in want]
        qi_ref, qs_ref = oracle_mod.process_burst(np.array([q for q, _ in want], np.int16), 8)
        assert np.array_equal(r.qidx, qi_ref) and np.array_equal(r.qstart, qs_ref)


def test_burst_api_mbufs(dev, oracle_mod):
    frames = synth_frames(oracle_mod, 3000, 0)
    pool, ptrs, stride = fake_mbufs(frames)
    c = oracle_mod.cfg(3, 3, 1, 1)
    want = [oracle_mod.toeplitz_dispatch(f, len(f), c) for f in frames]
    with SoftRss(3, 3, 1, 1, device=0, max_burst=1024) as eng:   # grows past max_burst
        r = eng.dispatch_burst(ptrs, write_rss=True)
        assert list(r.q) == [q for q, _ in want]
        assert list(r.hash) == [h for _, h in want]
        for i in range(0, 3000, 97):
            rss = int(np.frombuffer(pool[i * stride + 44: i * stride + 48].tobytes(), np.uint32)[0])
            assert rss == want[i][1]


@pytest.mark.parametrize("profile,nflows", [(abi.SYN_UDP4, 1 << 20), (abi.SYN_TCP4, 1 << 20),
                                            (abi.SYN_IMIX, 1 << 20), (abi.SYN_FUZZ, 1 << 20),
                                            (abi.SYN_VLAN6_TCP, 1 << 22),
                                            (abi.SYN_JUMBO_TCP4, 1 << 24)])
def test_full_size_bit_exact(dev, oracle_mod, profile, nflows):
    """BASELINE size (2^24 packets/GPU) compared packet-for-packet, configs[3] and
    configs[4] with their own flow counts (4M, 16M)."""
    n = 1 << 24
    with SoftRss(3, 3, 1, 1, device=0, max_burst=0) as eng:
        stride = 64
        win, lens = eng.synth(profile, n, 0, nflows=nflows, stride=stride)
        res = eng.dispatch_dev(win, lens, stride, n)
        torch.cuda.synchronize()
        c = oracle_mod.cfg(3, 3, 1, 1)
        q_ref, h_ref = oracle_mod.dispatch_windows(win.cpu().numpy(), stride,
                                                   to_np(lens[:n], np.uint16), c)
        assert np.array_equal(to_np(res.q[:n], np.int16), q_ref)
        assert np.array_equal(to_np(res.hash[:n], np.uint32), h_ref)
        qi_ref, qs_ref = oracle_mod.process_burst(q_ref, 3)
        assert np.array_equal(to_np(res.qstart, np.uint32), qs_ref)
        assert np.array_equal(to_np(res.qidx[:n], np.uint32), qi_ref)


def test_per_queue_properties_large(dev):
    """Size-independent invariants at 2^25 packets: permutation, FIFO order,
    counts equal the q histogram."""
    n = 1 << 25
    with SoftRss(8, 6, 1, 0, device=0, max_burst=0) as eng:
        win, lens = eng.synth(abi.SYN_IMIX, n, 7, stride=64)
        res = eng.dispatch_dev(win, lens, 64, n)
        torch.cuda.synchronize()
        q = res.q[:n].long()
        b = torch.where((q >= 0) & (q < 6), q, torch.full_like(q, 6))
        counts = torch.bincount(b, minlength=7)
        qs = res.qstart.long()
        assert torch.equal(qs[1:] - qs[:-1], counts)
        qi = res.qidx[:n].long()
        # each bucket strictly increasing (FIFO) and bucket ids consistent
        bk = torch.repeat_interleave(torch.arange(7, device=dev), counts)
        assert torch.equal(b[qi], bk)
        inc = qi[1:] > qi[:-1]
        same = bk[1:] == bk[:-1]
        assert bool(torch.all(inc | ~same))
        assert torch.equal(torch.sort(qi).values, torch.arange(n, device=dev))


def test_no_compaction_path(dev, oracle_mod):
    with SoftRss(8, 8, 1, 0, device=0, max_burst=0) as eng:
        run_and_compare(eng, oracle_mod, (8, 8, 1, 0), abi.SYN_FUZZ, 50000, 80, compact=False)
        out = eng.alloc_out(1000, dev, want_hash=False, compact=False)
        win, lens = eng.synth(abi.SYN_TCP4, 1000)
        eng.dispatch_dev(win, lens, 64, 1000, out=out, compact=False)
        torch.cuda.synchronize()
        c = oracle_mod.cfg(8, 8, 1, 0)
        q_ref, _ = oracle_mod.dispatch_windows(win.cpu().numpy(), 64,
                                               to_np(lens[:1000], np.uint16), c)
        assert np.array_equal(to_np(out.q[:1000], np.int16), q_ref)


def test_custom_key(dev, oracle_mod):
    key = bytes(range(7, 47))
    with SoftRss(8, 8, 1, 0, rss_key=key, device=0, max_burst=0) as eng:
        win, lens = eng.synth(abi.SYN_TCP4, 10000, stride=64)
        res = eng.dispatch_dev(win, lens, 64, 10000)
        torch.cuda.synchronize()
        c = oracle_mod.cfg(8, 8, 1, 0, key=key)
        q_ref, h_ref = oracle_mod.dispatch_windows(win.cpu().numpy(), 64,
                                                   to_np(lens[:10000], np.uint16), c)
        assert np.array_equal(to_np(res.hash[:10000], np.uint32), h_ref)
        assert np.array_equal(to_np(res.q[:10000], np.int16), q_ref)


def test_bad_args_rejected(dev):
    with SoftRss(3, device=0, max_burst=0) as eng:
        win, lens = eng.synth(abi.SYN_UDP4, 100)
        out = eng.alloc_out(100, dev)
        lib = abi.load()
        for stride in (0, 48, 72):
            rc = lib.yrss_dispatch_dev(eng._ctx, win.data_ptr(), stride, lens.data_ptr(), 100,
                                       out.q.data_ptr(), None, None, None, None)
            assert rc < 0
        rc = lib.yrss_dispatch_dev(eng._ctx, win.data_ptr() + 4, 64, lens.data_ptr(), 100,
                                   out.q.data_ptr(), None, None, None, None)
        assert rc < 0


def test_timing_hook(dev):
    with SoftRss(3, device=0, max_burst=0) as eng:
        win, lens = eng.synth(abi.SYN_UDP4, 1 << 20)
        eng.timing_enable((1 << abi.K_PARSE_HASH) | (1 << abi.K_SCATTER))
        for _ in range(3):
            eng.dispatch_dev(win, lens, 64)
        ms, cnt = eng.timing_read(abi.K_PARSE_HASH)
        assert cnt == 3 and ms > 0
        ms2, cnt2 = eng.timing_read(abi.K_SCAN)   # not in the mask
        assert cnt2 == 0
        ms3, cnt3 = eng.timing_read(abi.K_SCATTER)
        assert cnt3 == 3 and ms3 > 0
        eng.timing_enable(0)


@pytest.mark.parametrize("headroom", [128, 131, 134])
def test_burst_zero_copy(dev, oracle_mod, headroom):
    """yrss_dispatch_burst_zc: the GPU reads rte_mbuf headers and data from
    registered host memory (any data alignment), writes hash.rss back."""
    frames = synth_frames(oracle_mod, 5000, 11)
    pool, ptrs, stride = fake_mbufs(frames, headroom=headroom)
    c = oracle_mod.cfg(5, 4, 1, 1)
    want = [oracle_mod.toeplitz_dispatch(f, len(f), c) for f in frames]
    with SoftRss(5, 4, 1, 1, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        r = eng.dispatch_burst_zc(ptrs, write_rss=True)
        assert list(r.q) == [q for q, _ in want]
        assert list(r.hash) == [h for _, h in want]
        qi_ref, qs_ref = oracle_mod.process_burst(np.array([q for q, _ in want], np.int16), 4)
        assert np.array_equal(r.qidx, qi_ref) and np.array_equal(r.qstart, qs_ref)
        rss = pool.reshape(-1, stride)[:, 44:48].copy().view(np.uint32).ravel()
        assert rss.tolist() == [h for _, h in want]
        # a pointer outside every registered range is reported, not dereferenced
        bad = ptrs.copy()
        bad[17] = np.uint64(pool.ctypes.data + pool.nbytes + 4096)
        with pytest.raises(abi.YrssError):
            eng.dispatch_burst_zc(bad)
        eng.unregister_host_memory(pool.ctypes.data)


def test_frames_zero_copy(dev, oracle_mod):
    """yrss_dispatch_frames_zc with arrays both staged and registered in place."""
    frames = synth_frames(oracle_mod, 7000, 21)
    pool, ptrs, stride = fake_mbufs(frames, headroom=130)
    data = (ptrs + np.uint64(128 + 130)).astype(np.uint64)
    flen = np.array([len(f) for f in frames], np.uint16)
    c = oracle_mod.cfg(8, 8, 1, 0)
    want = [oracle_mod.toeplitz_dispatch(f, len(f), c) for f in frames]
    raw = np.zeros(7000 * 24 + 8192, np.uint8)           # page-aligned arena for in-place arrays
    off = (-raw.ctypes.data) % 4096
    arena = raw[off: off + 7000 * 24 + 4096]
    a_data = arena[:7000 * 8].view(np.uint64)
    a_len = arena[7000 * 8: 7000 * 10].view(np.uint16)
    a_q = arena[7000 * 10: 7000 * 12].view(np.int16)
    a_h = arena[7000 * 12: 7000 * 16].view(np.uint32)
    a_data[:] = data
    a_len[:] = flen
    lib = abi.load()
    with SoftRss(8, 8, 1, 0, device=0, max_burst=0) as eng:
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        # 1) pageable arrays: staged
        q = np.empty(7000, np.int16)
        h = np.empty(7000, np.uint32)
        rc = lib.yrss_dispatch_frames_zc(eng._ctx, data.ctypes.data, flen.ctypes.data, 7000,
                                         q.ctypes.data, h.ctypes.data, None, None)
        assert rc == 0
        assert q.tolist() == [x for x, _ in want] and h.tolist() == [y for _, y in want]
        # 2) registered arrays: read and written in place by the GPU / DMA
        eng.register_host_memory(arena.ctypes.data, arena.nbytes)
        rc = lib.yrss_dispatch_frames_zc(eng._ctx, a_data.ctypes.data, a_len.ctypes.data, 7000,
                                         a_q.ctypes.data, a_h.ctypes.data, None, None)
        assert rc == 0
        assert a_q.tolist() == [x for x, _ in want] and a_h.tolist() == [y for _, y in want]
        eng.unregister_host_memory(arena.ctypes.data)
        eng.unregister_host_memory(pool.ctypes.data)


def test_dispatch_across_streams(dev, oracle_mod):
    """One context, back-to-back dispatches on two different streams and a host
    burst on the context's own stream: the shared compaction workspace is
    handed from stream to stream, so every result is exact."""
    n = 1 << 20
    with SoftRss(5, 4, 1, 1, device=0, max_burst=0) as eng:
        win, lens = eng.synth(abi.SYN_FUZZ, n, 77, stride=80)
        torch.cuda.synchronize()
        s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
        o1 = eng.alloc_out(n, dev)
        o2 = eng.alloc_out(n, dev)
        for _ in range(3):
            eng.dispatch_dev(win, lens, 80, out=o1, stream=s1)
            eng.dispatch_dev(win, lens, 80, out=o2, stream=s2)
        w_h = win.cpu().numpy()
        l_h = to_np(lens[:n], np.uint16)
        frames = [w_h[i * 80: i * 80 + min(int(l_h[i]), 80)].tobytes() for i in range(3000)]
        r3 = eng.dispatch_frames(frames)        # host path, context stream
        torch.cuda.synchronize()
        c = oracle_mod.cfg(5, 4, 1, 1)
        q_ref, h_ref = oracle_mod.dispatch_windows(w_h, 80, l_h, c)
        qi_ref, qs_ref = oracle_mod.process_burst(q_ref, 4)
        for o in (o1, o2):
            assert np.array_equal(to_np(o.q[:n], np.int16), q_ref)
            assert np.array_equal(to_np(o.qstart, np.uint32), qs_ref)
            assert np.array_equal(to_np(o.qidx[:n], np.uint32), qi_ref)
        want = [oracle_mod.toeplitz_dispatch(f, len(f), c)[0] for f in frames]
        assert np.asarray(r3.q).tolist() == want
