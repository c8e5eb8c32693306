"""GPU parity of the extended mode (yrss_set_extended) against tests/ext_model.py:
q, hash and every list form in full, and an empty fault record.

The mode is this build's own semantics: the hashes are validated against the
82599 vectors, everything else against the model, which is the restated
reference on the stripped frame (test_ext_model.py checks the model itself).
"""
import errno
import json

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import ext_model as xm  # noqa: E402
from yastack_amd import SoftRss, abi, segments  # noqa: E402

from gpu_checks import SEG_KNI, dev, first_mismatch_qh, to_np, upload  # noqa: E402,F401
from hostbufs import assert_same, check_lists, fake_mbufs, frames_of  # noqa: E402

V, V6, U = abi.EXT_VLAN, abi.EXT_IPV6, abi.EXT_UDP
CFGS = ((3, 3, 1, 1), (8, 8, 1, 0))     # nb_procs 3 with dispatch_only_core, 8 without


def _engine(cfg, flags, **kw):
    eng = SoftRss(*cfg, device=0, max_burst=0, **kw)
    eng.set_extended(vlan=bool(flags & V), ipv6=bool(flags & V6), udp=bool(flags & U))
    assert eng.ext_flags == flags
    return eng


def _no_fault(eng):
    fault = eng.fault_info()
    assert fault[0] == abi.FAULT_NONE, f"device guard fired: {fault}"


def _check_global(eng, win, lens, stride, n, q_ref, h_ref, nq):
    """yrss_dispatch_dev: q, hash, qidx, qstart."""
    res = eng.dispatch_dev(win, lens, stride, n)
    torch.cuda.synchronize()
    _no_fault(eng)
    first_mismatch_qh(to_np(res.q[:n], np.int16), to_np(res.hash[:n], np.uint32), q_ref, h_ref)
    qi, qs = xm.lists(q_ref, nq)
    assert_same("qstart", to_np(res.qstart, np.uint32), qs)
    assert_same("qidx", to_np(res.qidx[:n], np.uint32), qi)
    return qs


def _check_seg(eng, win, lens, stride, n, q_ref, h_ref, nq):
    """yrss_dispatch_dev_seg: q, hash, seg_idx, seg_off."""
    res = eng.dispatch_dev_seg(win, lens, stride, n)
    torch.cuda.synchronize()
    _no_fault(eng)
    first_mismatch_qh(to_np(res.q[:n], np.int16), to_np(res.hash[:n], np.uint32), q_ref, h_ref)
    si, so = xm.seg_lists(q_ref, nq)
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


# ---- vectors ----------------------------------------------------------------------

@pytest.mark.parametrize("cfg", CFGS)
def test_ipv6_vectors(dev, golden_dir, cfg):
    """The three IPv6 82599 vectors as Eth/IPv6/TCP, Eth/VLAN/IPv6/TCP and QinQ
    on a context with the 82599 key: hash == hash_l3l4, q == hash % d + off, in
    the one-launch kernel, the grid kernels and the host frames call."""
    g = json.loads((golden_dir / "thash_82599.json").read_text())
    d, off = xm.modulo(cfg)
    frames, want_h = [], []
    for v in g["v6"]:
        t = bytes.fromhex(v["l3l4"])
        for tags, outer in ((0, 0), (1, 0x8100), (2, 0x88A8)):
            frames.append(xm.with_tags(xm.ipv6_frame(t[:16], t[16:32], t[32:], size=90), tags,
                                       outer)[:90])
            want_h.append(v["hash_l3l4"])
    assert len(frames) == 9
    h_ref = np.array(want_h, np.uint32)
    q_ref = (h_ref % d + off).astype(np.int16)
    win = np.frombuffer(b"".join(f[:80] for f in frames), np.uint8).copy()
    lens = np.full(9, 90, np.uint16)
    qm, hm = xm.classify_windows(win, 80, lens, V | V6, cfg, key=xm.KEY_82599)
    assert np.array_equal(qm, q_ref) and np.array_equal(hm, h_ref)
    w_d, l_d = upload(win, lens)
    for one_launch in (0, 2):
        with _engine(cfg, V | V6, rss_key=xm.KEY_82599) as eng:
            eng.set_tuning(one_launch=one_launch)
            _check_global(eng, w_d, l_d, 80, 9, q_ref, h_ref, cfg[1])
            _check_seg(eng, w_d, l_d, 80, 9, q_ref, h_ref, cfg[1])
            if one_launch == 0:
                r = eng.dispatch_frames(frames)
                check_lists(r, q_ref, h_ref, *xm.lists(q_ref, cfg[1]))
                _no_fault(eng)


# ---- boundary sweep -----------------------------------------------------------------

@pytest.mark.parametrize("stride", [64, 80])
@pytest.mark.parametrize("flags", xm.ALL_FLAG_SETS)
def test_boundary_sweep(dev, flags, stride):
    """Every data_len 0..90 of every frame kind under one flag set: each length
    check at its edge, ports at bytes 62..65, and the window rule.  The batch
    runs through the grid kernels (global and segmented lists) and, in two
    pieces, through the one-launch kernel."""
    cfg = CFGS[1]
    win, lens = xm.sweep_batch(stride)
    n = int(lens.size)
    assert n == 65 * 91
    q_ref, h_ref = xm.classify_windows(win, stride, lens, flags, cfg)
    # the window rule: IHL 12 and 15 at stride 64 under any flags; 80 bytes hold
    # every untagged port, so there it takes YRSS_EXT_VLAN (tags and IHL 15)
    trunc = np.count_nonzero(q_ref == abi.Q_TRUNCATED)
    assert (trunc > 0) == (stride == 64 or bool(flags & V)), trunc
    if flags == V | V6 | U:
        assert np.count_nonzero(h_ref) > 600
    w_d, l_d = upload(win, lens)
    with _engine(cfg, flags) as eng:
        _check_global(eng, w_d, l_d, stride, n, q_ref, h_ref, cfg[1])
        _check_seg(eng, w_d, l_d, stride, n, q_ref, h_ref, cfg[1])
        for lo, hi in ((0, 4096), (4096, n)):
            _check_global(eng, w_d[lo * stride:], l_d[lo:hi], stride, hi - lo, q_ref[lo:hi],
                          h_ref[lo:hi], cfg[1])


# ---- streams ------------------------------------------------------------------------

STREAMS = ((abi.SYN_VLAN6_TCP, V | V6, True), (abi.SYN_UDP4, U, True),
           (abi.SYN_IMIX, V | V6 | U, False), (abi.SYN_FUZZ, V | V6 | U, False))


@pytest.mark.parametrize("cfg", CFGS)
@pytest.mark.parametrize("profile,flags,spread", STREAMS)
def test_streams(dev, oracle_mod, profile, flags, spread, cfg):
    """Synthetic streams at n = 64 and 4096 (the one-launch kernel), 4097 and
    20000 (the grid kernels) through every list form.  spread: every reachable
    queue receives packets (test_ext_model.py confirms it for these seeds);
    without the flags these two streams sit on queue 2 whole."""
    nq = cfg[1]
    d, off = xm.modulo(cfg)
    lq = 1
    for n in (64, 4096, 4097, 20000):
        w_h, l_h = xm.stream(profile, n, 64)
        q_ref, h_ref = xm.stream_model(profile, n, 64, flags, cfg)
        with _engine(cfg, flags) as eng:
            win, lens = eng.synth(profile, n, stride=64)
            assert_same("synth windows", win[:n * 64].cpu().numpy(), w_h)
            qs = _check_global(eng, win, lens, 64, n, q_ref, h_ref, nq)
            if spread:
                counts = np.diff(qs.astype(np.int64))[:nq]
                assert np.all(counts[off:off + d] > 0), counts
            eng.set_tuning(scan_kernel=1)
            _check_global(eng, win, lens, 64, n, q_ref, h_ref, nq)
            eng.set_tuning()
            _check_seg(eng, win, lens, 64, n, q_ref, h_ref, nq)
            eng.set_kni(True, *SEG_KNI)
            _check_route_seg(eng, oracle_mod, win, lens, w_h, l_h, 64, n, q_ref, h_ref, nq, lq)
            if n == 20000:
                continue
            # The host forms: they stage 80 bytes of every frame once one is
            # longer than 64 (frames_of: the window and a zero tail), so what a
            # 64-byte window truncates is hashed here: the model per frame.
            frames = frames_of(w_h, l_h, stride=64)
            fq, fh = zip(*(xm.classify(f, len(f), flags, cfg, stride=80) for f in frames))
            fq, fh = np.array(fq, np.int16), np.array(fh, np.uint32)
            r = eng.dispatch_frames(frames)      # one launch; the staged batch at 4097
            _no_fault(eng)
            check_lists(r, fq, fh, *xm.lists(fq, nq))
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


def test_host_bursts_stage_enough_for_qinq_ipv6(dev):
    """The host forms stage 80 bytes when a frame is longer than 64: a QinQ +
    IPv6 frame (ports at bytes 62..65) is hashed, never YRSS_Q_TRUNCATED, by
    the frames call, the mbuf burst and both zero-copy forms; a tagged IPv4
    frame with IHL 15 (ports at 78..81) is the case 80 bytes do not hold."""
    cfg, flags = CFGS[1], V | V6 | U
    rng = np.random.default_rng(11)
    frames = []
    for i in range(70):
        tags, outer = ((2, 0x88A8), (1, 0x8100), (0, 0))[i % 3]
        f6 = xm.ipv6_frame(rng.bytes(16), rng.bytes(16), rng.bytes(4), (6, 17)[i % 2], 100)
        frames.append(xm.with_tags(f6, tags, outer)[:66 + i % 30])
    frames.append(xm.with_tags(xm.ipv4_frame(rng.bytes(4), rng.bytes(4), rng.bytes(4), 6, 15), 1))
    want = [xm.classify(f, len(f), flags, cfg, stride=80) for f in frames]
    q_ref = np.array([x for x, _ in want], np.int16)
    h_ref = np.array([y for _, y in want], np.uint32)
    assert np.count_nonzero(h_ref) >= 70 and q_ref[-1] == abi.Q_TRUNCATED
    assert not np.any(q_ref[:-1] == abi.Q_TRUNCATED)
    qi, qs = xm.lists(q_ref, cfg[1])
    pool, ptrs, _ = fake_mbufs(frames)
    with _engine(cfg, flags) as eng:
        check_lists(eng.dispatch_frames(frames), q_ref, h_ref, qi, qs)
        check_lists(eng.dispatch_burst(ptrs), q_ref, h_ref, qi, qs)
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        check_lists(eng.dispatch_burst_zc(ptrs), q_ref, h_ref, qi, qs)
        _no_fault(eng)
        eng.unregister_host_memory(pool.ctypes.data)


# ---- off means off -------------------------------------------------------------------

def test_off_means_off(dev, oracle_mod):
    """Flags set, a batch, flags cleared: SYN_FUZZ is the plain oracle's again,
    alternating with extended batches on one context, in both kernels."""
    cfg, stride = CFGS[0], 80
    c = oracle_mod.cfg(*cfg)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        for n in (3000, 9000):
            w_h, l_h = xm.stream(abi.SYN_FUZZ, n, stride)
            q0, h0 = oracle_mod.dispatch_windows(w_h, stride, l_h, c)
            q1, h1 = xm.stream_model(abi.SYN_FUZZ, n, stride, V | V6 | U, cfg)
            assert np.count_nonzero(h1) > np.count_nonzero(h0)
            win, lens = upload(w_h, l_h)
            _check_global(eng, win, lens, stride, n, q0, h0, cfg[1])
            for _ in range(2):
                eng.set_extended(vlan=True, ipv6=True, udp=True)
                _check_global(eng, win, lens, stride, n, q1, h1, cfg[1])
                _check_seg(eng, win, lens, stride, n, q1, h1, cfg[1])
                eng.set_extended()
                _check_global(eng, win, lens, stride, n, q0, h0, cfg[1])
                _check_seg(eng, win, lens, stride, n, q0, h0, cfg[1])


# ---- worker and shim: refused while flags are set ---------------------------------------

def test_worker_and_shim_contract(dev, oracle_mod):
    """The persistent worker has no extended variant: -ENOTSUP from
    yrss_worker_start* and every submit while flags are set (the shim on a
    worker context: -1), served again once they are cleared; -EBUSY while a
    worker burst is pending; -EINVAL on unknown bits.  The shim on a context
    without a worker honours the flags."""
    cfg = CFGS[1]
    w_h, l_h = xm.stream(abi.SYN_UDP4, 64, 80)
    frames = frames_of(w_h, l_h)
    pool, ptrs, _ = fake_mbufs(frames)
    plain = [oracle_mod.toeplitz_dispatch(f, len(f), oracle_mod.cfg(*cfg)) for f in frames]
    q0 = np.array([x for x, _ in plain], np.int16)
    h0 = np.array([y for _, y in plain], np.uint32)
    q1, h1 = xm.stream_model(abi.SYN_UDP4, 64, 80, U, cfg)
    assert np.all(q0 == 2) and np.all(h1 != 0) and len(set(q1[:8].tolist())) > 3
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        lib, ctx = eng._lib, eng._ctx
        assert lib.yrss_set_extended(ctx, 8) == -errno.EINVAL
        assert lib.yrss_set_extended(ctx, 0xFFFFFFFF) == -errno.EINVAL
        # the shim without a worker: one-packet launches under the flags
        eng.set_extended(udp=True)
        assert [eng.toeplitz_dispatch(f) for f in frames[:8]] == q1[:8].tolist()
        assert lib.yrss_worker_start(ctx, 4, 2) == -errno.ENOTSUP
        assert lib.yrss_worker_start_route(ctx, 4, 2, 1) == -errno.ENOTSUP
        eng.set_extended()
        assert [eng.toeplitz_dispatch(f) for f in frames[:4]] == [2, 2, 2, 2]
        # a worker context
        eng.register_host_memory(pool.ctypes.data, pool.nbytes)
        eng.worker_start(4, 2)
        t = eng.worker_submit(ptrs)
        assert lib.yrss_set_extended(ctx, U) == -errno.EBUSY      # a burst is pending
        check_lists(eng.worker_poll(t), q0, h0, *xm.lists(q0, cfg[1]))
        eng.set_extended(udp=True)                                # halts the worker
        with pytest.raises(abi.YrssError) as e:
            eng.worker_submit(ptrs)
        assert e.value.errno == errno.ENOTSUP
        assert eng.toeplitz_dispatch(frames[0]) == -1
        # the launch paths of the same context honour the flags meanwhile
        check_lists(eng.dispatch_burst(ptrs), q1, h1, *xm.lists(q1, cfg[1]))
        eng.set_extended()
        t = eng.worker_submit(ptrs)                               # relaunched
        check_lists(eng.worker_poll(t), q0, h0, *xm.lists(q0, cfg[1]))
        assert eng.toeplitz_dispatch(frames[0]) == 2
        _no_fault(eng)
        eng.worker_stop()
        eng.unregister_host_memory(pool.ctypes.data)
