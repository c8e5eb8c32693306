"""Segmented per-queue lists written by the parse kernel itself (GPU).

yrss_dispatch_dev_seg cuts the batch into segments of 256 consecutive packets
and returns each segment's finished per-queue lists (seg_idx bytes, seg_off
rows), the form of the reference's per-burst enqueue into
dispatch_ring[port][q] (fs/lib/ff_dpdk_if.c:1087-1093 inside the :1674-1683
loop).  Every case compares q / hash with the oracle, every segment's offsets
and index bytes with yastack_amd.segments.from_q of the oracle's q, and needs
an empty fault record.  The output buffers are allocated longer than the batch
and pre-filled, so a store past the batch's end shows.
"""
import ctypes
import errno

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from yastack_amd import SoftRss, abi, segments  # noqa: E402
from yastack_amd.dispatch import SegResult  # noqa: E402

PAD = 64          # spare elements behind every output, pre-filled
KNI = ("accept", "80", "53")


def to_np(t, dtype):
    return t.cpu().numpy().view(dtype)


def padded_out(eng, n, dev, want_filter=False):
    nseg = segments.nseg_for(n)
    return SegResult(
        q=torch.full((n + PAD,), 0x5A5A, dtype=torch.int16, device=dev),
        hash=torch.full((n + PAD,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
        filter=torch.full((n + PAD,), 0x5A, dtype=torch.int8, device=dev) if want_filter else None,
        seg_idx=torch.full((n + PAD,), 0xEE, dtype=torch.uint8, device=dev),
        seg_off=torch.full((nseg + 1, eng.nb_queues + 2), 0x7777, dtype=torch.int16, device=dev))


def check_seg(eng, oracle_mod, cfg, profile, n, stride=64, first=0, want_filter=False,
              traffic=None):
    """One segmented batch against the oracle; returns (result, q_ref).
    traffic: host-built (win uint8, lens uint16) instead of a synthetic profile."""
    npr, nq, soft, only = cfg
    dev = torch.device("cuda", 0)
    if traffic is None:
        win, lens = eng.synth(profile, n, first, stride=stride)
    else:
        win = torch.from_numpy(np.ascontiguousarray(traffic[0])).to(dev)
        lens = torch.from_numpy(np.ascontiguousarray(traffic[1]).view(np.int16)).to(dev)
    out = padded_out(eng, n, dev, want_filter)
    res = eng.dispatch_dev_seg(win, lens, stride, n, out=out)
    torch.cuda.synchronize()
    assert eng.status() == 0
    w_h = win[: n * stride].cpu().numpy()
    l_h = to_np(lens[:n], np.uint16)
    q_ref, h_ref = oracle_mod.dispatch_windows(w_h, stride, l_h, oracle_mod.cfg(npr, nq, soft, only))
    q = to_np(res.q, np.int16)
    h = to_np(res.hash, np.uint32)
    bad = np.nonzero((q[:n] != q_ref) | (h[:n] != h_ref))[0]
    assert bad.size == 0, f"{bad.size} q/hash mismatches, first at {bad[:5]}"
    si_ref, so_ref = segments.from_q(q_ref, nq)
    nseg = segments.nseg_for(n)
    so = to_np(res.seg_off, np.uint16)
    si = res.seg_idx.cpu().numpy()
    rows = np.nonzero((so[:nseg] != so_ref).any(axis=1))[0]
    assert rows.size == 0, f"seg_off differs in {rows.size} segments, first {rows[:3]}: " \
                           f"{so[rows[:1]]} vs {so_ref[rows[:1]]}"
    d = np.nonzero(si[:n] != si_ref)[0]
    assert d.size == 0, f"{d.size} seg_idx mismatches, first at {d[:5]}: {si[d[:5]]} vs " \
                        f"{si_ref[d[:5]]}"
    # nothing past the batch's end
    assert np.all(q[n:] == 0x5A5A) and np.all(h[n:] == 0x5A5A5A5A)
    assert np.all(si[n:] == 0xEE) and np.all(so[nseg] == 0x7777)
    if want_filter:
        want = oracle_mod.filter_windows(w_h, stride, l_h, True, oracle_mod.kni_bitmap(KNI[1]),
                                         oracle_mod.kni_bitmap(KNI[2]))
        f = res.filter.cpu().numpy()
        assert np.array_equal(f[:n], want)
        assert np.all(f[n:] == 0x5A)
    # the accessor: segment 0's buckets are the expected slices
    for b in range(nq + 1):
        assert np.array_equal(res.segment(0, b).cpu().numpy(),
                              si_ref[int(so_ref[0, b]):int(so_ref[0, b + 1])])
    return res, q_ref


@pytest.mark.parametrize("stride", [64, 80])
@pytest.mark.parametrize("profile", [abi.SYN_FUZZ, abi.SYN_TCP4])
def test_ragged_ends_and_both_store_paths(oracle_mod, profile, stride):
    """Batch ends inside a tile, at a tile, inside and at a segment: the
    16-byte stores of whole tiles and the lane-granular remainder."""
    cfg = (8, 8, 1, 0)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        for n in (1, 63, 64, 255, 256, 257, 1023, 1024, 4097):
            check_seg(eng, oracle_mod, cfg, profile, n, stride, first=n)


@pytest.mark.parametrize("cfg", [(1, 1, 1, 0), (15, 15, 1, 0), (5, 2, 0, 1), (3, 3, 1, 1)])
@pytest.mark.parametrize("profile", [abi.SYN_FUZZ, abi.SYN_IMIX, abi.SYN_UDP4])
def test_bucket_edges(oracle_mod, cfg, profile):
    """One queue, the 16-bucket limit, a populated drop bucket (nb_queues <
    nb_procs), the reference's shipped config; UDP4 is all one bucket."""
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        check_seg(eng, oracle_mod, cfg, profile, 70001, first=5)


@pytest.mark.parametrize("blocks", [1, 2])
def test_a_wave_owns_many_chunks(oracle_mod, blocks):
    """79 chunks over 8 or 16 waves: the one count slot is reused flush after
    flush."""
    cfg = (8, 8, 1, 0)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_tuning(parse_blocks=blocks)
        check_seg(eng, oracle_mod, cfg, abi.SYN_FUZZ, 20000, first=3)


def test_full_grid_two_chunks_a_wave(oracle_mod):
    cfg = (8, 8, 1, 0)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        check_seg(eng, oracle_mod, cfg, abi.SYN_FUZZ, (1 << 20) + 77)


def test_chunk_tiles_tuning_does_not_apply(oracle_mod):
    cfg = (8, 8, 1, 0)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_tuning(chunk_tiles=8)
        check_seg(eng, oracle_mod, cfg, abi.SYN_FUZZ, 70001, first=9)


@pytest.mark.parametrize("n", [257, 70001])
def test_filter_on(oracle_mod, n):
    cfg = (8, 8, 1, 0)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(True, *KNI)
        for profile in (abi.SYN_FUZZ, abi.SYN_IMIX):
            check_seg(eng, oracle_mod, cfg, profile, n, stride=80, first=17, want_filter=True)


def test_coexists_with_the_global_lists(oracle_mod):
    """Global-list batch, segmented batch, global-list batch on one context:
    the segmented call leaves the alternating totals of the fused global path
    alone, and its lists, converted, are the GPU's own qidx / qstart."""
    cfg = (3, 3, 1, 1)
    n = 100003
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        win, lens = eng.synth(abi.SYN_IMIX, n, 21)
        w_h = win[: n * 64].cpu().numpy()
        l_h = to_np(lens[:n], np.uint16)
        q_ref, _ = oracle_mod.dispatch_windows(w_h, 64, l_h, oracle_mod.cfg(*cfg))
        qi_ref, qs_ref = oracle_mod.process_burst(q_ref, 3)

        def global_lists():
            r = eng.dispatch_dev(win, lens, 64, n)
            torch.cuda.synchronize()
            assert eng.status() == 0
            qi, qs = to_np(r.qidx[:n], np.uint32), to_np(r.qstart, np.uint32)[:5]
            assert np.array_equal(qs, qs_ref) and np.array_equal(qi, qi_ref)
            return qi, qs

        global_lists()
        seg = eng.dispatch_dev_seg(win, lens, 64, n)
        torch.cuda.synchronize()
        assert eng.status() == 0
        qi, qs = global_lists()
        for fn in (segments.to_lists_c, segments.to_lists):
            si, so = fn(seg.seg_idx.cpu().numpy(), to_np(seg.seg_off, np.uint16), n, 4)
            assert np.array_equal(so, qs) and np.array_equal(si, qi)
        global_lists()


def test_refusals_before_any_launch():
    dev = torch.device("cuda", 0)
    with SoftRss(16, 16, 1, 0, device=0, max_burst=0) as eng:     # 17 buckets
        win, lens = eng.synth(abi.SYN_TCP4, 300)
        with pytest.raises(abi.YrssError) as e:
            eng.dispatch_dev_seg(win, lens, 64, 300)
        assert e.value.errno == errno.ENOTSUP
        torch.cuda.synchronize()
        assert eng.status() == 0
    with SoftRss(8, 8, 1, 0, device=0, max_burst=0) as eng:
        n = 300
        win, lens = eng.synth(abi.SYN_TCP4, n)
        out = padded_out(eng, n, dev)

        def call(n_arg, seg_idx_ptr, seg_off_ptr=None):
            b = abi.DevSegBatch(win.data_ptr(), 64, n_arg, lens.data_ptr(), out.q.data_ptr(),
                                out.hash.data_ptr(), None, seg_idx_ptr,
                                seg_off_ptr or out.seg_off.data_ptr())
            return eng._lib.yrss_dispatch_dev_seg(eng._ctx, ctypes.byref(b), None)

        # the sizes and alignments are refused before the buffers are touched
        assert call(abi.SEG_MAX_BATCH + 1, out.seg_idx.data_ptr()) == -errno.EINVAL
        assert call(n, out.seg_idx.data_ptr() + 1) == -errno.EINVAL
        assert call(n, out.seg_idx.data_ptr() + 8) == -errno.EINVAL
        assert call(n, out.seg_idx.data_ptr(), out.seg_off.data_ptr() + 1) == -errno.EINVAL
        assert call(n, None) == -errno.EINVAL
        assert call(0, None) == 0
        torch.cuda.synchronize()
        assert eng.status() == 0
        assert np.all(out.seg_idx.cpu().numpy() == 0xEE)
        assert np.all(to_np(out.q, np.uint16) == 0x5A5A)
        with pytest.raises(ValueError, match="seg_idx"):
            small = padded_out(eng, n, dev)
            small.seg_idx = small.seg_idx[: n - 1]
            eng.dispatch_dev_seg(win, lens, 64, n, out=small)
