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

from gpu_checks import SEG_KNI, check_seg, padded_seg_out, to_np  # noqa: E402
from yastack_amd import SoftRss, abi, segments  # noqa: E402


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
        eng.set_kni(True, *SEG_KNI)
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
        out = padded_seg_out(eng, n, dev, want_filter=False)

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
            small = padded_seg_out(eng, n, dev, want_filter=False)
            small.seg_idx = small.seg_idx[: n - 1]
            eng.dispatch_dev_seg(win, lens, 64, n, out=small)
