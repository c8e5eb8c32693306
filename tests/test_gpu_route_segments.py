"""Routed segmented lists written by the parse kernel (GPU).

yrss_route_dev_seg classifies every packet into process_packets' hand-off
class for the lcore whose queue is queue_id (fs/lib/ff_dpdk_if.c:1058-1140) and
writes the segmented lists over those nb_queues + 3 route buckets in its one
launch.  Every case compares seg_idx / seg_off with
yastack_amd.segments.route_from of the oracle's q and filter class, and q,
hash and filter with the oracle; the outputs are allocated longer than the
batch and pre-filled, so a store past the batch's end shows; status() is 0
after every call.  Input: route_helpers.stream (oracle.synth SYN_FUZZ from
packet 5), uploaded; its classes are asserted from the oracle where a test
claims them."""
import ctypes
import errno

import numpy as np
import pytest

import qpatterns as qp
import route_helpers as rh

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from yastack_amd import SoftRss, abi, segments  # noqa: E402
from yastack_amd.dispatch import SegResult  # noqa: E402

PAD = 64


def to_np(t, dtype):
    return t.cpu().numpy().view(dtype)


def padded_out(eng, n, dev, want_filter=True, want_hash=True):
    nseg = segments.nseg_for(n)
    return SegResult(
        q=torch.full((n + PAD,), 0x5A5A, dtype=torch.int16, device=dev),
        hash=torch.full((n + PAD,), 0x5A5A5A5A, dtype=torch.int32, device=dev) if want_hash
        else None,
        filter=torch.full((n + PAD,), 0x5A, dtype=torch.int8, device=dev) if want_filter else None,
        seg_idx=torch.full((n + PAD,), 0xEE, dtype=torch.uint8, device=dev),
        seg_off=torch.full((nseg + 1, eng.nb_queues + 4), 0x7777, dtype=torch.int16, device=dev))


def upload(win, lens):
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(np.array(win)).to(dev),
            torch.from_numpy(np.array(lens).view(np.int16)).to(dev))


def check_route(eng, win_t, lens_t, n, stride, queue_id, q_ref, h_ref, f_ref, enable, accept,
                want_filter=True, want_hash=True):
    """One routed batch against the oracle's q / hash / filter class."""
    nq = eng.nb_queues
    out = padded_out(eng, n, win_t.device, want_filter, want_hash)
    res = eng.route_dev_seg(win_t, lens_t, stride, queue_id, n, out=out)
    torch.cuda.synchronize()
    assert eng.status() == 0
    q = to_np(res.q, np.int16)
    assert np.array_equal(q[:n], q_ref) and np.all(q[n:] == 0x5A5A)
    if want_hash:
        h = to_np(res.hash, np.uint32)
        assert np.array_equal(h[:n], h_ref) and np.all(h[n:] == 0x5A5A5A5A)
    if want_filter:
        f = res.filter.cpu().numpy()
        assert np.array_equal(f[:n], f_ref) and np.all(f[n:] == 0x5A)
    si_ref, so_ref = segments.route_from(q_ref, f_ref, nq, queue_id, enable, accept)
    nseg = segments.nseg_for(n)
    so = to_np(res.seg_off, np.uint16)
    si = res.seg_idx.cpu().numpy()
    rows = np.nonzero((so[:nseg] != so_ref).any(axis=1))[0]
    assert rows.size == 0, f"seg_off differs in {rows.size} segments, first {rows[:3]}: " \
                           f"{so[rows[:1]]} vs {so_ref[rows[:1]]}"
    d = np.nonzero(si[:n] != si_ref)[0]
    assert d.size == 0, f"{d.size} seg_idx mismatches, first at {d[:5]}: {si[d[:5]]} vs " \
                        f"{si_ref[d[:5]]}"
    assert np.all(si[n:] == 0xEE) and np.all(so[nseg] == 0x7777)
    for b in (0, nq, nq + 2):
        assert np.array_equal(res.segment(0, b).cpu().numpy(),
                              si_ref[int(so_ref[0, b]):int(so_ref[0, b + 1])])
    return res


@pytest.mark.parametrize("kni", list(rh.KNI_MODES))
@pytest.mark.parametrize("cfg", rh.CONFIGS)
def test_bit_exact_routes(oracle_mod, cfg, kni):
    """Batch ends inside a tile, at a tile, inside and at a segment (the
    16-byte stores of whole tiles and the lane-granular remainder), strides 64
    and 80, every queue_id kind, with the filter output and with filter ==
    NULL."""
    nq = cfg[1]
    enable, method = rh.KNI_MODES[kni]
    accept = method == "accept"
    # what the matrix covers, from the oracle (n = 1000, stride 80)
    q, _ = rh.oracle_qh(cfg, 1000)
    f = rh.oracle_filter(enable, 1000)
    assert rh.class_counts(q, f, nq, 0, enable, accept)["arp"] > 0
    assert (rh.class_counts(q, f, nq, 2, enable, accept)["kni"] > 0) == enable
    assert (rh.class_counts(q, f, nq, 0, enable, accept)["freed"] > 0) == (nq < cfg[0])
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(enable, method, rh.TCP_PORTS, rh.UDP_PORTS)
        for stride in (64, 80):
            for n in (1, 63, 64, 255, 256, 257, 1000, 4097):
                win_t, lens_t = upload(*rh.stream(n, stride))
                q_ref, h_ref = rh.oracle_qh(cfg, n, stride)
                f_ref = rh.oracle_filter(enable, n, stride)
                for queue_id in (0, 2, nq):
                    for want_filter in (True, False):
                        check_route(eng, win_t, lens_t, n, stride, queue_id, q_ref, h_ref, f_ref,
                                    enable, accept, want_filter=want_filter)
                check_route(eng, win_t, lens_t, n, stride, 0, q_ref, h_ref, f_ref, enable, accept,
                            want_filter=False, want_hash=False)


@pytest.mark.parametrize("blocks,n", [(1, 79 * 256 + 17), (0, (1 << 20) + 77)])
def test_a_wave_owns_many_chunks(oracle_mod, blocks, n):
    """One workgroup: 80 chunks over 8 waves, the one count slot and the list
    behind it reused flush after flush; the full grid with two chunks a wave."""
    cfg, queue_id = (6, 4, 1, 0), 0
    q_ref, h_ref = rh.oracle_qh(cfg, n)
    f_ref = rh.oracle_filter(True, n)
    cnt = rh.class_counts(q_ref, f_ref, 4, queue_id, True, True)
    assert cnt["arp"] > 0 and cnt["kni"] > 0 and cnt["freed"] > 0
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(True, "accept", rh.TCP_PORTS, rh.UDP_PORTS)
        if blocks:
            eng.set_tuning(parse_blocks=blocks)
        else:
            assert segments.nseg_for(n) >= 2 * 8 * eng.grid_for(n)   # 8 waves a workgroup
        win_t, lens_t = upload(*rh.stream(n))
        check_route(eng, win_t, lens_t, n, rh.STRIDE, queue_id, q_ref, h_ref, f_ref, True, True)


@pytest.mark.parametrize("name", ["all_but_one", "runs"])
def test_directed_patterns_on_the_local_queue(oracle_mod, name):
    """The dominant bucket is the local queue, so nearly every packet lands in
    the local, KNI and ARP buckets: whole segments in one route bucket, runs
    that end on tile and segment boundaries."""
    n, stride = 2000, 64
    if name == "all_but_one":
        # dispatch_only_core: q = 0 is ARP alone, all of it local ARP on queue 0
        cfg, queue_id, enable, method = (3, 3, 1, 1), 0, True, "accept"
        ex = qp.exemplars(oracle_mod, cfg, stride)
        pattern = qp.all_but_one(n, 0, 1, 300)
    else:
        cfg, queue_id, enable, method = (6, 4, 1, 0), 2, True, "reject"
        ex = qp.exemplars(oracle_mod, cfg, stride)
        pattern = qp.runs(n, [2, 2, 2, 1, 2, 2, 4], 64)
    nq = cfg[1]
    accept = method == "accept"
    win, lens = qp.build(pattern, ex)
    q_ref, h_ref = oracle_mod.dispatch_windows(win, stride, lens, oracle_mod.cfg(*cfg))
    assert np.array_equal(qp.bucket_of(q_ref, nq), pattern)
    f_ref = oracle_mod.filter_windows(win, stride, lens, enable, oracle_mod.kni_bitmap(rh.TCP_PORTS),
                                      oracle_mod.kni_bitmap(rh.UDP_PORTS))
    bkt = segments.route_buckets(q_ref, f_ref, nq, queue_id, enable, accept)
    own = np.isin(bkt, (queue_id, nq + 1, nq + 2)).sum()
    assert own >= 0.7 * n
    if name == "all_but_one":
        assert (bkt == nq + 2).sum() == n - 1
    else:
        assert (bkt == nq + 1).sum() > 0 and (bkt == queue_id).sum() > 0 and (bkt == nq).sum() > 0
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(enable, method, rh.TCP_PORTS, rh.UDP_PORTS)
        win_t, lens_t = upload(win, lens)
        check_route(eng, win_t, lens_t, n, stride, queue_id, q_ref, h_ref, f_ref, enable, accept)


@pytest.mark.parametrize("queue_id", [0, 2])
def test_end_to_end_hand_off(oracle_mod, queue_id):
    """route_dev_seg, the arrays copied to the host, route_seg with bounded
    rings and failing clones: process_packets' result for the whole batch."""
    cfg, n, cap = (6, 4, 1, 0), 3000, 300
    nq = 4
    q_ref, _ = rh.oracle_qh(cfg, n)
    f_ref = rh.oracle_filter(True, n)
    cnt = rh.class_counts(q_ref, f_ref, nq, queue_id, True, True)
    assert cnt["freed"] > 0 and cnt["kni"] > 0 and (cnt["arp"] > 0) == (queue_id == 0)
    if queue_id == 0:
        arp = np.nonzero((q_ref == 0) & (f_ref == abi.FILTER_ARP))[0]
        assert any(not rh.clone_ok(int(i), j) for i in arp for j in range(1, nq))
    ptrs, addr_to_idx = rh.fake_objs(n)
    for with_filter in (True, False):
        cb = rh.Rings(addr_to_idx, [cap] * nq, rh.clone_ok)
        with SoftRss(*cfg, device=0, max_burst=0) as eng:
            eng.set_kni(True, "accept", rh.TCP_PORTS, rh.UDP_PORTS)
            win_t, lens_t = upload(*rh.stream(n))
            res = eng.route_dev_seg(win_t, lens_t, rh.STRIDE, queue_id, n,
                                    want_filter=with_filter)
            torch.cuda.synchronize()
            assert eng.status() == 0
            local, kni_list, rr = eng.route_seg(res, ptrs, queue_id, cb.enqueue, cb.clone,
                                                cb.release)
        _, _, _, freed_ref = rh.assert_matches_model(
            cb, [cb.obj(a) for a in local], [cb.obj(a) for a in kni_list], rr, q_ref, f_ref, nq,
            queue_id, True, True, cap, with_filter=with_filter)
        assert len(freed_ref) > cnt["freed"], "ring-full frees"


def test_kni_state_is_read_at_call_time(oracle_mod):
    cfg, n, queue_id = (6, 4, 1, 0), 1000, 2
    q_ref, h_ref = rh.oracle_qh(cfg, n)
    win_t, lens_t = upload(*rh.stream(n))
    lists = []
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        for kni in ("accept", "reject", "off", "accept"):
            enable, method = rh.KNI_MODES[kni]
            eng.set_kni(enable, method, rh.TCP_PORTS, rh.UDP_PORTS)
            f_ref = rh.oracle_filter(enable, n)
            res = check_route(eng, win_t, lens_t, n, rh.STRIDE, queue_id, q_ref, h_ref, f_ref,
                              enable, method == "accept")
            lists.append(to_np(res.seg_off, np.uint16)[:4].copy())
    assert not np.array_equal(lists[0], lists[1]) and not np.array_equal(lists[1], lists[2])
    assert np.array_equal(lists[0], lists[3])


def test_coexists_with_the_other_device_forms(oracle_mod):
    """dispatch_dev, dispatch_dev_seg and route_dev_seg alternate on one
    context; each result is what it is alone."""
    cfg, n, queue_id = (6, 4, 1, 0), 100003, 0
    nq = 4
    q_ref, h_ref = rh.oracle_qh(cfg, n)
    f_ref = rh.oracle_filter(True, n)
    qi_ref, qs_ref = oracle_mod.process_burst(q_ref, nq)
    si_ref, so_ref = segments.from_q(q_ref, nq)
    win_t, lens_t = upload(*rh.stream(n))
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.set_kni(True, "accept", rh.TCP_PORTS, rh.UDP_PORTS)

        def global_lists():
            r = eng.dispatch_dev(win_t, lens_t, rh.STRIDE, n)
            torch.cuda.synchronize()
            assert eng.status() == 0
            assert np.array_equal(to_np(r.qstart, np.uint32), qs_ref)
            assert np.array_equal(to_np(r.qidx[:n], np.uint32), qi_ref)

        def seg_lists():
            r = eng.dispatch_dev_seg(win_t, lens_t, rh.STRIDE, n, want_filter=True)
            torch.cuda.synchronize()
            assert eng.status() == 0
            assert np.array_equal(to_np(r.seg_off, np.uint16), so_ref)
            assert np.array_equal(r.seg_idx.cpu().numpy()[:n], si_ref)
            assert np.array_equal(r.filter.cpu().numpy()[:n], f_ref)

        def routed():
            check_route(eng, win_t, lens_t, n, rh.STRIDE, queue_id, q_ref, h_ref, f_ref, True, True)

        for step in (global_lists, routed, global_lists, seg_lists, routed, seg_lists, global_lists,
                     routed):
            step()


def test_refusals_before_any_launch():
    dev = torch.device("cuda", 0)
    with SoftRss(14, 14, 1, 0, device=0, max_burst=0) as eng:     # 17 route buckets
        win, lens = eng.synth(abi.SYN_TCP4, 300)
        with pytest.raises(abi.YrssError) as e:
            eng.route_dev_seg(win, lens, 64, 0, 300)
        assert e.value.errno == errno.ENOTSUP
        eng.dispatch_dev_seg(win, lens, 64, 300)      # 15 buckets: the plain form still runs
        torch.cuda.synchronize()
        assert eng.status() == 0
    with SoftRss(8, 8, 1, 0, device=0, max_burst=0) as eng:
        n = 300
        win, lens = eng.synth(abi.SYN_TCP4, n)
        out = padded_out(eng, n, dev)

        def call(n_arg, seg_idx_ptr, stride=64, seg_off_ptr=None):
            b = abi.DevRouteBatch(win.data_ptr(), stride, n_arg, lens.data_ptr(),
                                  out.q.data_ptr(), out.hash.data_ptr(), out.filter.data_ptr(),
                                  seg_idx_ptr, seg_off_ptr or out.seg_off.data_ptr(), 0)
            return eng._lib.yrss_route_dev_seg(eng._ctx, ctypes.byref(b), None)

        assert call(abi.SEG_MAX_BATCH + 1, out.seg_idx.data_ptr()) == -errno.EINVAL
        assert call(n, out.seg_idx.data_ptr() + 1) == -errno.EINVAL
        assert call(n, out.seg_idx.data_ptr() + 8) == -errno.EINVAL
        assert call(n, out.seg_idx.data_ptr(), stride=48) == -errno.EINVAL
        assert call(n, out.seg_idx.data_ptr(), seg_off_ptr=out.seg_off.data_ptr() + 1) == \
            -errno.EINVAL
        assert call(n, None) == -errno.EINVAL
        assert eng._lib.yrss_route_dev_seg(eng._ctx, None, None) == -errno.EINVAL
        assert call(0, None) == 0
        torch.cuda.synchronize()
        assert eng.status() == 0
        assert np.all(out.seg_idx.cpu().numpy() == 0xEE)
        assert np.all(to_np(out.seg_off, np.uint16) == 0x7777)
        assert np.all(to_np(out.q, np.uint16) == 0x5A5A)
        assert np.all(out.filter.cpu().numpy() == 0x5A)
        with pytest.raises(ValueError, match="seg_off"):
            small = padded_out(eng, n, dev)
            small.seg_off = small.seg_off[:1]      # two segments need two rows
            eng.route_dev_seg(win, lens, 64, 0, n, out=small)
