"""The torch side of the GPU tests' shared support: the two GPU fixtures (a
test module imports the one it uses by name), host/device copies, pre-filled
segmented outputs and three batch checkers.  The three assert different
things: run_and_compare the host generator against the device's and status(),
check an empty fault record, check_seg the untouched padding and the segment()
accessor.  (The routed form's check_route is in test_gpu_route_segments.py.)
As in hostbufs.py, every assertion carries its own message."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hostbufs import PAD, assert_same  # noqa: E402
from yastack_amd import abi, segments  # noqa: E402
from yastack_amd.dispatch import SegResult  # noqa: E402

LAYOUT_KNI = ("accept", "0-32767", "1000-40000,53,123")    # check sets it itself
SEG_KNI = ("accept", "80", "53")                            # check_seg's callers set it


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return torch.device("cuda", 0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def to_np(t, dtype):
    return t.cpu().numpy().view(dtype)


def upload(win, lens, dev=None):
    """Host-built (win uint8, lens uint16) arrays as device tensors."""
    dev = torch.device("cuda", 0) if dev is None else dev
    return (torch.from_numpy(np.array(win)).to(dev),
            torch.from_numpy(np.array(lens).view(np.int16)).to(dev))


def padded_seg_out(eng, n, dev, want_filter):
    """dispatch_dev_seg's outputs, PAD elements (one offsets row) longer than
    the batch needs, pre-filled."""
    nseg = segments.nseg_for(n)
    return SegResult(
        q=torch.full((n + PAD,), 0x5A5A, dtype=torch.int16, device=dev),
        hash=torch.full((n + PAD,), 0x5A5A5A5A, dtype=torch.int32, device=dev),
        filter=torch.full((n + PAD,), 0x5A, dtype=torch.int8, device=dev) if want_filter else None,
        seg_idx=torch.full((n + PAD,), 0xEE, dtype=torch.uint8, device=dev),
        seg_off=torch.full((nseg + 1, eng.nb_queues + 2), 0x7777, dtype=torch.int16, device=dev))


def first_mismatch_qh(q, h, q_ref, h_ref):
    """q and hash against the oracle's, packet for packet."""
    bad = np.nonzero((q != q_ref) | (h != h_ref))[0]
    b = bad[:5]
    assert bad.size == 0, f"{bad.size} q/hash mismatches, first at {b}: q {q[b]} vs {q_ref[b]}, " \
                          f"h {h[b]} vs {h_ref[b]}"


def _host_and_oracle(oracle_mod, cfg, win, lens, n, stride):
    """The batch's input back on the host and the oracle's q and hash of it."""
    w_h = win[: n * stride].cpu().numpy()
    l_h = to_np(lens[:n], np.uint16)
    return (w_h, l_h, *oracle_mod.dispatch_windows(w_h, stride, l_h, oracle_mod.cfg(*cfg)))


def _assert_seg_lists(res, n, nseg, si_ref, so_ref, buckets):
    """seg_off / seg_idx of the batch, their padding, and the segment()
    accessor on segment 0's `buckets`."""
    so = to_np(res.seg_off, np.uint16)
    si = res.seg_idx.cpu().numpy()
    rows = np.nonzero((so[:nseg] != so_ref).any(axis=1))[0]
    assert rows.size == 0, f"seg_off differs in {rows.size} segments, first {rows[:3]}: " \
                           f"{so[rows[:1]]} vs {so_ref[rows[:1]]}"
    d = np.nonzero(si[:n] != si_ref)[0]
    assert d.size == 0, f"{d.size} seg_idx mismatches, first at {d[:5]}: {si[d[:5]]} vs " \
                        f"{si_ref[d[:5]]}"
    assert_same("seg_idx past the batch", si[n:], 0xEE)
    assert_same("seg_off past the last segment", so[nseg], 0x7777)
    for b in buckets:
        assert_same(f"segment(0, {b})", res.segment(0, b).cpu().numpy(),
                    si_ref[int(so_ref[0, b]):int(so_ref[0, b + 1])])


def run_and_compare(eng, oracle_mod, cfg_tuple, profile, n, stride, first=0, nflows=1 << 20,
                    compact=True):
    nq = cfg_tuple[1]
    win, lens = eng.synth(profile, n, first, nflows=nflows, stride=stride)
    res = eng.dispatch_dev(win, lens, stride, n, compact=compact)
    torch.cuda.synchronize()
    w_h, l_h, q_ref, h_ref = _host_and_oracle(oracle_mod, cfg_tuple, win, lens, n, stride)
    # host generator produces the identical input
    w_o, l_o = oracle_mod.synth(profile, min(n, 4096), first, nflows=nflows, stride=stride)
    assert_same("synth windows (device vs host generator)", w_h[: min(n, 4096) * stride], w_o)
    assert_same("synth lengths (device vs host generator)", l_h[: min(n, 4096)], l_o)
    first_mismatch_qh(to_np(res.q[:n], np.int16), to_np(res.hash[:n], np.uint32), q_ref, h_ref)
    if compact:
        qi_ref, qs_ref = oracle_mod.process_burst(q_ref, nq)
        assert_same("qstart", to_np(res.qstart, np.uint32), qs_ref)
        assert_same("qidx", to_np(res.qidx[:n], np.uint32), qi_ref)
        assert eng.status() == 0, "status() is not 0 after the batch"
    return q_ref, h_ref


def check(eng, oracle_mod, cfg_tuple, profile, n, stride=64, first=0, want_filter=False,
          traffic=None, out=None):
    """One device batch against the oracle: q, hash, qstart, qidx (and the
    filter class when asked), plus an empty fault record.  traffic: host-built
    (win, lens) instead of a synthetic profile; out: the caller's buffers."""
    nq = cfg_tuple[1]
    if want_filter:
        eng.set_kni(True, *LAYOUT_KNI)
    if traffic is None:
        win, lens = eng.synth(profile, n, first, stride=stride)
    else:
        win, lens = upload(*traffic)
    res = eng.dispatch_dev(win, lens, stride, n, want_filter=want_filter, out=out)
    torch.cuda.synchronize()
    fault = eng.fault_info()
    assert fault[0] == abi.FAULT_NONE, f"device guard fired: {fault}"
    w_h, l_h, q_ref, h_ref = _host_and_oracle(oracle_mod, cfg_tuple, win, lens, n, stride)
    first_mismatch_qh(to_np(res.q[:n], np.int16), to_np(res.hash[:n], np.uint32), q_ref, h_ref)
    qi_ref, qs_ref = oracle_mod.process_burst(q_ref, nq)
    assert_same("qstart", to_np(res.qstart, np.uint32), qs_ref)
    assert_same("qidx", to_np(res.qidx[:n], np.uint32), qi_ref)
    if want_filter:
        want = oracle_mod.filter_windows(w_h, stride, l_h, True,
                                         oracle_mod.kni_bitmap(LAYOUT_KNI[1]),
                                         oracle_mod.kni_bitmap(LAYOUT_KNI[2]))
        assert_same("filter", res.filter[:n].cpu().numpy(), want)
    return res


def check_seg(eng, oracle_mod, cfg, profile, n, stride=64, first=0, want_filter=False,
              traffic=None):
    """One segmented batch against the oracle; returns (result, q_ref).
    traffic: host-built (win uint8, lens uint16) instead of a synthetic profile."""
    nq = cfg[1]
    dev = torch.device("cuda", 0)
    if traffic is None:
        win, lens = eng.synth(profile, n, first, stride=stride)
    else:
        win, lens = upload(*traffic)
    out = padded_seg_out(eng, n, dev, want_filter)
    res = eng.dispatch_dev_seg(win, lens, stride, n, out=out)
    torch.cuda.synchronize()
    assert eng.status() == 0, "status() is not 0 after the batch"
    w_h, l_h, q_ref, h_ref = _host_and_oracle(oracle_mod, cfg, win, lens, n, stride)
    q = to_np(res.q, np.int16)
    h = to_np(res.hash, np.uint32)
    first_mismatch_qh(q[:n], h[:n], q_ref, h_ref)
    # nothing past the batch's end
    assert_same("q past the batch", q[n:], 0x5A5A)
    assert_same("hash past the batch", h[n:], 0x5A5A5A5A)
    si_ref, so_ref = segments.from_q(q_ref, nq)
    _assert_seg_lists(res, n, segments.nseg_for(n), si_ref, so_ref, range(nq + 1))
    if want_filter:
        want = oracle_mod.filter_windows(w_h, stride, l_h, True, oracle_mod.kni_bitmap(SEG_KNI[1]),
                                         oracle_mod.kni_bitmap(SEG_KNI[2]))
        f = res.filter.cpu().numpy()
        assert_same("filter", f[:n], want)
        assert_same("filter past the batch", f[n:], 0x5A)
    return res, q_ref
