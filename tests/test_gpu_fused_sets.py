"""In-scatter prefixes: the two sets of sums across batches (GPU).

Up to 16 buckets no scan kernel runs: the parse kernel adds its counts to the
batch's totals and range bins, and every line-scatter workgroup scans them in
its prologue (yrss.hip yrss_parse_hash's count flush, yrss_scatter_lines'
fused prologue).  Two sets of sums alternate from batch to batch: a batch's
scatter zeroes the other set, ahead of its capacity check, and the host takes
the other set only once that scatter is queued.

What is checked, bit for bit against oracle.dispatch_windows and
oracle.process_burst: every batch size from the grid path's first (4097) to
2^20, 2, 4 and 16 buckets (16 is the most the sums serve) and 17 (the scan
kernel's), one-list, few-list and fuzz traffic, strides 64 and 80, filter on
and off; the same batch with and without the scan kernel; batches of
alternating size and traffic back to back on one context, alone and with
segmented calls between them.

The scatter's capacity-check return is not covered: with the sums in use (at
most 16 buckets, spans of at most 8192 packets) no plan exceeds what the
kernel holds, and the hook that launches an oversized plan anyway
(yrss_debug_line_groups) needs more than 128 buckets, where the scan kernel
runs and no set of sums exists.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from gpu_checks import check, check_seg, dev, to_np  # noqa: E402,F401
from yastack_amd import SoftRss, abi  # noqa: E402

SIZES = [4097, 8193, 60001, (1 << 18) + 17, 1 << 20]
# nb_queues 1, 3, 15 (2, 4, 16 buckets: the table) and 16 (17: the scan kernel)
CFGS = {1: (1, 1, 1, 0), 3: (3, 3, 1, 1), 15: (15, 15, 1, 0), 16: (16, 16, 1, 1)}
STREAMS = [abi.SYN_UDP4, abi.SYN_TCP4, abi.SYN_FUZZ]


@pytest.mark.parametrize("stride", [64, 80])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("nq", sorted(CFGS))
def test_shapes(dev, oracle_mod, nq, n, stride):
    cfg = CFGS[nq]
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        for profile in STREAMS:
            for want_filter in (False, True):
                check(eng, oracle_mod, cfg, profile, n, stride=stride, first=n + nq,
                      want_filter=want_filter)


@pytest.mark.parametrize("profile", STREAMS)
@pytest.mark.parametrize("nq", [1, 3, 15])
def test_same_batch_with_and_without_the_scan_kernel(dev, oracle_mod, nq, profile):
    cfg = CFGS[nq]
    n = (1 << 18) + 17
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        win, lens = eng.synth(profile, n, 5)
        got = []
        for scan in (1, 0, 1, 0):
            eng.set_tuning(scan_kernel=scan)
            r = eng.dispatch_dev(win, lens, 64, n)
            torch.cuda.synchronize()
            assert eng.status() == 0, f"status() is not 0 (scan_kernel={scan})"
            got.append((to_np(r.q[:n], np.int16).copy(), to_np(r.hash[:n], np.uint32).copy(),
                        to_np(r.qidx[:n], np.uint32).copy(), to_np(r.qstart, np.uint32).copy()))
        for k, g in enumerate(got[1:], 1):
            for name, a, b in zip(("q", "hash", "qidx", "qstart"), got[0], g):
                assert np.array_equal(a, b), f"{name} differs between run 0 and run {k}"


@pytest.mark.parametrize("with_seg", [False, True])
@pytest.mark.parametrize("nq", [3, 15])
def test_back_to_back_on_one_context(dev, oracle_mod, nq, with_seg):
    """Eight batches, sizes and traffic alternating, so both sets of sums
    are used four times each, after a larger and a smaller batch;
    with_seg: a segmented call between the batches (it touches no set)."""
    cfg = CFGS[nq]
    sizes = [60001, 4097, (1 << 18) + 17]
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        for k in range(8):
            n = sizes[k % 3]
            profile = abi.SYN_UDP4 if k % 2 == 0 else abi.SYN_TCP4
            check(eng, oracle_mod, cfg, profile, n, first=k)
            if with_seg:
                check_seg(eng, oracle_mod, cfg, abi.SYN_FUZZ, 5000 + k, first=k)
