"""The segmented per-queue list form on the host (no GPU): the C helper
yrss_seg_to_lists and its numpy twin turn segments built from the oracle's q
back into the oracle's batch-wide lists, refuse corrupted arrays, and the
header and the Python binding agree."""
import ctypes
import errno
import re
import subprocess

import numpy as np
import pytest

from yastack_amd import abi

CONFIGS = [(3, 3, 1, 1), (15, 15, 1, 0), (5, 2, 0, 1)]
SIZES = [1, 255, 256, 257, 4097]


def _q_ref(oracle_mod, profile, n, cfg):
    win, lens = oracle_mod.synth(profile, n, first=11)
    q, _ = oracle_mod.dispatch_windows(win, 64, lens, oracle_mod.cfg(*cfg))
    return q


@pytest.mark.parametrize("cfg", CONFIGS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("profile", [abi.SYN_FUZZ, abi.SYN_IMIX])
def test_segments_give_the_oracle_lists(oracle_mod, profile, n, cfg):
    from yastack_amd import segments

    nq = cfg[1]
    q = _q_ref(oracle_mod, profile, n, cfg)
    qi_ref, qs_ref = oracle_mod.process_burst(q, nq)
    si, so = segments.from_q(q, nq)
    assert si.dtype == np.uint8 and si.shape == (n,)
    assert so.dtype == np.uint16 and so.shape == (segments.nseg_for(n), nq + 2)
    for fn in (segments.to_lists_c, segments.to_lists):
        qi, qs = fn(si, so, n, nq + 1)
        assert np.array_equal(qs, qs_ref), fn.__name__
        assert np.array_equal(qi, qi_ref), fn.__name__
    # every segment on its own is process_burst of its slice of q
    for s in range(segments.nseg_for(n)):
        sl = q[s * 256:(s + 1) * 256]
        li, ls = oracle_mod.process_burst(sl, nq)
        assert so[s, 0] == 0 and so[s, nq + 1] == sl.size
        assert np.array_equal(so[s].astype(np.uint32), ls)
        assert np.array_equal(si[s * 256:s * 256 + sl.size].astype(np.uint32), li)


def test_empty_batch():
    from yastack_amd import segments

    for fn in (segments.to_lists_c, segments.to_lists):
        qi, qs = fn(np.zeros(0, np.uint8), np.zeros((0, 5), np.uint16), 0, 4)
        assert qi.size == 0 and not qs.any() and qs.size == 5


@pytest.mark.parametrize("case", ["non_monotone", "last_offset", "first_offset", "index"])
@pytest.mark.parametrize("n", [257, 700])
def test_corrupted_segments_are_refused(oracle_mod, case, n):
    from yastack_amd import segments

    nq = 3
    q = _q_ref(oracle_mod, abi.SYN_FUZZ, n, (3, 3, 1, 1))
    si, so = segments.from_q(q, nq)
    last = segments.nseg_for(n) - 1          # the short segment: len_s = n - 256 last
    len_s = n - 256 * last
    if case == "non_monotone":
        so[last, 2] = so[last, 1] + 300      # past the next offset
        so[last, 3] = so[last, 1]
    elif case == "last_offset":
        so[last, nq + 1] = 256 if len_s < 256 else 255
    elif case == "first_offset":
        so[0, 0] = 1
    else:
        si[256 * last] = len_s               # one past the segment's last packet
    lib = abi.load()
    qi = np.full(n + 64, 0xAAAAAAAA, np.uint32)
    qs = np.empty(nq + 2, np.uint32)
    rc = lib.yrss_seg_to_lists(si.ctypes.data, so.ctypes.data, n, nq + 1, qi.ctypes.data,
                               qs.ctypes.data)
    assert rc == -errno.EINVAL
    assert np.all(qi[n:] == 0xAAAAAAAA)      # nothing written past the list
    with pytest.raises(ValueError):
        segments.to_lists(si, so, n, nq + 1)
    with pytest.raises(ValueError):
        segments.to_lists_c(si, so, n, nq + 1)


def test_seg_to_lists_refuses_bad_arguments():
    lib = abi.load()
    si = np.zeros(4, np.uint8)
    so = np.zeros(5, np.uint16)
    qi = np.zeros(4, np.uint32)
    qs = np.zeros(5, np.uint32)
    args = (si.ctypes.data, so.ctypes.data, 4, 4, qi.ctypes.data, qs.ctypes.data)
    for k, bad in ((0, None), (1, None), (3, 0), (3, abi.MAX_QUEUES + 2), (4, None), (5, None)):
        a = list(args)
        a[k] = bad
        assert lib.yrss_seg_to_lists(*a) == -errno.EINVAL, k


def test_header_constants_and_exports():
    text = abi.HEADER_PATH.read_text()
    assert int(re.search(r"#define YRSS_SEG_PKTS (\d+)", text).group(1)) == abi.SEG_PKTS == 256
    assert int(re.search(r"#define YRSS_SEG_MAX_BUCKETS (\d+)", text).group(1)) == \
        abi.SEG_MAX_BUCKETS == 16
    sh = re.search(r"#define YRSS_SEG_MAX_BATCH \(1u << (\d+)\)", text)
    assert (1 << int(sh.group(1))) == abi.SEG_MAX_BATCH == 1 << 24
    names = abi.header_functions()
    assert "yrss_dispatch_dev_seg" in names and "yrss_seg_to_lists" in names
    for path in (abi.LIB_PATH, abi.TEST_LIB_PATH):
        out = subprocess.run(["nm", "-D", "--defined-only", str(path)], capture_output=True,
                             text=True, check=True).stdout
        exported = set(re.findall(r"\bT (yrss_\w+)", out))
        assert {"yrss_dispatch_dev_seg", "yrss_seg_to_lists"} <= exported, path
    # struct yrss_dev_seg_batch: five pointers after {win, stride, n}, as declared
    assert ctypes.sizeof(abi.DevSegBatch) == 8 + 4 + 4 + 6 * 8
    body = re.search(r"struct yrss_dev_seg_batch \{(.*?)\};", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(\w+);", body)
    assert fields == [f for f, _ in abi.DevSegBatch._fields_]


def test_dispatch_dev_seg_refuses_short_buffers():
    """SoftRss.dispatch_dev_seg checks the buffers against the batch before the
    C call (which sees raw pointers only)."""
    from yastack_amd import dispatch

    class T:
        def __init__(self, nbytes):
            self.nb = nbytes

        def numel(self):
            return self.nb

        def element_size(self):
            return 1

    n, nq = 300, 3
    good = dict(q=T(2 * n), hash=T(4 * n), filter=T(n), seg_idx=T(n), seg_off=T(2 * 2 * (nq + 2)))
    dispatch._check_seg_sizes(n, 64, T(64 * n), T(2 * n),
                              dispatch.SegResult(**good), nq)
    for name in good:
        bad = dict(good)
        bad[name] = T(good[name].nb - 1)
        with pytest.raises(ValueError, match=name):
            dispatch._check_seg_sizes(n, 64, T(64 * n), T(2 * n), dispatch.SegResult(**bad), nq)
    with pytest.raises(ValueError, match="win"):
        dispatch._check_seg_sizes(n, 64, T(64 * n - 1), T(2 * n), dispatch.SegResult(**good), nq)
