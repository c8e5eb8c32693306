"""The ABI surface of the redirection table (yrss_set_reta, yrss_get_reta,
yrss_reta_fill_weighted) and the weighted fill against a Python restatement of
the algorithm the header states.  No GPU: the fill is pure host code and the
two context calls are only checked for their argument errors.
"""
import ctypes
import errno
import re
import subprocess

import numpy as np
import pytest

from yastack_amd import abi
from yastack_amd.dispatch import SoftRss, reta_weighted

SIZES = (1, 2, 128, 512)


def swrr(weights, size):
    """Smooth weighted round-robin as include/yrss.h states it: a running value
    per queue, 0 at the start; for each slot add each queue's weight to its
    value, take the largest (the lowest index on ties), subtract the sum of
    the weights from it, write its id."""
    cur = [0] * len(weights)
    total = sum(weights)
    out = []
    for _ in range(size):
        cur = [c + w for c, w in zip(cur, weights)]
        best = max(range(len(weights)), key=lambda k: (cur[k], -k))
        cur[best] -= total
        out.append(best)
    return np.array(out, np.uint16)


BIG = 1 << 31
WEIGHTS = {
    "equal3": (1, 1, 1),
    "equal8": (7,) * 8,
    "1-0-3": (1, 0, 3),
    "one-nonzero": (0, 0, 5, 0),
    "255x1": (1,) * 255,
    "near-2^31": (BIG - 1, BIG, BIG + 1, 1, BIG - 2),
    "max-u32": (0xFFFFFFFF, 0xFFFFFFFE, 1),
}


def test_header_constants_and_entry_points():
    text = abi.HEADER_PATH.read_text()
    assert re.search(r"#define YRSS_RETA_MAX 512\b", text)
    assert abi.RETA_MAX == 512
    for proto in (r"int yrss_set_reta\(yrss_ctx \*ctx, const uint16_t \*table, uint32_t size\);",
                  r"int yrss_get_reta\(yrss_ctx \*ctx, uint16_t \*table, uint32_t cap\);",
                  r"int yrss_reta_fill_weighted\(uint16_t \*table, uint32_t size,\s*"
                  r"const uint32_t \*weights, uint32_t nb_queues\);"):
        assert re.search(proto, text), proto
    names = ("yrss_set_reta", "yrss_get_reta", "yrss_reta_fill_weighted")
    assert set(names) <= set(abi.header_functions())
    # labelled as the build's own semantics, like the extended mode
    assert re.search(r"redirection table: THIS BUILD'S OWN SEMANTICS, NOT fs/lib's", text)
    lib = abi.load()
    assert lib.yrss_set_reta.argtypes == [abi._vp, abi._vp, abi._u32]
    assert lib.yrss_get_reta.argtypes == [abi._vp, abi._vp, abi._u32]
    assert lib.yrss_reta_fill_weighted.argtypes == [abi._vp, abi._u32, abi._vp, abi._u32]
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    for n in names:
        assert re.search(rf"\bT {n}\b", out), n
    # no context: an argument error, and no GPU call
    t = np.zeros(4, np.uint16)
    assert lib.yrss_set_reta(None, t.ctypes.data, 4) == -errno.EINVAL
    assert lib.yrss_get_reta(None, t.ctypes.data, 4) == -errno.EINVAL
    assert hasattr(SoftRss, "set_reta") and hasattr(SoftRss, "get_reta")
    # struct yrss_config is untouched (its size is pinned by test_abi.py)
    assert ctypes.sizeof(abi.Config) == 68


@pytest.mark.parametrize("name", WEIGHTS)
def test_fill_weighted_is_the_stated_algorithm(name):
    w = WEIGHTS[name]
    total = sum(w)
    for size in SIZES:
        got = reta_weighted(w, size)
        assert got.dtype == np.uint16 and got.shape == (size,)
        assert np.array_equal(got, swrr(w, size)), (name, size)
        counts = np.bincount(got, minlength=len(w))
        for k, wk in enumerate(w):
            # within 1 of size * w / W, in exact integers
            assert abs(int(counts[k]) * total - size * wk) <= total, (name, size, k, counts[k])
            if wk == 0:
                assert counts[k] == 0, (name, size, k)


def test_equal_weights_are_round_robin():
    for nq in (1, 2, 3, 8, 61, 255, 256):
        for size in SIZES:
            assert np.array_equal(reta_weighted([5] * nq, size), np.arange(size) % nq), (nq, size)


def test_fill_weighted_argument_errors():
    lib = abi.load()
    t = np.full(1024, 0x7777, np.uint16)
    w = np.array([1, 2, 3], np.uint32)
    z = np.zeros(3, np.uint32)

    def fill(table, size, weights, nq):
        return lib.yrss_reta_fill_weighted(None if table is None else table.ctypes.data, size,
                                           None if weights is None else weights.ctypes.data, nq)
    assert fill(t, 128, w, 3) == 0
    assert np.all(t[128:] == 0x7777)               # nothing past the size
    t[:] = 0x7777
    for size in (0, 3, 96, 513, 1024, 1 << 31):
        assert fill(t, size, w, 3) == -errno.EINVAL, size
    assert fill(t, 128, z, 3) == -errno.EINVAL     # all weights 0
    assert fill(t, 128, w, 0) == -errno.EINVAL     # no queue
    assert fill(t, 128, np.ones(300, np.uint32), 257) == -errno.EINVAL   # > YRSS_MAX_QUEUES
    assert fill(None, 128, w, 3) == -errno.EINVAL
    assert fill(t, 128, None, 3) == -errno.EINVAL
    assert np.all(t == 0x7777)                     # a refused call writes nothing
    with pytest.raises(abi.YrssError) as e:
        reta_weighted((0, 0), 128)
    assert e.value.errno == errno.EINVAL
    with pytest.raises(abi.YrssError):
        reta_weighted((1, 2), 100)
    with pytest.raises(ValueError):
        reta_weighted((1, -2), 128)
    assert np.array_equal(reta_weighted((1, 1)), np.arange(128) % 2)   # size defaults to 128
