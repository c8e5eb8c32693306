"""The redirection table's model (tests/reta_model.py) against what is pinned,
and the facts the GPU tests (test_gpu_reta.py) rely on.  No GPU.

The table is this build's own semantics (include/yrss.h): an equal-weights
table over a power-of-two queue count must be the reference's own hash % d, and
that is what ties the table path to the reference.
"""
import numpy as np
import pytest

import ext_model as xm
import reta_model as rm
from yastack_amd import abi
from yastack_amd.dispatch import reta_weighted

V, V6, U = abi.EXT_VLAN, abi.EXT_IPV6, abi.EXT_UDP
CFGS = ((3, 3, 1, 1), (8, 8, 1, 0))
# (profile, flags) and the sizes of test_gpu_reta.py's streams
STREAMS = ((abi.SYN_TCP4, 0), (abi.SYN_IMIX, 0), (abi.SYN_UDP4, U), (abi.SYN_VLAN6_TCP, V | V6))
SIZES = (64, 4096, 4097, 20000)


@pytest.mark.parametrize("stride", [64, 80])
def test_equal_table_is_the_oracle(oracle_mod, stride):
    """128 entries of i % 8 under (8, 8, 1, 0): table[h & 127] == h % 8, so the
    table's q is the oracle's own, bit for bit, constants and the window rule
    included."""
    n = 6000
    win, lens = xm.stream(abi.SYN_FUZZ, n, stride)
    q_ref, h_ref = oracle_mod.dispatch_windows(win, stride, lens, oracle_mod.cfg(*rm.CFG_A))
    q0, h, hashed = rm.classify_windows(win, stride, lens, 0, rm.CFG_A)
    assert np.array_equal(q0, q_ref) and np.array_equal(h, h_ref)
    table = reta_weighted([1] * 8, 128)
    assert np.array_equal(table, np.arange(128) % 8)
    assert np.array_equal(rm.apply(table, q0, h, hashed), q_ref)
    # the sample holds every kind the hashed test must tell apart
    assert 1000 < np.count_nonzero(hashed) < n
    assert np.all(h[~hashed] == 0)
    unhashed = set(q_ref[~hashed].tolist())
    assert {0, abi.DEFAULT_Q} <= unhashed <= {0, abi.DEFAULT_Q, abi.Q_TRUNCATED}
    if stride == 64:
        assert abi.Q_TRUNCATED in unhashed
    # and a table that is not the modulo shows on it
    assert not np.array_equal(rm.apply(np.zeros(128, np.uint16), q0, h, hashed), q_ref)


def test_hashed_test_tells_constants_from_hashed_queues():
    """Queue 2 of a hashed packet moves with the offset; the constant 2 does
    not (nor 0, nor YRSS_Q_TRUNCATED)."""
    q_a = np.array([2, 2, 0, 0, abi.Q_TRUNCATED, 7], np.int16)
    q_b = np.array([3, 2, 1, 0, abi.Q_TRUNCATED, 8], np.int16)
    assert rm.hashed_of(q_a, q_b).tolist() == [True, False, True, False, False, True]
    table = np.array([5, 6], np.uint16)
    h = np.array([1, 1, 2, 2, 0, 3], np.uint32)
    assert rm.apply(table, q_a, h, rm.hashed_of(q_a, q_b)).tolist() == \
        [6, 2, 5, 0, abi.Q_TRUNCATED, 6]


def test_streams_are_prefixes():
    """reta_model models a stream's first STREAM_MAX packets once and slices."""
    for profile, _ in STREAMS:
        w_all, l_all = xm.stream(profile, rm.STREAM_MAX, 64)
        for n in SIZES[:3]:
            w, ln = xm.stream(profile, n, 64)
            assert np.array_equal(w, w_all[:n * 64]) and np.array_equal(ln, l_all[:n])


@pytest.mark.parametrize("profile,flags", STREAMS)
def test_weighted_table_moves_the_streams(profile, flags):
    """What the GPU tests assert holds for these seeds: under a (1, 0, 3) table
    no hashed packet goes to queue 1, some go to queues 0 and 2, and the queue
    differs from the table-free one, at every size and for both
    configurations; the table-free model is ext_model's own."""
    for size in (2, 128, 512):
        table = reta_weighted((1, 0, 3), size)
        assert set(table.tolist()) == ({0, 2} if size > 1 else {2})
        for cfg in CFGS:
            for n in SIZES:
                q0, h, hashed = rm.stream_model(profile, n, 64, flags, cfg)
                qx, hx = xm.stream_model(profile, n, 64, flags, cfg)
                assert np.array_equal(q0, qx) and np.array_equal(h, hx)
                q = rm.apply(table, q0, h, hashed)
                assert np.count_nonzero(hashed) >= n // 2
                assert not np.any(q[hashed] == 1), (cfg, n, size)
                assert np.any(q[hashed] == 0) and np.any(q[hashed] == 2), (cfg, n, size)
                assert np.array_equal(q[~hashed], q0[~hashed])
                assert not np.array_equal(q, q0), (cfg, n, size)


@pytest.mark.parametrize("stride", [64, 80])
def test_sweep_has_hashed_truncated_and_constant_packets(stride):
    """The boundary sweep under flags 0 and YRSS_EXT_ALL: a (1, 0, 3) table of
    every size moves some packet and leaves the unhashed and truncated alone."""
    win, lens = xm.sweep_batch(stride)
    for flags in (0, abi.EXT_ALL):
        q0, h, hashed = rm.classify_windows(win, stride, lens, flags, CFGS[0])
        assert np.any(hashed) and not np.all(hashed)
        if stride == 64 or flags:
            assert np.any(q0 == abi.Q_TRUNCATED)
        assert not np.any(hashed & (q0 == abi.Q_TRUNCATED))
        for size in (1, 2, 512):
            q = rm.apply(reta_weighted((1, 0, 3), size), q0, h, hashed)
            assert not np.array_equal(q, q0), (flags, size)
            assert np.array_equal(q[~hashed], q0[~hashed])
