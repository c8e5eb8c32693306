"""Per-packet model of the redirection table (yrss_set_reta; include/yrss.h).

The table is the build's own semantics, so, like tests/ext_model.py, the model
is built from what is already pinned:

* ``ext_model.classify`` for a packet's table-free ``(q0, hash)``: with flags 0
  that is the oracle's ``toeplitz_dispatch``;
* the hashed test: a packet is hashed exactly when its model queue moves with
  the configuration's offset.  ``CFG_A`` and ``CFG_B`` have the same divisor (8)
  and offsets 0 and 1, so a hashed packet has ``q_b == q_a + 1`` while the
  constants (0 for ARP / RARP, ``YRSS_DEFAULT_Q``) and ``YRSS_Q_TRUNCATED`` do
  not move and count as unhashed;
* the table rule itself: ``table[hash & (size - 1)]`` for hashed packets, ``q0``
  otherwise;
* ``oracle.process_burst`` / ``segments`` on that queue for the lists.
"""
from __future__ import annotations

import functools

import numpy as np

import ext_model as xm

CFG_A, CFG_B = (8, 8, 1, 0), (9, 9, 1, 1)
assert xm.modulo(CFG_A) == (8, 0) and xm.modulo(CFG_B) == (8, 1)
STREAM_MAX = 20000     # stream(profile, n) is the first n packets: one model, sliced


def hashed_of(q_a, q_b):
    """The hashed test on the queues under CFG_A and CFG_B."""
    return np.asarray(q_b).astype(np.int32) == np.asarray(q_a).astype(np.int32) + 1


def apply(table, q0, h, hashed):
    """The queue under ``table``: int16[n]."""
    table = np.asarray(table, dtype=np.uint16)
    size = int(table.size)
    assert 1 <= size <= 512 and size & (size - 1) == 0
    tq = table[np.asarray(h, dtype=np.uint32) & np.uint32(size - 1)].astype(np.int16)
    return np.where(hashed, tq, np.asarray(q0, dtype=np.int16)).astype(np.int16)


def classify_frames(frames, flags, cfg, stride=80):
    """(q0 int16[n], hash uint32[n], hashed bool[n]) of host frames staged in
    windows of ``stride`` bytes."""
    def run(c):
        got = [xm.classify(f, len(f), flags, c, stride=stride) for f in frames]
        return np.array([g[0] for g in got], np.int16), np.array([g[1] for g in got], np.uint32)
    q_a, h = run(CFG_A)
    q_b, _ = run(CFG_B)
    q0 = q_a if tuple(cfg) == CFG_A else run(cfg)[0]
    return q0, h, hashed_of(q_a, q_b)


def classify_windows(win, stride, lens, flags, cfg):
    """(q0, hash, hashed) of a batch of header windows."""
    q_a, h = xm.classify_windows(win, stride, lens, flags, CFG_A)
    q_b, h_b = xm.classify_windows(win, stride, lens, flags, CFG_B)
    assert np.array_equal(h, h_b)          # the hash knows no configuration
    q0 = q_a if tuple(cfg) == CFG_A else xm.classify_windows(win, stride, lens, flags, cfg)[0]
    return q0, h, hashed_of(q_a, q_b)


@functools.lru_cache(maxsize=None)
def _stream_full(profile, stride, flags, cfg):
    q_a, h = xm.stream_model(profile, STREAM_MAX, stride, flags, CFG_A)
    q_b, _ = xm.stream_model(profile, STREAM_MAX, stride, flags, CFG_B)
    q0, h0 = xm.stream_model(profile, STREAM_MAX, stride, flags, cfg)
    assert np.array_equal(h, h0)
    hashed = hashed_of(q_a, q_b)
    hashed.setflags(write=False)
    return q0, h, hashed


def stream_model(profile, n, stride, flags, cfg):
    """(q0, hash, hashed) of ext_model.stream(profile, n, stride): read-only
    views of one model of the first STREAM_MAX packets."""
    assert n <= STREAM_MAX
    return tuple(a[:n] for a in _stream_full(profile, stride, flags, tuple(cfg)))


lists = xm.lists
seg_lists = xm.seg_lists
