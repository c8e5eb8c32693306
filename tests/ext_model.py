"""Per-packet model of the extended mode (yrss_set_extended; include/yrss.h).

This is the build's own semantics, so there is no fs/lib code to restate.  The
model is built from what is already pinned instead:

* ``oracle.toeplitz_dispatch`` (the restated reference dispatcher) on the frame
  with its VLAN tags removed and ``len - 4t``, with byte 23 rewritten from 17
  to 6 where UDP takes the TCP branch: q and hash of every IPv4 / ARP / other
  frame, all the reference's length quirks included;
* ``oracle.toeplitz_hash`` (pinned to the reference's compiled toeplitz_hash
  for any data length) on the 36 wire-order bytes of an IPv6 tuple;
* ``oracle.process_burst`` / ``segments`` for the lists.

The one rule added at the boundary is the window rule the plain mode already
has: a hashed packet whose ports end beyond the staged window is
``YRSS_Q_TRUNCATED`` with hash 0.
"""
from __future__ import annotations

import functools

import numpy as np

from oracle import oracle
from yastack_amd import abi, segments

KEY_82599 = bytes.fromhex(
    "6d5a56da255b0ec24167253d43a38fb0d0ca2bcbae7b30b477cb2da38030f20c6a42b73bbeac01fa")
ALL_FLAG_SETS = tuple(range(8))


def modulo(cfg_tuple):
    """(d, offset) of hash % d + offset (ff_dpdk_if.c:2031-2034)."""
    npr, _nq, soft, only = cfg_tuple
    return (npr - 1, 1) if soft and only else (npr, 0)


def strip_tags(frame: bytes, length: int, flags: int):
    """(stripped frame, stripped length, tags) or None when the frame is too
    short to hold its tag(s) and the inner ethertype."""
    t = 0
    if (flags & abi.EXT_VLAN) and length >= 14 and frame[12:14] in (b"\x81\x00", b"\x88\xa8"):
        if length < 18:
            return None
        t = 1
        if frame[16:18] == b"\x81\x00":
            if length < 22:
                return None
            t = 2
    return frame[:12] + frame[12 + 4 * t:], length - 4 * t, t


def classify(frame: bytes, length: int, flags: int, cfg_tuple, key: bytes = oracle.MLX_KEY,
             stride: int | None = None):
    """(q, hash) of one frame under ``flags``.  frame: at least the bytes the
    rules may read (it is zero-padded here); stride: the staged window, None
    for a window that holds everything."""
    c = oracle.cfg(*cfg_tuple, key=key)
    frame = bytes(frame) + bytes(112)
    st = strip_tags(frame, length, flags)
    if st is None:
        return abi.DEFAULT_Q, 0
    s, ls, t = st
    o = 14 + 4 * t
    et = s[12:14] if ls >= 14 else b""
    if et == b"\x86\xdd" and (flags & abi.EXT_IPV6):
        nh = s[20]
        if ls - 14 >= 44 and (nh == 6 or (nh == 17 and (flags & abi.EXT_UDP))):
            if stride is not None and o + 44 > stride:
                return abi.Q_TRUNCATED, 0
            h = oracle.toeplitz_hash(s[22:58], key)
            d, off = modulo(cfg_tuple)
            return h % d + off, h
        return abi.DEFAULT_Q, 0
    if et == b"\x08\x00":
        real = s
        if (flags & abi.EXT_UDP) and s[23] == 17:
            s = s[:23] + b"\x06" + s[24:]
        ihl4 = (s[14] & 0x0F) << 2
        # the reference's own conditions for hashing (ff_dpdk_if.c:1968-1986)
        hashed = ls - 14 >= 20 and ls - 14 >= ihl4 and ls - ihl4 >= 20 and s[23] == 6
        if hashed and stride is not None and o + ihl4 + 4 > stride:
            return abi.Q_TRUNCATED, 0
        p = 14 + ihl4
        if hashed and s is not real and p <= 23 < p + 4:
            # IHL 2 puts the "ports" on bytes 22..25: the rewritten protocol
            # byte is one of them.  The rewrite only selects the TCP branch;
            # the tuple is the frame's own bytes, in the order of :1998-2021.
            t12 = bytes(real[i] for i in (29, 28, 27, 26, 33, 32, 31, 30, p + 1, p, p + 3, p + 2))
            h = oracle.toeplitz_hash(t12, key)
            d, off = modulo(cfg_tuple)
            return h % d + off, h
    return oracle.toeplitz_dispatch(s, ls, c)


def classify_windows(win: np.ndarray, stride: int, lens: np.ndarray, flags: int, cfg_tuple,
                     key: bytes = oracle.MLX_KEY):
    """(q int16[n], hash uint32[n]) of a batch of header windows."""
    lens = np.asarray(lens).view(np.uint16)
    n = int(lens.size)
    raw = np.ascontiguousarray(win, dtype=np.uint8).tobytes()
    q = np.empty(n, np.int16)
    h = np.empty(n, np.uint32)
    for i in range(n):
        q[i], h[i] = classify(raw[i * stride:(i + 1) * stride], int(lens[i]), flags, cfg_tuple,
                              key, stride)
    return q, h


@functools.lru_cache(maxsize=None)
def stream(profile: int, n: int, stride: int):
    """The first n packets of a synthetic stream on the host (read-only)."""
    win, lens = oracle.synth(profile, n, stride=stride)
    win.setflags(write=False)
    lens.setflags(write=False)
    return win, lens


@functools.lru_cache(maxsize=None)
def stream_model(profile: int, n: int, stride: int, flags: int, cfg_tuple):
    """The model's (q, hash) of stream(profile, n, stride), computed once."""
    win, lens = stream(profile, n, stride)
    q, h = classify_windows(win, stride, lens, flags, cfg_tuple)
    q.setflags(write=False)
    h.setflags(write=False)
    return q, h


def lists(q: np.ndarray, nb_queues: int):
    """(qidx, qstart) of a q array: process_packets' per-queue FIFO lists."""
    return oracle.process_burst(np.ascontiguousarray(q), nb_queues)


def seg_lists(q: np.ndarray, nb_queues: int):
    return segments.from_q(q, nb_queues)


# ---- frames ---------------------------------------------------------------------

ETH = bytes.fromhex("020000000002020000000001")


def tag_bytes(tags: int, outer: int = 0x8100) -> bytes:
    """0, 1 or 2 VLAN tags (TPID + TCI each, without the final ethertype):
    ``outer`` as the first TPID, 0x8100 as the second."""
    out = b""
    for k in range(tags):
        tpid = outer if k == 0 else 0x8100
        out += tpid.to_bytes(2, "big") + (0x0064 + k).to_bytes(2, "big")
    return out


def with_tags(frame: bytes, tags: int, outer: int = 0x8100) -> bytes:
    """An untagged frame with ``tags`` tags put in front of its ethertype."""
    return frame[:12] + tag_bytes(tags, outer) + frame[12:]


def ipv6_frame(src: bytes, dst: bytes, ports: bytes, nh: int = 6, size: int = 96) -> bytes:
    """Untagged Eth/IPv6 frame: 16-byte addresses, the four port bytes."""
    b = bytearray(size)
    b[0:12] = ETH
    b[12:14] = b"\x86\xdd"
    b[14] = 0x60
    b[18:20] = (size - 54).to_bytes(2, "big") if size >= 54 else b"\0\0"
    b[20] = nh
    b[21] = 64
    b[22:38] = src
    b[38:54] = dst
    b[54:58] = ports
    return bytes(b)


def ipv4_frame(src: bytes, dst: bytes, ports: bytes, proto: int = 6, ihl: int = 5,
               size: int = 112) -> bytes:
    """Untagged Eth/IPv4 frame with the ports at 14 + 4 IHL; the bytes between
    are a non-zero pattern, so a parse that looks in the wrong place shows."""
    b = bytearray((0xA0 + (i & 0x3F)) for i in range(size))
    b[0:12] = ETH
    b[12:14] = b"\x08\x00"
    b[14] = 0x40 | ihl
    b[23] = proto
    b[26:30] = src
    b[30:34] = dst
    p = 14 + 4 * ihl
    b[p:p + 4] = ports
    return bytes(b)


def arp_frame(size: int = 96) -> bytes:
    b = bytearray(size)
    b[0:12] = ETH
    b[12:14] = b"\x08\x06"
    return bytes(b)


def sweep_batch(stride: int):
    """The boundary sweep's batch for one stride: (win uint8[n * stride], lens
    uint16[n]).  Every data_len 0..90 of every frame kind: 0, 1 and 2 tags
    (0x88A8 outside when there are two, both TPIDs when there is one) in front
    of IPv4 TCP / UDP at IHL 5, 11, 12, 15, IPv6 TCP / UDP / next-header 0 and
    44, and ARP.  The window holds min(len, stride) frame bytes and 0xEE
    beyond, so a rule that reads past the data shows."""
    rng = np.random.default_rng(82599)
    kinds = []
    for tags, outer in ((0, 0), (1, 0x8100), (1, 0x88A8), (2, 0x88A8), (2, 0x8100)):
        def put(f, tags=tags, outer=outer):
            kinds.append(with_tags(f, tags, outer) if tags else f)
        for proto in (6, 17):
            for ihl in (5, 11, 12, 15):
                put(ipv4_frame(rng.bytes(4), rng.bytes(4), rng.bytes(4), proto, ihl))
        for nh in (6, 17, 0, 44):
            put(ipv6_frame(rng.bytes(16), rng.bytes(16), rng.bytes(4), nh, 112))
        put(arp_frame(112))
    wins, lens = [], []
    for f in kinds:
        for length in range(0, 91):
            have = min(length, stride)
            wins.append(f[:have] + b"\xEE" * (stride - have))
            lens.append(length)
    return (np.frombuffer(b"".join(wins), np.uint8).copy(), np.array(lens, np.uint16))
