"""Tuples with a chosen Toeplitz hash, for directed tests of the modulo.

The Toeplitz hash is linear over GF(2): the hash of a 12-byte tuple is the XOR
of the key's 32-bit windows at the positions of its set bits (bit 8 j + b is
bit 0x80 >> b of byte j).  Where the windows of the free bytes have rank 32,
every 32-bit hash is reachable, and a tuple for it falls out of Gaussian
elimination.  Plain Python integers throughout; nothing here touches a GPU.
"""
from __future__ import annotations

import socket

from frames import ipv4_frame


class UnreachableHash(ValueError):
    """No choice of the free tuple bytes gives the hash asked for."""


def key_windows(key: bytes, keylen: int) -> list[int]:
    """The 96 32-bit key windows of a 12-byte input (oracle_build_tables): window
    k holds key bits k .. k + 31, MSB first; bits past keylen bytes are zero."""
    bits = int.from_bytes(bytes(key[:keylen]).ljust(16, b"\0")[:16], "big")
    return [(bits >> (128 - 32 - k)) & 0xFFFFFFFF for k in range(96)]


def _hash(windows, t: bytes) -> int:
    h = 0
    for j in range(12):
        for b in range(8):
            if t[j] & (0x80 >> b):
                h ^= windows[8 * j + b]
    return h


def _basis(windows, free_bytes):
    """XOR basis of the free bytes' windows: {pivot bit: (vector, the set of
    tuple bits (bit i = 1 << i) whose windows XOR to it)}."""
    basis = {}
    for j in free_bytes:
        for i in range(8 * j, 8 * j + 8):
            v, combo = windows[i], 1 << i
            while v:
                p = v.bit_length() - 1
                if p not in basis:
                    basis[p] = (v, combo)
                    break
                v ^= basis[p][0]
                combo ^= basis[p][1]
    return basis


def window_rank(key: bytes, keylen: int, free_bytes=range(12)) -> int:
    """Rank over GF(2) of the windows under the free tuple bytes: the hashes
    reachable by varying them form a coset of dimension rank."""
    return len(_basis(key_windows(key, keylen), tuple(free_bytes)))


def solve_tuple(key: bytes, keylen: int, h: int, free_bytes=range(12),
                base: bytes = bytes(12)) -> bytes:
    """A 12-byte tuple, equal to ``base`` outside ``free_bytes``, whose Toeplitz
    hash under key[:keylen] is ``h``.  Raises UnreachableHash where none is."""
    if not 0 <= h < 1 << 32:
        raise ValueError(f"hash {h:#x} is not a 32-bit value")
    if len(base) != 12:
        raise ValueError("base must be 12 bytes")
    free_bytes = tuple(free_bytes)
    windows = key_windows(key, keylen)
    basis = _basis(windows, free_bytes)
    v = h ^ _hash(windows, base)       # what flipping free bits has to add
    flip = 0
    while v:
        p = v.bit_length() - 1
        if p not in basis:
            raise UnreachableHash(
                f"hash {h:#010x} is not reachable from base {bytes(base).hex()} through bytes "
                f"{list(free_bytes)} at key length {keylen} (rank {len(basis)})")
        v ^= basis[p][0]
        flip ^= basis[p][1]
    t = bytearray(base)
    for i in range(96):
        if flip >> i & 1:
            t[i >> 3] ^= 0x80 >> (i & 7)
    assert _hash(windows, t) == h
    return bytes(t)


def tcp_frame_for_tuple(t: bytes, ihl: int = 5, length: int = 64) -> bytes:
    """An Ethernet/IPv4/TCP frame whose toeplitz_dispatch tuple is ``t``.  The
    dispatcher hashes ntohl(src), ntohl(dst), ntohs(sport), ntohs(dport) as
    they lie in little-endian memory (oracle/yrss_oracle.c, dispatch_one), so
    each field of ``t`` is the wire field reversed."""
    if len(t) != 12:
        raise ValueError("tuple must be 12 bytes")
    src = socket.inet_ntoa(bytes(t[3::-1]))
    dst = socket.inet_ntoa(bytes(t[7:3:-1]))
    sport = t[9] << 8 | t[8]
    dport = t[11] << 8 | t[10]
    return ipv4_frame(src, sport, dst, dport, ihl=ihl, length=length)


def edge_hashes(d: int) -> list[int]:
    """The hashes at which a reciprocal modulo by d, or a mask of the wrong
    width, goes wrong: around 0, d and 2 d, around the largest multiple of d
    below 2^32, around 2^31 and at the top of the range."""
    m = ((2**32 - 1) // d) * d
    vals = {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d,
            m - 1, m, m + 1,
            2**31 - 1, 2**31, 2**32 - d, 2**32 - 2, 2**32 - 1}
    return sorted(v for v in vals if 0 <= v < 2**32)
