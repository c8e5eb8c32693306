"""The directed-hash helper (tests/rss_tuples.py) against the oracle, on the CPU:
solved tuples hash to their targets, the frames built from them dispatch to
the queue plain integers give, and an unreachable hash is an error."""
import numpy as np
import pytest

from rss_tuples import (UnreachableHash, edge_hashes, key_windows, solve_tuple,
                        tcp_frame_for_tuple, window_rank)

KEY2 = bytes(range(7, 47))
DIVISORS = (3, 7, 255, 4095)


def _keys(oracle_mod):
    return [(k, kl) for k in (oracle_mod.MLX_KEY, KEY2) for kl in (5, 15, 16, 40)]


def test_key_windows_are_the_hash_of_single_bits(oracle_mod):
    for key, kl in _keys(oracle_mod) + [(KEY2, 4), (KEY2, 10), (KEY2, 11)]:
        w = key_windows(key, kl)
        assert len(w) == 96
        for i in range(96):
            t = bytearray(12)
            t[i >> 3] = 0x80 >> (i & 7)
            assert oracle_mod.toeplitz_hash(bytes(t), key[:kl]) == w[i], (kl, i)


def test_rank_32_from_key_length_5(oracle_mod):
    for key, kl in _keys(oracle_mod):
        assert window_rank(key, kl) == 32, kl


@pytest.mark.parametrize("kl", [5, 15, 16, 40])
@pytest.mark.parametrize("which", [0, 1])
def test_solved_tuples_hash_and_dispatch(oracle_mod, which, kl):
    key = (oracle_mod.MLX_KEY, KEY2)[which]
    rng = np.random.default_rng(100 * which + kl)
    cases = [(int(h), None) for h in rng.integers(0, 1 << 32, 200, dtype=np.uint64)]
    cases += [(h, d) for d in DIVISORS for h in edge_hashes(d)]
    for k, (h, d) in enumerate(cases):
        base = bytes(rng.integers(0, 256, 12, dtype=np.uint8))
        t = solve_tuple(key, kl, h, base=base)
        assert len(t) == 12
        assert oracle_mod.toeplitz_hash(t, key[:kl]) == h
        f = tcp_frame_for_tuple(t)
        for dd in (DIVISORS if d is None else (d,)):
            for only in (0, 1):       # h % d, and h % d + 1 behind a dispatch-only core
                c = oracle_mod.cfg(dd + only, min(dd + only, 256), 1, only, key=key[:kl])
                assert oracle_mod.toeplitz_dispatch(f, 64, c) == (h % dd + only, h), (h, dd)


def test_frame_tuple_byte_order(oracle_mod):
    """Every tuple byte lands where the dispatcher reads it, at every header
    length the tests use."""
    t = bytes(range(1, 13))
    want = oracle_mod.toeplitz_hash(t)
    for ihl, length in ((5, 64), (12, 100), (15, 100)):
        f = tcp_frame_for_tuple(t, ihl=ihl, length=length)
        assert len(f) >= length
        assert oracle_mod.toeplitz_dispatch(f, length, oracle_mod.cfg(8, 8, 1, 0)) == \
            (want % 8, want)
    f = tcp_frame_for_tuple(t)
    assert f[26:30] == bytes([4, 3, 2, 1]) and f[30:34] == bytes([8, 7, 6, 5])
    assert f[34:38] == bytes([10, 9, 12, 11])


def test_base_kept_outside_free_bytes(oracle_mod):
    base = bytes(range(0x50, 0x5C))
    t = solve_tuple(KEY2, 40, 0xDEADBEEF, free_bytes=range(4, 12), base=base)
    assert t[:4] == base[:4]
    assert oracle_mod.toeplitz_hash(t, KEY2) == 0xDEADBEEF


def test_key_length_4_is_rank_deficient_and_says_so(oracle_mod):
    for key in (oracle_mod.MLX_KEY, KEY2):
        r = window_rank(key, 4)
        assert r < 32
        missing = []
        for b in range(32):
            try:
                t = solve_tuple(key, 4, 1 << b)
            except UnreachableHash:
                missing.append(1 << b)
            else:
                assert oracle_mod.toeplitz_hash(t, key[:4]) == 1 << b
        assert missing, "rank < 32 leaves some single-bit hash out of reach"
        with pytest.raises(UnreachableHash, match="not reachable"):
            solve_tuple(key, 4, missing[0])
    with pytest.raises(ValueError):
        solve_tuple(KEY2, 40, 1 << 32)


def test_lport_bytes_rank(oracle_mod):
    """Bytes 10..11 (the lport of the connect-side check) meet key bytes 10..15:
    rank 16 under a full key, rank 0 under a key of 10 bytes or less."""
    for key in (oracle_mod.MLX_KEY, KEY2):
        assert window_rank(key, 40, (10, 11)) == 16
        assert window_rank(key, 15, (10, 11)) == 16
        assert window_rank(key, 5, (10, 11)) == 0
        assert window_rank(key, 10, (10, 11)) == 0
        assert window_rank(key, 11, (10, 11)) > 0
        base = bytes(range(12))
        h0 = oracle_mod.toeplitz_hash(base, key[:5])
        assert solve_tuple(key, 5, h0, free_bytes=(10, 11), base=base) == base
        with pytest.raises(UnreachableHash):
            solve_tuple(key, 5, h0 ^ 1, free_bytes=(10, 11), base=base)


def test_edge_hashes():
    # 2^32 - 1 is a multiple of 3: m + 1 falls outside and is dropped
    assert edge_hashes(3) == [0, 1, 2, 3, 4, 5, 6, 2**31 - 1, 2**31, 2**32 - 3, 2**32 - 2,
                              2**32 - 1]
    # 7 * 613566756 = 4294967292 is the largest multiple of 7 below 2^32
    assert edge_hashes(7) == [0, 1, 6, 7, 8, 13, 14, 2**31 - 1, 2**31, 2**32 - 7, 4294967291,
                              4294967292, 4294967293, 2**32 - 2, 2**32 - 1]
    for d in (1, 2, 3, 7, 255, 256, 4095, 4096, 65535):
        e = edge_hashes(d)
        m = (2**32 - 1) // d * d
        assert e == sorted(set(e)) and all(0 <= v < 2**32 for v in e)
        assert {0, d - 1, d, m, 2**32 - 1} <= set(e)
        assert m % d == 0 and m + d > 2**32 - 1
        # every remainder class the modulo's ends can take is present
        assert {0, d - 1} <= {v % d for v in e}
