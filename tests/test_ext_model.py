"""The extended mode's model (tests/ext_model.py) against what is pinned, and
the ABI surface of yrss_set_extended.  No GPU.

The extended mode is this build's own semantics (include/yrss.h), so its
hashes are checked against the 82599 datasheet vectors, its IPv4 side against
the restated reference on the stripped frame, and with no flag it must be the
reference itself.
"""
import json
import re
import subprocess

import numpy as np
import pytest

import ext_model as xm
from yastack_amd import abi

V, V6, U = abi.EXT_VLAN, abi.EXT_IPV6, abi.EXT_UDP
CFGS = ((3, 3, 1, 1), (8, 8, 1, 0))
FRAMINGS = ((0, 0), (1, 0x8100), (2, 0x88A8))   # Eth/IPv6/TCP, Eth/VLAN/IPv6/TCP, QinQ


@pytest.fixture(scope="module")
def v6_vectors(golden_dir):
    g = json.loads((golden_dir / "thash_82599.json").read_text())
    assert bytes.fromhex(g["key"]) == xm.KEY_82599
    return [(bytes.fromhex(v["l3l4"]), v["hash_l3l4"]) for v in g["v6"]]


def test_ipv6_vectors_in_three_framings(v6_vectors):
    assert len(v6_vectors) == 3
    for tup, want in v6_vectors:
        assert len(tup) == 36
        for tags, outer in FRAMINGS:
            f = xm.with_tags(xm.ipv6_frame(tup[:16], tup[16:32], tup[32:]), tags, outer)
            for cfg in CFGS:
                d, off = xm.modulo(cfg)
                q, h = xm.classify(f, len(f), V | V6, cfg, key=xm.KEY_82599)
                assert (q, h) == (want % d + off, want)
            # without the flag that reaches it the frame is the reference's queue 2
            assert xm.classify(f, len(f), V, CFGS[0], key=xm.KEY_82599) == (2, 0)
            if tags:
                assert xm.classify(f, len(f), V6 | U, CFGS[0], key=xm.KEY_82599) == (2, 0)


def _sample_frames(oracle_mod):
    """Untagged frames of every kind the rules tell apart, from the synthetic
    streams (80-byte windows) and hand-built IPv6."""
    out = []
    for prof in (abi.SYN_FUZZ, abi.SYN_IMIX, abi.SYN_TCP4, abi.SYN_UDP4):
        win, lens = oracle_mod.synth(prof, 300, stride=80)
        for i in range(300):
            f = win[i * 80:(i + 1) * 80].tobytes()
            if f[12:14] not in (b"\x81\x00", b"\x88\xa8"):
                out.append((f, int(lens[i])))
    rng = np.random.default_rng(6)
    for nh in (6, 17, 0, 44):
        for size in (57, 58, 64, 90):
            f = xm.ipv6_frame(rng.bytes(16), rng.bytes(16), rng.bytes(4), nh, 96)
            out.append((f, size))
    out.append((xm.arp_frame(), 60))
    return out


def test_tag_invariance(oracle_mod):
    """A tagged frame is classified as the same frame without its tags and with
    len - 4t, under every flag set that has YRSS_EXT_VLAN."""
    frames = _sample_frames(oracle_mod)
    assert len(frames) > 900
    differs = 0
    for flags in (V, V | V6, V | U, V | V6 | U):
        for f, length in frames:
            want = xm.classify(f, length, flags, CFGS[1])
            for tags, outer in ((1, 0x8100), (1, 0x88A8), (2, 0x88A8), (2, 0x8100)):
                got = xm.classify(xm.with_tags(f, tags, outer), length + 4 * tags, flags, CFGS[1])
                assert got == want, (flags, tags, hex(outer), length, f[:40].hex())
            differs += want != (2, 0)
    assert differs > 1000    # (the sample is not all queue 2)


def test_udp_takes_the_tcp_branch(oracle_mod):
    rng = np.random.default_rng(17)
    for _ in range(50):
        a, b, p = rng.bytes(4), rng.bytes(4), rng.bytes(4)
        for ihl in (5, 8, 15):
            tcp, udp = xm.ipv4_frame(a, b, p, 6, ihl), xm.ipv4_frame(a, b, p, 17, ihl)
            want = xm.classify(tcp, 100, 0, CFGS[1])
            assert want == oracle_mod.toeplitz_dispatch(tcp, 100, oracle_mod.cfg(*CFGS[1]))
            assert want[1] != 0
            assert xm.classify(udp, 100, U, CFGS[1]) == want
            assert xm.classify(udp, 100, V | V6, CFGS[1]) == (2, 0)
        a6, b6 = rng.bytes(16), rng.bytes(16)
        tcp6, udp6 = xm.ipv6_frame(a6, b6, p, 6), xm.ipv6_frame(a6, b6, p, 17)
        want = xm.classify(tcp6, 90, V6, CFGS[1])
        assert want[1] == oracle_mod.toeplitz_hash(a6 + b6 + p)
        assert xm.classify(udp6, 90, V6 | U, CFGS[1]) == want
        assert xm.classify(udp6, 90, V6, CFGS[1]) == (2, 0)


@pytest.mark.parametrize("stride", [64, 80])
def test_no_flag_is_the_oracle(oracle_mod, stride):
    n = 6000
    win, lens = xm.stream(abi.SYN_FUZZ, n, stride)
    for cfg in CFGS:
        q_ref, h_ref = oracle_mod.dispatch_windows(win, stride, lens, oracle_mod.cfg(*cfg))
        q, h = xm.classify_windows(win, stride, lens, 0, cfg)
        assert np.array_equal(q, q_ref) and np.array_equal(h, h_ref)
        if stride == 64:
            assert np.any(q_ref == abi.Q_TRUNCATED)   # the window rule is in the sample


def test_window_rule_on_tagged_frames():
    """Ports that end beyond the staged window: QinQ + IPv6 at stride 64 (byte
    66) but not at 80; tags + a large IHL at both."""
    rng = np.random.default_rng(3)
    f6 = xm.with_tags(xm.ipv6_frame(rng.bytes(16), rng.bytes(16), rng.bytes(4)), 2, 0x88A8)
    assert xm.classify(f6, 90, V | V6, CFGS[1], stride=64) == (abi.Q_TRUNCATED, 0)
    assert xm.classify(f6, 90, V | V6, CFGS[1], stride=80) == xm.classify(f6, 90, V | V6, CFGS[1])
    assert xm.classify(f6, 90, V | V6, CFGS[1], stride=80)[1] != 0
    f4 = xm.with_tags(xm.ipv4_frame(rng.bytes(4), rng.bytes(4), rng.bytes(4), 6, 15), 1)
    assert xm.classify(f4, 100, V, CFGS[1], stride=80) == (abi.Q_TRUNCATED, 0)
    assert xm.classify(f4, 100, V, CFGS[1], stride=96)[1] != 0
    # the sweep holds the rule at both strides, and more of it at 64
    for stride, flags in ((64, V | V6 | U), (80, V | V6 | U)):
        win, lens = xm.sweep_batch(stride)
        q, _ = xm.classify_windows(win, stride, lens, flags, CFGS[1])
        assert np.count_nonzero(q == abi.Q_TRUNCATED) > (200 if stride == 64 else 20)
    win, lens = xm.sweep_batch(80)
    q, _ = xm.classify_windows(win, 80, lens, V6 | U, CFGS[1])
    assert not np.any(q == abi.Q_TRUNCATED)   # untagged: 80 bytes hold every port


STREAM_CASES = ((abi.SYN_VLAN6_TCP, V | V6), (abi.SYN_UDP4, U))
STREAM_SIZES = (64, 4096, 4097, 20000)


@pytest.mark.parametrize("profile,flags", STREAM_CASES)
def test_streams_reach_every_queue(profile, flags):
    """What the GPU test asserts of the device's lists holds for these seeds:
    every reachable queue of both configs is non-empty at every size, and with
    no flag the whole stream sits on queue 2."""
    for cfg in CFGS:
        d, off = xm.modulo(cfg)
        for n in STREAM_SIZES:
            q, h = xm.stream_model(profile, n, 64, flags, cfg)
            assert set(q.tolist()) == set(range(off, off + d)), (cfg, n)
            assert np.all(h != 0)
        q0, h0 = xm.stream_model(profile, 4097, 64, 0, cfg)
        assert np.all(q0 == 2) and not h0.any()


def test_header_constants_and_entry_point():
    text = abi.HEADER_PATH.read_text()
    consts = dict(re.findall(r"#define (YRSS_EXT_\w+)\s+(0x[0-9a-f]+)u", text))
    assert {k: int(v, 16) for k, v in consts.items()} == {
        "YRSS_EXT_VLAN": abi.EXT_VLAN, "YRSS_EXT_IPV6": abi.EXT_IPV6, "YRSS_EXT_UDP": abi.EXT_UDP,
        "YRSS_EXT_ALL": abi.EXT_ALL}
    assert abi.EXT_ALL == abi.EXT_VLAN | abi.EXT_IPV6 | abi.EXT_UDP == 7
    assert "yrss_set_extended" in abi.header_functions()
    assert re.search(r"int yrss_set_extended\(yrss_ctx \*ctx, uint32_t flags\);", text)
    # labelled as the build's own semantics in the header
    assert "THIS BUILD'S OWN SEMANTICS, NOT fs/lib's" in text
    lib = abi.load()
    assert lib.yrss_set_extended.argtypes == [abi._vp, abi._u32]
    out = subprocess.run(["nm", "-D", "--defined-only", str(abi.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    assert re.search(r"\bT yrss_set_extended\b", out)
    # no context: an argument error, and no GPU call
    import errno
    assert lib.yrss_set_extended(None, 0) == -errno.EINVAL
    # struct yrss_config is untouched (its size is pinned by test_abi.py)
    import ctypes
    assert ctypes.sizeof(abi.Config) == 68
