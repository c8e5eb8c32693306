"""GPU parity for SURVEY §8(f) rank 2: ff_rss_check (fs/lib/ff_dpdk_if.c:1904-1940)
as a device batch and as the full ephemeral-lport sweep of in_pcbconnect_setup
(fs/freebsd/netinet/in_pcb.c:1131-1170), against the oracle restatement."""
import ctypes
import socket
import struct

import numpy as np
import pytest

from rss_tuples import edge_hashes, solve_tuple, window_rank

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from yastack_amd import SoftRss, abi  # noqa: E402

from hostbufs import check_lists, expect_lists, fake_mbufs, synth_frames  # noqa: E402

CFGS = [(1, 128, 0), (2, 128, 1), (3, 512, 2), (8, 128, 5), (4, 0, 3), (5, 64, 0)]


@pytest.mark.parametrize("nq,reta,qid", CFGS)
def test_rss_check_batch(oracle_mod, nq, reta, qid):
    rng = np.random.default_rng(nq * 1000 + reta)
    tuples = rng.integers(0, 256, (100003, 12), dtype=np.uint8)
    ok_ref, h_ref = oracle_mod.rss_check_batch(tuples, nq, reta, qid)
    with SoftRss(3, device=0, max_burst=0) as eng:
        ok, h = eng.rss_check_dev(torch.from_numpy(tuples.reshape(-1)).cuda(), nq, reta, qid)
        torch.cuda.synchronize()
        assert np.array_equal(ok.cpu().numpy(), ok_ref)
        assert np.array_equal(h.cpu().numpy().view(np.uint32), h_ref)


@pytest.mark.parametrize("nq,reta,qid", CFGS)
def test_lport_sweep(oracle_mod, nq, reta, qid):
    faddr = struct.unpack("<I", socket.inet_aton("172.31.27.43"))[0]
    laddr = struct.unpack("<I", socket.inet_aton("192.168.1.100"))[0]
    fport = struct.unpack("<H", struct.pack(">H", 443))[0]
    lports = np.arange(65536, dtype=np.uint32)
    tup = np.zeros((65536, 12), np.uint8)
    tup[:, 0:4] = np.frombuffer(struct.pack("<I", faddr), np.uint8)
    tup[:, 4:8] = np.frombuffer(struct.pack("<I", laddr), np.uint8)
    tup[:, 8:10] = np.frombuffer(struct.pack("<H", fport), np.uint8)
    tup[:, 10] = lports & 0xFF
    tup[:, 11] = lports >> 8
    ok_ref, _ = oracle_mod.rss_check_batch(tup, nq, reta, qid)
    want = np.zeros(2048, np.uint32)
    for w in range(2048):
        bits = ok_ref[w * 32:(w + 1) * 32].astype(np.uint64)
        want[w] = int((bits << np.arange(32, dtype=np.uint64)).sum())
    with SoftRss(3, device=0, max_burst=0) as eng:
        got = eng.rss_lport_sweep(faddr, laddr, fport, nq, reta, qid)
    assert np.array_equal(got, want)
    if nq > 1:
        frac = ok_ref.mean()
        assert 0.5 / nq < frac < 2.0 / nq


# ---------------------------------------------------------------------------
# Everything below calls the batch kernel and the sweep where they can go
# wrong unnoticed by the two tests above: sizes around the wave and the block,
# a NULL hash, stores that end at n, odd pointers, another stream, parameters
# at their ends, hashes chosen by solving for them (rss_tuples.py), short and
# foreign keys, and a context that has done and is doing other work.  Every
# expectation on ok is computed twice, from plain integers and by the oracle.
# ---------------------------------------------------------------------------
KEY2 = bytes(range(7, 47))
EBUSY, EINVAL = 16, 22
CANARY8, CANARY32 = 0xA5, 0xA5A5A5A5
_RNG = np.random.default_rng(20240607)
TUPLES = _RNG.integers(0, 256, (4096, 12), dtype=np.uint8)    # shared, never written


def _py_ok(h, nq, reta, qid):
    """ff_rss_check from the hash, in Python integers: the reference masks with
    reta_size - 1 as a 32-bit value whatever reta_size is."""
    if nq <= 1:
        return 1
    return 1 if ((h & ((reta - 1) & 0xFFFFFFFF)) % nq) == qid else 0


def _py_ok_all(h_ref, nq, reta, qid):
    return np.array([_py_ok(int(h), nq, reta, qid) for h in h_ref], np.uint8)


def _raw_check(eng, tup_ptr, n, nq, reta, qid, ok_ptr, hash_ptr, stream=None):
    """yrss_rss_check_dev itself, on raw device addresses."""
    return abi.load().yrss_rss_check_dev(eng._ctx, tup_ptr, n, nq, reta, qid, ok_ptr, hash_ptr,
                                         eng._stream(stream))


def _bitmap(ok):
    """Bit (p & 31) of word p >> 5 = ok[p], for p in 0..65535."""
    return np.packbits(ok.reshape(2048, 32), axis=1, bitorder="little").view("<u4").ravel()


def _sweep_tuples(faddr, laddr, fport):
    tup = np.zeros((65536, 12), np.uint8)
    tup[:, 0:4] = np.frombuffer(struct.pack("<I", faddr), np.uint8)
    tup[:, 4:8] = np.frombuffer(struct.pack("<I", laddr), np.uint8)
    tup[:, 8:10] = np.frombuffer(struct.pack("<H", fport), np.uint8)
    lports = np.arange(65536, dtype=np.uint32)
    tup[:, 10] = lports & 0xFF
    tup[:, 11] = lports >> 8
    return tup


def _sweep_want(oracle_mod, faddr, laddr, fport, nq, reta, qid, key=None):
    key = oracle_mod.MLX_KEY if key is None else key
    ok, h = oracle_mod.rss_check_batch(_sweep_tuples(faddr, laddr, fport), nq, reta, qid, key=key)
    return _bitmap(ok), ok, h


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 511, 513])
def test_rss_check_sizes_and_bounds(oracle_mod, n):
    """Sizes around the 64-lane wave and the 256-thread block, with and without
    d_hash: the results equal the oracle and nothing is stored at or past n."""
    nq, reta, qid = 3, 128, 1
    tuples = TUPLES[:n]
    ok_ref, h_ref = oracle_mod.rss_check_batch(tuples, nq, reta, qid)
    assert np.array_equal(ok_ref, _py_ok_all(h_ref, nq, reta, qid))
    with SoftRss(3, device=0, max_burst=0) as eng:
        t_d = torch.from_numpy(np.ascontiguousarray(TUPLES[:max(n, 1)]).reshape(-1)).cuda()
        for with_hash in (False, True):
            ok_d = torch.full((n + 64,), CANARY8, dtype=torch.uint8, device="cuda")
            h_d = torch.full((4 * (n + 64),), CANARY8, dtype=torch.uint8, device="cuda")
            rc = _raw_check(eng, t_d.data_ptr(), n, nq, reta, qid, ok_d.data_ptr(),
                            h_d.data_ptr() if with_hash else None)
            assert rc == 0
            torch.cuda.synchronize()
            ok = ok_d.cpu().numpy()
            h = h_d.cpu().numpy().view(np.uint32)
            assert np.array_equal(ok[:n], ok_ref), with_hash
            assert np.all(ok[n:] == CANARY8), with_hash
            if with_hash:
                assert np.array_equal(h[:n], h_ref)
                assert np.all(h[n:] == CANARY32)
            else:
                assert np.all(h == CANARY32)     # a NULL d_hash: the spare buffer stays as it was


def test_rss_check_pointer_alignment(oracle_mod):
    """Tuples and d_hash need 4-byte alignment and no more; a 2-byte offset is
    refused before anything is launched."""
    n, (nq, reta, qid) = 257, (5, 64, 4)
    ok_ref, h_ref = oracle_mod.rss_check_batch(TUPLES[:n], nq, reta, qid)
    assert np.array_equal(ok_ref, _py_ok_all(h_ref, nq, reta, qid))
    with SoftRss(3, device=0, max_burst=0) as eng:
        raw = torch.zeros(n * 12 + 16, dtype=torch.uint8, device="cuda")
        raw[4:4 + n * 12] = torch.from_numpy(np.ascontiguousarray(TUPLES[:n]).reshape(-1)).cuda()
        raw[2:4] = 0x77
        ok_d = torch.full((n + 64,), CANARY8, dtype=torch.uint8, device="cuda")
        h_d = torch.full((4 * (n + 64),), CANARY8, dtype=torch.uint8, device="cuda")
        assert raw.data_ptr() % 16 == 0 and h_d.data_ptr() % 16 == 0
        rc = _raw_check(eng, raw.data_ptr() + 4, n, nq, reta, qid, ok_d.data_ptr(),
                        h_d.data_ptr() + 4)
        assert rc == 0
        torch.cuda.synchronize()
        h = h_d.cpu().numpy()
        assert np.array_equal(ok_d.cpu().numpy()[:n], ok_ref)
        assert np.all(ok_d.cpu().numpy()[n:] == CANARY8)
        assert np.array_equal(h[4:4 + 4 * n].view(np.uint32), h_ref)
        assert np.all(h[:4] == CANARY8) and np.all(h[4 + 4 * n:] == CANARY8)
        # 2-byte offsets: -EINVAL, nothing written
        ok_d.fill_(CANARY8)
        h_d.fill_(CANARY8)
        assert _raw_check(eng, raw.data_ptr() + 2, n, nq, reta, qid, ok_d.data_ptr(),
                          h_d.data_ptr()) == -EINVAL
        assert _raw_check(eng, raw.data_ptr() + 4, n, nq, reta, qid, ok_d.data_ptr(),
                          h_d.data_ptr() + 2) == -EINVAL
        torch.cuda.synchronize()
        assert bool(torch.all(ok_d == CANARY8)) and bool(torch.all(h_d == CANARY8))


def test_rss_check_other_stream(oracle_mod):
    nq, reta, qid = 7, 512, 3
    ok_ref, h_ref = oracle_mod.rss_check_batch(TUPLES, nq, reta, qid)
    with SoftRss(3, device=0, max_burst=0) as eng:
        t_d = torch.from_numpy(TUPLES.reshape(-1).copy()).cuda()
        torch.cuda.synchronize()
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):      # the outputs are allocated on s as well
            ok, h = eng.rss_check_dev(t_d, nq, reta, qid, stream=s)
        s.synchronize()
        assert np.array_equal(ok.cpu().numpy(), ok_ref)
        assert np.array_equal(h.cpu().numpy().view(np.uint32), h_ref)


NQS = [0, 1, 2, 3, 7, 8, 255, 256, 65535]
RETAS = [0, 1, 2, 64, 100, 128, 512, 32768, 65535]


def _param_cases():
    """Every (nb_queues, reta_size) pair once: 81 launches of 4096 tuples on one
    context, far cheaper than a context each.  The queueid kind (0, nq - 1,
    nq, 65535) rotates with i + j, so each kind meets every nb_queues and
    every reta_size: all pairs of the three parameters, not their product."""
    out = []
    for i, nq in enumerate(NQS):
        for j, reta in enumerate(RETAS):
            qid = (0, (nq - 1) & 0xFFFF, nq, 65535)[(i + j) % 4]
            out.append((nq, reta, qid))
    return out


def test_rss_check_parameter_edges(oracle_mod):
    """nb_queues 0, 1 and 65535, a reta_size that is no power of two (the
    reference masks with reta_size - 1 whatever it is), queueid at and past
    nb_queues."""
    kinds, bad = set(), []
    with SoftRss(3, device=0, max_burst=0) as eng:
        t_d = torch.from_numpy(TUPLES.reshape(-1).copy()).cuda()
        h_ref0 = None
        for nq, reta, qid in _param_cases():
            ok_ref, h_ref = oracle_mod.rss_check_batch(TUPLES, nq, reta, qid)
            assert np.array_equal(ok_ref, _py_ok_all(h_ref, nq, reta, qid)), (nq, reta, qid)
            h_ref0 = h_ref if h_ref0 is None else h_ref0
            assert np.array_equal(h_ref, h_ref0)
            kinds.add("all" if ok_ref.all() else "none" if not ok_ref.any() else "some")
            ok, h = eng.rss_check_dev(t_d, nq, reta, qid)
            torch.cuda.synchronize()
            if not (np.array_equal(ok.cpu().numpy(), ok_ref) and
                    np.array_equal(h.cpu().numpy().view(np.uint32), h_ref)):
                bad.append((nq, reta, qid))
    assert not bad, f"mismatch at (nb_queues, reta_size, queueid) {bad}"
    assert kinds == {"all", "none", "some"}


def _directed_hashes(nq, reta):
    """Hashes whose masked value sits at the ends of the modulo, the bits the
    mask drops once all zero and once all one, and edge_hashes(nq).  Returns
    (hashes, the masked values aimed at)."""
    mask = (reta - 1) & 0xFFFFFFFF
    mvs = {0, nq - 1, nq, 2 * nq - 1, mask // nq * nq, mask}
    if bin(mask).count("1") <= 16:
        # a mask with holes (reta_size no power of two) reaches only its
        # submasks: the largest of them in remainder classes 0 and nq - 1
        subs, s = [], mask
        while True:
            subs.append(s)
            if s == 0:
                break
            s = (s - 1) & mask
        for r in (0, nq - 1):
            mvs.add(max(s for s in subs if s % nq == r))
    mvs = sorted(v for v in mvs if v & mask == v)
    hs = {v | hi for v in mvs for hi in (0, ~mask & 0xFFFFFFFF)}
    return sorted(hs | set(edge_hashes(nq))), mvs


@pytest.mark.parametrize("nq,reta", [(3, 128), (7, 512), (5, 0), (255, 65535), (6, 100)])
def test_rss_check_directed_hashes(oracle_mod, nq, reta):
    """(h & mask) % nq at the values that break a reciprocal modulo or a mask of
    the wrong width; random tuples essentially never produce them."""
    mask = (reta - 1) & 0xFFFFFFFF
    targets, mvs = _directed_hashes(nq, reta)
    assert window_rank(oracle_mod.MLX_KEY, 40) == 32
    rng = np.random.default_rng(nq * 65536 + reta)
    tup = np.array([np.frombuffer(solve_tuple(
        oracle_mod.MLX_KEY, 40, h, base=bytes(rng.integers(0, 256, 12, dtype=np.uint8))),
        np.uint8) for h in targets])
    n = len(targets)
    with SoftRss(3, device=0, max_burst=0) as eng:
        t_d = torch.from_numpy(tup.reshape(-1).copy()).cuda()
        seen = set()
        for qid in range(min(nq, 8) + 1):
            ok_ref, h_ref = oracle_mod.rss_check_batch(tup, nq, reta, qid)
            # the edges aimed at are in the input, by the oracle's own account
            assert h_ref.tolist() == targets
            assert set(mvs) <= {int(h) & mask for h in h_ref}
            ok_py = np.array([_py_ok(h, nq, reta, qid) for h in targets], np.uint8)
            assert np.array_equal(ok_ref, ok_py)
            seen.add("some" if 0 < ok_ref.sum() < n else "none" if not ok_ref.any() else "all")
            ok, h = eng.rss_check_dev(t_d, nq, reta, qid)
            torch.cuda.synchronize()
            assert h.cpu().numpy().view(np.uint32).tolist() == targets, qid
            assert np.array_equal(ok.cpu().numpy(), ok_py), qid
    assert "some" in seen
    if nq <= 8:
        assert "none" in seen          # queueid == nb_queues


@pytest.mark.parametrize("kl", [4, 5, 10, 11, 15, 16, 39, 40])
def test_rss_check_short_keys(oracle_mod, kl):
    """rss_key_len 4..40: key bits past the length are zero.  A 12-byte tuple
    consumes key bytes 0..15, so every length below 16 changes the hashes."""
    nq, reta, qid = 7, 512, 3
    key = KEY2[:kl]
    ok_ref, h_ref = oracle_mod.rss_check_batch(TUPLES, nq, reta, qid, key=key)
    _, h_full = oracle_mod.rss_check_batch(TUPLES, nq, reta, qid, key=KEY2)
    assert np.array_equal(ok_ref, _py_ok_all(h_ref, nq, reta, qid))
    if kl >= 16:
        assert np.array_equal(h_ref, h_full)
    else:
        # fewest at 15: key byte 15 (0x16) meets tuple bits 92..95 alone, so
        # 15 tuples in 16 change their hash (4096 samples: 0.9375 +- 0.004)
        assert (h_ref != h_full).mean() > 0.9
    with SoftRss(3, rss_key=key, device=0, max_burst=0) as eng:
        assert eng.cfg.rss_key_len == kl
        ok, h = eng.rss_check_dev(torch.from_numpy(TUPLES.reshape(-1).copy()).cuda(), nq, reta, qid)
        torch.cuda.synchronize()
        assert np.array_equal(h.cpu().numpy().view(np.uint32), h_ref)
        assert np.array_equal(ok.cpu().numpy(), ok_ref)


# ---- the lport sweep ----------------------------------------------------------

_EXISTING = (struct.unpack("<I", socket.inet_aton("172.31.27.43"))[0],
             struct.unpack("<I", socket.inet_aton("192.168.1.100"))[0],
             struct.unpack("<H", struct.pack(">H", 443))[0])
_R = np.random.default_rng(77)
ADDRS = [(0, 0, 0), (0xFFFFFFFF, 0xFFFFFFFF, 0xFFFF), _EXISTING] + \
        [(int(_R.integers(0, 1 << 32)), int(_R.integers(0, 1 << 32)), int(_R.integers(0, 1 << 16)))
         for _ in range(2)]
# nq = 1: every port; queueid >= nq: none; a RETA mask; and reta_size 0, whose
# all-ones mask alone keeps the hash's top bits (see the short keys below)
SWEEP_CFGS = [(1, 128, 0), (3, 128, 5), (7, 512, 3), (5, 0, 2)]


def _uniform(bm):
    return bool(np.all(bm == 0) or np.all(bm == 0xFFFFFFFF))


@pytest.mark.parametrize("kl", [None, 5, 10, 11, 40])
def test_lport_sweep_inputs_and_keys(oracle_mod, kl):
    """The sweep at the ends of its address range and under short keys.  With
    rss_key_len <= 10 the lport bytes meet only zero key bits (rank 0): every
    port hashes alike and the bitmap is all zeros or all ones.  At 11 they
    meet key byte 10, which reaches hash bits 24..31 only."""
    key = oracle_mod.MLX_KEY if kl is None else KEY2[:kl]
    rank = window_rank(key, len(key), (10, 11))
    if kl == 11:
        assert 0 < rank <= 8
    else:
        assert rank == (0 if kl in (5, 10) else 16)
    varied = 0
    with SoftRss(3, rss_key=None if kl is None else key, device=0, max_burst=0) as eng:
        for faddr, laddr, fport in ADDRS:
            for nq, reta, qid in SWEEP_CFGS:
                want, ok_ref, h_ref = _sweep_want(oracle_mod, faddr, laddr, fport, nq, reta, qid,
                                                  key)
                mask = (reta - 1) & 0xFFFFFFFF
                ok_py = np.uint8(1) if nq <= 1 else \
                    (((h_ref & np.uint32(mask)).astype(np.uint64) % nq) == qid).astype(np.uint8)
                assert np.array_equal(ok_ref, np.broadcast_to(ok_py, ok_ref.shape))
                got = eng.rss_lport_sweep(faddr, laddr, fport, nq, reta, qid)
                where = (kl, hex(faddr), hex(laddr), hex(fport), nq, reta, qid)
                assert np.array_equal(got, want), where
                if nq == 1:
                    assert np.all(got == 0xFFFFFFFF), where
                if qid >= nq > 1:
                    assert np.all(got == 0), where
                if kl in (5, 10):
                    assert _uniform(want) and _uniform(got), where
                if nq > 1 and not _uniform(want):
                    assert not _uniform(got), where
                    varied += 1
    if kl in (5, 10):
        assert varied == 0
    else:
        assert varied > 0       # (at 11: through reta_size 0, the unmasked hash)


BIT_ORDER_CFGS = ((2, 128), (2, 0), (3, 512))


def test_lport_sweep_bit_and_byte_order(oracle_mod):
    """Single bits against ff_rss_check called one tuple at a time: bit p & 31
    of word p >> 5 belongs to the STORED lport value p, whose little-endian
    image is tuple bytes 10..11.  Independent of the batch helper."""
    faddr, laddr, fport = _EXISTING
    c = oracle_mod.cfg(8, 8, 1, 0)
    ports = [0, 1, 0x0100, 0x00FF, 0x1234, 0x3412, 0xFFFF]
    one = oracle_mod.lib().oracle_ff_rss_check
    with SoftRss(3, device=0, max_burst=0) as eng:
        for nq, reta in BIT_ORDER_CFGS:
            bits = {}
            for qid in range(nq):
                bm = eng.rss_lport_sweep(faddr, laddr, fport, nq, reta, qid)
                for p in ports:
                    got = int(bm[p >> 5]) >> (p & 31) & 1
                    assert got == one(ctypes.byref(c), nq, reta, qid, faddr, laddr, fport, p), \
                        (nq, reta, qid, hex(p))
                    t = struct.pack("<IIHH", faddr, laddr, fport, p)
                    assert got == _py_ok(oracle_mod.toeplitz_hash(t), nq, reta, qid)
                    bits.setdefault(p, []).append(got)
            # each port is accepted by exactly one queue
            assert all(sum(v) == 1 for v in bits.values())
    # a port and its byte-swapped twin go to different queues under some
    # configuration above, so swapped bytes in the kernel could not pass
    h = {p: oracle_mod.toeplitz_hash(struct.pack("<IIHH", faddr, laddr, fport, p)) for p in ports}
    def owner(p, nq, reta):
        return (h[p] & ((reta - 1) & 0xFFFFFFFF)) % nq

    for a, b in ((0x1234, 0x3412), (0x0100, 0x0001)):
        assert any(owner(a, nq, reta) != owner(b, nq, reta) for nq, reta in BIT_ORDER_CFGS), hex(a)


def test_lport_sweep_between_bursts(oracle_mod):
    """The sweep borrows the host-burst staging: on one context, before, between
    and after bursts that grow that staging, every sweep and every burst is
    exact."""
    cfg = (5, 4, 1, 1)
    faddr, laddr, fport = _EXISTING
    nq, reta, qid = 4, 128, 1
    want, _, _ = _sweep_want(oracle_mod, faddr, laddr, fport, nq, reta, qid)
    assert not _uniform(want)
    f1 = synth_frames(oracle_mod, 1000, 31)
    f2 = synth_frames(oracle_mod, 3000, 32)
    pool, ptrs, _ = fake_mbufs(f2)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        first = eng.rss_lport_sweep(faddr, laddr, fport, nq, reta, qid)
        assert np.array_equal(first, want)
        check_lists(eng.dispatch_frames(f1), *expect_lists(oracle_mod, f1, cfg))
        assert np.array_equal(eng.rss_lport_sweep(faddr, laddr, fport, nq, reta, qid), first)
        check_lists(eng.dispatch_burst(ptrs), *expect_lists(oracle_mod, f2, cfg))
        assert np.array_equal(eng.rss_lport_sweep(faddr, laddr, fport, nq, reta, qid), first)
        assert eng.status() == 0
    del pool


def test_lport_sweep_refused_mid_burst(oracle_mod):
    """One burst in flight per context holds for the sweep too: while a
    YRSS_F_ASYNC burst is pending it returns -EBUSY on the host, before it
    touches the staging the burst's kernel and copies own, and leaves the
    caller's bitmap alone; after yrss_wait the burst is exact and the sweep
    runs."""
    cfg = (5, 4, 1, 1)
    n = 1000
    faddr, laddr, fport = _EXISTING
    nq, reta, qid = 4, 128, 1
    want, _, _ = _sweep_want(oracle_mod, faddr, laddr, fport, nq, reta, qid)
    frames = synth_frames(oracle_mod, n, 41)
    q, h, qi, qs = expect_lists(oracle_mod, frames, cfg)
    pool, ptrs, _ = fake_mbufs(frames)
    lib = abi.load()
    oq, oh = np.empty(n, np.int16), np.empty(n, np.uint32)
    oqi, oqs = np.empty(n, np.uint32), np.empty(cfg[1] + 2, np.uint32)
    bm = np.full(2048, CANARY32, np.uint32)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        rc = lib.yrss_dispatch_burst(eng._ctx, ptrs.ctypes.data, n, oq.ctypes.data,
                                     oh.ctypes.data, oqi.ctypes.data, oqs.ctypes.data,
                                     abi.F_ASYNC)
        assert rc == 0
        rc = lib.yrss_rss_lport_sweep(eng._ctx, faddr, laddr, fport, nq, reta, qid,
                                      bm.ctypes.data)
        assert rc == -EBUSY
        assert np.all(bm == CANARY32)
        assert lib.yrss_wait(eng._ctx) == 0
        assert np.array_equal(oq, q) and np.array_equal(oh, h)
        assert np.array_equal(oqi, qi) and np.array_equal(oqs[: qs.size], qs)
        assert np.array_equal(eng.rss_lport_sweep(faddr, laddr, fport, nq, reta, qid), want)
        assert eng.status() == 0
    del pool
