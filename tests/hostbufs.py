"""Host-side support shared by the GPU tests and the soak tools: frames from
window streams, rte_mbuf pools, the oracle's per-queue lists for a burst, and
pre-filled output arrays with their checkers.  numpy and the oracle only: no
pytest and no torch, so a tool or a child process can import it in a bare
interpreter.  pytest rewrites assertions in test_*.py modules only, so every
assertion here carries its own message (what differed, where first, the values)."""
import ctypes
import functools
from collections import namedtuple

import numpy as np

import route_helpers as rh
from yastack_amd import abi, segments

PAD = 64          # spare elements behind every output, pre-filled


def assert_same(name, got, want):
    """np.array_equal(got, want), or every element of got == the scalar want (a
    pre-filled stretch that must stay as it was), with the first mismatches."""
    got = np.asarray(got)
    want = np.broadcast_to(want, got.shape) if np.ndim(want) == 0 else np.asarray(want)
    assert got.shape == want.shape, f"{name}: shape {got.shape} vs {want.shape}"
    d = np.flatnonzero(got != want)
    assert d.size == 0, f"{d.size} {name} mismatches, first at {d[:5]}: " \
                        f"{got.ravel()[d[:5]]} vs {want.ravel()[d[:5]]}"


def fake_mbufs(frames, headroom=128):
    """Lay frames out like an rte_mbuf pool: 128-B mbuf header + headroom + data.
    The pool is page-aligned (hipHostRegister-able, like a hugepage memzone)."""
    stride = 128 + headroom + 2048 + 64
    raw = np.zeros(len(frames) * stride + 8192, np.uint8)
    off = (-raw.ctypes.data) % 4096
    pool = raw[off: off + len(frames) * stride]
    base = pool.ctypes.data
    ptrs = np.empty(len(frames), np.uint64)
    b, o, dl = abi.MBUF_OFF_BUF_ADDR, abi.MBUF_OFF_DATA_OFF, abi.MBUF_OFF_DATA_LEN
    for i, f in enumerate(frames):
        m = i * stride
        buf = base + m + 128
        data = np.frombuffer(f[:2048], np.uint8)
        pool[m + 128 + headroom: m + 128 + headroom + data.size] = data
        pool[m + b: m + b + 8] = np.frombuffer(np.uint64(buf).tobytes(), np.uint8)
        pool[m + o: m + o + 2] = np.frombuffer(np.uint16(headroom).tobytes(), np.uint8)
        pool[m + dl: m + dl + 2] = np.frombuffer(np.uint16(min(len(f), 2048)).tobytes(), np.uint8)
        ptrs[i] = base + m
    return pool, ptrs, stride


def frames_of(win, lens, stride=80, cap=2048):
    """Frame i is window i (win[i * stride:(i + 1) * stride]) and a zero tail,
    cut to min(lens[i], cap) bytes (cap: one mbuf segment)."""
    out = []
    for i, L in enumerate(lens):
        L = min(int(L), cap)
        out.append((win[i * stride:(i + 1) * stride].tobytes() + bytes(max(0, L - stride)))[:L])
    return out


def synth_frames(oracle_mod, n, seed):
    """n frames of the SYN_FUZZ stream from packet `seed` on."""
    win, lens = oracle_mod.synth(abi.SYN_FUZZ, n, seed, stride=80)
    return frames_of(win, lens[:n])


def expect_lists(oracle_mod, frames, cfg):
    """The oracle's (q, hash, qidx, qstart) of frames as one burst."""
    c = oracle_mod.cfg(*cfg)
    want = [oracle_mod.toeplitz_dispatch(f, len(f), c) for f in frames]
    q = np.array([x for x, _ in want], np.int16)
    h = np.array([y for _, y in want], np.uint32)
    qi, qs = oracle_mod.process_burst(q, cfg[1])
    return q, h, qi, qs


def check_lists(r, q, h, qi, qs):
    assert_same("q", r.q, q)
    assert_same("hash", r.hash, h)
    assert_same("qidx", r.qidx, qi)
    assert_same("qstart", np.asarray(r.qstart)[: qs.size], qs)


MbufPool = namedtuple("MbufPool", "win lens frames mem ptrs data")


@functools.lru_cache(maxsize=None)
def mbuf_pool(npkts, headroom=130):
    """The first npkts packets of route_helpers.stream as one rte_mbuf pool:
    win uint8[npkts * 80], lens (data_len, capped at 2048: one mbuf segment),
    frames, the pool's memory, mbuf pointers, frame data pointers.  stream(n)
    is oracle.synth from packet 5 on, so the 4200-packet pool is a prefix of
    the 5000-packet one (test_support.py).  mem is shared: a test that reads
    hash.rss back zeroes it before and after."""
    win, lens = rh.stream(npkts)
    lens = np.minimum(lens, 2048).astype(np.uint16)
    frames = frames_of(win, lens)
    mem, ptrs, _ = fake_mbufs(frames, headroom=headroom)
    data = (ptrs + np.uint64(128 + headroom)).astype(np.uint64)
    lens.setflags(write=False)
    return MbufPool(win, lens, frames, mem, ptrs, data)


class Out:
    """Output arrays of a routed burst, longer than the burst, pre-filled; in
    `arena` (registered memory) when given."""

    def __init__(self, n, nq, want_hash=True, want_filter=True, arena=None):
        def arr(count, dtype, fill):
            if arena is None:
                return np.full(count, fill, dtype)
            return arena.take(count, dtype, fill)
        self.n, self.nq = n, nq
        self.q = arr(n + PAD, np.int16, 0x5A5A)
        self.h = arr(n + PAD, np.uint32, 0x5A5A5A5A) if want_hash else None
        self.f = np.full(n + PAD, 0x5A, np.int8) if want_filter else None
        self.ri = arr(n + PAD, np.uint32, 0xEEEEEEEE)
        self.rs = arr(nq + 4 + PAD, np.uint32, 0x77777777)

    @staticmethod
    def p(a):
        return None if a is None else a.ctypes.data

    def check(self, q, h, f, queue_id, enable, accept, filter_written=True):
        n, nq = self.n, self.nq
        assert_same("q", self.q[:n], q)
        assert_same("q past the burst", self.q[n:], 0x5A5A)
        if self.h is not None:
            assert_same("hash", self.h[:n], h)
            assert_same("hash past the burst", self.h[n:], 0x5A5A5A5A)
        if self.f is not None:
            if filter_written:
                assert_same("filter", self.f[:n], f)
                assert_same("filter past the burst", self.f[n:], 0x5A)
            else:
                assert_same("filter", self.f, 0x5A)
        ri_ref, rs_ref = segments.route_lists_from(q, f, nq, queue_id, enable, accept)
        assert_same("rstart", self.rs[:nq + 4], rs_ref)
        assert_same("rstart past nb_queues + 4 entries", self.rs[nq + 4:], 0x77777777)
        assert_same("ridx", self.ri[:n], ri_ref)
        assert_same("ridx past the burst", self.ri[n:], 0xEEEEEEEE)

    def untouched(self):
        return (np.all(self.q == 0x5A5A) and np.all(self.ri == 0xEEEEEEEE) and
                np.all(self.rs == 0x77777777) and (self.h is None or np.all(self.h == 0x5A5A5A5A))
                and (self.f is None or np.all(self.f == 0x5A)))


class Arena:
    """A page-aligned stretch of host memory to register, handed out in
    64-byte-aligned pieces."""

    def __init__(self, nbytes):
        raw = np.zeros(nbytes + 8192, np.uint8)
        off = (-raw.ctypes.data) % 4096
        self.mem = raw[off:off + (nbytes + 4095) // 4096 * 4096]
        self.used = 0

    def take(self, count, dtype, fill):
        nbytes = count * np.dtype(dtype).itemsize
        a = self.mem[self.used:self.used + nbytes].view(dtype)
        assert a.size == count, f"arena exhausted: {count} wanted, {a.size} left"
        self.used += (nbytes + 63) // 64 * 64
        a[:] = fill
        return a


def submit(eng, form, lo, n, o, src, wreg=None, stride=80, write_rss=False):
    """One worker burst into the Out `o`; returns its ticket.  src: (lens, mbuf
    ptrs, frame data ptrs), sliced from lo; wreg.mem: registered windows."""
    lens, ptrs, data = src
    t = ctypes.c_uint64()
    lib, ctx = eng._lib, eng._ctx
    if form == "mbufs":
        rc = lib.yrss_worker_submit(ctx, ptrs[lo:].ctypes.data, n, o.p(o.q), o.p(o.h), o.p(o.ri),
                                    o.p(o.rs), abi.F_WRITE_RSS if write_rss else 0,
                                    ctypes.byref(t))
    elif form == "frames":
        rc = lib.yrss_worker_submit_frames(ctx, data[lo:].ctypes.data, lens[lo:].ctypes.data, n,
                                           o.p(o.q), o.p(o.h), o.p(o.ri), o.p(o.rs),
                                           ctypes.byref(t))
    else:
        rc = lib.yrss_worker_submit_windows(ctx, wreg.mem[lo * 80:].ctypes.data, stride,
                                            lens[lo:].ctypes.data, n, o.p(o.q), o.p(o.h),
                                            o.p(o.ri), o.p(o.rs), ctypes.byref(t))
    assert rc == 0, (form, n, rc)
    return t.value
