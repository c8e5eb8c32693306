"""CPU checks of the GPU tests' host-side support (tests/hostbufs.py): the mbuf
layout the kernels will read, the frame builder, the two pools the tests slice,
and that the moved checkers still reject a wrong result."""
from types import SimpleNamespace

import numpy as np
import pytest

import route_helpers as rh
from hostbufs import PAD, Out, check_lists, expect_lists, fake_mbufs, frames_of, mbuf_pool
from yastack_amd import abi, segments


def test_fake_mbufs_layout():
    frames = [b"", bytes(range(60)), bytes(i % 251 for i in range(3000))]
    mem, ptrs, stride = fake_mbufs(frames, headroom=129)
    base = mem.ctypes.data
    assert base % 4096 == 0
    assert ptrs.tolist() == [base + i * stride for i in range(3)]

    def field(i, off, dtype):
        at = i * stride + off
        return int(mem[at:at + np.dtype(dtype).itemsize].copy().view(dtype)[0])

    for i, f in enumerate(frames):
        buf_addr = field(i, abi.MBUF_OFF_BUF_ADDR, np.uint64)
        assert buf_addr == base + i * stride + 128
        assert field(i, abi.MBUF_OFF_DATA_OFF, np.uint16) == 129
        data_len = field(i, abi.MBUF_OFF_DATA_LEN, np.uint16)
        assert data_len == (0, 60, 2048)[i]                     # capped at one mbuf segment
        at = buf_addr + 129 - base
        assert mem[at:at + data_len].tobytes() == f[:2048]


def test_frames_of():
    win = np.arange(1, 3 * 80 + 1, dtype=np.uint32).astype(np.uint8)
    short, padded, capped = frames_of(win, np.array([50, 200, 3000], np.uint16))
    assert short == win[:50].tobytes()                                 # below 80: the window cut
    assert padded == win[80:160].tobytes() + bytes(120)                # above: a zero tail
    assert capped == win[160:240].tobytes() + bytes(2048 - 80)         # above the cap: the cap
    assert frames_of(win, [70], stride=64, cap=66) == [win[:64].tobytes() + bytes(2)]


def _bites(make, check, flips):
    """check accepts make()'s result, and rejects it with any one element of
    `flips` (array name -> indices) changed."""
    check(make())
    for name, idxs in flips.items():
        for i in idxs:
            r = make()
            getattr(r, name)[i] ^= 1
            with pytest.raises(AssertionError):
                check(r)


def test_check_lists_bites(oracle_mod):
    n = 300
    q, h, qi, qs = expect_lists(oracle_mod, frames_of(*rh.stream(n)), (6, 4, 1, 0))
    assert len(set(q.tolist())) > 2       # several queues: qidx is no identity
    # (qstart as the library returns it: nb_queues + 2 entries, one more than the oracle's)
    _bites(lambda: SimpleNamespace(q=q.copy(), hash=h.copy(), qidx=qi.copy(),
                                   qstart=np.append(qs, np.uint32(0))),
           lambda r: check_lists(r, q, h, qi, qs),
           {"q": (0, n - 1), "hash": (0, n - 1), "qidx": (0, n // 2, n - 1),
            "qstart": range(qs.size)})


def test_out_check_bites():
    cfg, nq, queue_id, n = (6, 4, 1, 0), 4, 2, 300
    q, h = rh.oracle_qh(cfg, n)
    f = rh.oracle_filter(True, n)
    ri, rs = segments.route_lists_from(q, f, nq, queue_id, True, True)
    assert np.count_nonzero(np.diff(rs)) > 3      # several route classes populated

    def out():
        o = Out(n, nq)
        o.q[:n], o.h[:n], o.f[:n], o.ri[:n], o.rs[:nq + 4] = q, h, f, ri, rs
        return o

    # results (first, last), then padding (first, last)
    ends = {"q": n, "h": n, "f": n, "ri": n, "rs": nq + 4}
    _bites(out, lambda o: o.check(q, h, f, queue_id, True, True),
           {name: (0, end - 1, end, end + PAD - 1) for name, end in ends.items()})
    with pytest.raises(AssertionError, match="filter"):    # a filter the call must not write
        out().check(q, h, f, queue_id, True, True, filter_written=False)


def test_the_two_pools_are_prefixes_of_one_stream():
    small, large = mbuf_pool(4200), mbuf_pool(5000)
    assert np.array_equal(small.win, large.win[:4200 * 80])
    assert np.array_equal(small.lens, large.lens[:4200])
    assert small.frames == large.frames[:4200]
    assert int(large.lens.max()) == 2048 and max(len(f) for f in large.frames) == 2048
