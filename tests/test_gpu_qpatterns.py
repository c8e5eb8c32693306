"""Directed, skewed queue patterns through every per-queue list path (GPU).

The other list tests feed the kernels synthetic profiles: hashed TCP (every
bucket populated, about equal, interleaved at random) or all-UDP (one bucket:
the one-list shortcut, no ranked scatter at all).  Here the windows are built
on the host (tests/qpatterns.py) so that the oracle's q follows a chosen bucket
sequence: all packets but one in one bucket (the full-skew case the shortcut
hides: a whole chunk in one bucket, rank 2^cshift - 1, the packed rank word's
0xFFFF at 128 buckets), runs on line / tile / chunk / span boundaries and one
either side, buckets empty over the whole batch, a bucket's line carried over
spans that bring it nothing, a staircase through every line phase, and a
heavy-tailed draw.  Paths: the line scatter with in-scatter prefixes and with
the scan kernel, kG = 2 packed, kG = 4 with the rank beside q, the fallback
scatter, the parse kernel without lists, the segmented lists, the one-launch
burst kernel and the batch kernels behind the host entry points, the persistent
worker.  Every case compares q, hash, qstart and qidx (seg_idx / seg_off) with
the oracle in full, needs an empty fault record, and gives the kernels outputs
longer than the batch, pre-filled, so a store past the end shows.  The layout
restated in qpatterns.layout only aims the patterns; nothing here asserts it.
"""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import qpatterns as qp  # noqa: E402
from gpu_checks import check, check_seg, dev, to_np, upload  # noqa: E402,F401
from hostbufs import PAD  # noqa: E402
from yastack_amd import SoftRss, abi  # noqa: E402
from yastack_amd.dispatch import DispatchResult  # noqa: E402

_EX = {}


def ex_for(oracle_mod, cfg, stride):
    if (cfg, stride) not in _EX:
        _EX[(cfg, stride)] = qp.exemplars(oracle_mod, cfg, stride)
    return _EX[(cfg, stride)]


def members(ex, n, chunk, span):
    """Every member of every family as (name, bucket sequence)."""
    for fam in qp.FAMILIES:
        for label, pat in qp.family(fam, n, ex, chunk, span):
            yield f"{fam}/{label}", pat


class Padded:
    """Outputs of a global-list batch, each PAD elements longer than the batch
    needs and pre-filled; .out is what the call gets (16-byte aligned views)."""

    def __init__(self, n, nq, dev, lists=True):
        self.n, self.nq = n, nq
        self.q = torch.empty(n + PAD, dtype=torch.int16, device=dev)
        self.h = torch.empty(n + PAD, dtype=torch.int32, device=dev)
        self.qi = torch.empty(n + PAD, dtype=torch.int32, device=dev) if lists else None
        self.qs = torch.empty(nq + 2 + PAD, dtype=torch.int32, device=dev) if lists else None
        self.refill()
        self.out = DispatchResult(self.q[:n], self.h[:n], self.qi[:n] if lists else None,
                                  self.qs[:nq + 2] if lists else None)

    def refill(self):
        self.q.fill_(0x5A5A)
        self.h.fill_(0x5A5A5A5A)
        if self.qi is not None:
            self.qi.fill_(-1)
            self.qs.fill_(0x77777777)

    def untouched_past_the_end(self):
        n, nq = self.n, self.nq
        assert np.all(to_np(self.q[n:], np.uint16) == 0x5A5A), "q written past the batch"
        assert np.all(to_np(self.h[n:], np.uint32) == 0x5A5A5A5A), "hash written past the batch"
        if self.qi is not None:
            assert np.all(self.qi[n:].cpu().numpy() == -1), "qidx written past the batch"
            assert np.all(to_np(self.qs[nq + 2:], np.uint32) == 0x77777777), \
                "qstart written past nb_queues + 2 entries"


def _id(case):
    path, cfg, tune, n = case
    return f"{path}-{'x'.join(map(str, cfg))}-{qp.tune_id(tune)}"


@pytest.mark.parametrize("case", qp.GLOBAL_CASES, ids=_id)
def test_global_lists(dev, oracle_mod, case):
    """Parse ranks, scan or in-scatter prefixes, line or fallback scatter: one
    context, every pattern in turn (the alternating totals sets of the fused
    path stay in step from batch to batch)."""
    _path, cfg, tune, n = case
    nq = cfg[1]
    ex = ex_for(oracle_mod, cfg, 64)
    chunk, span = qp.aim_of(nq + 1, tune)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        if tune:
            eng.set_tuning(**tune)
        bufs = Padded(n, nq, dev)
        for name, pat in members(ex, n, chunk, span):
            bufs.refill()
            try:
                res = check(eng, oracle_mod, cfg, None, n, traffic=qp.build(pat, ex), out=bufs.out)
                # the traffic is the pattern (tests/test_qpatterns.py proves it on the CPU)
                assert np.array_equal(qp.bucket_of(to_np(res.q, np.int16), nq), pat)
                bufs.untouched_past_the_end()
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from e


@pytest.mark.parametrize("cfg", [(8, 8, 1, 0), (128, 127, 1, 1), (4096, 256, 1, 1)],
                         ids=lambda c: "x".join(map(str, c)))
def test_parse_without_lists(dev, oracle_mod, cfg):
    """compact=False: no counts, no ranks, no scatter; q and hash stay exact
    on the same traffic (the ranks are no input of q)."""
    nq, n = cfg[1], 33011
    ex = ex_for(oracle_mod, cfg, 64)
    chunk, span = qp.layout(nq + 1)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        bufs = Padded(n, nq, dev, lists=False)
        for name, pat in members(ex, n, chunk, span):
            bufs.refill()
            win_h, lens_h = qp.build(pat, ex)
            win, lens = upload(win_h, lens_h, dev)
            res = eng.dispatch_dev(win, lens, 64, n, out=bufs.out, compact=False)
            torch.cuda.synchronize()
            assert eng.fault_info()[0] == abi.FAULT_NONE, name
            q_ref, h_ref = oracle_mod.dispatch_windows(win_h, 64, lens_h, oracle_mod.cfg(*cfg))
            assert np.array_equal(to_np(res.q, np.int16), q_ref), name
            assert np.array_equal(to_np(res.hash, np.uint32), h_ref), name
            bufs.untouched_past_the_end()


@pytest.mark.parametrize("cfg,blocks,n", qp.SEG_CASES,
                         ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_segmented_lists(dev, oracle_mod, cfg, blocks, n):
    """flush_seg: segments wholly in one bucket (the first, the last queue, the
    drop bucket: byte rank 255, offset 256), runs of 255 / 256 / 257, buckets
    empty in the middle of a segment's offset row; one parse workgroup
    (parse_blocks=1: a wave owns many chunks) and the default grid."""
    ex = ex_for(oracle_mod, cfg, 64)
    chunk, span = qp.SEG_AIM
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        if blocks:
            eng.set_tuning(parse_blocks=blocks)
        for name, pat in members(ex, n, chunk, span):
            try:
                _res, q_ref = check_seg(eng, oracle_mod, cfg, None, n, traffic=qp.build(pat, ex))
                assert np.array_equal(qp.bucket_of(q_ref, cfg[1]), pat)
                assert eng.fault_info()[0] == abi.FAULT_NONE
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from e


def _frame_pool(ex):
    """The pool's packets as frames in one array: frame i is min(len, 80) window
    bytes, then zeros up to data_len, at offs[i]."""
    lens = ex.lens.astype(np.int64)
    offs = np.concatenate(([0], np.cumsum((lens + 15) & ~15)))
    pool = np.zeros(int(offs[-1]) + 80, np.uint8)
    for i in np.unique(ex.table[ex.table >= 0]):
        k = min(int(lens[i]), ex.stride)
        pool[offs[i]:offs[i] + k] = ex.win[i, :k]
    return pool, offs[:-1]


@pytest.mark.parametrize("n", qp.HOST_SIZES)
@pytest.mark.parametrize("cfg", qp.HOST_CFGS, ids=lambda c: "x".join(map(str, c)))
def test_host_frames(dev, oracle_mod, cfg, n):
    """yrss_dispatch_frames: the one-launch burst kernel (per-tile ranks, lists
    in LDS) up to 4096 packets and the batch kernels past that or when forced
    (one_launch=2), on the same frames."""
    nq = cfg[1]
    ex = ex_for(oracle_mod, cfg, qp.HOST_STRIDE)
    pool, offs = _frame_pool(ex)
    chunk, span = qp.host_aim(nq + 1, n)
    c = oracle_mod.cfg(*cfg)
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        for name, pat in members(ex, n, chunk, span):
            idx = qp.choose(pat, ex)
            ptrs = (np.uint64(pool.ctypes.data) + offs[idx].astype(np.uint64)).astype(np.uint64)
            lens = np.ascontiguousarray(ex.lens[idx])
            win_h, lens_h = qp.build(pat, ex)
            q_ref, h_ref = oracle_mod.dispatch_windows(win_h, qp.HOST_STRIDE, lens_h, c)
            assert np.array_equal(qp.bucket_of(q_ref, nq), pat), name
            qi_ref, qs_ref = oracle_mod.process_burst(q_ref, nq)
            for one_launch in (0, 2):
                eng.set_tuning(one_launch=one_launch)
                q = np.full(n + PAD, 0x5A5A, np.int16)
                h = np.full(n + PAD, 0x5A5A5A5A, np.uint32)
                qi = np.full(n + PAD, 0xFFFFFFFF, np.uint32)
                qs = np.full(nq + 2 + PAD, 0x77777777, np.uint32)
                rc = eng._lib.yrss_dispatch_frames(eng._ctx, ptrs.ctypes.data, lens.ctypes.data, n,
                                                   q.ctypes.data, h.ctypes.data, qi.ctypes.data,
                                                   qs.ctypes.data)
                where = f"{name} one_launch={one_launch}"
                assert rc == 0, where
                assert eng.fault_info()[0] == abi.FAULT_NONE, where
                assert np.array_equal(q[:n], q_ref) and np.array_equal(h[:n], h_ref), where
                assert np.array_equal(qs[:nq + 2], qs_ref), where
                d = np.nonzero(qi[:n] != qi_ref)[0]
                assert d.size == 0, f"{where}: {d.size} qidx mismatches, first at {d[:5]}"
                assert np.all(q[n:] == 0x5A5A) and np.all(h[n:] == 0x5A5A5A5A), where
                assert np.all(qi[n:] == 0xFFFFFFFF) and np.all(qs[nq + 2:] == 0x77777777), where


@pytest.mark.parametrize("n", qp.WORKER_SIZES)
@pytest.mark.parametrize("cfg", qp.HOST_CFGS, ids=lambda c: "x".join(map(str, c)))
def test_worker_windows(dev, oracle_mod, cfg, n):
    """The persistent worker on staged windows (yrss_worker_submit_windows):
    F-Stack's burst of 32 and the largest burst, every pattern as one burst."""
    nq, stride = cfg[1], qp.HOST_STRIDE
    ex = ex_for(oracle_mod, cfg, stride)
    chunk, span = qp.host_aim(nq + 1, n)
    c = oracle_mod.cfg(*cfg)
    raw = np.zeros(n * stride + 128, np.uint8)
    stage = raw[(-raw.ctypes.data) % 64:][:n * stride]     # 64-byte aligned staging
    with SoftRss(*cfg, device=0, max_burst=0) as eng:
        eng.register_host_memory(raw.ctypes.data, raw.nbytes)
        eng.worker_start(4, 2)
        try:
            for name, pat in members(ex, n, chunk, span):
                win_h, lens_h = qp.build(pat, ex)
                stage[:] = win_h
                r = eng.worker_poll(eng.worker_submit_windows(stage, stride, lens_h))
                q_ref, h_ref = oracle_mod.dispatch_windows(win_h, stride, lens_h, c)
                assert np.array_equal(qp.bucket_of(q_ref, nq), pat), name
                qi_ref, qs_ref = oracle_mod.process_burst(q_ref, nq)
                assert np.array_equal(r.q, q_ref) and np.array_equal(r.hash, h_ref), name
                assert np.array_equal(r.qstart, qs_ref), name
                d = np.nonzero(r.qidx != qi_ref)[0]
                assert d.size == 0, f"{name}: {d.size} qidx mismatches, first at {d[:5]}"
        finally:
            eng.worker_stop()
            eng.unregister_host_memory(raw.ctypes.data)
        assert eng.fault_info()[0] == abi.FAULT_NONE
