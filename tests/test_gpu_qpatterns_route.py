"""Directed route-class patterns through every routed list path (GPU).

The other routed tests feed the kernels oracle.synth's SYN_FUZZ stream: most
packets on q = 2, the hashed ones thin over the queues, and the classes that
routing adds (local, KNI, local ARP) interleaved at random.  Here the windows
are built on the host (qpatterns.route_exemplars) so that the route class of
every packet follows a chosen sequence: a whole tile, segment or burst in the
local queue, the freed, the KNI or the local ARP class with one stray packet
(byte rank 255 at the 16-class cap of the segmented form; class 63 with all six
ballot bits of peer_mask at the 64-class cap of the burst forms), the roles
swapped, runs over those classes that end on tile, segment and 1024-packet
edges and one either side, classes empty over the whole batch beside full ones,
a staircase, heavy-tailed draws.  Paths: yrss_route_dev_seg (the routed parse
variant and its segment flush), yrss_route_lists_burst / _frames (the routed
one-launch burst) and the route worker, whose slots meet one skew after the
opposite one.  Every batch is compared in full with the oracle: q, hash and
filter class, seg_idx / seg_off with segments.route_from and ridx / rstart
with segments.route_lists_from of the oracle's q and filter class; outputs are
longer than the batch and pre-filled; status() is 0 and the fault record empty
after every call.  Each test runs every member of every family in turn on one
context.  tests/test_qpatterns_route.py proves on the CPU that the windows
realise the requested classes."""
from types import SimpleNamespace

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import qpatterns as qp  # noqa: E402
import route_helpers as rh  # noqa: E402
from hostbufs import PAD, Arena, Out, fake_mbufs, frames_of, submit  # noqa: E402
from test_gpu_route_segments import check_route, upload  # noqa: E402
from yastack_amd import SoftRss, abi, segments  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    assert torch.cuda.is_available(), "GPU tests need a GPU"


def _mode(kind):
    enable, method = rh.KNI_MODES[kind[2]]
    return enable, method, method == "accept"


def _engine(kind):
    eng = SoftRss(*kind[0], device=0, max_burst=0)
    enable, method, _ = _mode(kind)
    eng.set_kni(enable, method, rh.TCP_PORTS, rh.UDP_PORTS)
    return eng


# ---- segmented form ------------------------------------------------------------------


@pytest.mark.parametrize("n", qp.ROUTE_SEG_SIZES)
@pytest.mark.parametrize("blocks", qp.ROUTE_SEG_BLOCKS)
@pytest.mark.parametrize("kind", qp.ROUTE_SEG_KINDS, ids=qp.route_kind_id)
def test_routed_segments(oracle_mod, kind, blocks, n):
    """route_dev_seg: process_tile over route_bucket and the routed segment
    flush, with one parse workgroup (a wave owns many chunks) and the default
    grid; the filter output wanted, and for the first member also not."""
    cfg, queue_id, _kni, stride = kind
    enable, _method, accept = _mode(kind)
    ex = qp.route_ex_for(oracle_mod, kind)
    chunk, span = qp.SEG_AIM
    with _engine(kind) as eng:
        if blocks:
            eng.set_tuning(parse_blocks=blocks)
        for k, (name, pat) in enumerate(qp.route_members(ex, n, chunk, span)):
            win, lens = qp.build(pat, ex)
            q_ref, h_ref, f_ref = qp.route_oracle(oracle_mod, kind, win, lens)
            win_t, lens_t = upload(win, lens)
            try:
                # the traffic is the pattern (test_qpatterns_route.py proves it on the CPU)
                assert np.array_equal(
                    segments.route_buckets(q_ref, f_ref, cfg[1], queue_id, enable, accept), pat)
                for want_filter in ((True, False) if k == 0 else (True,)):
                    check_route(eng, win_t, lens_t, n, stride, queue_id, q_ref, h_ref, f_ref,
                                enable, accept, want_filter=want_filter)
                    assert eng.fault_info()[0] == abi.FAULT_NONE
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from e


# ---- one-launch bursts -----------------------------------------------------------------

HEADROOM = 130
_MBUFS = {}


def mbufs_for(oracle_mod, kind):
    """The exemplars of a case as an rte_mbuf pool: (mem, mbuf ptr and frame
    data ptr of every pool index in the table, as arrays indexed by pool index)."""
    if kind not in _MBUFS:
        ex = qp.route_ex_for(oracle_mod, kind)
        used = np.unique(ex.table[ex.table >= 0])
        frames = frames_of(ex.win[used].reshape(-1), ex.lens[used], ex.stride)
        mem, ptrs, _ = fake_mbufs(frames, headroom=HEADROOM)
        mp = np.zeros(ex.lens.size, np.uint64)
        mp[used] = ptrs
        dp = np.zeros(ex.lens.size, np.uint64)
        dp[used] = ptrs + np.uint64(128 + HEADROOM)
        _MBUFS[kind] = (mem, mp, dp)
    return _MBUFS[kind]


def burst_of(oracle_mod, kind, ex, pat, stride=None):
    """(lens, mbuf ptrs, data ptrs, oracle q, hash, filter class) of a member.
    stride None: the host gather's rule (64-byte windows when every frame of
    the burst fits, else 80); the worker's gather always stages 80."""
    _mem, mp, dp = mbufs_for(oracle_mod, kind)
    idx = qp.choose(pat, ex)
    lens = np.ascontiguousarray(ex.lens[idx])
    if stride is None:
        stride = 64 if int(lens.max()) <= 64 else 80
    win = np.ascontiguousarray(ex.win[idx][:, :stride]).reshape(-1)
    q, h, f = qp.route_oracle(oracle_mod, kind, win, lens, stride)
    return lens, np.ascontiguousarray(mp[idx]), np.ascontiguousarray(dp[idx]), q, h, f


@pytest.mark.parametrize("n", qp.ROUTE_BURST_SIZES)
@pytest.mark.parametrize("kind", qp.ROUTE_BURST_KINDS, ids=qp.route_kind_id)
def test_routed_one_launch_bursts(oracle_mod, kind, n):
    """route_lists_burst on an mbuf pool and route_lists_frames: the kRoute
    burst body at 6, 16, 17 and 64 classes; a tile, 16 tiles (every wave one)
    and 64 tiles (every wave four)."""
    cfg, queue_id, _kni, _stride = kind
    nq = cfg[1]
    enable, _method, accept = _mode(kind)
    ex = qp.route_ex_for(oracle_mod, kind)
    chunk, span = qp.ROUTE_BURST_AIM
    with _engine(kind) as eng:
        for k, (name, pat) in enumerate(qp.route_members(ex, n, chunk, span)):
            lens, mp, dp, q, h, f = burst_of(oracle_mod, kind, ex, pat)
            try:
                assert np.array_equal(
                    segments.route_buckets(q, f, nq, queue_id, enable, accept), pat)
                for form in ("mbufs", "frames"):
                    o = Out(n, nq, want_hash=bool(k & 1) or form == "frames")
                    if form == "mbufs":
                        rc = eng._lib.yrss_route_lists_burst(
                            eng._ctx, mp.ctypes.data, n, queue_id, o.p(o.q), o.p(o.h), o.p(o.f),
                            o.p(o.ri), o.p(o.rs), 0)
                    else:
                        rc = eng._lib.yrss_route_lists_frames(
                            eng._ctx, dp.ctypes.data, lens.ctypes.data, n, queue_id, o.p(o.q),
                            o.p(o.h), o.p(o.f), o.p(o.ri), o.p(o.rs))
                    assert rc == 0, (form, rc)
                    assert eng.status() == 0
                    o.check(q, h, f, queue_id, enable, accept)
                    assert eng.fault_info()[0] == abi.FAULT_NONE
            except AssertionError as e:
                raise AssertionError(f"{name}: {e}") from e


# ---- route worker ----------------------------------------------------------------------

NSLOTS = 4


@pytest.mark.parametrize("n", qp.WORKER_SIZES)
@pytest.mark.parametrize("kind", qp.ROUTE_WORKER_KINDS, ids=qp.route_kind_id)
def test_route_worker(oracle_mod, kind, n):
    """One workgroup over a ring of four slots: every member of every family in
    turn, so each slot is reused many times and meets one skew after the
    opposite one.  The three submit forms rotate; the outputs alternate between
    registered memory and slot staging.  Every ticket of a flight is polled
    before the ring would wrap."""
    cfg, queue_id, _kni, _stride = kind
    nq = cfg[1]
    enable, _method, accept = _mode(kind)
    ex = qp.route_ex_for(oracle_mod, kind)
    chunk, span = qp.ROUTE_BURST_AIM
    mem = mbufs_for(oracle_mod, kind)[0]
    members = list(qp.route_members(ex, n, chunk, span))
    assert len(members) >= 7 * NSLOTS      # every slot is reused at least six times
    stage = Arena(NSLOTS * (n * 80 + 64))
    arena = Arena(NSLOTS * ((n + PAD) * 10 + (nq + 4 + PAD) * 4 + 256))
    with _engine(kind) as eng:
        for a in (mem, stage.mem, arena.mem):
            eng.register_host_memory(a.ctypes.data, a.nbytes)
        eng.worker_start(NSLOTS, 1, route_queue_id=queue_id)
        try:
            for first in range(0, len(members), NSLOTS):
                flight = []
                stage.used = arena.used = 0
                for k in range(first, min(first + NSLOTS, len(members))):
                    name, pat = members[k]
                    lens, mp, dp, q, h, f = burst_of(oracle_mod, kind, ex, pat, stride=80)
                    assert np.array_equal(
                        segments.route_buckets(q, f, nq, queue_id, enable, accept), pat), name
                    form = ("mbufs", "frames", "windows")[k % 3]
                    o = Out(n, nq, want_hash=k % 4 != 3, want_filter=False,
                            arena=arena if k % 2 else None)
                    wreg = SimpleNamespace(mem=stage.take(n * 80, np.uint8, 0))
                    if form == "windows":
                        wreg.mem[:] = np.ascontiguousarray(ex.win[qp.choose(pat, ex)]).reshape(-1)
                    t = submit(eng, form, 0, n, o, (lens, mp, dp), wreg)
                    flight.append((t, name, o, q, h, f, (lens, mp, dp, wreg)))
                for t, name, o, q, h, f, _keep in flight:
                    assert eng._lib.yrss_worker_poll(eng._ctx, t, 1) == 0, name
                    try:
                        o.check(q, h, f, queue_id, enable, accept)
                    except AssertionError as e:
                        raise AssertionError(f"{name}: {e}") from e
        finally:
            eng.worker_stop()
            for a in (mem, stage.mem, arena.mem):
                eng.unregister_host_memory(a.ctypes.data)
        assert eng.fault_info()[0] == abi.FAULT_NONE
