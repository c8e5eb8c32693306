"""The directed-traffic builder (tests/qpatterns.py) and the oracle's lists on
its patterns (no GPU).

For every configuration, size, layout aim and pattern family that
tests/test_gpu_qpatterns.py uses, the oracle's q of the built windows must map,
through the bucket rule, to exactly the intended bucket sequence: a condition on
the builder, with no case skipped.  On the same patterns oracle.process_burst
must equal a stable argsort and a bincount written here in numpy, and up to 16
buckets the segmented form (segments.from_q / to_lists / to_lists_c) must lead
to the same lists.
"""
import numpy as np
import pytest

import qpatterns as qp
from frames import ethertype_frame
from yastack_amd import segments

_EX = {}


def ex_for(oracle_mod, cfg, stride):
    if (cfg, stride) not in _EX:
        _EX[(cfg, stride)] = qp.exemplars(oracle_mod, cfg, stride)
    return _EX[(cfg, stride)]


def _aims():
    """Every (cfg, stride, n, chunk, span) some GPU case builds patterns for."""
    seen = {}
    for _path, cfg, tune, n in qp.GLOBAL_CASES:
        seen[(cfg, 64, n) + qp.aim_of(cfg[1] + 1, tune)] = None
    for cfg, _blocks, n in qp.SEG_CASES:
        seen[(cfg, 64, n) + qp.SEG_AIM] = None
    for cfg in qp.HOST_CFGS:
        for n in qp.HOST_SIZES + qp.WORKER_SIZES:
            seen[(cfg, qp.HOST_STRIDE, n) + qp.host_aim(cfg[1] + 1, n)] = None
    return list(seen)


AIMS = _aims()
ALL_CFGS = sorted({(a[0], a[1]) for a in AIMS})


def _id(a):
    cfg, stride, n, chunk, span = a
    return f"{'x'.join(map(str, cfg))}-s{stride}-n{n}-c{chunk}-g{span}"


@pytest.mark.parametrize("family", qp.FAMILIES)
@pytest.mark.parametrize("aim", AIMS, ids=_id)
def test_patterns_realise_and_lists_are_a_stable_partition(oracle_mod, aim, family):
    cfg, stride, n, chunk, span = aim
    nq, nb = cfg[1], cfg[1] + 1
    ex = ex_for(oracle_mod, cfg, stride)
    members = qp.family(family, n, ex, chunk, span)
    assert members
    for label, pat in members:
        assert pat.shape == (n,), label
        win, lens = qp.build(pat, ex)
        assert win.shape == (n * stride,) and lens.shape == (n,)
        q, _h = oracle_mod.dispatch_windows(win, stride, lens, oracle_mod.cfg(*cfg))
        bkt = qp.bucket_of(q, nq)
        assert np.array_equal(bkt, pat), f"{label}: not realised at {np.nonzero(bkt != pat)[0][:5]}"
        if family == "all_but_one":     # (one bucket alone would be the one-list shortcut)
            assert np.sort(np.bincount(pat))[-2:].tolist() == [1, n - 1], label
        # the oracle's lists against the numpy statement.  process_burst returns
        # nb_queues + 2 offsets: entry nb_queues is the drop bucket's start and
        # the trailing entry nb_queues + 1 its end, the batch size
        qi_ref, qs_ref = qp.expected_lists(bkt, nb)
        qi, qs = oracle_mod.process_burst(q, nq)
        assert qs.shape == (nq + 2,) and qs[0] == 0 and qs[nq + 1] == n
        assert np.array_equal(qs, qs_ref), label
        assert np.array_equal(qi, qi_ref), label
        if nb <= 16:
            si, so = segments.from_q(q, nq)
            for fn in (segments.to_lists, segments.to_lists_c):
                li, ls = fn(si, so, n, nb)
                assert np.array_equal(ls, qs_ref), (label, fn.__name__)
                assert np.array_equal(li, qi_ref), (label, fn.__name__)


@pytest.mark.parametrize("cfg,stride", ALL_CFGS, ids=lambda v: str(v).replace(" ", ""))
def test_exemplars_reach_every_bucket(oracle_mod, cfg, stride):
    """Every bucket 0 .. nb_queues has a packet, with one exception that no
    frame can lift: at full windows (the host paths) nothing truncates, so with
    nb_procs == nb_queues and hashing over all of them no q leaves the range and
    the drop bucket stays empty."""
    npr, nq, soft, only = cfg
    ex = ex_for(oracle_mod, cfg, stride)
    want = list(range(nq + 1))
    if stride >= 80 and npr == nq:
        want = want[:-1]
    assert ex.reachable == want
    # the table is what the oracle says
    for b in ex.reachable:
        assert np.all(qp.bucket_of(ex.q[ex.table[b]], nq) == b)
    # several flows a bucket wherever the bucket is fed by hashing
    hashed = [b for b in ex.queues() if np.unique(ex.table[b]).size > 1]
    assert len(hashed) >= min(nq, npr) - 2
    for b in hashed:
        assert np.unique(ex.hash[ex.table[b]]).size == np.unique(ex.table[b]).size
    if stride < 66:
        kinds = ex.q[ex.table[nq]]
        assert (kinds == -2).any()                      # YRSS_Q_TRUNCATED
        if npr > nq:
            assert (kinds >= nq).any()


def test_arp_is_the_only_q0_with_dispatch_only_core(oracle_mod):
    for cfg in ((3, 3, 1, 1), (128, 127, 1, 1), (4096, 256, 1, 1)):
        ex = ex_for(oracle_mod, cfg, 64)
        zero = np.nonzero(ex.q == 0)[0]
        arp = np.frombuffer(ethertype_frame(0x0806)[:64], np.uint8)
        assert zero.size == 1 and np.array_equal(ex.win[zero[0]], arp)


def test_unreachable_bucket_is_refused(oracle_mod):
    ex = ex_for(oracle_mod, (63, 63, 1, 0), 80)
    with pytest.raises(ValueError, match="unreachable"):
        qp.build(np.array([0, 63, 1]), ex)


def test_full_windows_equal_the_per_frame_oracle(oracle_mod):
    """The host paths' expected values come from dispatch_windows at stride 80:
    the same as toeplitz_dispatch frame by frame (nothing truncates at 80)."""
    cfg = (5, 4, 1, 1)
    ex = ex_for(oracle_mod, cfg, 80)
    c = oracle_mod.cfg(*cfg)
    pick = np.concatenate([np.arange(0, ex.lens.size, 97), ex.table[ex.table >= 0]])
    for i in pick:
        q, h = oracle_mod.toeplitz_dispatch(ex.win[i].tobytes(), int(ex.lens[i]), c)
        assert (q, h) == (int(ex.q[i]), int(ex.hash[i]))


def test_generators():
    n, chunk, span = 5000, 256, 1024
    p = qp.all_but_one(n, 3, 7, 255)
    assert (p == 3).sum() == n - 1 and p[255] == 7
    p = qp.runs(n, [4, 0, 9], 17)
    assert p[:17].tolist() == [4] * 17 and p[17] == 0 and p[34] == 9 and p[51] == 4
    p = qp.sparse(n, [2, 6], seed=3)
    assert set(np.unique(p)) == {2, 6} and p.size == n
    # first / last / carried / spread
    p = qp.late_and_early(n, [1, 2, 3, 4, 5], span)
    last0 = (n - 1) // span * span
    assert np.nonzero(p == 1)[0].max() < span
    assert np.nonzero(p == 2)[0].min() >= last0
    assert np.nonzero(p == 3)[0].tolist() == [1, n - 1]
    for s in range(1, last0 // span):
        assert set(np.unique(p[s * span:(s + 1) * span])) <= {4, 5}
    # the staircase's counts, span by span
    bk = list(range(9))
    p = qp.staircase(n, bk, 4, span)
    others = [b for b in bk if b != 4]
    for s in range(n // span):          # whole spans
        cnt = np.bincount(p[s * span:(s + 1) * span], minlength=9)
        assert [cnt[b] for b in others] == [(7 * j + s) % 33 for j in range(8)]
    phases = {int(np.bincount(p[:(s + 1) * span], minlength=9)[1]) % 16 for s in range(n // span)}
    assert len(phases) > 1
    a, b = qp.zipf(n, bk, 5), qp.zipf(n, bk, 5)
    assert np.array_equal(a, b) and np.bincount(a, minlength=9).max() > 2 * n // 9


def test_families_hold_the_boundary_members(oracle_mod):
    ex = ex_for(oracle_mod, (16, 15, 1, 0), 64)
    n, chunk, span = 33011, 256, 8192
    labels = [m[0] for m in qp.family("runs", n, ex, chunk, span)]
    assert labels == [f"R{r}" for r in (1, 15, 16, 17, 63, 64, 65, 255, 256, 257, 8191, 8192, 8193)]
    abo = qp.family("all_but_one", n, ex, chunk, span)
    big = {int(np.bincount(p).argmax()) for _, p in abo}
    assert big == {0, 7, 14, 15}                      # first, middle, last queue, drop
    pos = {int(np.nonzero(p != np.bincount(p).argmax())[0][0]) for _, p in abo}
    assert pos == {0, n - 1, (n // 2) // chunk * chunk, (n // span) * span - 1}
    assert len(abo) == 16
    keeps = [set(np.unique(p).tolist()) for _, p in qp.family("sparse", n, ex, chunk, span)]
    assert keeps == [{0, 15}, set(range(1, 16, 2)), {7, 15}]
