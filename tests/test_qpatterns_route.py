"""The directed route-class builder (qpatterns.route_exemplars and the route
members of qpatterns.family) and the host side of the routed lists on its
patterns (no GPU).

For every route case, size, aim and family that tests/test_gpu_qpatterns_route.py
uses: the oracle's q and filter class of the built windows map, through
segments.route_buckets, to exactly the requested class sequence; the set of
reachable classes of every case is pinned; all_but_one, runs and zipf each
reach every reachable class; the numpy twins (segments.route_from per segment,
route_lists_from per burst) equal a stable argsort and a bincount; the class
rule equals the destination the per-packet model (oracle.process_packets_route,
unbounded rings, clones that succeed) gives every packet; and yrss_route_seg /
yrss_route_lists with bounded rings and failing clones hand off what the model
hands off, on batches that are all local ARP but one packet, all one foreign
ring but one, and a run sequence.
"""
import numpy as np
import pytest

import qpatterns as qp
import route_helpers as rh
import route_lists_helpers as rl
from yastack_amd import abi, segments

AIMS = qp.route_aims()
KINDS = list(dict.fromkeys(a[0] for a in AIMS))

# Route classes no packet of the pool reaches, case by case (nq = nb_queues;
# nq freed, nq + 1 KNI, nq + 2 local ARP).  From the class rule one expects:
# local ARP iff queue_id == 0; KNI iff KNI is enabled and queue_id < nq; local
# iff queue_id < nq; freed iff some q >= nq or the stride is 64 (the truncated
# frame).  The oracle disagrees in one place, and wins: with
# dispatch_only_core = 1 queue 0 receives ARP and RARP only, RARP's filter class
# is UNKNOWN, and under "accept" UNKNOWN is local: KNI is unreachable there
# ((3,3,1,1) and (5,3,1,1) on queue 0).  (Under "reject" it would be local that
# stays empty; no case here has that.)
UNREACHABLE = {
    "13x13x1x0-q0-accept-s64": [],
    "13x13x1x0-q2-reject-s64": [15],
    "13x13x1x0-q13-off-s64": [14, 15],
    "6x4x1x0-q0-accept-s64": [],
    "6x4x1x0-q2-reject-s64": [6],
    "3x3x1x1-q0-accept-s64": [4],
    "3x3x1x1-q2-off-s64": [4, 5],
    "1x1x1x0-q0-reject-s64": [],
    "13x13x1x0-q0-reject-s80": [13],
    "5x3x1x1-q0-accept-s80": [4],
    "5x3x1x0-q2-reject-s80": [5],
    "16x13x1x0-q2-accept-s80": [15],
    "14x14x1x0-q0-accept-s80": [14],
    "17x14x1x0-q2-reject-s80": [16],
    "64x61x1x0-q0-accept-s80": [],
    "61x61x1x0-q2-reject-s80": [61, 63],
    "64x61x1x0-q61-off-s80": [62, 63],
    "64x61x1x0-q0-reject-s80": [],
    "5x3x1x0-q0-accept-s80": [],
    "5x3x1x1-q2-reject-s80": [5],
    "64x61x1x0-q2-accept-s80": [63],
}


def _aim_id(a):
    kind, n, chunk, span = a
    return f"{qp.route_kind_id(kind)}-n{n}-c{chunk}-g{span}"


def _classes(oracle_mod, kind, pat, ex):
    """(q, f, route classes) the oracle gives the windows built for `pat`."""
    cfg, queue_id, kni, stride = kind
    enable, method = rh.KNI_MODES[kni]
    win, lens = qp.build(pat, ex)
    assert win.shape == (pat.size * stride,) and lens.shape == (pat.size,)
    q, _h, f = qp.route_oracle(oracle_mod, kind, win, lens)
    return q, f, segments.route_buckets(q, f, cfg[1], queue_id, enable, method == "accept")


def _model_classes(oracle_mod, q, f, nq, queue_id, enable, accept):
    """Every packet's destination in oracle.process_packets_route with rings
    that never fill and clones that always succeed, as a route class."""
    n = len(q)
    rings, local, kni, freed = oracle_mod.process_packets_route(
        q, f, nq, queue_id, enable, accept, True, [n * (nq + 1) + 1] * nq)
    dest = np.full(n, -1, np.int64)
    for j, objs in rings.items():
        for o in objs:
            if o[0] == "pkt":
                assert dest[o[1]] == -1
                dest[o[1]] = j
            else:                       # only ARP on the local queue is cloned
                assert f[o[1]] == abi.FILTER_ARP and q[o[1]] == queue_id
    for o in local:
        assert o[0] == "pkt" and dest[o[1]] == -1
        dest[o[1]] = nq + 2 if f[o[1]] == abi.FILTER_ARP else queue_id
    for o in kni:
        if o[0] == "pkt":
            assert dest[o[1]] == -1
            dest[o[1]] = nq + 1
    for o in freed:
        assert o[0] == "pkt" and dest[o[1]] == -1
        dest[o[1]] = nq
    return dest


@pytest.mark.parametrize("family", qp.FAMILIES)
@pytest.mark.parametrize("aim", AIMS, ids=_aim_id)
def test_patterns_realise_and_twins_are_a_stable_partition(oracle_mod, aim, family):
    kind, n, chunk, span = aim
    cfg, queue_id, kni, _stride = kind
    nq, nb = cfg[1], cfg[1] + 3
    enable, method = rh.KNI_MODES[kni]
    accept = method == "accept"
    ex = qp.route_ex_for(oracle_mod, kind)
    members = qp.family(family, n, ex, chunk, span)
    assert members
    for k, (label, pat) in enumerate(members):
        assert pat.shape == (n,), label
        q, f, bkt = _classes(oracle_mod, kind, pat, ex)
        assert np.array_equal(bkt, pat), f"{label}: not realised at {np.nonzero(bkt != pat)[0][:5]}"
        if family == "all_but_one":
            assert np.sort(np.bincount(pat))[-2:].tolist() == [1, n - 1], label
        # the twins against a stable argsort and a bincount of the requested classes
        ri_ref, rs_ref = qp.expected_lists(pat, nb)
        ri, rs = segments.route_lists_from(q, f, nq, queue_id, enable, accept)
        assert np.array_equal(rs, rs_ref) and np.array_equal(ri, ri_ref), label
        si, so = segments.route_from(q, f, nq, queue_id, enable, accept)
        assert so.shape == (segments.nseg_for(n), nb + 1)
        for s in range(segments.nseg_for(n)):
            i_ref, o_ref = qp.expected_lists(pat[256 * s:256 * (s + 1)], nb)
            assert np.array_equal(so[s], o_ref), (label, s)
            assert np.array_equal(si[256 * s:256 * s + i_ref.size], i_ref), (label, s)
        # the class rule against the per-packet model (one packet at a time in
        # Python: every member up to 4097 packets, the first of a longer batch)
        if n <= 4097 or k == 0:
            dest = _model_classes(oracle_mod, q, f, nq, queue_id, enable, accept)
            assert np.array_equal(dest, pat), label


def _rule(kind):
    """The reachable classes the class rule predicts (see UNREACHABLE)."""
    (npr, nq, _soft, only), queue_id, kni, stride = kind
    enable, method = rh.KNI_MODES[kni]
    hashed = range(1, npr) if only else range(npr)
    qs = set(hashed) | {0, 2}                  # ARP / RARP, UDP
    want = {b for b in qs if b < nq and b != queue_id}
    if queue_id < nq and queue_id in qs:
        want.add(queue_id)
        if enable:
            want.add(nq + 1)
    if queue_id == 0:
        want.add(nq + 2)
    if stride < 66 or max(qs) >= nq:
        want.add(nq)
    return want


@pytest.mark.parametrize("kind", KINDS, ids=qp.route_kind_id)
def test_reachable_classes_are_pinned(oracle_mod, kind):
    cfg, queue_id, kni, stride = kind
    nq = cfg[1]
    enable, method = rh.KNI_MODES[kni]
    ex = qp.route_ex_for(oracle_mod, kind)
    unreachable = UNREACHABLE[qp.route_kind_id(kind)]
    assert ex.reachable == [b for b in range(nq + 3) if b not in unreachable]
    want = _rule(kind)
    if cfg[3] and queue_id == 0:
        # the oracle wins: queue 0 holds ARP and RARP only, RARP is UNKNOWN
        want.discard(nq + 1 if method == "accept" else 0)
    assert set(ex.reachable) == want
    # the table is what the oracle and the class rule say, and the model agrees
    pool = np.unique(ex.table[ex.table >= 0])
    bkt = segments.route_buckets(ex.q[pool], ex.fclass[pool], nq, queue_id, enable,
                                 method == "accept")
    for b in ex.reachable:
        assert np.all(bkt[np.isin(pool, ex.table[b])] == b)
    dest = _model_classes(oracle_mod, ex.q[pool], ex.fclass[pool], nq, queue_id, enable,
                          method == "accept")
    assert np.array_equal(dest, bkt)
    # the frames the added classes are there for
    special = {int(i) for i in pool if i >= ex.lens.size - (7 if stride < 66 else 6)}
    kinds = {int(ex.fclass[i]) for i in special} | {int(ex.q[i]) for i in special}
    if queue_id == 0:
        assert abi.FILTER_ARP in kinds
    if stride < 66:
        assert abi.Q_TRUNCATED in ex.q[ex.table[nq]]
    if queue_id == 2 and enable:      # UDP on and off the list: local and KNI
        udp = [i for i in special if ex.q[i] == 2 and ex.win[i, 23] == 17]
        assert {int(bkt[np.nonzero(pool == i)[0][0]]) for i in udp} == {2, nq + 1}


@pytest.mark.parametrize("aim", AIMS, ids=_aim_id)
def test_no_family_runs_empty(oracle_mod, aim):
    kind, n, chunk, span = aim
    ex = qp.route_ex_for(oracle_mod, kind)
    for family in ("all_but_one", "runs", "zipf"):
        seen = set()
        for _label, pat in qp.family(family, n, ex, chunk, span):
            seen |= set(np.unique(pat).tolist())
        assert seen == set(ex.reachable), (family, sorted(set(ex.reachable) - seen))
    # the added classes are the subject: each is the big class of an all_but_one
    # member, and there are members with the roles swapped
    abo = qp.family("all_but_one", n, ex, chunk, span)
    big = {int(np.bincount(p).argmax()) for _, p in abo} if n > 2 else set()
    assert set(ex.own()) <= big
    if ex.foreign():
        assert big & set(ex.foreign())
    labels = [m[0] for m in qp.family("runs", n, ex, chunk, span)]
    for R in qp.ROUTE_RUNS + (1023, 1024, 1025):
        if R <= n:
            assert f"all-R{R}" in labels
            assert len(ex.own()) < 2 or f"own-R{R}" in labels


def _hand_off_members(ex, n, chunk, span):
    nq = ex.nb_queues
    abo = qp.family("all_but_one", n, ex, chunk, span)
    out = []
    arp = [m for m in abo if np.bincount(m[1]).argmax() == nq + 2]
    ring = [m for m in abo if np.bincount(m[1]).argmax() in ex.foreign()]
    out += arp[:1] + ring[:1]
    out += [m for m in qp.family("runs", n, ex, chunk, span) if m[0] == "all-R64"]
    return out


@pytest.mark.parametrize("kind", KINDS, ids=qp.route_kind_id)
def test_host_hand_off_on_directed_batches(oracle_mod, kind):
    """yrss_route_seg (up to 16 classes) and yrss_route_lists on the twins'
    arrays: bounded rings that fill (every local ARP packet is cloned to every
    other queue) and clones that fail, against the per-packet model."""
    cfg, queue_id, kni, _stride = kind
    nq = cfg[1]
    enable, method = rh.KNI_MODES[kni]
    accept = method == "accept"
    ex = qp.route_ex_for(oracle_mod, kind)
    seg = nq + 3 <= abi.SEG_MAX_BUCKETS
    for n in ((257, 4097) if seg else (1024,)):
        chunk, span = qp.SEG_AIM if seg else qp.ROUTE_BURST_AIM
        members = _hand_off_members(ex, n, chunk, span)
        assert len(members) >= (2 if ex.foreign() else 1)
        assert (queue_id == 0) == any(np.bincount(p).argmax() == nq + 2 for _, p in members)
        cap = n // 4
        ptrs, addr_to_idx = rh.fake_objs(n)
        for label, pat in members:
            q, f, bkt = _classes(oracle_mod, kind, pat, ex)
            assert np.array_equal(bkt, pat), label
            freed_ref = None
            if seg:
                cb = rh.Rings(addr_to_idx, [cap] * nq, rh.clone_ok)
                si, so = segments.route_from(q, f, nq, queue_id, enable, accept)
                rc, local, kni_list, res = rh.route_seg_c(si, so, n, nq, queue_id, enable, f, ptrs,
                                                          cb)
                assert rc == 0, label
                rh.assert_matches_model(cb, local, kni_list, res, q, f, nq, queue_id, enable,
                                        accept, cap)
            cb = rh.Rings(addr_to_idx, [cap] * nq, rh.clone_ok)
            ri, rs = segments.route_lists_from(q, f, nq, queue_id, enable, accept)
            rc, local, kni_list, res = rl.route_lists_c(ri, rs, n, nq, queue_id, enable, f, ptrs, cb)
            assert rc == 0, label
            _, _, _, freed_ref = rh.assert_matches_model(cb, local, kni_list, res, q, f, nq,
                                                         queue_id, enable, accept, cap)
            if np.bincount(pat).argmax() == nq + 2 and nq > 1:
                assert any(o[0] == "clone" for o in freed_ref), f"{label}: rings filled"
