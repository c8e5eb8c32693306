"""Directed traffic: header windows built so that the oracle's q follows a
chosen bucket sequence.

The synthetic profiles give two queue distributions only: hashed TCP (near
uniform over the queues, all buckets populated and interleaved at random) and
all-UDP (one bucket: the lists' one-list shortcut).  The per-queue list kernels
are a stable partition by bucket, and a stable partition goes wrong at the
shapes those never reach: a whole chunk in one bucket, buckets empty for spans
or for the whole batch, runs that end on a line, tile, chunk or span boundary.

`exemplars` finds, with the oracle, packets for every bucket of a
configuration (bucket = q, or nb_queues where process_packets frees the
packet, fs/lib/ff_dpdk_if.c:1080-1083); `build` fancy-indexes them by an integer
bucket sequence into (win, lens); the generators below make the sequences.
Pure numpy, no GPU.  Whether a sequence was realised is checked by the caller
(tests/test_qpatterns.py: exactly, for every configuration the GPU tests use).

`route_exemplars` does the same over the nb_queues + 3 route classes of the
routed lists (segments.route_buckets: the foreign rings, local, freed, KNI,
local ARP), from the oracle's q and filter class; `family` then adds members
whose subject is those classes (tests/test_qpatterns_route.py proves them,
tests/test_gpu_qpatterns_route.py runs them).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from frames import ethertype_frame, ipv4_frame

PER_BUCKET = 4      # flows kept per bucket (fewer where the pool has fewer)
SYN_TCP4 = 5        # include/yrss_synth.h (yastack_amd.abi.SYN_TCP4)


@dataclass
class Exemplars:
    win: np.ndarray        # [m, stride] uint8: the pool's windows
    lens: np.ndarray       # [m] uint16
    q: np.ndarray          # [m] the oracle's q of every pool packet
    hash: np.ndarray       # [m] its hash
    table: np.ndarray      # [nb, PER_BUCKET] pool indices, -1 = bucket unreachable
    nb_queues: int
    stride: int
    # route_exemplars only: the buckets are the nb_queues + 3 route classes of
    # segments.route_buckets for the lcore whose queue is queue_id
    fclass: np.ndarray | None = None      # [m] the oracle's filter class
    queue_id: int = -1

    @property
    def route(self) -> bool:
        return self.fclass is not None

    @property
    def nb(self) -> int:
        return self.nb_queues + (3 if self.route else 1)

    def own(self) -> list:
        """Reachable route classes the lcore keeps or frees itself: local,
        freed, KNI, local ARP (every class but the foreign rings)."""
        nq = self.nb_queues
        return [b for b in self.reachable if b == self.queue_id or b >= nq]

    def foreign(self) -> list:
        """Reachable rings of the other queues."""
        return [b for b in self.queues() if b != self.queue_id]

    @property
    def reachable(self) -> list:
        """Buckets some pool packet lands in, ascending."""
        return [b for b in range(self.nb) if self.table[b, 0] >= 0]

    def queues(self) -> list:
        """Reachable buckets without the drop bucket."""
        return [b for b in self.reachable if b < self.nb_queues]


def bucket_of(q, nb_queues: int) -> np.ndarray:
    """The bucket rule of process_packets' dispatcher block (ff_dpdk_if.c:
    1080-1094): ret < 0 || ret >= nb_queues is freed (bucket nb_queues)."""
    q = np.asarray(q).astype(np.int64)
    return np.where((q >= 0) & (q < nb_queues), q, nb_queues)


def exemplars(oracle_mod, cfg, stride: int = 64, n_tcp: int | None = None) -> Exemplars:
    """A pool of windows and, per bucket of cfg = (nb_procs, nb_queues,
    soft_dispatch, dispatch_only_core), up to PER_BUCKET pool packets the
    oracle puts there.  The pool: hashed TCP4 flows, one ARP frame (the only
    q = 0 when dispatch_only_core = 1), one UDP frame (q = 2) and, at stride 64,
    one TCP frame whose ports lie past the window (YRSS_Q_TRUNCATED: dropped).
    The drop bucket's exemplars hold one packet of each kind that reaches it
    (q >= nb_queues, truncated) before further flows."""
    npr, nq, _soft, _only = cfg
    extra = [(ethertype_frame(0x0806), 64),
             (ipv4_frame("10.1.2.3", 5353, "10.3.2.1", 53, proto=17, length=64), 64)]
    if stride < 66:
        # IHL 12: ports at 14 + 48 .. 66 > 64, data_len 100: hashed by the
        # reference, not decidable from a 64-byte window
        extra.append((ipv4_frame("10.9.8.7", 4321, "10.7.8.9", 443, ihl=12, length=100,
                                 total_len=None), 100))
    win, lens, n_tcp = _pool(oracle_mod, npr, stride, n_tcp, extra)
    q, h = oracle_mod.dispatch_windows(win.reshape(-1), stride, lens, oracle_mod.cfg(*cfg))
    bkt = bucket_of(q, nq)
    table = np.full((nq + 1, PER_BUCKET), -1, np.int64)
    order = np.argsort(bkt, kind="stable")
    start = np.searchsorted(bkt[order], np.arange(nq + 2))
    for b in range(nq + 1):
        mine = order[start[b]:start[b + 1]]
        # one packet a flow (the pool repeats flows): distinct (q, hash)
        key = (h[mine].astype(np.int64) << 16) | (q[mine].astype(np.int64) & 0xFFFF)
        mine = mine[np.sort(np.unique(key, return_index=True)[1])]
        if b == nq and mine.size:
            # one of each kind first: q >= nb_queues, truncated (and below 0 in general)
            over = mine[q[mine] >= nq][:1]
            neg = mine[q[mine] < 0][:1]
            rest = np.setdiff1d(mine, np.concatenate([over, neg]), assume_unique=True)
            mine = np.concatenate([over, neg, rest])
        k = min(mine.size, PER_BUCKET)
        if k:
            table[b] = np.resize(mine[:k], PER_BUCKET)    # cycle when fewer
    return Exemplars(win, lens, q, h, table, nq, stride)


def _pool(oracle_mod, npr: int, stride: int, n_tcp: int | None, extra):
    """(win [m, stride], lens [m], n_tcp): hashed TCP4 flows, then `extra`
    (frame, data_len) pairs cut to the stride."""
    if n_tcp is None:
        n_tcp = 65536 if npr > 1024 else 8192
    w, l = oracle_mod.synth(SYN_TCP4, n_tcp, first=12345, stride=stride)
    ew = np.stack([np.frombuffer(f[:stride], np.uint8) for f, _ in extra])
    win = np.concatenate([w.reshape(n_tcp, stride), ew])
    lens = np.concatenate([l, np.array([x for _, x in extra], np.uint16)])
    return win, lens, n_tcp


UDP_DPORTS = (53, 9999, 25000, 40000)     # some on, some off any sensible udp_port list


def route_exemplars(oracle_mod, cfg, queue_id: int, kni, tcp_ports, udp_ports,
                    stride: int = 64, n_tcp: int | None = None) -> Exemplars:
    """The same over the nb_queues + 3 route classes of segments.route_buckets
    (b < nq, b != queue_id: ring of queue b; queue_id: local; nq: freed; nq + 1:
    KNI; nq + 2: local ARP) for kni = (enable, "accept" | "reject") and the two
    KNI port lists.  The pool is that of `exemplars` (the TCP flows carry
    destination ports on both sides of a list such as "0-30000") plus what the
    added classes need: UDP frames (q = 2) with several destination ports, a
    RARP frame (q = 0, filter class UNKNOWN: with dispatch_only_core = 1 the
    only packet on queue 0 that is not ARP) and, at stride 64, the truncated TCP
    frame.  Classes come from the oracle's q (dispatch_windows) and filter class
    (filter_windows) through the class rule; a class's exemplars hold the
    frames that are no TCP flows first."""
    from yastack_amd import segments
    npr, nq, _soft, _only = cfg
    enable, method = kni
    extra = [(ethertype_frame(0x0806), 64), (ethertype_frame(0x8035), 64)]
    extra += [(ipv4_frame("10.1.2.3", 5353, "10.3.2.1", dp, proto=17, length=64), 64)
              for dp in UDP_DPORTS]
    if stride < 66:
        extra.append((ipv4_frame("10.9.8.7", 4321, "10.7.8.9", 443, ihl=12, length=100,
                                 total_len=None), 100))
    win, lens, n_tcp = _pool(oracle_mod, npr, stride, n_tcp, extra)
    q, h = oracle_mod.dispatch_windows(win.reshape(-1), stride, lens, oracle_mod.cfg(*cfg))
    f = oracle_mod.filter_windows(win.reshape(-1), stride, lens, enable,
                                  oracle_mod.kni_bitmap(tcp_ports), oracle_mod.kni_bitmap(udp_ports))
    bkt = segments.route_buckets(q, f, nq, queue_id, enable, method == "accept")
    nb = nq + 3
    table = np.full((nb, PER_BUCKET), -1, np.int64)
    for b in range(nb):
        mine = np.nonzero(bkt == b)[0]
        # one packet a flow and filter class: distinct (q, hash, class)
        key = ((h[mine].astype(np.int64) << 24) | ((q[mine].astype(np.int64) & 0xFFFF) << 8) |
               (f[mine].astype(np.int64) & 0xFF))
        mine = mine[np.sort(np.unique(key, return_index=True)[1])]
        special = mine[mine >= n_tcp]
        over = mine[(mine < n_tcp) & (q[mine] >= nq)][:1]
        rest = np.setdiff1d(mine, np.concatenate([special, over]), assume_unique=True)
        mine = np.concatenate([special[:PER_BUCKET - 1], over, rest])
        k = min(mine.size, PER_BUCKET)
        if k:
            table[b] = np.resize(mine[:k], PER_BUCKET)
    return Exemplars(win, lens, q, h, table, nq, stride, fclass=f, queue_id=queue_id)


def choose(pattern, ex: Exemplars) -> np.ndarray:
    """Pool index of every packet of a bucket sequence: among a bucket's
    exemplars by position, so several flows (hashes) share a bucket."""
    pattern = np.asarray(pattern, np.int64)
    pos = np.arange(pattern.size, dtype=np.uint64)
    pick = ((pos * np.uint64(0x9E3779B1)) >> np.uint64(13)) % np.uint64(PER_BUCKET)
    idx = ex.table[pattern, pick.astype(np.int64)]
    if pattern.size and idx.min() < 0:
        raise ValueError(f"pattern uses unreachable bucket(s) "
                         f"{sorted(set(pattern[idx < 0].tolist()))[:8]}")
    return idx


def build(pattern, ex: Exemplars):
    """(win uint8[n * stride], lens uint16[n]) whose oracle buckets are `pattern`."""
    idx = choose(pattern, ex)
    return np.ascontiguousarray(ex.win[idx]).reshape(-1), np.ascontiguousarray(ex.lens[idx])


# ---- bucket sequences --------------------------------------------------------

def all_but_one(n: int, B: int, other: int, pos: int) -> np.ndarray:
    """Every packet in bucket B except one in `other` at `pos`: the worst skew
    that is not the one-list shortcut."""
    p = np.full(n, B, np.int64)
    p[pos] = other
    return p


def runs(n: int, buckets, R: int) -> np.ndarray:
    """The buckets cycle in runs of R packets."""
    b = np.asarray(buckets, np.int64)
    return b[(np.arange(n) // R) % b.size]


def sparse(n: int, keep, seed: int = 1) -> np.ndarray:
    """Only the buckets in `keep` are used, interleaved at random with runs of
    1 to 40; every other bucket is empty over the whole batch."""
    keep = np.asarray(keep, np.int64)
    rng = np.random.default_rng(seed)
    nr = n // 2 + 2
    which = rng.integers(0, keep.size, nr)
    length = rng.integers(1, 41, nr)
    return np.repeat(keep[which], length)[:n] if n else np.zeros(0, np.int64)


def late_and_early(n: int, buckets, span: int, seed: int = 2) -> np.ndarray:
    """buckets[0] only in the first span of the batch, buckets[1] only in the
    last, buckets[2] one packet in the first span and one in the last (its line
    stays carried over the spans between, which bring it nothing), the rest
    spread over buckets[3:].  With fewer buckets the roles are given up from
    the front of that list: 3 buckets keep the carried one, the first-span one
    and the spread; 2 the carried one and the spread."""
    b = list(buckets)
    if len(b) < 2:
        raise ValueError("late_and_early needs two buckets")
    rest = b[3:] if len(b) >= 4 else b[-1:]
    carried = b[2] if len(b) >= 4 else b[1] if len(b) == 3 else b[0]
    first = b[0] if len(b) >= 3 else None
    last = b[1] if len(b) >= 4 else None
    rng = np.random.default_rng(seed)
    p = np.asarray(rest, np.int64)[rng.integers(0, len(rest), n)]
    last0 = (n - 1) // span * span
    if first is not None:
        p[0:min(span, n):2] = first
    if last is not None and last0 > 0:
        p[last0:n:2] = last
    p[min(1, n - 1)] = carried
    p[n - 1] = carried
    return p


def staircase(n: int, buckets, filler: int, span: int) -> np.ndarray:
    """Per span s, the j-th of `buckets` gets (7 j + s) % 33 packets in one
    run, the runs spread over the span, and the rest goes to `filler`: a
    bucket's list phase inside a 64-byte line walks 0-15 from span to span,
    with totals on the multiples of 16 and either side."""
    others = [b for b in buckets if b != filler]
    p = np.full(n, filler, np.int64)
    step = span // max(len(others), 1)
    for s in range(-(-n // span)):
        at = s * span
        for j, b in enumerate(others):
            c = (7 * j + s) % 33
            lo = s * span + j * step if step >= 33 else at
            p[lo:min(lo + c, n, (s + 1) * span)] = b
            at = lo + c
    return p


def zipf(n: int, buckets, seed: int, a: float = 1.3) -> np.ndarray:
    """Seeded heavy-tailed draw: the k-th bucket of a seeded shuffle has weight
    1 / k^a."""
    rng = np.random.default_rng(seed)
    b = rng.permutation(np.asarray(buckets, np.int64))
    w = 1.0 / np.arange(1, b.size + 1) ** a
    return b[rng.choice(b.size, size=n, p=w / w.sum())]


# ---- the list kernels' layout, restated to aim the patterns ------------------

def layout(nb: int, chunk_tiles: int = 0, span_tiles: int = 0):
    """(chunk, span) in packets that a context with nb buckets uses for a batch
    of a few ten thousand packets (yrss.hip layout_for / line_plan): chunks of
    4 tiles up to 16 buckets, 8 up to 128, 16 past that (or chunk_tiles, a
    power of two); line-scatter spans of up to 8192 packets up to 128 buckets
    and 16 384 past that (or span_tiles), as many chunks as keep nb x chunks
    within the prefix table; chunks past the span take the fallback scatter,
    whose span is 32 tiles (or span_tiles) or the chunk if longer.  It only aims
    the patterns: no test asserts it."""
    ct = chunk_tiles or (4 if nb <= 16 else 8 if nb <= 128 else 16)
    ct = 1 << (ct - 1).bit_length()
    chunk = ct * 64
    groups = 4 if nb > 128 else 2
    smax, tmax = 4096 * groups, 512 * (5 if groups == 2 else 9)
    if chunk > smax:
        st = span_tiles or 32
        sh = 0
        while (ct << sh) < st:
            sh += 1
        return chunk, chunk << sh
    target = min(max(span_tiles * 64 if span_tiles else smax, chunk), smax)
    g = 0
    while (chunk << (g + 1)) <= target and (nb << (g + 1)) <= tmax:
        g += 1
    return chunk, chunk << g


def family(name: str, n: int, ex: Exemplars, chunk: int, span: int) -> list:
    """The members of one pattern family for a configuration as (label,
    bucket sequence); buckets the configuration cannot reach are left out of
    the choices (test_qpatterns.py pins which ones those are)."""
    nq, reach, queues = ex.nb_queues, ex.reachable, ex.queues()
    drop = nq if nq in reach else None
    mid = queues[len(queues) // 2]
    out = []
    if ex.route and name in ("all_but_one", "runs", "zipf"):
        return _route_family(name, n, ex, chunk, span)
    if name == "all_but_one":
        big = list(dict.fromkeys([queues[0], mid, queues[-1]] + ([drop] if drop is not None else [])))
        if len(reach) < 2:
            raise ValueError("all_but_one needs two buckets")
        pos = list(dict.fromkeys(p for p in (0, n - 1, (n // 2) // chunk * chunk,
                                              max(n // span, 1) * span - 1) if 0 <= p < n))
        for k, B in enumerate(big):
            others = [b for b in reach if b != B]
            for j, p in enumerate(pos):
                o = others[(k + j) % len(others)]
                out.append((f"B{B}-o{o}@{p}", all_but_one(n, B, o, p)))
    elif name == "runs":
        for R in (1, 15, 16, 17, 63, 64, 65, chunk - 1, chunk, chunk + 1, span - 1, span, span + 1):
            if R >= 1:
                out.append((f"R{R}", runs(n, reach, R)))
    elif name == "sparse":
        sets = [[reach[0], reach[-1]], reach[1::2] or reach[:1],
                [mid] + ([drop] if drop is not None else [queues[0]])]
        for k, keep in enumerate(sets):
            keep = list(dict.fromkeys(keep))
            if len(keep) == 1:       # one bucket only would be the one-list shortcut
                keep = list(dict.fromkeys(keep + [reach[0], reach[-1]]))[:2]
            out.append((f"keep{k}", sparse(n, keep, seed=k + 1)))
        if ex.route and len(ex.own()) >= 2:      # the foreign rings all stay empty
            out.append(("keep-own", sparse(n, ex.own(), seed=4)))
    elif name == "late_and_early":
        # the carried bucket from the middle, the first-/last-span ones from the ends
        if len(reach) >= 4:
            order = [reach[0], reach[-1], mid if mid not in (reach[0], reach[-1]) else reach[1]]
            order += [b for b in reach if b not in order]
        else:
            order = list(reach)
        out.append(("le", late_and_early(n, order, span)))
        out.append(("le-rev", late_and_early(n, order[::-1], span, seed=3)))
    elif name == "staircase":
        out.append((f"fill{mid}", staircase(n, reach, mid, span)))
        out.append((f"fill{reach[-1]}", staircase(n, reach, reach[-1], span)))
    elif name == "zipf":
        for seed in (11, 12):
            out.append((f"s{seed}", zipf(n, reach, seed)))
    else:
        raise ValueError(name)
    return out


ROUTE_RUNS = (1, 15, 16, 17, 63, 64, 65, 255, 256, 257)


def _route_family(name: str, n: int, ex: Exemplars, chunk: int, span: int) -> list:
    """all_but_one, runs and zipf over route classes: the classes the routing
    adds (local, freed, KNI, local ARP: ex.own()) are the subject, and every
    reachable class appears in some member of each family."""
    reach, own, foreign = ex.reachable, ex.own(), ex.foreign()
    out = []
    if name == "all_but_one":
        if len(reach) < 2:
            raise ValueError("all_but_one needs two buckets")
        pos = list(dict.fromkeys(p for p in (0, n - 1, (n // 2) // chunk * chunk,
                                              max(n // span, 1) * span - 1) if 0 <= p < n))
        rings = list(dict.fromkeys([foreign[0], foreign[len(foreign) // 2], foreign[-1]])) \
            if foreign else []
        used = set()
        # the big class is local, KNI, local ARP, freed; the stray a foreign ring
        # (with one queue: another of the lcore's own classes)
        for k, B in enumerate(own):
            strays = rings or [b for b in own if b != B]
            for j, p in enumerate(pos):
                o = strays[(k + j) % len(strays)]
                out.append((f"B{B}-o{o}@{p}", all_but_one(n, B, o, p)))
                used |= {B, o}
        # the roles swapped
        for k, o in enumerate(own):
            for j in range(2 if rings else 0):
                B, p = rings[(k + j) % len(rings)], pos[(k + 2 * j) % len(pos)]
                out.append((f"B{B}-o{o}@{p}", all_but_one(n, B, o, p)))
                used |= {B, o}
        # every ring not met so far strays once into a batch of an own class
        for k, o in enumerate(b for b in reach if b not in used):
            B, p = (own or reach)[k % len(own or reach)], pos[k % len(pos)]
            if B == o:
                B = reach[0] if reach[0] != o else reach[1]
            out.append((f"B{B}-o{o}@{p}", all_but_one(n, B, o, p)))
    elif name == "runs":
        rs = sorted(set(ROUTE_RUNS + (chunk - 1, chunk, chunk + 1, span - 1, span, span + 1)))
        for R in rs:
            if R < 1 or (R > n and R != rs[0]):
                continue
            if len(own) >= 2:
                out.append((f"own-R{R}", runs(n, own, R)))
            out.append((f"all-R{R}", runs(n, reach, R)))
        if len(own) == 1:            # the whole batch in that class
            out.append(("own-all", runs(n, own, n)))
        # a batch shorter than the class list: the rest of the list, R = 1
        for off in range(n, len(reach), n):
            out.append((f"all-R1+{off}", runs(n, reach[off:] + reach[:off], 1)))
    else:
        for seed in (11, 12):
            out.append((f"s{seed}", zipf(n, reach, seed)))
        # one packet of every class planted in a heavy-tailed draw over the own
        # classes (as many members as a short batch needs to hold them all)
        per = max(min(n // 2, len(reach)), 1)
        m = -(-len(reach) // per)
        for k in range(m):
            p = zipf(n, own or reach, 13 + k)
            plant = np.asarray(reach[k::m], np.int64)
            at = np.random.default_rng(13 + k).choice(n, plant.size, replace=False)
            p[at] = plant
            out.append((f"s{13 + k}-every", p))
    return out


FAMILIES = ("all_but_one", "runs", "sparse", "late_and_early", "staircase", "zipf")


def expected_lists(bucket: np.ndarray, nb: int):
    """The lists stated independently of the oracle: a stable sort by bucket
    and the running bucket totals (nb + 1 offsets: the last is n, the end of
    the drop bucket)."""
    qidx = np.argsort(bucket, kind="stable").astype(np.uint32)
    qstart = np.concatenate(([0], np.cumsum(np.bincount(bucket, minlength=nb)))).astype(np.uint32)
    return qidx, qstart


# ---- the cases of tests/test_gpu_qpatterns.py ---------------------------------
# (path, cfg, tuning for SoftRss.set_tuning, n).  n is ragged and three to five
# of the layout's spans at default tuning; the forced small layouts give many
# spans to a workgroup's range at the same n.  test_qpatterns.py realises every
# family for every entry on the CPU.

GLOBAL_CASES = (
    # line scatter with in-scatter prefixes (<= 16 buckets), and the scan kernel
    [("line16", cfg, tune, 33011)
     for cfg in ((8, 8, 1, 0), (16, 15, 1, 0), (3, 3, 1, 1), (5, 2, 0, 1))
     for tune in ({}, {"scan_kernel": 1}, {"chunk_tiles": 1, "span_tiles": 1},
                  {"chunk_tiles": 1, "span_tiles": 64})] +
    # line scatter kG = 2: the bucket packed beside the rank at default chunks
    # ((128, 127, 1, 1): 128 buckets, the rank word reaches 0xFFFF)
    [("line_kg2", cfg, tune, 41003)
     for cfg in ((64, 64, 1, 0), (128, 127, 1, 1))
     for tune in ({}, {"chunk_tiles": 16, "span_tiles": 64})] +
    # line scatter kG = 4: the rank beside q
    [("line_kg4", cfg, tune, 57351)
     for cfg in ((255, 255, 1, 0), (4096, 256, 1, 1))
     for tune in ({}, {"scatter_xcd": 0}, {"scatter_xcd": 1})] +
    # fallback scatter: a chunk past the line scatter's span
    [("fallback", (5, 5, 1, 1), {"chunk_tiles": 256, "span_tiles": 256}, 40009)]
)

SEG_CASES = [(cfg, blocks, n)
             for cfg in ((15, 15, 1, 0), (8, 8, 1, 0), (1, 1, 1, 0), (5, 2, 0, 1))
             for blocks in (0, 1)
             for n in (256, 257, 4097, 20000)]
SEG_AIM = (256, 1024)      # a segment; the four segments of a parse wave's 16 tiles

HOST_CFGS = ((5, 4, 1, 1), (63, 63, 1, 0))
HOST_SIZES = (64, 1024, 4096, 4097)
WORKER_SIZES = (32, 1024)      # F-Stack's burst (ff_dpdk_if.c:83) and YRSS_WORKER_MAX_BURST
HOST_STRIDE = 80               # the host paths stage full windows: nothing truncates


def aim_of(nb: int, tune: dict):
    return layout(nb, tune.get("chunk_tiles", 0), tune.get("span_tiles", 0))


def host_aim(nb: int, n: int):
    """One-launch kernels rank per 64-packet tile; past 4096 packets the batch
    kernels' layout applies."""
    return layout(nb) if n > 4096 else (64, 1024)


def tune_id(tune: dict) -> str:
    return "-".join(f"{k}{v}" for k, v in tune.items()) or "default"


# ---- the cases of tests/test_gpu_qpatterns_route.py -------------------------------
# A route case is (cfg, queue_id, kni mode of route_helpers.KNI_MODES, stride);
# the KNI port lists are route_helpers.TCP_PORTS / UDP_PORTS.
# tests/test_qpatterns_route.py realises every family for every entry on the
# CPU and pins each case's reachable classes.

ROUTE_SEG_KINDS = tuple(
    [((13, 13, 1, 0), qid, kni, 64) for qid, kni in ((0, "accept"), (2, "reject"), (13, "off"))] +
    [((6, 4, 1, 0), qid, kni, 64) for qid, kni in ((0, "accept"), (2, "reject"))] +
    [((3, 3, 1, 1), qid, kni, 64) for qid, kni in ((0, "accept"), (2, "off"))] +
    [((1, 1, 1, 0), 0, "reject", 64)] +
    [((13, 13, 1, 0), 0, "reject", 80)]           # full windows: nothing truncates
)
ROUTE_SEG_SIZES = (256, 257, 4097, 20000)
ROUTE_SEG_BLOCKS = (0, 1)

# one-launch bursts: 6, 16, 17 (one more ballot bit in peer_mask) and 64 route
# classes (all six ballot bits; class 63 is local ARP).  nb_procs > nb_queues
# where the freed class is to be reachable: the host paths stage what the frames
# hold, so nothing truncates
ROUTE_BURST_KINDS = (
    ((5, 3, 1, 1), 0, "accept", 80), ((5, 3, 1, 0), 2, "reject", 80),
    ((13, 13, 1, 0), 0, "reject", 80), ((16, 13, 1, 0), 2, "accept", 80),
    ((14, 14, 1, 0), 0, "accept", 80), ((17, 14, 1, 0), 2, "reject", 80),
    ((64, 61, 1, 0), 0, "accept", 80), ((61, 61, 1, 0), 2, "reject", 80),
    ((64, 61, 1, 0), 61, "off", 80), ((64, 61, 1, 0), 0, "reject", 80),
)
ROUTE_BURST_SIZES = (64, 1024, 4096)
ROUTE_BURST_AIM = (64, 1024)

ROUTE_WORKER_KINDS = (
    ((5, 3, 1, 0), 0, "accept", 80), ((5, 3, 1, 1), 2, "reject", 80),
    ((64, 61, 1, 0), 0, "reject", 80), ((64, 61, 1, 0), 2, "accept", 80),
)


def route_kind_id(kind) -> str:
    cfg, queue_id, kni, stride = kind
    return f"{'x'.join(map(str, cfg))}-q{queue_id}-{kni}-s{stride}"


def route_aims():
    """Every (kind, n, chunk, span) some routed GPU case builds patterns for."""
    seen = {}
    for kind in ROUTE_SEG_KINDS:
        for n in ROUTE_SEG_SIZES:
            seen[(kind, n) + SEG_AIM] = None
    for kind in ROUTE_BURST_KINDS:
        for n in ROUTE_BURST_SIZES:
            seen[(kind, n) + ROUTE_BURST_AIM] = None
    for kind in ROUTE_WORKER_KINDS:
        for n in WORKER_SIZES:
            seen[(kind, n) + ROUTE_BURST_AIM] = None
    return list(seen)


_ROUTE_EX = {}


def route_ex_for(oracle_mod, kind) -> Exemplars:
    """route_exemplars of a route case, computed once."""
    import route_helpers as rh
    if kind not in _ROUTE_EX:
        cfg, queue_id, kni, stride = kind
        _ROUTE_EX[kind] = route_exemplars(oracle_mod, cfg, queue_id, rh.KNI_MODES[kni],
                                          rh.TCP_PORTS, rh.UDP_PORTS, stride)
    return _ROUTE_EX[kind]


def route_oracle(oracle_mod, kind, win, lens, stride=None):
    """The oracle's (q, hash, filter class) of built windows under a route case."""
    import route_helpers as rh
    cfg, _queue_id, kni, kstride = kind
    stride = stride or kstride
    q, h = oracle_mod.dispatch_windows(win, stride, lens, oracle_mod.cfg(*cfg))
    f = oracle_mod.filter_windows(win, stride, lens, rh.KNI_MODES[kni][0],
                                  oracle_mod.kni_bitmap(rh.TCP_PORTS),
                                  oracle_mod.kni_bitmap(rh.UDP_PORTS))
    return q, h, f


def route_members(ex: Exemplars, n: int, chunk: int, span: int):
    """Every member of every family as (name, class sequence)."""
    for fam in FAMILIES:
        for label, pat in family(fam, n, ex, chunk, span):
            yield f"{fam}/{label}", pat
