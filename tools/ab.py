#!/usr/bin/env python3
"""Alternating A/B runs in ONE process on one GPU.  Every leg of a round gets
its own context (and, for device batches, fresh buffers behind a random
spacer); the legs run in shuffled order round after round, so box drift and
buffer placement (worth up to ~5 % of the parse kernel for one and the same
build) hit all legs alike.  Per leg and metric: median [min-max] over the
rounds; per non-base leg the difference of the medians beside the base leg's
own max - min over its repeats.  The base is the first leg given.

    python tools/ab.py dev --legs LEG,LEG,... [--profiles udp4,imix] [--nb-procs 3,64]
        [--rounds 7] [--steps 20] [--kni] [--ignore-faults] [--json out.json]
    python tools/ab.py worker [--legs plain=cur:plain,route=cur:route] [--sizes 32,1024]
        [--rounds 7] [--bursts 3000] [--depth 4] [--json out.json]

A leg is [name=]lib[@k=v;k=v][:form].  lib: cur, test (libyrss_test.so) or a
path, relative to the repository root or absolute (tools/build_ab_lib.sh).
k=v: yrss_set_tuning fields, side=1 (the batches on a non-default stream),
ext=N (yrss_set_extended flags: 1 VLAN, 2 IPv6, 4 UDP), reta=SIZE (yrss_set_reta: an
equal-weights table of SIZE entries over the context's queues), dbg_groups /
dbg_merge (the test library's hooks); dev legs only.  form, dev:
global (default), seg, seg-filter, route; worker: plain (default), route.
A worker leg takes two keys of its own: ext=N starts the worker with
YRSS_WORKER_F_EXTENDED under flags N (ext=0: that worker with the flags off;
no ext: yrss_worker_start[_route], all an older library has), prof=N takes the
frames from synthetic profile N (abi.SYN_*: 1 udp4, 3 vlan6_tcp, 5 tcp4; default
6, the fuzz stream).

dev times --steps back-to-back batches by wall clock (step, ms, no events) and,
in a separate block, the form's kernels by events (us; a kernel the
configuration never launches, as the scan kernel where the line scatter scans
in its prologue, has no sample: the former tools printed 0).  worker submits
--bursts bursts in frames form with --depth in flight (submit, then poll the
oldest) through the C ABI, ctypes overhead included for all legs alike.

The tools this one replaces:
    ab_inproc.py --libs cur,ab/lib/x.so    dev --legs cur,ab/lib/x.so
    ab_seg.py --parent P                   dev --legs parent-global=P,new-global=cur,new-seg=cur:seg
    ab_route_seg.py                        dev --legs seg-filter=cur:seg-filter,route=cur:route
    rocprofv3 --kernel-trace --stats ... -- python tools/ab.py dev --legs cur:seg \
        --rounds 1 --steps 5 --profiles udp4
"""
from __future__ import annotations

import argparse
import ctypes
import json
import random
import statistics
import sys
import time
from collections import namedtuple
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from yastack_amd import SoftRss, abi  # noqa: E402
from yastack_amd.dispatch import reta_weighted  # noqa: E402

Leg = namedtuple("Leg", "name lib tune form")

PROFILES = {"udp4": abi.SYN_UDP4, "tcp4": abi.SYN_TCP4, "imix": abi.SYN_IMIX,
            "jumbo_tcp4": abi.SYN_JUMBO_TCP4, "vlan6_tcp": abi.SYN_VLAN6_TCP}
KERNELS = {"parse": abi.K_PARSE_HASH, "scan": abi.K_SCAN, "scatter": abi.K_SCATTER}
# dev form: (call, allocator, want_filter, kernels timed, needs KNI)
DEV_FORMS = {
    "global": ("dispatch_dev", "alloc_out", False, ("parse", "scan", "scatter"), False),
    "seg": ("dispatch_dev_seg", "alloc_seg_out", False, ("parse",), False),
    "seg-filter": ("dispatch_dev_seg", "alloc_seg_out", True, ("parse",), True),
    "route": ("route_dev_seg", "alloc_route_out", True, ("parse",), True),
}
WORKER_FORMS = ("plain", "route")
KNI = (True, "accept", "80,443,8000-8080", "53")
UNITS = {"step": ("ms", ".4f"), "us_burst": ("us", ".2f")}   # every other metric: us, .2f


# ---- harness: rounds, order, statistics, output ----------------------------

def parse_legs(text, forms):
    """--legs text -> [Leg]; forms[0] is the default form."""
    legs = []
    for s in filter(None, text.split(",")):
        head, sep, form = s.rpartition(":")
        head, form = (head, form) if sep else (s, forms[0])
        head, _, tune = head.partition("@")
        name, sep, lib = head.partition("=")
        name, lib = (name, lib) if sep else (s, head)
        if form not in forms:
            raise argparse.ArgumentTypeError(f"{s}: form {form!r} is not one of {', '.join(forms)}")
        if not lib or name in [x.name for x in legs]:
            raise argparse.ArgumentTypeError(f"{s}: no library, or the name {name!r} twice")
        try:
            tune = {k: int(v) for k, v in (kv.split("=") for kv in tune.split(";") if kv)}
        except ValueError:
            raise argparse.ArgumentTypeError(f"{s}: tuning is k=v;k=v with integer v") from None
        legs.append(Leg(name, lib, tune, form))
    if not legs:
        raise argparse.ArgumentTypeError("no leg given")
    return legs


def lib_path(lib):
    if lib == "cur":
        return None
    return str(abi.TEST_LIB_PATH) if lib == "test" else str(ROOT / lib)   # ROOT / absolute: absolute


def alternate(legs, rounds, seed, run_leg, tag=""):
    """rounds rounds of every leg in an order shuffled anew each round from
    random.Random(seed) (or from the generator given as seed, which a second
    call then continues); run_leg(leg, rng) returns {metric: value}.
    Returns {leg name: {metric: [one value per round]}}."""
    rng = seed if isinstance(seed, random.Random) else random.Random(seed)
    res = {leg.name: {} for leg in legs}
    for r in range(rounds):
        order = list(range(len(legs)))
        rng.shuffle(order)
        for i in order:
            for metric, v in run_leg(legs[i], rng).items():
                res[legs[i].name].setdefault(metric, []).append(v)
        print(f"{tag} round {r + 1} done".lstrip(), flush=True)
    return res


def verdict(v, base):
    """(median(v) - median(base), base's max - min, inside|outside)."""
    d, spread = statistics.median(v) - statistics.median(base), max(base) - min(base)
    return d, spread, "inside" if abs(d) <= spread else "outside"


def report(res, base, metrics, label="", rate=None):
    """Per leg: median [min-max] of every metric it has, and rate = (metric,
    numerator, unit) as numerator / median.  Per non-base leg and metric it
    shares with the base leg: verdict() in words."""
    for name, v in res.items():
        line = f"{label} {name:14s}"
        for m in (m for m in metrics if m in v):
            unit, f = UNITS.get(m, ("us", ".2f"))
            line += (f"  {m} {unit} median {statistics.median(v[m]):{f}} "
                     f"[{min(v[m]):{f}}-{max(v[m]):{f}}]")
        if rate:
            line += f"  {rate[1] / statistics.median(v[rate[0]]):7.2f} {rate[2]}"
        print(line)
    for name, v in res.items():
        for m in (m for m in metrics if name != base and m in v and m in res[base]):
            unit, f = UNITS.get(m, ("us", ".2f"))
            d, spread, word = verdict(v[m], res[base][m])
            print(f"{label} {name} - {base}, {m}: {d:+{f}} {unit} ({base} spread over its "
                  f"repeats: {spread:{f}} {unit}): {word} that spread")


def write_json(path, out):
    if path:
        Path(path).parent.mkdir(parents=True, exist_ok=True)
        Path(path).write_text(json.dumps(out, indent=1))


# ---- device-batch legs -------------------------------------------------------

def run_dev_leg(leg, rng, args, npr, profile):
    import torch

    call, alloc, want_filter, kernels, needs_kni = DEV_FORMS[leg.form]
    n, stride = args.pkts, 64
    # fresh buffers behind a random spacer each time: parse time moves by up to
    # ~5 % with where the buffers land (same build, same process), so every
    # leg sees many placements
    spacer = torch.empty(rng.randrange(0, 64) << 21, dtype=torch.uint8, device="cuda")
    e = SoftRss(npr, npr, 1, 1, device=0, max_burst=0, lib_path=lib_path(leg.lib))
    tn = dict(leg.tune)
    # side=1: the caller's work on a non-default (non-blocking) stream
    st = torch.cuda.Stream() if tn.pop("side", 0) else None
    grp = tn.pop("dbg_groups", 0)
    ext = tn.pop("ext", 0)
    if ext:
        e.set_extended(vlan=bool(ext & 1), ipv6=bool(ext & 2), udp=bool(ext & 4))
    reta = tn.pop("reta", 0)
    if reta:
        e.set_reta(reta_weighted([1] * npr, reta))
    if tn.pop("dbg_merge", 0):
        assert e._lib.yrss_debug_partial_merge(e._ctx, 1) == 0
    if grp:
        assert e._lib.yrss_debug_line_groups(e._ctx, grp, 0) == 0
    if tn:
        e.set_tuning(**tn)
    if needs_kni or args.kni:
        e.set_kni(*KNI)
    wins = [e.synth(PROFILES[profile], n, k * n, stride=stride) for k in range(args.batches)]
    kw = {"want_filter": True} if want_filter else {}
    outs = [getattr(e, alloc)(n, wins[0][0].device, **kw) for _ in range(args.batches)]
    pre = (stride, args.queue_id) if leg.form == "route" else (stride,)
    torch.cuda.synchronize()

    def run(steps, it=[0]):
        for _ in range(steps):
            k = it[0] % args.batches
            it[0] += 1
            getattr(e, call)(wins[k][0], wins[k][1], *pre, n, out=outs[k], stream=st)

    run(4)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(args.steps)
    torch.cuda.synchronize()
    got = {"step": (time.perf_counter() - t0) / args.steps * 1e3}
    e.timing_enable(sum(1 << KERNELS[k] for k in kernels))
    run(args.steps)
    torch.cuda.synchronize()
    for k in kernels:
        ms, cnt = e.timing_read(KERNELS[k])
        if cnt:   # never launched (the scan, where the line scatter does it): no sample, not 0
            got[k] = ms / cnt * 1e3
    e.timing_enable(0)
    if e.status() != 0 and not args.ignore_faults:
        raise RuntimeError(f"{leg.name}: device fault {e.fault_info()}")
    e.close()
    del wins, outs, spacer
    torch.cuda.empty_cache()
    return got


def main_dev(args):
    rng = random.Random(args.seed)   # one generator over all profiles and bucket counts
    out = {}
    for npr in args.nb_procs:
        for pname in args.profiles:
            res = alternate(args.legs, args.rounds, rng,
                            lambda leg, rng: run_dev_leg(leg, rng, args, npr, pname), pname)
            out[pname if len(args.nb_procs) == 1 else f"{pname}.q{npr}"] = res
            report(res, args.legs[0].name, ("step", *KERNELS), f"{pname:5s} q{npr}",
                   ("step", args.pkts / 1e6, "Gpkt/s"))
    write_json(args.json, out)


# ---- worker legs -------------------------------------------------------------

def make_pool(n, profile=abi.SYN_FUZZ):
    """n synthetic frames (SYN_FUZZ: TCP, UDP, ARP, IPIP) at 2048-byte pitch
    in page-aligned memory: (memory, data pointers, data_len)."""
    import numpy as np

    from oracle import oracle

    win, lens = oracle.synth(profile, n, 7, stride=80)
    lens = np.minimum(lens, 1500).astype(np.uint16)
    raw = np.zeros(n * 2048 + 8192, np.uint8)
    mem = raw[(-raw.ctypes.data) % 4096:][:n * 2048]
    mem.reshape(n, 2048)[:, :80] = win.reshape(n, 80)
    data = (mem.ctypes.data + 2048 * np.arange(n, dtype=np.uint64)).astype(np.uint64)
    return mem, data, lens


def run_worker_leg(leg, args, burst, mem, data, lens):
    import numpy as np

    npr = args.nb_procs
    ext = leg.tune.get("ext")
    with SoftRss(npr, npr, 1, 1, device=0, max_burst=0, lib_path=lib_path(leg.lib)) as e:
        e.set_kni(*KNI)
        e.register_host_memory(mem.ctypes.data, mem.nbytes)
        if ext:
            e.set_extended(vlan=bool(ext & 1), ipv6=bool(ext & 2), udp=bool(ext & 4))
        e.worker_start(args.nslots, args.nblocks,
                       route_queue_id=args.queue_id if leg.form == "route" else None,
                       **({} if ext is None else {"extended": True}))
        lib, ctx = e._lib, e._ctx
        nslot = args.nslots
        outs = [(np.empty(burst, np.int16), np.empty(burst, np.uint32),
                 np.empty(burst, np.uint32), np.empty(npr + 4, np.uint32)) for _ in range(nslot)]
        span = data.size - burst
        t = ctypes.c_uint64()

        def loop(count):
            pending = []
            for k in range(count):
                lo = (k * 977) % span
                q, h, qi, qs = outs[k % nslot]
                rc = lib.yrss_worker_submit_frames(ctx, data[lo:].ctypes.data,
                                                   lens[lo:].ctypes.data, burst, q.ctypes.data,
                                                   h.ctypes.data, qi.ctypes.data, qs.ctypes.data,
                                                   ctypes.byref(t))
                if rc:
                    raise RuntimeError(f"submit: {rc}")
                pending.append(t.value)
                if len(pending) >= args.depth:
                    rc = lib.yrss_worker_poll(ctx, pending.pop(0), 1)
                    if rc:
                        raise RuntimeError(f"poll: {rc}")
            for tk in pending:
                rc = lib.yrss_worker_poll(ctx, tk, 1)
                if rc:
                    raise RuntimeError(f"poll: {rc}")

        loop(200)
        t0 = time.perf_counter()
        loop(args.bursts)
        dt = time.perf_counter() - t0
        e.worker_stop()
        e.unregister_host_memory(mem.ctypes.data)
        if e.status() != 0:
            raise RuntimeError(f"{leg.name}: device fault")
    return {"us_burst": dt / args.bursts * 1e6}


def main_worker(args):
    rng = random.Random(args.seed)
    pools = {p: make_pool(8192, p)
             for p in {leg.tune.get("prof", abi.SYN_FUZZ) for leg in args.legs}}
    out = {}
    for burst in args.sizes:
        res = alternate(args.legs, args.rounds, rng,
                        lambda leg, rng: run_worker_leg(
                            leg, args, burst, *pools[leg.tune.get("prof", abi.SYN_FUZZ)]),
                        f"burst {burst}")
        out[str(burst)] = res
        report(res, args.legs[0].name, ("us_burst",), f"burst {burst:4d}",
               ("us_burst", burst, "Mpkt/s"))
    write_json(args.json, out)


# ---- command line ------------------------------------------------------------

def ints(text):
    return [int(x) for x in text.split(",")]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    dev = sub.add_parser("dev", help="device batches: library builds, tuning, list forms")
    dev.set_defaults(run=main_dev)
    dev.add_argument("--legs", type=lambda s: parse_legs(s, tuple(DEV_FORMS)), default="cur")
    dev.add_argument("--nb-procs", type=ints, default="3")
    dev.add_argument("--profiles", type=lambda s: s.split(","), default="udp4,imix")
    dev.add_argument("--steps", type=int, default=20)
    dev.add_argument("--pkts", type=int, default=1 << 24)
    dev.add_argument("--batches", type=int, default=4)
    dev.add_argument("--kni", action="store_true", help="KNI on in every leg (the filter "
                     "forms turn it on themselves: method accept)")
    dev.add_argument("--ignore-faults", action="store_true",
                     help="measurement builds whose lists are wrong by design (a guard fires)")
    wrk = sub.add_parser("worker", help="the persistent worker, plain or in route mode")
    wrk.set_defaults(run=main_worker)
    wrk.add_argument("--legs", type=lambda s: parse_legs(s, WORKER_FORMS),
                     default="plain=cur:plain,route=cur:route")
    wrk.add_argument("--nb-procs", type=int, default=3)
    wrk.add_argument("--bursts", type=int, default=3000)
    wrk.add_argument("--depth", type=int, default=4)
    wrk.add_argument("--nslots", type=int, default=8)
    wrk.add_argument("--nblocks", type=int, default=2)
    wrk.add_argument("--sizes", type=ints, default="32,1024")
    for p in (dev, wrk):
        p.add_argument("--queue-id", type=int, default=2, help="of the route legs")
        p.add_argument("--rounds", type=int, default=7)
        p.add_argument("--seed", type=int, default=1)
        p.add_argument("--json", default="")
    args = ap.parse_args(argv)
    if args.cmd == "dev" and [p for p in args.profiles if p not in PROFILES]:
        ap.error(f"--profiles: one of {', '.join(PROFILES)}")
    if args.cmd == "worker" and [leg for leg in args.legs if set(leg.tune) - {"ext", "prof"}]:
        ap.error("--legs: a worker leg takes no tuning (its own keys: ext=N, prof=N)")
    if args.cmd == "worker" and [leg for leg in args.legs
                                 if not 0 <= leg.tune.get("prof", 0) <= abi.SYN_FUZZ
                                 or not 0 <= leg.tune.get("ext", 0) <= abi.EXT_ALL]:
        ap.error("--legs: prof is an abi.SYN_* profile, ext a set of abi.EXT_* flags")
    try:
        args.run(args)
    except RuntimeError as err:   # a device fault or a failed submit: nothing more runs
        print(err)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
