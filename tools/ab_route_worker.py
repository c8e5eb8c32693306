#!/usr/bin/env python3
"""The persistent worker in route mode (yrss_worker_start_route) against the
plain worker (yrss_worker_start), in ONE process on one GPU: frames form,
bursts of 32 and 1024 packets, the legs interleaved in shuffled order round
after round, each leg of a round on its own context and worker.  A leg submits
--bursts bursts with --depth in flight (submit, then poll the oldest) through
the C ABI; the time is the wall clock over the whole loop, ctypes call
overhead included for both legs alike.  Per leg: median [min-max] over the
rounds of the burst time and the packet rate.  The plain leg's own max - min
over its repeats is the yardstick for the difference.

    python tools/ab_route_worker.py [--rounds 7] [--bursts 3000] [--depth 4]
        [--nb-procs 3] [--queue-id 2] [--json out.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

from oracle import oracle  # noqa: E402
from yastack_amd import SoftRss, abi  # noqa: E402

LEGS = ("plain", "route")


def make_pool(n):
    """n synthetic frames (SYN_FUZZ: TCP, UDP, ARP, IPIP) at 2048-byte pitch
    in page-aligned memory: (memory, data pointers, data_len)."""
    win, lens = oracle.synth(abi.SYN_FUZZ, n, 7, stride=80)
    lens = np.minimum(lens, 1500).astype(np.uint16)
    raw = np.zeros(n * 2048 + 8192, np.uint8)
    mem = raw[(-raw.ctypes.data) % 4096:][:n * 2048]
    mem.reshape(n, 2048)[:, :80] = win.reshape(n, 80)
    data = (mem.ctypes.data + 2048 * np.arange(n, dtype=np.uint64)).astype(np.uint64)
    return mem, data, lens


def run_leg(name, args, burst, mem, data, lens):
    npr = args.nb_procs
    with SoftRss(npr, npr, 1, 1, device=0, max_burst=0) as e:
        e.set_kni(True, "accept", "80,443,8000-8080", "53")
        e.register_host_memory(mem.ctypes.data, mem.nbytes)
        e.worker_start(args.nslots, args.nblocks,
                       route_queue_id=args.queue_id if name == "route" else None)
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
            raise RuntimeError(f"{name}: device fault")
    return dt / args.bursts * 1e6


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--bursts", type=int, default=3000)
    ap.add_argument("--depth", type=int, default=4)
    ap.add_argument("--nslots", type=int, default=8)
    ap.add_argument("--nblocks", type=int, default=2)
    ap.add_argument("--nb-procs", type=int, default=3)
    ap.add_argument("--queue-id", type=int, default=2)
    ap.add_argument("--sizes", default="32,1024")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    rng = random.Random(args.seed)
    mem, data, lens = make_pool(8192)
    report = {}
    for burst in (int(s) for s in args.sizes.split(",")):
        res = {name: [] for name in LEGS}
        for r in range(args.rounds):
            order = list(LEGS)
            rng.shuffle(order)
            for name in order:
                res[name].append(run_leg(name, args, burst, mem, data, lens))
            print(f"burst {burst} round {r + 1} done", flush=True)
        report[str(burst)] = res
        for name in LEGS:
            v = res[name]
            med = statistics.median(v)
            print(f"burst {burst:4d} {name:5s} us/burst median {med:8.2f} [{min(v):.2f}-{max(v):.2f}]"
                  f"  {burst / med:7.2f} Mpkt/s")
        d = statistics.median(res["route"]) - statistics.median(res["plain"])
        spread = max(res["plain"]) - min(res["plain"])
        inside = "inside" if abs(d) <= spread else "outside"
        print(f"burst {burst:4d} route - plain: {d:+.2f} us/burst (plain spread over its repeats: "
              f"{spread:.2f} us): {inside} that spread")
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(report, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
