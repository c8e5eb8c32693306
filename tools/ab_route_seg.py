#!/usr/bin/env python3
"""Routed segmented lists (yrss_route_dev_seg) against the segmented lists with
the filter output on (yrss_dispatch_dev_seg, the kCount == 3 filter variant it
differs from by the bucket function alone), in ONE process on one GPU, in the
manner of tools/ab_seg.py: every leg gets its own context and fresh buffers
behind a random spacer, the legs alternate in shuffled order round after round.
Legs: "seg-filter" and "route" (queue_id --queue-id, KNI on, method accept).
Per leg: median, min and max over the rounds of the step time (wall clock over
--steps back-to-back batches, no events) and, in a separate block, of the parse
kernel's event time.  The seg-filter leg's own max - min over its repeats is
the yardstick for the difference.

    python tools/ab_route_seg.py [--profiles imix,udp4] [--nb-procs 3] [--rounds 7]
        [--steps 20] [--json out.json]
"""
from __future__ import annotations

import argparse
import json
import random
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from yastack_amd import SoftRss, abi  # noqa: E402

PROFILES = {"udp4": abi.SYN_UDP4, "tcp4": abi.SYN_TCP4, "imix": abi.SYN_IMIX}
LEGS = ("seg-filter", "route")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--profiles", default="imix,udp4")
    ap.add_argument("--nb-procs", type=int, default=3)
    ap.add_argument("--queue-id", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pkts", type=int, default=1 << 24)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    n, stride, npr = args.pkts, 64, args.nb_procs
    legs = [leg for leg in LEGS if leg in args.legs.split(",")]
    if not legs:
        ap.error("no leg selected")
    rng = random.Random(args.seed)
    report = {}
    for pname in args.profiles.split(","):
        res = {name: {"step": [], "parse": []} for name in legs}
        for r in range(args.rounds):
            order = list(legs)
            rng.shuffle(order)
            for name in order:
                route = name == "route"
                spacer = torch.empty(rng.randrange(0, 64) << 21, dtype=torch.uint8, device="cuda")
                e = SoftRss(npr, npr, 1, 1, device=0, max_burst=0)
                e.set_kni(True, "accept", "80,443,8000-8080", "53")
                wins = [e.synth(PROFILES[pname], n, k * n, stride=stride)
                        for k in range(args.batches)]
                dev = wins[0][0].device
                outs = [e.alloc_route_out(n, dev, want_filter=True) if route
                        else e.alloc_seg_out(n, dev, want_filter=True)
                        for _ in range(args.batches)]
                torch.cuda.synchronize()

                def run(steps, it=[0]):
                    for _ in range(steps):
                        k = it[0] % args.batches
                        it[0] += 1
                        if route:
                            e.route_dev_seg(wins[k][0], wins[k][1], stride, args.queue_id, n,
                                            out=outs[k])
                        else:
                            e.dispatch_dev_seg(wins[k][0], wins[k][1], stride, n, out=outs[k])

                run(4)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(args.steps)
                torch.cuda.synchronize()
                res[name]["step"].append((time.perf_counter() - t0) / args.steps * 1e3)
                e.timing_enable(1 << abi.K_PARSE_HASH)
                run(args.steps)
                torch.cuda.synchronize()
                ms, cnt = e.timing_read(abi.K_PARSE_HASH)
                res[name]["parse"].append(ms / max(cnt, 1) * 1e3)
                e.timing_enable(0)
                if e.status() != 0:
                    print(f"{name}: device fault {e.fault_info()}")
                    return 1
                e.close()
                del wins, outs, spacer
                torch.cuda.empty_cache()
            print(f"{pname} round {r + 1} done", flush=True)
        report[pname] = res
        for name in legs:
            v = res[name]
            med = {k: statistics.median(x) for k, x in v.items()}
            print(f"{pname:5s} q{npr} {name:10s} step ms median {med['step']:.4f} "
                  f"[{min(v['step']):.4f}-{max(v['step']):.4f}]  "
                  f"{n / med['step'] / 1e6:6.2f} Gpkt/s  parse us {med['parse']:6.1f} "
                  f"[{min(v['parse']):.1f}-{max(v['parse']):.1f}]")
        if len(legs) == 2:
            base = res["seg-filter"]
            for key in ("step", "parse"):
                scale = 1e3 if key == "step" else 1.0
                d = (statistics.median(res["route"][key]) - statistics.median(base[key])) * scale
                spread = (max(base[key]) - min(base[key])) * scale
                print(f"{pname:5s} q{npr} route - seg-filter, {key}: {d:+7.2f} us "
                      f"(seg-filter spread over its repeats: {spread:.2f} us)")
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(report, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
