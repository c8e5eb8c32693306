#!/usr/bin/env python3
"""Segmented lists (yrss_dispatch_dev_seg) against the global lists
(yrss_dispatch_dev) of this build and of the parent commit's build, in ONE
process on one GPU, in the manner of tools/ab_inproc.py: every leg gets its own
context and fresh buffers behind a random spacer, the legs alternate in
shuffled order round after round, so box drift and buffer placement hit all
legs alike.  Legs: "parent-global" (the parent library), "new-global" and
"new-seg" (the in-tree library).  Per leg: median, min and max over the rounds
of the step time (wall clock over --steps back-to-back batches, no events),
and of the kernels' event times (a separate block).  The spread of the
parent-global leg over its own repeats is the yardstick for both comparisons.

    YRSS_AB_SRC=<parent checkout> tools/build_ab_lib.sh parent
    python tools/ab_seg.py --parent ab/lib/libyrss_parent.so \
        [--profiles udp4,imix] [--nb-procs 3] [--rounds 7] [--steps 20] [--json out.json]
    rocprofv3 --kernel-trace --stats ... -- python tools/ab_seg.py --legs new-seg \
        --rounds 1 --steps 5 --profiles udp4
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
KERNELS = (("parse", abi.K_PARSE_HASH), ("scan", abi.K_SCAN), ("scatter", abi.K_SCATTER))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default="", help="the parent commit's libyrss build")
    ap.add_argument("--legs", default="parent-global,new-global,new-seg",
                    help="subset of the legs (a single leg: a short run to profile)")
    ap.add_argument("--profiles", default="udp4,imix")
    ap.add_argument("--nb-procs", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pkts", type=int, default=1 << 24)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    n, stride, npr = args.pkts, 64, args.nb_procs
    parent = str((ROOT / args.parent) if not Path(args.parent).is_absolute() else args.parent)
    legs = [leg for leg in (("parent-global", parent, False), ("new-global", None, False),
                            ("new-seg", None, True)) if leg[0] in args.legs.split(",")]
    if not legs or (legs[0][0] == "parent-global" and not args.parent):
        ap.error("no leg selected, or the parent-global leg without --parent")
    rng = random.Random(args.seed)
    report = {}
    for pname in args.profiles.split(","):
        res = {name: {"step": [], "parse": [], "scan": [], "scatter": []} for name, _, _ in legs}
        for r in range(args.rounds):
            order = list(range(len(legs)))
            rng.shuffle(order)
            for i in order:
                name, path, seg = legs[i]
                spacer = torch.empty(rng.randrange(0, 64) << 21, dtype=torch.uint8, device="cuda")
                e = SoftRss(npr, npr, 1, 1, device=0, max_burst=0, lib_path=path)
                wins = [e.synth(PROFILES[pname], n, k * n, stride=stride)
                        for k in range(args.batches)]
                dev = wins[0][0].device
                outs = [e.alloc_seg_out(n, dev) if seg else e.alloc_out(n, dev)
                        for _ in range(args.batches)]
                torch.cuda.synchronize()

                def run(steps, it=[0]):
                    for _ in range(steps):
                        k = it[0] % args.batches
                        it[0] += 1
                        if seg:
                            e.dispatch_dev_seg(wins[k][0], wins[k][1], stride, n, out=outs[k])
                        else:
                            e.dispatch_dev(wins[k][0], wins[k][1], stride, n, out=outs[k])

                run(4)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                run(args.steps)
                torch.cuda.synchronize()
                res[name]["step"].append((time.perf_counter() - t0) / args.steps * 1e3)
                e.timing_enable(sum(1 << k for _, k in KERNELS))
                run(args.steps)
                torch.cuda.synchronize()
                for kname, k in KERNELS:
                    ms, cnt = e.timing_read(k)
                    res[name][kname].append(ms / max(cnt, 1) * 1e3)
                e.timing_enable(0)
                if e.status() != 0:
                    print(f"{name}: device fault {e.fault_info()}")
                    return 1
                e.close()
                del wins, outs, spacer
                torch.cuda.empty_cache()
            print(f"{pname} round {r + 1} done", flush=True)
        report[pname] = res
        base = res.get("parent-global", res[legs[0][0]])["step"]
        spread = max(base) - min(base)
        for name, _, _ in legs:
            v = res[name]
            med = {k: statistics.median(x) for k, x in v.items()}
            print(f"{pname:5s} q{npr} {name:14s} step ms median {med['step']:.4f} "
                  f"[{min(v['step']):.4f}-{max(v['step']):.4f}]  "
                  f"{n / med['step'] / 1e6:6.2f} Gpkt/s  parse us {med['parse']:6.1f} "
                  f"[{min(v['parse']):.1f}-{max(v['parse']):.1f}]  scan {med['scan']:5.2f}  "
                  f"scatter {med['scatter']:6.2f} [{min(v['scatter']):.2f}-{max(v['scatter']):.2f}]")
        mb = statistics.median(base)
        for name in [x for x, _, _ in legs if x != "parent-global" and "parent-global" in res]:
            d = statistics.median(res[name]["step"]) - mb
            print(f"{pname:5s} q{npr} {name:14s} - parent-global: {d * 1e3:+7.2f} us "
                  f"(parent-global spread over its repeats: {spread * 1e3:.2f} us)")
    if args.json:
        Path(args.json).parent.mkdir(parents=True, exist_ok=True)
        Path(args.json).write_text(json.dumps(report, indent=1))
    return 0


if __name__ == "__main__":
    sys.exit(main())
