#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds of yrss.hip, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S \
          -I include yastack_amd/csrc/yrss.hip -o new.s        (and the parent's: old.s)
    tools/kernel_code_diff.py old.s new.s

Prints one line per kernel: SAME when the instruction stream is identical,
DIFF (with both instruction counts) when it is not, NEW / GONE when only one
build has it, with [VGPRs, AGPRs, SGPRs, scratch bytes/lane, occupancy] from
the kernel's own metadata comments.  A trailing ", false" template argument
(a parameter added with a default) is dropped from the names, so a kernel that
only gained such a parameter is matched with its earlier self.  Labels and
symbol names inside the code are normalised the same way.
"""
import re
import subprocess
import sys


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                         check=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(path):
    text = open(path).read()
    res = {}
    # a kernel: from its label to its .end_amdhsa_kernel's function end (.Lfunc_end)
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
        name, body = m.group(1), m.group(2)
        if ".amdhsa_kernel " + name not in text:
            continue
        ins = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith("."):
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            line = re.sub(r"_Z\w+", "SYM", line)
            ins.append(line)
        meta = {}
        tail = text[m.end():m.end() + 6000]
        for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"),
                         ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
                         ("occ", r"; Occupancy: (\d+)")):
            mm = re.search(pat, tail)
            meta[key] = mm.group(1) if mm else "-"
        res[name] = (ins, [meta[k] for k in ("vgpr", "agpr", "sgpr", "scratch", "occ")])
    dm = demangle(list(res))
    out = {}
    for k, v in res.items():
        n = dm[k].replace("(anonymous namespace)::", "")
        n = re.sub(r"\(.*\)$", "", n)
        n = re.sub(r"(, false)+>$", ">", n)
        n = re.sub(r"^void ", "", n)
        out[n] = v
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for n in sorted(set(old) | set(new)):
        if n not in new:
            print("GONE", n, old[n][1])
            bad += 1
        elif n not in old:
            print("NEW ", n, new[n][1])
        elif old[n][0] == new[n][0] and old[n][1] == new[n][1]:
            print("SAME", n, new[n][1])
        else:
            print("DIFF", n, old[n][1], len(old[n][0]), "->", new[n][1], len(new[n][0]))
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
