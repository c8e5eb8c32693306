#!/bin/bash
# Build a library variant for same-process A/B runs (a path leg of
# tools/ab.py): tools/build_ab_lib.sh NAME -DMACRO=V ...
#   -> ab/lib/libyrss_NAME.so
# From the current tree, or from another checkout of the project named by
# YRSS_AB_SRC (e.g. the parent commit exported with `git archive`).
set -eu
cd "$(dirname "$0")/.."
name=$1; shift
mkdir -p ab/lib
S=${YRSS_AB_SRC:-.}
C=$S/yastack_amd/csrc
srcs="$C/yrss.hip $C/yrss_pcap.cpp $C/yrss_shard.cpp $C/yrss_fanout.cpp"
[ -f $C/yrss_seg.cpp ] && srcs="$srcs $C/yrss_seg.cpp"
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -Wall -Wno-unused-result \
    -Wno-pass-failed -DYRSS_TOOLS_BUILD=1 "$@" -I $S/include $srcs \
    -o ab/lib/libyrss_$name.so
echo "built ab/lib/libyrss_$name.so"
