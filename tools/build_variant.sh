#!/bin/bash
# A/B builds of ONE kernel file (default: the v4 file): tools/build_variant.sh <tag> "<extra hipcc flags>"  ->  pda_amd/csrc/ab/libpda_hip_<tag>.so
# (select it with PDA_HIP_LIB=<path>; the other objects and the generated pda_v6_free_asm.h are the ones of the regular build; SRC=<file>.hip
# rebuilds that file instead)
#   tools/build_variant.sh nofree -DPDA_V5_NO_FREE      the huge geometry with every half-tile tested (no decided half-tile: pda_v5_sweep.h)
#   tools/build_variant.sh exitprof -DPDA_V5_EXITPROF   the huge geometry with wall-clock counters around its loop exits (tools/time_huge_exits.py)
set -e
cd "$(dirname "$0")/../pda_amd/csrc"
mkdir -p ab
SRC=${SRC:-pda_score_topk_v4.hip}
OBJS=""
for o in $(make -s print-objs); do      # (the Makefile's list of the library's objects: the only one)
    [ "$o" = "${SRC%.hip}.o" ] || OBJS="$OBJS $o"
done
/opt/rocm/bin/hipcc $2 --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I../../include -ffp-contract=off -c $SRC -o ab/v4_$1.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ab/libpda_hip_$1.so $OBJS ab/v4_$1.o
rm ab/v4_$1.o
echo built ab/libpda_hip_$1.so
