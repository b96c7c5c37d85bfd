#!/bin/bash
# timing / debugging variants of the emitting loop: tools/ab_emit.sh <tag> "<VAR=val ...>"  ->  pda_amd/csrc/ab/libpda_hip_<tag>.so (select with PDA_HIP_LIB)
set -e
cd "$(dirname "$0")/.."
mkdir -p pda_amd/csrc/ab
env $2 python tools/gen_v7_emit_loop_asm.py > pda_amd/csrc/ab/loop7_$1.h
cd pda_amd/csrc
sed "s#pda_v7_emit_loop_asm.h#loop7_$1.h#" pda_v7_funnel.h > ab/funnel_$1.h
sed "s#pda_v7_funnel.h#ab/funnel_$1.h#" pda_score_funnel.hip > ab_funnel_$1.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I../../include -ffp-contract=off $EXTRA -c ab_funnel_$1.hip -o ab/funnel_$1.o
OBJS=""
for o in $(make -s print-objs); do      # (the Makefile's list of the library's objects: the only one)
    [ "$o" = pda_score_funnel.o ] || OBJS="$OBJS $o"
done
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ab/libpda_hip_$1.so $OBJS ab/funnel_$1.o
rm -f ab/funnel_$1.o ab_funnel_$1.hip
echo built ab/libpda_hip_$1.so
