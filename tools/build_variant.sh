#!/bin/bash
# A/B builds of ONE kernel file (default: the v4 file): tools/build_variant.sh <tag> "<extra hipcc flags>"  ->  pda_amd/csrc/ab/libpda_hip_<tag>.so
# (select it with PDA_HIP_LIB=<path>; the other objects and the generated pda_v6_free_asm.h are the ones of the regular build; SRC=<file>.hip
# rebuilds that file instead)
#   tools/build_variant.sh nofree -DPDA_V5_NO_FREE      the huge geometry with every half-tile tested (no decided half-tile: pda_v5_sweep.h)
#   tools/build_variant.sh uprep -DPDA_V5_UPREP         the huge geometry's user image by uprep5_kernel in every call (warm4_kernel writes none)
#   tools/build_variant.sh handover -DPDA_V5_HANDOVER   the dense call's warm-up hands its rows over through the workspace AND writes out_keys
#   tools/build_variant.sh extractold -DPDA_V5_EXTRACT_OLD   the huge geometry's exit path before the fused extract (one pass per half-tile, a block at a time)
#   tools/build_variant.sh exitprof -DPDA_V5_EXITPROF   the huge geometry with wall-clock counters around its loop exits (tools/time_huge_exits.py)
#   SRC=pda_score_topk.hip tools/build_variant.sh merge1 -DPDA_MERGE_R1_GENERAL    pda_topk_merge sends R = 1 through the general merge kernel
set -e
cd "$(dirname "$0")/../pda_amd/csrc"
mkdir -p ab
SRC=${SRC:-pda_score_topk_v4.hip}
OBJS=""
for o in pda_score_topk.o pda_score_prep.o pda_score_topk_v3.o pda_score_topk_v4.o pda_score_funnel.o pda_bpr_step.o pda_bpr_plan.o pda_bpr_plan_large.o pda_aux.o pda_temp_pop.o pda_pc.o pda_deep_topk.o pda_xquad.o pda_dice.o; do
    [ "$o" = "${SRC%.hip}.o" ] || OBJS="$OBJS $o"
done
/opt/rocm/bin/hipcc $2 --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I../../include -ffp-contract=off -c $SRC -o ab/v4_$1.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o ab/libpda_hip_$1.so $OBJS ab/v4_$1.o
rm ab/v4_$1.o
echo built ab/libpda_hip_$1.so
