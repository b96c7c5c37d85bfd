// The 32 x 32 logit tile of the softmax steps that take their logits as matrix products (pda_inbatch.hip, pda_fullsm.hip): the LDS image of 32
// rows, the tile's dot products on v_mfma_f32_32x32x2_f32 (exact f32), the accumulator layout, and the merge of two (max, sum of exp) pairs.
// One definition each: both steps recompute a tile in a later pass and rely on getting, bit for bit, the logits their statistics pass saw.
#pragma once
#include <cmath>
#include "pda_common.h"

constexpr int kT = 32;                  // tile edge
constexpr float kNormFloor = 1e-12f;

// the sum of v over the D / 4 lanes of a row's group: every lane holds it
template <int D>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = D / 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// LDS image of 32 packed rows, row stride D + 4 floats (16-byte rows, and the b128 reads of 32 rows at one k fall on distinct banks)
template <int D>
__device__ __forceinline__ void load_tile(float* s, const float* P, int row0, int rows_end) {
    constexpr int Q = D / 4;
    for (int idx = threadIdx.x; idx < kT * Q; idx += 64) {
        const int row = idx / Q, q = idx % Q;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + row < rows_end) v = *reinterpret_cast<const f32x4*>(P + (size_t)(row0 + row) * D + 4 * q);
        *reinterpret_cast<f32x4*>(s + row * (D + 4) + 4 * q) = v;
    }
}

// this lane's row of accumulator register `reg`: the C/D layout of the 32 x 32 MFMA (column = lane & 31)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// a[reg] = (row acc_row(reg, h) of sU) . (row lane & 31 of sI): d / 2 MFMAs on two independent accumulators (even and odd groups of 8 k), added
// at the end.  Lane (i, h) feeds k = 8 q + 4 h + j of its row in MFMA j of group q: A and B take the same k, the order of the sum is fixed.
template <int D>
__device__ __forceinline__ f32x16 tile_dots(const float* sU, const float* sI) {
    const int i = threadIdx.x & 31, h = threadIdx.x >> 5;
    f32x16 acc0 = {0.f}, acc1 = {0.f};
#pragma unroll
    for (int q = 0; q < D / 8; q += 2) {
        const f32x4 a0 = *reinterpret_cast<const f32x4*>(sU + i * (D + 4) + 8 * q + 4 * h);
        const f32x4 b0 = *reinterpret_cast<const f32x4*>(sI + i * (D + 4) + 8 * q + 4 * h);
        const f32x4 a1 = *reinterpret_cast<const f32x4*>(sU + i * (D + 4) + 8 * (q + 1) + 4 * h);
        const f32x4 b1 = *reinterpret_cast<const f32x4*>(sI + i * (D + 4) + 8 * (q + 1) + 4 * h);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[j], b0[j], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[j], b1[j], acc1, 0, 0, 0);
        }
    }
    return acc0 + acc1;
}

// (m, se) <- (m, se) merged with (m2, se2); a side with no admitted column is (-inf, 0) and stays out of the arithmetic
__device__ __forceinline__ void merge_stats(float& m, float& se, float m2, float se2) {
    const float M = fmaxf(m, m2);
    if (M == -INFINITY) return;                     // both empty
    const float s1 = (m == -INFINITY) ? 0.f : se * expf(m - M);
    const float s2 = (m2 == -INFINITY) ? 0.f : se2 * expf(m2 - M);
    m = M, se = s1 + s2;
}
