// The in-batch softmax with logQ correction (include/pda_hip_inbatch.h) on MI355X (gfx950): the B positives of the batch are the
// columns of one [B, B] logit matrix, which exists only as 32 x 32 tiles in the accumulators of v_mfma_f32_32x32x2_f32 (exact f32).
//
// Four launches:
//   pack   the 2 B rows gathered once into an image in the workspace (u^ / i^ under norm, the raw rows otherwise) with 1 / max(|x|, 1e-12), |x|^2,
//          the column's logq and the validated ids beside it; the two [B, d] gradient buffers zeroed.
//   stats  workgroup (row tile, column split): the logit tiles of the split, each lane's running (m, se) over its 16 rows, merged over the 32
//          lanes of a row at the end -> (m, se) per (split, row); the tile on the diagonal also stores S_rr.
//   grad   the same tiles recomputed by the same code (bit for bit the logits the statistics saw), C for the tile, and both products from it:
//          C^T U^ straight from the accumulator layout (it sums over the tile's ROW index, which sits in the registers), C I^ with the tile
//          transposed through LDS.  C I^ stays in accumulators over the split's column tiles; both go into the [B, d] buffers by float atomics.
//   tail   d / 4 lanes per row: the projection of the normalisation, c_reg x, the scatter to gU / gI through the shared pieces of
//          pda_train_common.h, the tags and loss_acc.
// A workgroup of the two tile passes is ONE wave: nothing but the wave's own LDS traffic orders it.
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_sample.h"
#include "pda_softmax_tiles.h"
#include "pda_hip_inbatch.h"

namespace {

constexpr int kTargetGroups = 1024;     // workgroups of one wave the tile passes aim at: one per SIMD of the chip
static_assert(PDA_INBATCH_ROW_TILE == kT && PDA_INBATCH_COL_TILE == kT, "the tile passes are written for 32 x 32 tiles");

// ---- the workspace ------------------------------------------------------------------------------------------------------------------------------
struct Ws {
    float* P;           // [2 Bp, d]: rows [0, B) the user rows, rows [Bp, Bp + B) the item rows
    float* GU;          // [Bp, d]   sum_c C_rc i^_c
    float* GI;          // [Bp, d]   sum_r C_rc u^_r
    float* inv;         // [2 Bp]    1 / max(|x|, 1e-12)
    float* sq;          // [2 Bp]    |x|^2
    float* lq;          // [Bp]      logq[pos[c]] or 0
    float* diag;        // [Bp]      S_rr
    int32_t* vpos;      // [Bp]      pos[r], -1 for an invalid row
    float* part;        // [splits, Bp, 2]  (m, se)
    size_t bytes;
};

inline int tiles_of(int B) { return (B + kT - 1) / kT; }
// column tiles per split, and the number of splits that leaves
inline int tiles_per_split(int B) {
    const int nt = tiles_of(B);
    int want = (kTargetGroups + nt - 1) / nt;       // splits that would give kTargetGroups workgroups
    if (want > nt) want = nt;
    return (nt + want - 1) / want;
}
inline int col_splits(int B) {
    const int nt = tiles_of(B), tps = tiles_per_split(B);
    return (nt + tps - 1) / tps;
}

Ws carve(void* base, int B, int d) {
    const size_t Bp = (size_t)tiles_of(B) * kT, S = (size_t)col_splits(B);
    char* p = reinterpret_cast<char*>(base);
    Ws w;
    size_t off = 0;
    auto take = [&](size_t n_words) {
        char* at = p + off;
        off += ((n_words * 4 + 15) / 16) * 16;
        return at;
    };
    w.P = reinterpret_cast<float*>(take(2 * Bp * d));
    w.GU = reinterpret_cast<float*>(take(Bp * d));
    w.GI = reinterpret_cast<float*>(take(Bp * d));
    w.inv = reinterpret_cast<float*>(take(2 * Bp));
    w.sq = reinterpret_cast<float*>(take(2 * Bp));
    w.lq = reinterpret_cast<float*>(take(Bp));
    w.diag = reinterpret_cast<float*>(take(Bp));
    w.vpos = reinterpret_cast<int32_t*>(take(Bp));
    w.part = reinterpret_cast<float*>(take(S * Bp * 2));
    w.bytes = off;
    return w;
}

struct InbatchArgs {
    const float* U;
    const float* I;
    const int32_t* users;
    const int32_t* pos;
    const float* logq;
    const uint32_t* mask;
    float* gU;
    float* gI;
    int32_t* tagU;
    int32_t* tagI;
    float* loss_acc;
    Ws ws;
    unsigned n_users, n_items;
    int tag;
    int B, Bp, W;           // W: words per mask row
    int tps, splits;        // column tiles per split, splits
    float inv_B, inv_tau, reg_c;
    int any_order, users_distinct;
};

// ---- pack: d / 4 lanes per row, 2 B rows ----------------------------------------------------------------------------------------------------------
template <int D, bool NORM>
__device__ __forceinline__ void pack_body(const InbatchArgs& a) {
    constexpr int L = D / 4, TPB = 512 / L;
    const int g = threadIdx.x / L, e = threadIdx.x % L;
    const int t = blockIdx.x * TPB + g;             // [0, B): user rows, [B, 2 B): item rows
    if (t >= 2 * a.B) return;                       // (whole lane groups leave)
    const bool item = t >= a.B;
    const int r = item ? t - a.B : t;
    const int u = a.users[r], p = a.pos[r];
    const bool ok = (unsigned)u < a.n_users && (unsigned)p < a.n_items;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (ok) x = *reinterpret_cast<const f32x4*>((item ? a.I + (size_t)p * D : a.U + (size_t)u * D) + 4 * e);
    const float sq = group_sum<D>(dot4(x, x));
    const float inv = 1.f / fmaxf(sqrtf(sq), kNormFloor);
    const size_t row = (size_t)(item ? a.Bp + r : r);
    if constexpr (NORM) x = x * inv;
    *reinterpret_cast<f32x4*>(a.ws.P + row * D + 4 * e) = x;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    *reinterpret_cast<f32x4*>((item ? a.ws.GI : a.ws.GU) + (size_t)r * D + 4 * e) = zero;
    if (e == 0) {
        a.ws.inv[row] = inv;
        a.ws.sq[row] = sq;
        if (item) {
            a.ws.lq[r] = (ok && a.logq) ? a.logq[p] : 0.f;
            a.ws.vpos[r] = ok ? p : -1;
        }
    }
}
template <int D>
__global__ void __launch_bounds__(512) inbatch_pack_kernel(InbatchArgs a) { pack_body<D, false>(a); }
template <int D>
__global__ void __launch_bounds__(512) inbatch_pack_norm_kernel(InbatchArgs a) { pack_body<D, true>(a); }

// ---- the tile passes (the tile itself: pda_softmax_tiles.h) --------------------------------------------------------------------------------------------------------------------------------
// What a lane knows of its column c = c0 + (lane & 31) and of its 16 rows
struct ColInfo {
    float lq;
    int pos;        // -1: invalid or past B
    int c;
};
__device__ __forceinline__ ColInfo col_info(const InbatchArgs& a, int c0) {
    ColInfo ci;
    ci.c = c0 + (threadIdx.x & 31);
    const bool in = ci.c < a.B;
    ci.pos = in ? a.ws.vpos[ci.c] : -1;
    ci.lq = in ? a.ws.lq[ci.c] : 0.f;
    return ci;
}
// is column ci in E_r?  (pos_r: vpos of row r, -1 for a row that is dropped; mword: the row's mask word of this column tile)
__device__ __forceinline__ bool admitted(int r, int pos_r, const ColInfo& ci, uint32_t mword) {
    if (pos_r < 0 || ci.pos < 0) return false;
    if (r == ci.c) return true;
    return ci.pos != pos_r && ((mword >> (threadIdx.x & 31)) & 1u) == 0u;
}

template <int D>
__global__ void __launch_bounds__(64) inbatch_stats_kernel(InbatchArgs a) {
    __shared__ __attribute__((aligned(16))) float sU[kT * (D + 4)];
    __shared__ __attribute__((aligned(16))) float sI[kT * (D + 4)];
    const int lane = threadIdx.x, h = lane >> 5;
    const int r0 = blockIdx.x * kT, split = blockIdx.y;
    const int ct0 = split * a.tps, ct1 = min(ct0 + a.tps, a.Bp / kT);
    load_tile<D>(sU, a.ws.P, r0, a.B);
    float m[16], se[16];
    int pos_r[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int r = r0 + acc_row(reg, h);
        m[reg] = -INFINITY, se[reg] = 0.f;
        pos_r[reg] = r < a.B ? a.ws.vpos[r] : -1;
    }
    for (int ct = ct0; ct < ct1; ++ct) {
        const int c0 = ct * kT;
        __syncthreads();                            // (the previous tile's reads of sI)
        load_tile<D>(sI, a.ws.P + (size_t)a.Bp * D, c0, a.B);
        __syncthreads();
        const ColInfo ci = col_info(a, c0);
        const f32x16 dots = tile_dots<D>(sU, sI);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int r = r0 + acc_row(reg, h);
            const uint32_t mw = (a.mask && r < a.B) ? a.mask[(size_t)r * a.W + ct] : 0u;
            if (!admitted(r, pos_r[reg], ci, mw)) continue;
            const float s = dots[reg] * a.inv_tau - ci.lq;
            if (r == ci.c) a.ws.diag[r] = s;
            // one exp per logit: the smaller of (m, s) is the one rescaled.  m == -inf: dlt = +inf, e = 0, se = 1.
            const float dlt = s - m[reg], e = expf(-fabsf(dlt));
            se[reg] = dlt <= 0.f ? se[reg] + e : se[reg] * e + 1.f;
            m[reg] = fmaxf(m[reg], s);
        }
    }
    // the 32 lanes of a half hold the same 16 rows: merge them
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float m2 = __shfl_xor(m[reg], o, 64), se2 = __shfl_xor(se[reg], o, 64);
            merge_stats(m[reg], se[reg], m2, se2);
        }
        const int r = r0 + acc_row(reg, h);
        if ((lane & 31) == 0 && r < a.B) {
            float* out = a.ws.part + ((size_t)split * a.Bp + r) * 2;
            out[0] = m[reg], out[1] = se[reg];
        }
    }
}

// the row's (m, se) over all splits; a dropped row gives (-inf, 0)
__device__ __forceinline__ void row_stats(const InbatchArgs& a, int r, float& m, float& se) {
    m = -INFINITY, se = 0.f;
    for (int s = 0; s < a.splits; ++s) {
        const float* in = a.ws.part + ((size_t)s * a.Bp + r) * 2;
        merge_stats(m, se, in[0], in[1]);
    }
}

template <int D>
__global__ void __launch_bounds__(64) inbatch_grad_kernel(InbatchArgs a) {
    constexpr int NC = D / 32;                      // 32-wide chunks of the embedding
    __shared__ __attribute__((aligned(16))) float sU[kT * (D + 4)];
    __shared__ __attribute__((aligned(16))) float sI[kT * (D + 4)];
    __shared__ float sC[kT * (kT + 1)];
    __shared__ float sM[kT], sInvSe[kT];
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * kT, split = blockIdx.y;
    const int ct0 = split * a.tps, ct1 = min(ct0 + a.tps, a.Bp / kT);
    load_tile<D>(sU, a.ws.P, r0, a.B);
    if (lane < kT) {
        float m = -INFINITY, se = 0.f;
        if (r0 + lane < a.B) row_stats(a, r0 + lane, m, se);
        sM[lane] = m;
        sInvSe[lane] = se > 0.f ? 1.f / se : 0.f;
    }
    __syncthreads();
    float m[16], inv_se[16];
    int pos_r[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int rr = acc_row(reg, h), r = r0 + rr;
        m[reg] = sM[rr], inv_se[reg] = sInvSe[rr];
        pos_r[reg] = r < a.B ? a.ws.vpos[r] : -1;
    }
    const float cscale = a.inv_tau * a.inv_B;
    f32x16 accG[NC];                                // sum_c C_rc i^_c of the split's columns: rows in the registers, 32 floats of d on the lanes
#pragma unroll
    for (int k = 0; k < NC; ++k) accG[k] = f32x16{0.f};
    for (int ct = ct0; ct < ct1; ++ct) {
        const int c0 = ct * kT;
        __syncthreads();                            // (the previous tile's reads of sI and sC)
        load_tile<D>(sI, a.ws.P + (size_t)a.Bp * D, c0, a.B);
        __syncthreads();
        const ColInfo ci = col_info(a, c0);
        const f32x16 dots = tile_dots<D>(sU, sI);
        float C[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int rr = acc_row(reg, h), r = r0 + rr;
            const uint32_t mw = (a.mask && r < a.B) ? a.mask[(size_t)r * a.W + ct] : 0u;
            float c = 0.f;
            if (admitted(r, pos_r[reg], ci, mw)) {
                const float s = dots[reg] * a.inv_tau - ci.lq;
                const float p = expf(s - m[reg]) * inv_se[reg];
                c = (r == ci.c ? p - 1.f : p) * cscale;
            }
            C[reg] = c;
            sC[rr * (kT + 1) + i] = c;
        }
        // C^T U^ for the column block: it sums over the tile's row index -- the accumulator registers themselves are the A operand (A[col][k = row]),
        // the B operand is row acc_row(reg, h) of sU.  One chunk of 32 floats of d at a time, added to GI.
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            f32x16 accH = {0.f};
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                accH = __builtin_amdgcn_mfma_f32_32x32x2f32(C[reg], sU[acc_row(reg, h) * (D + 4) + 32 * k + i], accH, 0, 0, 0);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int c = c0 + acc_row(reg, h);
                if (c < a.B) unsafeAtomicAdd(a.ws.GI + (size_t)c * D + 32 * k + i, accH[reg]);
            }
        }
        // C I^ for the row block: it sums over the column (lane) index, so the tile goes through LDS: A[row][k = col] = sC[row][col]
        __syncthreads();
        float ca[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) ca[s] = sC[i * (kT + 1) + 2 * s + h];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
#pragma unroll
            for (int s = 0; s < 16; ++s)
                accG[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[s], sI[(2 * s + h) * (D + 4) + 32 * k + i], accG[k], 0, 0, 0);
        }
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int r = r0 + acc_row(reg, h);
            if (r < a.B) unsafeAtomicAdd(a.ws.GU + (size_t)r * D + 32 * k + i, accG[k][reg]);
        }
    }
}

// ---- the tail: d / 4 lanes per row, the layout of the other step kernels ----------------------------------------------------------------------------
template <int D, bool NORM>
__device__ __forceinline__ void tail_body(const InbatchArgs& a) {
    constexpr int L = D / 4, TPB = 512 / L;
    __shared__ float red[2][8];
    __shared__ int s_pos[TPB];
    __shared__ __attribute__((aligned(16))) float s_dpe[TPB * D];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;
    float maxi = 0.f, sq = 0.f;
    int p = -1;
    if (t < a.B) p = a.ws.vpos[t];
    const bool active = p >= 0;
    float* ptarget = nullptr;
    if (active) {
        const int u = a.users[t];
        const f32x4 uq = *reinterpret_cast<const f32x4*>(a.ws.P + (size_t)t * D + 4 * e);
        const f32x4 iq = *reinterpret_cast<const f32x4*>(a.ws.P + (size_t)(a.Bp + t) * D + 4 * e);
        const f32x4 gq = *reinterpret_cast<const f32x4*>(a.ws.GU + (size_t)t * D + 4 * e);
        const f32x4 hq = *reinterpret_cast<const f32x4*>(a.ws.GI + (size_t)t * D + 4 * e);
        f32x4 due, die;
        if constexpr (NORM) {
            // the image holds x^ = x inv: the raw row is x^ max(|x|, 1e-12) to a rounding
            const float inv_u = a.ws.inv[t], inv_i = a.ws.inv[a.Bp + t];
            const float nu = fmaxf(sqrtf(a.ws.sq[t]), kNormFloor), ni = fmaxf(sqrtf(a.ws.sq[a.Bp + t]), kNormFloor);
            const float pu = group_sum<D>(dot4(uq, gq)), pi = group_sum<D>(dot4(iq, hq));
            due = inv_u * (gq - pu * uq) + (a.reg_c * nu) * uq;
            die = inv_i * (hq - pi * iq) + (a.reg_c * ni) * iq;
        } else {
            due = gq + a.reg_c * uq;
            die = hq + a.reg_c * iq;
        }
        if (e == 0) {
            float m, se;
            row_stats(a, t, m, se);
            maxi = -((m - a.ws.diag[t]) + logf(se));            // block_loss_terms takes -sum(maxi) / B
            sq = a.ws.sq[t] + a.ws.sq[a.Bp + t];
            a.tagU[u] = a.tag;                                  // same value from every writer of a row: plain stores
            a.tagI[p] = a.tag;
        }
        // (the dense-gradient writes of a tagged step: pda_train_common.h has the precondition of the plain store)
        if (a.users_distinct) *reinterpret_cast<f32x4*>(a.gU + (size_t)u * D + 4 * e) = due;
        else atomic_add4(a.gU + (size_t)u * D + 4 * e, due);
        *reinterpret_cast<f32x4*>(s_dpe + g * D + 4 * e) = die;
        ptarget = a.gI + (size_t)p * D + 4 * e;
    }
    if (e == 0) s_pos[g] = p;
    __syncthreads();
    if (active && a.any_order) pos_scatter_any<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);
    else if (active && pos_run_head(s_pos, g, p)) pos_scatter_run<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);     // (grouped batch)
    block_loss_reduce(maxi, sq, red);
    if (tid == 0 && a.loss_acc) block_loss_add(red, a.inv_B, a.reg_c, a.loss_acc);
}
template <int D>
__global__ void __launch_bounds__(512) inbatch_tail_kernel(InbatchArgs a) { tail_body<D, false>(a); }
template <int D>
__global__ void __launch_bounds__(512) inbatch_tail_norm_kernel(InbatchArgs a) { tail_body<D, true>(a); }

// ---- the train mask: one thread per (row, column), the 32 verdicts of a word gathered by a ballot: every word has one writer ----------------------------
__global__ void __launch_bounds__(256) inbatch_mask_kernel(const int32_t* users, const int32_t* pos, int B, int W, const int64_t* indptr,
                                                           const int32_t* indices, unsigned n_users, unsigned n_items, uint32_t* mask) {
    const size_t n_bits = (size_t)B * (size_t)W * 32;                   // a multiple of 32: a half wave is one word
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    bool bit = false;
    if (idx < n_bits) {
        const int r = (int)(idx / ((size_t)W * 32)), c = (int)(idx % ((size_t)W * 32));
        const int u = users[r];
        if (c < B && c != r && (unsigned)u < n_users && (unsigned)pos[r] < n_items) {
            const int n = pos[c];
            if ((unsigned)n < n_items && (unsigned)users[c] < n_users) bit = train_row_has(indices, indptr[u], indptr[u + 1], n);
        }
    }
    const unsigned long long votes = __ballot(bit);                     // (every lane of the wave is here)
    if ((threadIdx.x & 31) == 0 && idx < n_bits) mask[idx / 32] = (uint32_t)(votes >> (threadIdx.x & 32));
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------
int check_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float tau,
               int norm, float reg_div, const float* gU, const float* gI, const int32_t* tagU, const int32_t* tagI, int step_tag, int flags,
               const void* ws, size_t ws_bytes) {
    if (!U || !I || !users || !pos || !gU || !gI || !tagU || !tagI || !ws) return PDA_ERR_ARG;
    if (B < 1 || B > PDA_INBATCH_MAX_B || !(reg_div > 0.f) || step_tag <= 0 || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (!(tau > 0.f) || !std::isfinite(tau) || (norm != 0 && norm != 1)) return PDA_ERR_ARG;
    if (flags & ~(PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT)) return PDA_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) & 15u) != 0) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (ws_bytes < pda_inbatch_workspace_bytes(B, d)) return PDA_ERR_ARG;
    return PDA_OK;
}

#define INBATCH_TILE_LAUNCH(KERNEL, W, GRID, STREAM, ARGS)                                      \
    switch (W) {                                                                                \
        case 32: hipLaunchKernelGGL(KERNEL<32>, GRID, dim3(64), 0, STREAM, ARGS); break;        \
        case 64: hipLaunchKernelGGL(KERNEL<64>, GRID, dim3(64), 0, STREAM, ARGS); break;        \
        case 128: hipLaunchKernelGGL(KERNEL<128>, GRID, dim3(64), 0, STREAM, ARGS); break;      \
        default: hipLaunchKernelGGL(KERNEL<256>, GRID, dim3(64), 0, STREAM, ARGS); break;       \
    }

// (arguments checked by the callers)
int launch_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float tau,
                int norm, const float* logq, const uint32_t* mask, float regs, float reg_div, float* gU, float* gI, int32_t* tagU, int32_t* tagI,
                int step_tag, int flags, void* ws, float* loss_acc, hipStream_t s) {
    InbatchArgs a{U, I, users, pos, logq, mask, gU, gI, tagU, tagI, loss_acc, carve(ws, B, d), (unsigned)n_users, (unsigned)n_items, step_tag, B,
                  tiles_of(B) * kT, (B + 31) / 32, tiles_per_split(B), col_splits(B), 1.0f / (float)B, 1.0f / tau, regs / reg_div,
                  (flags & PDA_UPD_ANY_ORDER) ? 1 : 0, (flags & PDA_UPD_USERS_DISTINCT) ? 1 : 0};
    const dim3 tiles((unsigned)tiles_of(B), (unsigned)a.splits);
    if (norm) {
        PDA_STEP_LAUNCH(inbatch_pack_norm_kernel, d, 2 * B, s, a)
    } else {
        PDA_STEP_LAUNCH(inbatch_pack_kernel, d, 2 * B, s, a)
    }
    PDA_CHECK_LAUNCH();
    INBATCH_TILE_LAUNCH(inbatch_stats_kernel, d, tiles, s, a)
    PDA_CHECK_LAUNCH();
    INBATCH_TILE_LAUNCH(inbatch_grad_kernel, d, tiles, s, a)
    PDA_CHECK_LAUNCH();
    if (norm) {
        PDA_STEP_LAUNCH(inbatch_tail_norm_kernel, d, B, s, a)
    } else {
        PDA_STEP_LAUNCH(inbatch_tail_kernel, d, B, s, a)
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" int pda_inbatch_col_splits(int B) { return (B < 1 || B > PDA_INBATCH_MAX_B) ? 0 : col_splits(B); }

extern "C" size_t pda_inbatch_workspace_bytes(int B, int d) {
    if (B < 1 || B > PDA_INBATCH_MAX_B || !pda_d_ok(d)) return 0;
    return carve(nullptr, B, d).bytes;
}

extern "C" int pda_inbatch_mask(const int32_t* users, const int32_t* pos, int B, const int64_t* train_indptr, const int32_t* train_indices,
                                size_t n_users, size_t n_items, uint32_t* mask, void* stream) {
    if (!users || !pos || !train_indptr || !train_indices || !mask) return PDA_ERR_ARG;
    if (B < 1 || B > PDA_INBATCH_MAX_B || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    const int W = (B + 31) / 32;
    const size_t n = (size_t)B * (size_t)W * 32;    // <= 2^28
    hipLaunchKernelGGL(inbatch_mask_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), users, pos, B, W,
                       train_indptr, train_indices, (unsigned)n_users, (unsigned)n_items, mask);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_inbatch_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B,
                                    int d, float tau, int norm, const float* logq, const uint32_t* mask, float regs, float reg_div, float* gU,
                                    float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags, void* ws, size_t ws_bytes, float* loss_acc,
                                    void* stream) {
    const int rc = check_step(U, I, n_users, n_items, users, pos, B, d, tau, norm, reg_div, gU, gI, tagU, tagI, step_tag, flags, ws, ws_bytes);
    if (rc != PDA_OK) return rc;
    return launch_step(U, I, n_users, n_items, users, pos, B, d, tau, norm, logq, mask, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags, ws,
                       loss_acc, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_inbatch_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                         float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float tau,
                                         int norm, const float* logq, const uint32_t* mask, float regs, float reg_div, int step_tag, float lr_t,
                                         float beta1, float beta2, float eps, int flags, int cache_policy, void* ws, size_t ws_bytes,
                                         float* loss_acc, void* stream) {
    if (!mU || !vU || !mI || !vI) return PDA_ERR_ARG;
    if (cache_policy < PDA_ADAM_CACHE_AUTO || cache_policy > PDA_ADAM_CACHE_STREAM) return PDA_ERR_ARG;
    int rc = check_step(U, I, n_users, n_items, users, pos, B, d, tau, norm, reg_div, gU, gI, tagU, tagI, step_tag, flags, ws, ws_bytes);
    if (rc != PDA_OK) return rc;
    rc = launch_step(U, I, n_users, n_items, users, pos, B, d, tau, norm, logq, mask, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags, ws, loss_acc,
                     reinterpret_cast<hipStream_t>(stream));
    if (rc != PDA_OK) return rc;
    return pda_adam_dense_sweep4_f32(U, mU, vU, gU, n_users, tagU, I, mI, vI, gI, n_items, tagI, d, step_tag, lr_t, beta1, beta2, eps, cache_policy,
                                     stream);
}
