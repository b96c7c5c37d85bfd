// The LightGCN backbone (include/pda_hip_gcn.h) on MI355X (gfx950): the weighted CSR x dense product over the train graph that
// the forward pass (the layer mean) and the backward pass (the Horner step) are made of, and the regulariser of the batch's ego rows.  The
// triplet gradient is pda_bpr_step_f32 on the final tables and the update pda_adam_dense_sweep2_f32 on the ego tables themselves.
//
// Product layout: the one of the step kernels -- d/4 lanes per entry of the work list, each lane one float4 of every gathered row (at d = 64
// four entries per wave, sixteen per workgroup).  An entry is a whole row of at most PDA_GCN_CHUNK edges or one chunk of a longer row; the
// caller sorts the list by length, so the entries of a wave run about equally long.  Four edges' column, weight and row loads are issued
// before the first of them is added; the adds stay in edge order onto ONE accumulator, so the order of a sum is the CSR's.  The row's owner
// applies the fused forms (addend, running sum, scale) and stores; a chunk stores its partial sum for the second launch, which adds a cut
// row's partials in chunk order and applies the same forms.  No atomics, no LDS, no MFMA: the pass is a gather.
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_hip_gcn.h"

namespace {

struct GcnSpmmArgs {
    const int64_t* indptr;
    const int32_t* indices;
    const float* w;
    const int64_t* work;        // [n_work, 4]: row, first edge, end edge, slot
    const int64_t* long_rows;   // [n_long, 3]: row, first slot, chunks
    const float* X;
    const float* add;
    float* Y;
    const float* sum_in;
    float* sum_out;
    float* partials;            // [n_slots, d]
    size_t n_work, n_long;
    float scale;
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }

// the fused forms, by the lane group that owns row `row`: y = add + acc; Y = scale y, or Y = y and sum_out = scale (sum_in + y)
template <int D>
__device__ __forceinline__ void gcn_finish(const GcnSpmmArgs& a, int64_t row, int e, f32x4 acc) {
    const size_t off = (size_t)row * D + 4 * e;
    f32x4 y = acc;
    if (a.add != nullptr) y = ld4(a.add + off) + acc;
    if (a.sum_in != nullptr) {
        if (a.Y != nullptr) st4(a.Y + off, y);
        const f32x4 s = ld4(a.sum_in + off) + y;
        st4(a.sum_out + off, s * a.scale);
    } else {
        st4(a.Y + off, y * a.scale);
    }
}

template <int D>
__global__ __launch_bounds__(256) void gcn_spmm_kernel(GcnSpmmArgs a) {
    constexpr int G = D / 4;            // lanes per entry
    constexpr int PER = 256 / G;        // entries per workgroup
    const int e = threadIdx.x % G;
    const size_t item = (size_t)blockIdx.x * PER + threadIdx.x / G;
    if (item >= a.n_work) return;
    const int64_t* wk = a.work + 4 * item;
    const int64_t row = wk[0], e1 = wk[2], slot = wk[3];
    int64_t k = wk[1];
    const float* X = a.X + 4 * e;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (; k + 4 <= e1; k += 4) {
        const int c0 = a.indices[k], c1 = a.indices[k + 1], c2 = a.indices[k + 2], c3 = a.indices[k + 3];
        const float w0 = a.w[k], w1 = a.w[k + 1], w2 = a.w[k + 2], w3 = a.w[k + 3];
        const f32x4 x0 = ld4(X + (size_t)c0 * D), x1 = ld4(X + (size_t)c1 * D), x2 = ld4(X + (size_t)c2 * D), x3 = ld4(X + (size_t)c3 * D);
        acc = acc + x0 * w0;
        acc = acc + x1 * w1;
        acc = acc + x2 * w2;
        acc = acc + x3 * w3;
    }
    for (; k < e1; ++k) acc = acc + ld4(X + (size_t)a.indices[k] * D) * a.w[k];
    if (slot >= 0) {
        st4(a.partials + (size_t)slot * D + 4 * e, acc);
        return;
    }
    gcn_finish<D>(a, row, e, acc);
}

// the cut rows: the partial sums of a row in chunk order, then the fused forms
template <int D>
__global__ __launch_bounds__(256) void gcn_long_rows_kernel(GcnSpmmArgs a) {
    constexpr int G = D / 4;
    constexpr int PER = 256 / G;
    const int e = threadIdx.x % G;
    const size_t item = (size_t)blockIdx.x * PER + threadIdx.x / G;
    if (item >= a.n_long) return;
    const int64_t* lr = a.long_rows + 3 * item;
    const int64_t row = lr[0], s0 = lr[1], n = lr[2];
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int64_t j = 0; j < n; ++j) acc = acc + ld4(a.partials + (size_t)(s0 + j) * D + 4 * e);
    gcn_finish<D>(a, row, e, acc);
}

struct GcnRegArgs {
    const float* U0;
    const float* I0;
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    float* gU;
    float* gI;
    float* loss_acc;
    unsigned n_users, n_items;
    int B;
    float reg_c;        // regs / reg_div
};

template <int D>
__global__ __launch_bounds__(512) void gcn_reg_kernel(GcnRegArgs a) {
    constexpr int G = D / 4;
    constexpr int TPB = 512 / G;
    __shared__ float red[2][8];
    const int e = threadIdx.x % G;
    const int t = blockIdx.x * TPB + threadIdx.x / G;
    float sq = 0.f;
    if (t < a.B) {
        const int u = a.users[t], p = a.pos[t], n = a.neg[t];
        if ((unsigned)u < a.n_users && (unsigned)p < a.n_items && (unsigned)n < a.n_items) {
            const size_t ou = (size_t)u * D + 4 * e, op = (size_t)p * D + 4 * e, on = (size_t)n * D + 4 * e;
            const f32x4 ue = ld4(a.U0 + ou), pe = ld4(a.I0 + op), ne = ld4(a.I0 + on);
            sq = triplet_sq(ue, pe, ne);
            atomic_add4(a.gU + ou, ue * a.reg_c);
            atomic_add4(a.gI + op, pe * a.reg_c);
            atomic_add4(a.gI + on, ne * a.reg_c);
        }
    }
    if (a.loss_acc == nullptr) return;      // (uniform over the launch)
    block_loss_reduce(0.f, sq, red);
    if (threadIdx.x == 0) {
        float mf, rg;
        block_loss_terms(red, 0.f, a.reg_c, mf, rg);
        unsafeAtomicAdd(a.loss_acc + 0, rg);
        unsafeAtomicAdd(a.loss_acc + 2, rg);
    }
}

}  // namespace

extern "C" size_t pda_gcn_spmm_workspace_bytes(size_t n_slots, int d) {
    if (!pda_d_ok(d)) return 0;
    return n_slots * (size_t)d * sizeof(float);
}

extern "C" int pda_gcn_spmm_f32(const int64_t* indptr, const int32_t* indices, const float* w, size_t n_rows, const int64_t* work, size_t n_work,
                                const int64_t* long_rows, size_t n_long, size_t n_slots, const float* X, int d, const float* add, float* Y,
                                const float* sum_in, float* sum_out, float scale, void* workspace, size_t workspace_bytes, void* stream) {
    if (!indptr || !indices || !w || !work || !X) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu || n_work < n_rows || n_work > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if ((sum_in == nullptr) != (sum_out == nullptr)) return PDA_ERR_ARG;
    if (sum_out == nullptr && Y == nullptr) return PDA_ERR_ARG;
    if (X == Y || X == sum_out || (add != nullptr && (add == Y || add == sum_out)) || (Y != nullptr && Y == sum_out)) return PDA_ERR_ARG;
    if (!std::isfinite(scale)) return PDA_ERR_ARG;
    if (n_long > n_rows || (n_long != 0 && (!long_rows || n_slots < 2 * n_long)) || (n_long == 0 && n_slots != 0)) return PDA_ERR_ARG;
    if (n_work != n_rows - n_long + n_slots) return PDA_ERR_ARG;      // one entry per whole row, one per chunk of a cut row
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (n_slots != 0 && (!workspace || workspace_bytes < pda_gcn_spmm_workspace_bytes(n_slots, d))) return PDA_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const GcnSpmmArgs a{indptr, indices, w, work, long_rows, X, add, Y, sum_in, sum_out, reinterpret_cast<float*>(workspace), n_work, n_long, scale};
    switch (d) {
#define PDA_GCN_SPMM(DD)                                                                                                                      \
    hipLaunchKernelGGL(gcn_spmm_kernel<DD>, dim3((unsigned)((n_work + 256 / (DD / 4) - 1) / (256 / (DD / 4)))), dim3(256), 0, s, a);         \
    if (n_long != 0)                                                                                                                          \
        hipLaunchKernelGGL(gcn_long_rows_kernel<DD>, dim3((unsigned)((n_long + 256 / (DD / 4) - 1) / (256 / (DD / 4)))), dim3(256), 0, s, a); \
    break;
        case 32: PDA_GCN_SPMM(32)
        case 64: PDA_GCN_SPMM(64)
        case 128: PDA_GCN_SPMM(128)
        default: PDA_GCN_SPMM(256)
#undef PDA_GCN_SPMM
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_gcn_reg_f32(const float* U0, const float* I0, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                               const int32_t* neg, int B, int d, float regs, float reg_div, float* gU, float* gI, float* loss_acc, void* stream) {
    if (!U0 || !I0 || !users || !pos || !neg || !gU || !gI) return PDA_ERR_ARG;
    if (B <= 0 || B > (1 << 28) || !(reg_div > 0.f) || !std::isfinite(regs)) return PDA_ERR_ARG;
    if (!pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const GcnRegArgs a{U0, I0, users, pos, neg, gU, gI, loss_acc, (unsigned)n_users, (unsigned)n_items, B, regs / reg_div};
    switch (d) {
#define PDA_GCN_REG(DD)                                                                                                          \
    hipLaunchKernelGGL(gcn_reg_kernel<DD>, dim3((unsigned)((B + 512 / (DD / 4) - 1) / (512 / (DD / 4)))), dim3(512), 0, s, a); \
    break;
        case 32: PDA_GCN_REG(32)
        case 64: PDA_GCN_REG(64)
        case 128: PDA_GCN_REG(128)
        default: PDA_GCN_REG(256)
#undef PDA_GCN_REG
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
