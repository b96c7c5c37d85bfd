// Inverse propensity scoring on the BPR loss (include/pda_hip_ips.h) on MI355X (gfx950): the batch's weight sum, and the gradient
// step of pda_bpr_step.hip's dense-gradient mode with every triplet's loss scaled by the weight of its positive.  The Adam update is
// pda_adam_dense_sweep4_f32 itself.
//
// Step layout: the one of pda_bpr_step.hip -- d/4 lanes per triplet, each lane owns one float4 of the three gathered rows, the dots by the
// xor-shuffle ladder of triplet_dots.  The only new traffic is one 4-byte gather per triplet (ipw[pos]) and, self-normalised, one uniform load
// of S.  Equal positives inside a workgroup are summed by their first triplet through LDS, as there (they carry the same weight: a hot item is
// still one atomic per element and workgroup).  A kernel of its own, on the helpers every step kernel shares (pda_train_common.h).
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_hip_ips.h"

namespace {

struct IpsStepArgs {
    const float* U;
    const float* I;
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    const float* ipw;
    const float* wsum;      // NULL: the triplets are scaled by w_t / B; else by w_t / *wsum
    float* gU;
    float* gI;
    int32_t* tagU;
    int32_t* tagI;
    float* loss_acc;
    unsigned n_users, n_items;
    int tag;
    int B;
    float inv_B;
    float reg_c;            // regs / reg_div
    int any_order;          // PDA_UPD_ANY_ORDER
    int users_distinct;     // PDA_UPD_USERS_DISTINCT
};

// One workgroup of 1 024 threads.  float64 partial sums: the one rounding to fp32 at the end keeps the result within an ulp of the exact sum
// whatever the weights, and a fixed order (thread: t = tid, tid + 1024, ...; wave: xor ladder; workgroup: waves 0 .. 15) keeps its bits.
__global__ void __launch_bounds__(1024) ips_weight_sum_kernel(const float* __restrict__ ipw, const int32_t* __restrict__ users,
                                                              const int32_t* __restrict__ pos, const int32_t* __restrict__ neg, int B,
                                                              unsigned n_users, unsigned n_items, float* __restrict__ wsum) {
    __shared__ double part[16];
    double acc = 0.0;
    for (int t = (int)threadIdx.x; t < B; t += 1024) {
        const int u = users[t], p = pos[t], n = neg[t];
        if (triplet_ids_ok(u, p, n, n_users, n_items)) acc += (double)ipw[p];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
#pragma unroll
        for (int w = 0; w < 16; ++w) s += part[w];
        *wsum = (float)s;
    }
}

template <int D>
__global__ void __launch_bounds__(512) ips_step_kernel(IpsStepArgs a) {
    constexpr int L = D / 4;        // lanes per triplet
    constexpr int TPB = 512 / L;    // triplets per block
    __shared__ float red[2][8];
    __shared__ int s_pos[TPB];
    __shared__ __attribute__((aligned(16))) float s_dpe[TPB * D];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;

    // the scale every triplet's weight is multiplied by: 1 / B, or 1 / S with S in device memory (uniform over the grid)
    float scale = a.inv_B;
    if (a.wsum != nullptr) {
        const float S = *a.wsum;
        scale = S > 0.f ? 1.f / S : 0.f;
    }

    float maxi = 0.f, sq = 0.f;
    int u = 0, p = -1, n = 0;
    bool active = t < a.B;
    if (active) {
        u = a.users[t], p = a.pos[t], n = a.neg[t];
        active = triplet_ids_ok(u, p, n, a.n_users, a.n_items);
        if (!active) p = -1;
    }
    float* ptarget = nullptr;
    if (active) {
        const float wt = a.ipw[p] * scale;
        const f32x4 ue = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * D + 4 * e);
        const f32x4 pe = *reinterpret_cast<const f32x4*>(a.I + (size_t)p * D + 4 * e);
        const f32x4 ne = *reinterpret_cast<const f32x4*>(a.I + (size_t)n * D + 4 * e);
        float ps, ns, ls = 0.f;
        triplet_dots<D>(ue, pe, ne, ps, ns);
        const float gg = bpr_dloss_dx(ps - ns, wt, e, ls);       // -w_t scale d ls / dx
        if (e == 0) maxi = wt * ls;                              // the triplet's share of -mf
        sq = triplet_sq(ue, pe, ne);
        f32x4 due, dpe, dne;
        triplet_row_grads(ue, pe, ne, gg, gg, a.reg_c, due, dpe, dne);
        // (the dense-gradient writes of a tagged step: pda_train_common.h has the precondition of the plain store)
        if (a.users_distinct) *reinterpret_cast<f32x4*>(a.gU + (size_t)u * D + 4 * e) = due;
        else atomic_add4(a.gU + (size_t)u * D + 4 * e, due);
        atomic_add4(a.gI + (size_t)n * D + 4 * e, dne);
        ptarget = a.gI + (size_t)p * D + 4 * e;
        if (e == 0) {                   // same value from every writer of a row: plain stores
            a.tagU[u] = a.tag;
            a.tagI[p] = a.tag;
            a.tagI[n] = a.tag;
        }
        *reinterpret_cast<f32x4*>(s_dpe + g * D + 4 * e) = dpe;
    }
    if (e == 0) s_pos[g] = p;
    __syncthreads();
    if (active && a.any_order) pos_scatter_any<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);
    else if (active && pos_run_head(s_pos, g, p)) pos_scatter_run<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);     // (grouped batch)
    block_loss_reduce(maxi, sq, red);
    if (tid == 0 && a.loss_acc) block_loss_add(red, 1.f, a.reg_c, a.loss_acc);     // (maxi carries its weight and scale already)
}

// (arguments checked by the callers)
int launch_weight_sum(const float* ipw, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg, int B,
                      float* wsum, hipStream_t s) {
    hipLaunchKernelGGL(ips_weight_sum_kernel, dim3(1), dim3(1024), 0, s, ipw, users, pos, neg, B, (unsigned)n_users, (unsigned)n_items, wsum);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

int launch_step(const IpsStepArgs& a, int d, hipStream_t s) {
    PDA_STEP_LAUNCH(ips_step_kernel, d, a.B, s, a)
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

int check_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
               const float* ipw, int B, int d, float reg_div, const float* gU, const float* gI, const int32_t* tagU, const int32_t* tagI,
               int step_tag, int flags) {
    if (!U || !I || !users || !pos || !neg || !ipw || !gU || !gI || !tagU || !tagI) return PDA_ERR_ARG;
    if (B <= 0 || B > (1 << 28) || !(reg_div > 0.f) || step_tag <= 0 || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (flags & ~(PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT)) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    return PDA_OK;
}

IpsStepArgs step_args(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                      const float* ipw, const float* wsum, int B, float regs, float reg_div, float* gU, float* gI, int32_t* tagU, int32_t* tagI,
                      int step_tag, int flags, float* loss_acc) {
    return IpsStepArgs{U, I, users, pos, neg, ipw, wsum, gU, gI, tagU, tagI, loss_acc, (unsigned)n_users, (unsigned)n_items, step_tag, B,
                       1.0f / (float)B, regs / reg_div, (flags & PDA_UPD_ANY_ORDER) ? 1 : 0, (flags & PDA_UPD_USERS_DISTINCT) ? 1 : 0};
}

}  // namespace

extern "C" int pda_ips_weight_sum(const float* ipw, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                                  int B, float* wsum, void* stream) {
    if (!ipw || !users || !pos || !neg || !wsum || B <= 0 || B > (1 << 28) || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    return launch_weight_sum(ipw, n_users, n_items, users, pos, neg, B, wsum, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_ips_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                                const int32_t* neg, const float* ipw, const float* wsum, int B, int d, float regs, float reg_div, float* gU,
                                float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags, float* loss_acc, void* stream) {
    const int rc = check_step(U, I, n_users, n_items, users, pos, neg, ipw, B, d, reg_div, gU, gI, tagU, tagI, step_tag, flags);
    if (rc != PDA_OK) return rc;
    return launch_step(step_args(U, I, n_users, n_items, users, pos, neg, ipw, wsum, B, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags, loss_acc),
                       d, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_ips_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                     float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                                     const float* ipw, float* wsum_ws, int B, int d, float regs, float reg_div, int step_tag, float lr_t,
                                     float beta1, float beta2, float eps, int flags, int cache_policy, float* loss_acc, void* stream) {
    if (!mU || !vU || !mI || !vI) return PDA_ERR_ARG;
    if (cache_policy < PDA_ADAM_CACHE_AUTO || cache_policy > PDA_ADAM_CACHE_STREAM) return PDA_ERR_ARG;
    int rc = check_step(U, I, n_users, n_items, users, pos, neg, ipw, B, d, reg_div, gU, gI, tagU, tagI, step_tag, flags);
    if (rc != PDA_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (wsum_ws) {
        rc = launch_weight_sum(ipw, n_users, n_items, users, pos, neg, B, wsum_ws, s);
        if (rc != PDA_OK) return rc;
    }
    rc = launch_step(step_args(U, I, n_users, n_items, users, pos, neg, ipw, wsum_ws, B, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags,
                               loss_acc),
                     d, s);
    if (rc != PDA_OK) return rc;
    return pda_adam_dense_sweep4_f32(U, mU, vU, gU, n_users, tagU, I, mI, vI, gI, n_items, tagI, d, step_tag, lr_t, beta1, beta2, eps, cache_policy,
                                     stream);
}
