// MACR (include/pda_hip_macr.h) on MI355X (gfx950): the gradient step of the three-branch loss, and the two small kernels its
// counterfactual inference needs in front of the bias head of pda_temp_pop.hip.  The Adam updates are pda_adam_dense_sweep4_f32 (tables) and
// pda_adam_dense_sweep2_f32 (the two branch vectors) themselves.
//
// Step layout: the one of pda_bpr_step.hip -- d/4 lanes per triplet, each lane owns one float4 of the three gathered rows and of the two
// branch vectors (two 16-byte loads per thread, the same 2 d floats for every triplet: they stay in the caches and then in registers).  The
// three branch dots ride the xor-shuffle ladder beside triplet_dots.  Equal positives inside a workgroup are summed by their first triplet
// through LDS, as there.  The branch gradients are reduced inside the workgroup -- the triplets of a wave by shuffles, the eight waves through
// LDS -- and leave it as 2 d atomics.  A kernel of its own, on the helpers every step kernel shares (pda_train_common.h).
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_hip_macr.h"

namespace {

struct MacrStepArgs {
    const float* U;
    const float* I;
    const float* w_item;
    const float* w_user;
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    float* gU;
    float* gI;
    float* gW;              // [2, d]: w_item, w_user
    int32_t* tagU;
    int32_t* tagI;
    float* loss_acc;
    unsigned n_users, n_items;
    int tag;
    int B;
    float inv_B;
    float alpha_B, beta_B;  // alpha / B, beta / B
    float alpha, beta;
    float reg_c;            // regs / reg_div
    int any_order;          // PDA_UPD_ANY_ORDER
    int users_distinct;     // PDA_UPD_USERS_DISTINCT
};

__device__ __forceinline__ float sigmoidf(float x) { return 1.f / (1.f + expf(-x)); }

// bp = <p, w_item>, bn = <n, w_item>, bu = <u, w_user> over the D/4 lanes of the group: the ladder of triplet_dots
template <int D>
__device__ __forceinline__ void branch_dots(f32x4 ue, f32x4 pe, f32x4 ne, f32x4 wi, f32x4 wu, float& bp, float& bn, float& bu) {
    bp = dot4(pe, wi), bn = dot4(ne, wi), bu = dot4(ue, wu);
#pragma unroll
    for (int o = D / 8; o > 0; o >>= 1) {
        bp += __shfl_xor(bp, o, 64);
        bn += __shfl_xor(bn, o, 64);
        bu += __shfl_xor(bu, o, 64);
    }
}

// -log(s + 1e-10) - log(1 - z + 1e-10), s and z two sigmoids (a positive and a negative): the log terms into lg (their sum, without the sign),
// and the derivatives of the NEGATED sum by s and by z
__device__ __forceinline__ void bce_pair(float s, float z, float& lg, float& d_s, float& d_z) {
    const float ps = s + 1e-10f, nz = 1.f - z + 1e-10f;         // MF/model_api.py:640-644
    lg = logf(ps) + logf(nz);
    d_s = -1.f / ps;
    d_z = 1.f / nz;
}

template <int D>
__global__ void __launch_bounds__(512) macr_step_kernel(MacrStepArgs a) {
    constexpr int L = D / 4;        // lanes per triplet
    constexpr int TPB = 512 / L;    // triplets per block
    __shared__ float red[2][2][8];
    __shared__ int s_pos[TPB];
    __shared__ __attribute__((aligned(16))) float s_dpe[TPB * D];
    __shared__ __attribute__((aligned(16))) float s_gw[8][2 * D];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;

    float lo = 0.f, li = 0.f, lu = 0.f, sq = 0.f;
    f32x4 gwi = {0.f, 0.f, 0.f, 0.f}, gwu = {0.f, 0.f, 0.f, 0.f};
    int u = 0, p = -1, n = 0;
    bool active = t < a.B;
    if (active) {
        u = a.users[t], p = a.pos[t], n = a.neg[t];
        active = triplet_ids_ok(u, p, n, a.n_users, a.n_items);
        if (!active) p = -1;
    }
    float* ptarget = nullptr;
    if (active) {
        const f32x4 wi = *reinterpret_cast<const f32x4*>(a.w_item + 4 * e);
        const f32x4 wu = *reinterpret_cast<const f32x4*>(a.w_user + 4 * e);
        const f32x4 ue = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * D + 4 * e);
        const f32x4 pe = *reinterpret_cast<const f32x4*>(a.I + (size_t)p * D + 4 * e);
        const f32x4 ne = *reinterpret_cast<const f32x4*>(a.I + (size_t)n * D + 4 * e);
        float yp, yn, bp, bn, bu;
        triplet_dots<D>(ue, pe, ne, yp, yn);
        branch_dots<D>(ue, pe, ne, wi, wu, bp, bn, bu);
        const float sp = sigmoidf(bp), sn = sigmoidf(bn), su = sigmoidf(bu);
        const float ap = yp * sp * su, an = yn * sn * su;        // :633-634
        const float zp = sigmoidf(ap), zn = sigmoidf(an);
        float lgo, lgi, lgu, dzp, dzn, dsp, dsn, dsu_p, dsu_n;
        bce_pair(zp, zn, lgo, dzp, dzn);                          // L_O  :640
        bce_pair(sp, sn, lgi, dsp, dsn);                          // L_I  :642
        bce_pair(su, su, lgu, dsu_p, dsu_n);                      // L_U  :644
        if (e == 0) lo = lgo, li = lgi, lu = lgu;
        // d loss / d a_p, d loss / d a_n (the mean's 1 / B inside)
        const float gap = a.inv_B * dzp * (zp * (1.f - zp)), gan = a.inv_B * dzn * (zn * (1.f - zn));
        // d loss / d y_p and MINUS d loss / d y_n: what triplet_row_grads takes
        const float gp = gap * (sp * su), gn = -(gan * (sn * su));
        // d loss / d (branch dot): the chain through a_p / a_n plus the branch's own loss term, times the sigmoid's slope
        const float hp = (gap * (yp * su) + a.alpha_B * dsp) * (sp * (1.f - sp));
        const float hn = (gan * (yn * su) + a.alpha_B * dsn) * (sn * (1.f - sn));
        const float hu = (gap * (yp * sp) + gan * (yn * sn) + a.beta_B * (dsu_p + dsu_n)) * (su * (1.f - su));
        sq = triplet_sq(ue, pe, ne);
        f32x4 due, dpe, dne;
        triplet_row_grads(ue, pe, ne, gp, gn, a.reg_c, due, dpe, dne);
        due += hu * wu;
        dpe += hp * wi;
        dne += hn * wi;
        gwi = hp * pe + hn * ne;
        gwu = hu * ue;
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
    // the branch gradients of the wave's triplets onto its first L lanes (a triplet off the batch holds zeros), then one row of LDS per wave
#pragma unroll
    for (int o = 32; o >= L; o >>= 1) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            gwi[k] += __shfl_xor(gwi[k], o, 64);
            gwu[k] += __shfl_xor(gwu[k], o, 64);
        }
    }
    if ((tid & 63) < L) {
        *reinterpret_cast<f32x4*>(&s_gw[tid >> 6][4 * e]) = gwi;
        *reinterpret_cast<f32x4*>(&s_gw[tid >> 6][D + 4 * e]) = gwu;
    }
    __syncthreads();
    if (active && a.any_order) pos_scatter_any<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);
    else if (active && pos_run_head(s_pos, g, p)) pos_scatter_run<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);     // (grouped batch)
    // the workgroup's 2 d branch gradients: waves 0 .. 7 in order, one atomic per element (a wave of L == 64 lanes holds one triplet, so
    // with D == 256 every wave wrote its row; below, too -- every wave has lanes < L)
    if (tid < 2 * D) {
        float s = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) s += s_gw[w][tid];
        if (s != 0.f) unsafeAtomicAdd(a.gW + tid, s);
    }
    block_loss_reduce(lo, sq, red[0]);
    block_loss_reduce(li, lu, red[1]);
    if (tid == 0 && a.loss_acc) {
        float so = 0.f, ss = 0.f, si = 0.f, su = 0.f;
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            so += red[0][0][w];
            ss += red[0][1][w];
            si += red[1][0][w];
            su += red[1][1][w];
        }
        const float LO = -so * a.inv_B, LI = -si * a.inv_B, LU = -su * a.inv_B, rg = a.reg_c * 0.5f * ss;
        unsafeAtomicAdd(a.loss_acc + 0, LO + a.alpha * LI + a.beta * LU + rg);
        unsafeAtomicAdd(a.loss_acc + 1, LO);
        unsafeAtomicAdd(a.loss_acc + 2, LI);
        unsafeAtomicAdd(a.loss_acc + 3, LU);
        unsafeAtomicAdd(a.loss_acc + 4, rg);
    }
}

// 256 threads, d/4 lanes per item row
template <int D>
__global__ void __launch_bounds__(256) macr_item_prep_kernel(const float* __restrict__ I, const float* __restrict__ w_item, size_t n_items,
                                                             float* __restrict__ sig, float* __restrict__ J) {
    constexpr int L = D / 4, RPB = 256 / L;
    const int e = threadIdx.x % L;
    const size_t i = (size_t)blockIdx.x * RPB + threadIdx.x / L;
    // (a row off the table computes on zeros and stores nothing: every lane of a wave reaches the shuffles)
    const bool live = i < n_items;
    const f32x4 wi = *reinterpret_cast<const f32x4*>(w_item + 4 * e);
    f32x4 row = {0.f, 0.f, 0.f, 0.f};
    if (live) row = *reinterpret_cast<const f32x4*>(I + i * D + 4 * e);
    float b = dot4(row, wi);
#pragma unroll
    for (int o = D / 8; o > 0; o >>= 1) b += __shfl_xor(b, o, 64);
    const float s = sigmoidf(b);
    if (live) {
        *reinterpret_cast<f32x4*>(J + i * D + 4 * e) = s * row;
        if (e == 0) sig[i] = s;
    }
}

__global__ void __launch_bounds__(256) macr_item_bias_kernel(const float* __restrict__ sig, float neg_c, float* __restrict__ beta, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) beta[i] = neg_c * sig[i];
}

int launch_step(const MacrStepArgs& a, int d, hipStream_t s) {
    PDA_STEP_LAUNCH(macr_step_kernel, d, a.B, s, a)
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

int check_step(const float* U, const float* I, const float* w_item, const float* w_user, size_t n_users, size_t n_items, const int32_t* users,
               const int32_t* pos, const int32_t* neg, int B, int d, float alpha, float beta, float reg_div, const float* gU, const float* gI,
               const float* gW, const int32_t* tagU, const int32_t* tagI, int step_tag, int flags) {
    if (!U || !I || !w_item || !w_user || !users || !pos || !neg || !gU || !gI || !gW || !tagU || !tagI) return PDA_ERR_ARG;
    if (B <= 0 || B > (1 << 28) || !(reg_div > 0.f) || step_tag <= 0 || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (!std::isfinite(alpha) || !std::isfinite(beta)) return PDA_ERR_ARG;
    if (flags & ~(PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT)) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    return PDA_OK;
}

MacrStepArgs step_args(const float* U, const float* I, const float* w_item, const float* w_user, size_t n_users, size_t n_items,
                       const int32_t* users, const int32_t* pos, const int32_t* neg, int B, float alpha, float beta, float regs, float reg_div,
                       float* gU, float* gI, float* gW, int32_t* tagU, int32_t* tagI, int step_tag, int flags, float* loss_acc) {
    const float inv_B = 1.0f / (float)B;
    return MacrStepArgs{U, I, w_item, w_user, users, pos, neg, gU, gI, gW, tagU, tagI, loss_acc, (unsigned)n_users, (unsigned)n_items, step_tag, B,
                        inv_B, alpha * inv_B, beta * inv_B, alpha, beta, regs / reg_div, (flags & PDA_UPD_ANY_ORDER) ? 1 : 0,
                        (flags & PDA_UPD_USERS_DISTINCT) ? 1 : 0};
}

}  // namespace

extern "C" int pda_macr_step_f32(const float* U, const float* I, const float* w_item, const float* w_user, size_t n_users, size_t n_items,
                                 const int32_t* users, const int32_t* pos, const int32_t* neg, int B, int d, float alpha, float beta, float regs,
                                 float reg_div, float* gU, float* gI, float* gW, int32_t* tagU, int32_t* tagI, int step_tag, int flags,
                                 float* loss_acc, void* stream) {
    const int rc = check_step(U, I, w_item, w_user, n_users, n_items, users, pos, neg, B, d, alpha, beta, reg_div, gU, gI, gW, tagU, tagI, step_tag,
                              flags);
    if (rc != PDA_OK) return rc;
    return launch_step(step_args(U, I, w_item, w_user, n_users, n_items, users, pos, neg, B, alpha, beta, regs, reg_div, gU, gI, gW, tagU, tagI,
                                 step_tag, flags, loss_acc),
                       d, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_macr_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                      float* gI, int32_t* tagI, size_t n_items, float* w_item, float* w_user, float* mW, float* vW, float* gW,
                                      const int32_t* users, const int32_t* pos, const int32_t* neg, int B, int d, float alpha, float beta,
                                      float regs, float reg_div, int step_tag, float lr_t, float beta1, float beta2, float eps, int flags,
                                      int cache_policy, float* loss_acc, void* stream) {
    if (!mU || !vU || !mI || !vI || !mW || !vW) return PDA_ERR_ARG;
    if (cache_policy < PDA_ADAM_CACHE_AUTO || cache_policy > PDA_ADAM_CACHE_STREAM) return PDA_ERR_ARG;
    int rc = check_step(U, I, w_item, w_user, n_users, n_items, users, pos, neg, B, d, alpha, beta, reg_div, gU, gI, gW, tagU, tagI, step_tag, flags);
    if (rc != PDA_OK) return rc;
    rc = launch_step(step_args(U, I, w_item, w_user, n_users, n_items, users, pos, neg, B, alpha, beta, regs, reg_div, gU, gI, gW, tagU, tagI,
                               step_tag, flags, loss_acc),
                     d, reinterpret_cast<hipStream_t>(stream));
    if (rc != PDA_OK) return rc;
    rc = pda_adam_dense_sweep4_f32(U, mU, vU, gU, n_users, tagU, I, mI, vI, gI, n_items, tagI, d, step_tag, lr_t, beta1, beta2, eps, cache_policy,
                                   stream);
    if (rc != PDA_OK) return rc;
    return pda_adam_dense_sweep2_f32(w_item, mW, vW, gW, (size_t)d, w_user, mW + d, vW + d, gW + d, (size_t)d, lr_t, beta1, beta2, eps, stream);
}

extern "C" int pda_macr_item_prep_f32(const float* I, const float* w_item, size_t n_items, int d, float* sig, float* J, void* stream) {
    if (!I || !w_item || !sig || !J || n_items == 0 || n_items > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (d) {
#define PDA_MACR_PREP(DD)                                                                                                                   \
    hipLaunchKernelGGL(macr_item_prep_kernel<DD>, dim3((unsigned)((n_items + 256 / (DD / 4) - 1) / (256 / (DD / 4)))), dim3(256), 0, s, I, \
                       w_item, n_items, sig, J);                                                                                            \
    break;
        case 32: PDA_MACR_PREP(32)
        case 64: PDA_MACR_PREP(64)
        case 128: PDA_MACR_PREP(128)
        default: PDA_MACR_PREP(256)
#undef PDA_MACR_PREP
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_macr_item_bias_f32(const float* sig, float c, float* beta, size_t n, void* stream) {
    if (!sig || !beta || n == 0 || n > 0x7FFFFFFFu || !std::isfinite(c)) return PDA_ERR_ARG;
    hipLaunchKernelGGL(macr_item_bias_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), sig, -c,
                       beta, n);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
