// The popularity-correlation regulariser on the BPR loss (include/pda_hip_pcc.h) on MI355X (gfx950): the gradient of every triplet
// depends on a statistic of the whole batch -- Pearson's r between a score and the positive's popularity -- and the statistic depends on the
// scores.  Three launches in front of pda_adam_dense_sweep4_f32:
//   score    the step layout (d/4 lanes per triplet, the xor-shuffle ladder of triplet_dots): z_t -> z_ws
//   moments  ONE workgroup of 1 024 threads: the centred moments of (z_t, pop[p_t]) in float64, in a fixed order, no atomics -> stat
//   step     the gradient kernel of pda_ips.hip with a per-triplet coefficient d (gamma r^2) / d z_t on top of the BPR one, from z_ws and stat
// The step gathers the three rows a second time; what that costs beside the IPS-CN step is measured in profiles/pcc_timing.txt.
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_hip_pcc.h"

namespace {

struct PccScoreArgs {
    const float* U;
    const float* I;
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    float* z_ws;
    unsigned n_users, n_items;
    int B;
    int margin;             // PDA_PCC_ON_MARGIN
};

struct PccStepArgs {
    const float* U;
    const float* I;
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    const float* pop;
    const float* z_ws;
    const double* stat;
    float* gU;
    float* gI;
    int32_t* tagU;
    int32_t* tagI;
    float* loss_acc;
    float* pcc_acc;
    unsigned n_users, n_items;
    int tag;
    int B;
    float inv_B;
    float gamma;
    float reg_c;            // regs / reg_div
    int margin;             // PDA_PCC_ON_MARGIN
    int any_order;          // PDA_UPD_ANY_ORDER
    int users_distinct;     // PDA_UPD_USERS_DISTINCT
};

template <int D>
__global__ void __launch_bounds__(512) pcc_score_kernel(PccScoreArgs a) {
    constexpr int L = D / 4;        // lanes per triplet
    constexpr int TPB = 512 / L;    // triplets per block
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;
    if (t >= a.B) return;           // (no barrier below; L divides 64, so the lanes of a triplet leave together)
    const int u = a.users[t], p = a.pos[t], n = a.neg[t];
    float z = 0.f;                  // a refused triplet: the moments and the step test the ids themselves
    if (triplet_ids_ok(u, p, n, a.n_users, a.n_items)) {
        const f32x4 ue = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * D + 4 * e);
        const f32x4 pe = *reinterpret_cast<const f32x4*>(a.I + (size_t)p * D + 4 * e);
        const f32x4 ne = *reinterpret_cast<const f32x4*>(a.I + (size_t)n * D + 4 * e);
        float ps, ns;
        triplet_dots<D>(ue, pe, ne, ps, ns);
        z = a.margin ? ps - ns : ps;
    }
    if (e == 0) a.z_ws[t] = z;
}

// The sum of three float64 over the 1 024 threads of the workgroup in a fixed order (wave: xor ladder; workgroup: waves 0 .. 15); every thread
// returns with the three sums.  part: __shared__ double [3][16].
__device__ __forceinline__ void block_sum3(double& a, double& b, double& c, double (&part)[3][16]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
        c += __shfl_xor(c, o, 64);
    }
    __syncthreads();                // (the readers of the call before are through)
    if ((threadIdx.x & 63) == 0) {
        part[0][threadIdx.x >> 6] = a;
        part[1][threadIdx.x >> 6] = b;
        part[2][threadIdx.x >> 6] = c;
    }
    __syncthreads();
    a = b = c = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) {
        a += part[0][w];
        b += part[1][w];
        c += part[2][w];
    }
}

// One workgroup of 1 024 threads, two passes over the batch (thread: t = tid, tid + 1024, ... in that order): the means, then the centred sums.
// Centring makes the degenerate cases exact: n_v copies of one float sum and divide back to that float in float64, so Sqq = 0 when every positive
// has one popularity, and Szz = 0 when n_v = 1.
__global__ void __launch_bounds__(1024) pcc_moments_kernel(const float* __restrict__ z_ws, const float* __restrict__ pop,
                                                           const int32_t* __restrict__ users, const int32_t* __restrict__ pos,
                                                           const int32_t* __restrict__ neg, int B, unsigned n_users, unsigned n_items,
                                                           double* __restrict__ stat) {
    __shared__ double part[3][16];
    double nv = 0.0, sz = 0.0, sq = 0.0;
    for (int t = (int)threadIdx.x; t < B; t += 1024) {
        const int u = users[t], p = pos[t], n = neg[t];
        if (triplet_ids_ok(u, p, n, n_users, n_items)) {
            nv += 1.0;
            sz += (double)z_ws[t];
            sq += (double)pop[p];
        }
    }
    block_sum3(nv, sz, sq, part);
    const double zbar = nv > 0.0 ? sz / nv : 0.0, qbar = nv > 0.0 ? sq / nv : 0.0;
    double szz = 0.0, sqq = 0.0, szq = 0.0;
    // (the second pass reads the batch again: keeping a thread's first four triplets in registers instead did not shorten it, profiles/pcc_timing.txt)
    for (int t = (int)threadIdx.x; t < B; t += 1024) {
        const int u = users[t], p = pos[t], n = neg[t];
        if (triplet_ids_ok(u, p, n, n_users, n_items)) {
            const double dz = (double)z_ws[t] - zbar, dq = (double)pop[p] - qbar;
            szz += dz * dz;
            sqq += dq * dq;
            szq += dz * dq;
        }
    }
    block_sum3(szz, sqq, szq, part);
    if (threadIdx.x == 0) {
        const double r = (nv >= 2.0 && szz > 0.0 && sqq > 0.0) ? szq / sqrt(szz * sqq) : 0.0;
        stat[0] = nv;
        stat[1] = zbar;
        stat[2] = qbar;
        stat[3] = szz;
        stat[4] = sqq;
        stat[5] = szq;
        stat[6] = r;
        stat[7] = 0.0;
    }
}

template <int D>
__global__ void __launch_bounds__(512) pcc_step_kernel(PccStepArgs a) {
    constexpr int L = D / 4;        // lanes per triplet
    constexpr int TPB = 512 / L;    // triplets per block
    __shared__ float red[2][8];
    __shared__ int s_pos[TPB];
    __shared__ __attribute__((aligned(16))) float s_dpe[TPB * D];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;

    // the batch's statistic (uniform over the grid): d pen / d z_t = ca ((q_t - qbar) - cb (z_t - zbar)); r == 0 by rule leaves the BPR step
    const double zbar = a.stat[1], qbar = a.stat[2], r = a.stat[6];
    double ca = 0.0, cb = 0.0;
    if (r != 0.0) {
        const double szz = a.stat[3], sqq = a.stat[4], szq = a.stat[5];
        ca = 2.0 * (double)a.gamma * r / sqrt(szz * sqq);
        cb = szq / szz;
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
        const double zt = (double)a.z_ws[t], qt = (double)a.pop[p];       // the bits the moments were taken from
        const float ct = (float)(ca * ((qt - qbar) - cb * (zt - zbar)));
        const f32x4 ue = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * D + 4 * e);
        const f32x4 pe = *reinterpret_cast<const f32x4*>(a.I + (size_t)p * D + 4 * e);
        const f32x4 ne = *reinterpret_cast<const f32x4*>(a.I + (size_t)n * D + 4 * e);
        float ps, ns;
        triplet_dots<D>(ue, pe, ne, ps, ns);
        const float gg = bpr_dloss_dx(ps - ns, a.inv_B, e, maxi);
        sq = triplet_sq(ue, pe, ne);
        // d loss / d s_p = gg + ct; -d loss / d s_n = gg (pos: the penalty does not see the negative) or gg + ct (margin: z = s_p - s_n)
        const float gp = gg + ct, gn = a.margin ? gp : gg;
        f32x4 due, dpe, dne;
        triplet_row_grads(ue, pe, ne, gp, gn, a.reg_c, due, dpe, dne);
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
    if (tid == 0) {
        if (a.loss_acc) block_loss_add(red, a.inv_B, a.reg_c, a.loss_acc);
        if (blockIdx.x == 0) {          // once per step, not once per workgroup: the penalty and the epoch's record of r
            const float pen = (float)((double)a.gamma * r * r);
            if (a.loss_acc) {
                unsafeAtomicAdd(a.loss_acc + 0, pen);
                unsafeAtomicAdd(a.loss_acc + 1, pen);
            }
            if (a.pcc_acc) {
                unsafeAtomicAdd(a.pcc_acc + 0, (float)r);
                unsafeAtomicAdd(a.pcc_acc + 1, (float)(r * r));
            }
        }
    }
}

// (arguments checked by the callers)
int launch_stats(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                 const float* pop, int B, int d, int on, float* z_ws, double* stat, hipStream_t s) {
    const PccScoreArgs a{U, I, users, pos, neg, z_ws, (unsigned)n_users, (unsigned)n_items, B, on == PDA_PCC_ON_MARGIN ? 1 : 0};
    PDA_STEP_LAUNCH(pcc_score_kernel, d, B, s, a)
    PDA_CHECK_LAUNCH();
    hipLaunchKernelGGL(pcc_moments_kernel, dim3(1), dim3(1024), 0, s, (const float*)z_ws, pop, users, pos, neg, B, (unsigned)n_users,
                       (unsigned)n_items, stat);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

int launch_step(const PccStepArgs& a, int d, hipStream_t s) {
    PDA_STEP_LAUNCH(pcc_step_kernel, d, a.B, s, a)
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

int check_stats(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                const float* pop, int B, int d, int on, const float* z_ws, const double* stat) {
    if (!U || !I || !users || !pos || !neg || !pop || !z_ws || !stat) return PDA_ERR_ARG;
    if (B <= 0 || B > (1 << 28) || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (on != PDA_PCC_ON_POS && on != PDA_PCC_ON_MARGIN) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    return PDA_OK;
}

int check_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
               const float* pop, const float* z_ws, const double* stat, int B, int d, float gamma, int on, float reg_div, const float* gU,
               const float* gI, const int32_t* tagU, const int32_t* tagI, int step_tag, int flags) {
    if (!gU || !gI || !tagU || !tagI) return PDA_ERR_ARG;
    if (!(gamma >= 0.f) || !(reg_div > 0.f) || step_tag <= 0) return PDA_ERR_ARG;
    if (flags & ~(PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT)) return PDA_ERR_ARG;
    return check_stats(U, I, n_users, n_items, users, pos, neg, pop, B, d, on, z_ws, stat);
}

PccStepArgs step_args(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                      const float* pop, const float* z_ws, const double* stat, int B, float gamma, int on, float regs, float reg_div, float* gU,
                      float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags, float* loss_acc, float* pcc_acc) {
    return PccStepArgs{U, I, users, pos, neg, pop, z_ws, stat, gU, gI, tagU, tagI, loss_acc, pcc_acc, (unsigned)n_users, (unsigned)n_items,
                       step_tag, B, 1.0f / (float)B, gamma, regs / reg_div, on == PDA_PCC_ON_MARGIN ? 1 : 0, (flags & PDA_UPD_ANY_ORDER) ? 1 : 0,
                       (flags & PDA_UPD_USERS_DISTINCT) ? 1 : 0};
}

}  // namespace

extern "C" int pda_pcc_stats_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                                 const int32_t* neg, const float* pop, int B, int d, int on, float* z_ws, double* stat, void* stream) {
    const int rc = check_stats(U, I, n_users, n_items, users, pos, neg, pop, B, d, on, z_ws, stat);
    if (rc != PDA_OK) return rc;
    return launch_stats(U, I, n_users, n_items, users, pos, neg, pop, B, d, on, z_ws, stat, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_pcc_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                                const int32_t* neg, const float* pop, const float* z_ws, const double* stat, int B, int d, float gamma, int on,
                                float regs, float reg_div, float* gU, float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags,
                                float* loss_acc, float* pcc_acc, void* stream) {
    const int rc = check_step(U, I, n_users, n_items, users, pos, neg, pop, z_ws, stat, B, d, gamma, on, reg_div, gU, gI, tagU, tagI, step_tag, flags);
    if (rc != PDA_OK) return rc;
    return launch_step(step_args(U, I, n_users, n_items, users, pos, neg, pop, z_ws, stat, B, gamma, on, regs, reg_div, gU, gI, tagU, tagI, step_tag,
                                 flags, loss_acc, pcc_acc),
                       d, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_pcc_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                     float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                                     const float* pop, float* z_ws, double* stat, int B, int d, float gamma, int on, float regs, float reg_div,
                                     int step_tag, float lr_t, float beta1, float beta2, float eps, int flags, int cache_policy, float* loss_acc,
                                     float* pcc_acc, void* stream) {
    if (!mU || !vU || !mI || !vI) return PDA_ERR_ARG;
    if (cache_policy < PDA_ADAM_CACHE_AUTO || cache_policy > PDA_ADAM_CACHE_STREAM) return PDA_ERR_ARG;
    int rc = check_step(U, I, n_users, n_items, users, pos, neg, pop, z_ws, stat, B, d, gamma, on, reg_div, gU, gI, tagU, tagI, step_tag, flags);
    if (rc != PDA_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    rc = launch_stats(U, I, n_users, n_items, users, pos, neg, pop, B, d, on, z_ws, stat, s);
    if (rc != PDA_OK) return rc;
    rc = launch_step(step_args(U, I, n_users, n_items, users, pos, neg, pop, z_ws, stat, B, gamma, on, regs, reg_div, gU, gI, tagU, tagI, step_tag,
                               flags, loss_acc, pcc_acc),
                     d, s);
    if (rc != PDA_OK) return rc;
    return pda_adam_dense_sweep4_f32(U, mU, vU, gU, n_users, tagU, I, mI, vI, gI, n_items, tagI, d, step_tag, lr_t, beta1, beta2, eps, cache_policy,
                                     stream);
}
