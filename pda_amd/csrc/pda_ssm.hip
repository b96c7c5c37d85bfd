// The sampled-softmax loss (include/pda_hip_ssm.h) on MI355X (gfx950): the gradient step over one positive and N sampled negatives
// per row, the sampler of the [B, N] block of negatives, and the row normalisation of a norm == 1 model's evaluation tables.  The Adam update is
// pda_adam_dense_sweep4_f32 itself.
//
// Step layout: the one of pda_bpr_step.hip -- 512 threads, d/4 lanes per row, each lane owns one float4 of every gathered row, the dots by the
// xor-shuffle ladder, 2048/d rows per workgroup.  A row's lane group walks its N + 1 item rows TWICE and keeps no logit anywhere: pass 1 takes
// the dots (under norm the rows' squared norms on the same ladder) and the running max and sum of the log-sum-exp; pass 2 gathers the rows again
// (they sit in L2), recomputes s_k by the very same expressions, forms c_k, accumulates the user gradient in registers and adds the item row's
// gradient.  The rows are gathered four at a time, ids first, so that four loads are in flight under every ladder.  The positive's gradient goes
// through the LDS scatter every step kernel shares (pda_train_common.h); the negatives are uniform draws and take atomic_add4 directly.
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_sample.h"
#include "pda_hip_ssm.h"
#include "pda_hip_negpop.h"   // (the logQ entries of the step)

namespace {

struct SsmStepArgs {
    const float* U;
    const float* I;
    const int32_t* users;
    const int32_t* pos;
    const int32_t* negs;
    float* gU;
    float* gI;
    int32_t* tagU;
    int32_t* tagI;
    float* loss_acc;
    unsigned n_users, n_items;
    int tag;
    int B, N;
    float inv_B;
    float inv_tau;
    float reg_c;            // regs / reg_div
    int any_order;          // PDA_UPD_ANY_ORDER
    int users_distinct;     // PDA_UPD_USERS_DISTINCT
};

constexpr int kChunk = 4;       // item rows gathered per round of a pass
constexpr float kNormFloor = 1e-12f;

// the sum of v over the D/4 lanes of the row's group: every lane holds it
template <int D>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int o = D / 8; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// s_k of one item row (this lane's float4 of it: ie) against the user row as the passes hold it (uq: u, under NORM u^).  cs (NORM): u^ . i^_k;
// inv_in (NORM): 1 / max(|i_k|, 1e-12).  Both passes compile THIS, so pass 2 sees the logits pass 1 summed.
template <int D, bool NORM>
__device__ __forceinline__ float ssm_logit(f32x4 uq, f32x4 ie, float inv_tau, float& cs, float& inv_in) {
    const float dt = group_sum<D>(dot4(uq, ie));
    if constexpr (NORM) {
        const float sq = group_sum<D>(dot4(ie, ie));
        inv_in = 1.f / fmaxf(sqrtf(sq), kNormFloor);
        cs = dt * inv_in;
        return cs * inv_tau;
    } else {
        cs = dt, inv_in = 1.f;
        return dt * inv_tau;
    }
}

// item k of row t: the positive for k == 0, negative k - 1 otherwise; past N (the tail of the last round) the positive again, never used
__device__ __forceinline__ int ssm_item(const int32_t* negs_row, int p, int k, int N) { return (k == 0 || k > N) ? p : negs_row[k - 1]; }

// log q of a round's kChunk items, loaded with the round's gathers; without LOGQ it holds nothing and a logit passes through unchanged
template <bool LOGQ>
struct LogqChunk {
    float v[kChunk];
    __device__ __forceinline__ void load(const float* logq, const int (&id)[kChunk]) {
#pragma unroll
        for (int j = 0; j < kChunk; ++j) v[j] = logq[id[j]];
    }
    __device__ __forceinline__ float less(float s, int j) const { return s - v[j]; }
};
template <>
struct LogqChunk<false> {
    __device__ __forceinline__ void load(const float*, const int (&)[kChunk]) {}
    __device__ __forceinline__ float less(float s, int) const { return s; }
};

// LOGQ: s_k takes - logq[item_k], the positive's own logit included (include/pda_hip_negpop.h); the value rides with the row's gather
template <int D, bool NORM, bool LOGQ = false>
__device__ __forceinline__ void ssm_step_body(const SsmStepArgs& a, const float* logq = nullptr) {
    constexpr int L = D / 4;        // lanes per row
    constexpr int TPB = 512 / L;    // rows per block
    __shared__ float red[2][8];
    __shared__ int s_pos[TPB];
    __shared__ __attribute__((aligned(16))) float s_dpe[TPB * D];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;
    const int N = a.N;

    float maxi = 0.f, sq = 0.f;
    int u = 0, p = -1;
    bool active = t < a.B;
    const int32_t* negs_row = a.negs + (size_t)(active ? t : 0) * N;
    if (active) {
        u = a.users[t], p = a.pos[t];
        // the N + 2 ids: lane e tests negatives e, e + L, ..; one ladder makes the verdict the group's
        int bad = ((unsigned)u < a.n_users && (unsigned)p < a.n_items) ? 0 : 1;
        for (int k = e; k < N; k += L) bad |= ((unsigned)negs_row[k] < a.n_items) ? 0 : 1;
#pragma unroll
        for (int o = L / 2; o > 0; o >>= 1) bad |= __shfl_xor(bad, o, 64);
        active = bad == 0;
        if (!active) p = -1;
    }
    float* ptarget = nullptr;
    if (active) {
        const f32x4 ue = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * D + 4 * e);
        f32x4 uq = ue;
        float inv_un = 1.f;
        if constexpr (NORM) {
            inv_un = 1.f / fmaxf(sqrtf(group_sum<D>(dot4(ue, ue))), kNormFloor);
            uq = ue * inv_un;
        }
        sq = dot4(ue, ue);
        // ---- pass 1: the logits' running max m and sum of exp(s_k - m); this lane's share of the squared norms
        float m = 0.f, se = 0.f, s0 = 0.f;
        for (int k0 = 0; k0 <= N; k0 += kChunk) {
            int id[kChunk];
            f32x4 ie[kChunk];
#pragma unroll
            for (int j = 0; j < kChunk; ++j) id[j] = ssm_item(negs_row, p, k0 + j, N);
#pragma unroll
            for (int j = 0; j < kChunk; ++j) ie[j] = *reinterpret_cast<const f32x4*>(a.I + (size_t)id[j] * D + 4 * e);
            LogqChunk<LOGQ> lq;
            lq.load(logq, id);
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                if (k0 + j > N) break;
                float cs, inv_in;
                const float s = lq.less(ssm_logit<D, NORM>(uq, ie[j], a.inv_tau, cs, inv_in), j);
                sq += dot4(ie[j], ie[j]);
                if (k0 + j == 0) {
                    m = s, se = 1.f, s0 = s;
                } else {
                    const float mn = fmaxf(m, s);
                    se = se * expf(m - mn) + expf(s - mn);      // (both arguments <= 0: nothing overflows)
                    m = mn;
                }
            }
        }
        // l_r = lse - s_0 = (m - s_0) + log(se) and p_k = exp(s_k - m) / se: lse = m + log(se) itself is never formed -- at |m| of several hundred its
        // float32 spacing (6e-5 at 800) would go into every p_k
        const float inv_se = 1.f / se;
        if (e == 0) maxi = -((m - s0) + logf(se));              // block_loss_terms takes -sum(maxi) / B
        // ---- pass 2: c_k, the user gradient in registers, the item rows' gradients
        const float cscale = a.inv_tau * a.inv_B;
        f32x4 gq = {0.f, 0.f, 0.f, 0.f};                        // sum_k c_k i_k (NORM: sum_k c_k i^_k)
        float proj = 0.f;                                       // (NORM) u^ . g_u^ = sum_k c_k (u^ . i^_k)
        for (int k0 = 0; k0 <= N; k0 += kChunk) {
            int id[kChunk];
            f32x4 ie[kChunk];
#pragma unroll
            for (int j = 0; j < kChunk; ++j) id[j] = ssm_item(negs_row, p, k0 + j, N);
#pragma unroll
            for (int j = 0; j < kChunk; ++j) ie[j] = *reinterpret_cast<const f32x4*>(a.I + (size_t)id[j] * D + 4 * e);
            LogqChunk<LOGQ> lq;
            lq.load(logq, id);
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                if (k0 + j > N) break;
                float cs, inv_in;
                const float s = lq.less(ssm_logit<D, NORM>(uq, ie[j], a.inv_tau, cs, inv_in), j);
                const float pk = expf(s - m) * inv_se;
                const float c = (k0 + j == 0 ? pk - 1.f : pk) * cscale;
                f32x4 die;
                if constexpr (NORM) {
                    const f32x4 ih = ie[j] * inv_in;
                    gq += c * ih;
                    proj += c * cs;
                    die = (c * inv_in) * (uq - cs * ih) + a.reg_c * ie[j];
                } else {
                    gq += c * ie[j];
                    die = c * ue + a.reg_c * ie[j];
                }
                if (k0 + j == 0) {
                    *reinterpret_cast<f32x4*>(s_dpe + g * D + 4 * e) = die;
                } else {
                    atomic_add4(a.gI + (size_t)id[j] * D + 4 * e, die);
                    if (e == 0) a.tagI[id[j]] = a.tag;
                }
            }
        }
        f32x4 due;
        if constexpr (NORM) due = inv_un * (gq - proj * uq) + a.reg_c * ue;
        else due = gq + a.reg_c * ue;
        // (the dense-gradient writes of a tagged step: pda_train_common.h has the precondition of the plain store)
        if (a.users_distinct) *reinterpret_cast<f32x4*>(a.gU + (size_t)u * D + 4 * e) = due;
        else atomic_add4(a.gU + (size_t)u * D + 4 * e, due);
        ptarget = a.gI + (size_t)p * D + 4 * e;
        if (e == 0) {                   // same value from every writer of a row: plain stores
            a.tagU[u] = a.tag;
            a.tagI[p] = a.tag;
        }
    }
    if (e == 0) s_pos[g] = p;
    __syncthreads();
    if (active && a.any_order) pos_scatter_any<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);
    else if (active && pos_run_head(s_pos, g, p)) pos_scatter_run<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);     // (grouped batch)
    block_loss_reduce(maxi, sq, red);
    if (tid == 0 && a.loss_acc) block_loss_add(red, a.inv_B, a.reg_c, a.loss_acc);
}

template <int D>
__global__ void __launch_bounds__(512) ssm_step_kernel(SsmStepArgs a) { ssm_step_body<D, false>(a); }
template <int D>
__global__ void __launch_bounds__(512) ssm_step_norm_kernel(SsmStepArgs a) { ssm_step_body<D, true>(a); }

struct SsmLogqArgs {
    SsmStepArgs a;
    const float* logq;      // f32 [n_items]
};
template <int D>
__global__ void __launch_bounds__(512) ssm_step_logq_kernel(SsmLogqArgs q) { ssm_step_body<D, false, true>(q.a, q.logq); }
template <int D>
__global__ void __launch_bounds__(512) ssm_step_norm_logq_kernel(SsmLogqArgs q) { ssm_step_body<D, true, true>(q.a, q.logq); }

// ---- the sampler: one thread per (row r, negative j) -----------------------------------------------------------------------------------------
// the pieces are pda_sample.h's (sample_block_entry); the negatives are uniform
__global__ void __launch_bounds__(64) ssm_sample_kernel(SsmSampleArgs a) {
    sample_block_entry(a, (size_t)blockIdx.x * 64 + threadIdx.x, [](const SsmSampleArgs& a, int r, uint32_t first_draw, int64_t b, int64_t e) {
        return sample_negative(a.seed, a.step, r, first_draw, (uint32_t)(a.neg_hi - a.neg_lo), a.indices, b, e,
                               [&](uint32_t x) { return a.neg_lo + (int)x; });
    });
}

// ---- Y[r] = X[r] / max(|X[r]|, 1e-12): d/4 lanes per row, the sum of squares in float64 (order: include/pda_hip_ssm.h) ---------------------------
template <int D>
__global__ void __launch_bounds__(512) ssm_normalize_kernel(const float* X, size_t n_rows, float* Y) {
    constexpr int L = D / 4;
    const size_t r = (size_t)blockIdx.x * (512 / L) + threadIdx.x / L;
    const int e = threadIdx.x % L;
    if (r >= n_rows) return;            // (whole lane groups leave: L divides 64)
    const f32x4 x = *reinterpret_cast<const f32x4*>(X + r * D + 4 * e);
    double ss = (double)x[0] * (double)x[0];
    ss += (double)x[1] * (double)x[1];
    ss += (double)x[2] * (double)x[2];
    ss += (double)x[3] * (double)x[3];
#pragma unroll
    for (int o = L / 2; o > 0; o >>= 1) ss += __shfl_xor(ss, o, 64);
    const double nrm = fmax(sqrt(ss), 1e-12);
    f32x4 y;
#pragma unroll
    for (int k = 0; k < 4; ++k) y[k] = (float)((double)x[k] / nrm);
    *reinterpret_cast<f32x4*>(Y + r * D + 4 * e) = y;
}

// (arguments checked by the callers)
int launch_step(const SsmStepArgs& a, const float* logq, int d, int norm, hipStream_t s) {
    if (logq) {
        const SsmLogqArgs q{a, logq};
        if (norm) {
            PDA_STEP_LAUNCH(ssm_step_norm_logq_kernel, d, a.B, s, q)
        } else {
            PDA_STEP_LAUNCH(ssm_step_logq_kernel, d, a.B, s, q)
        }
    } else if (norm) {
        PDA_STEP_LAUNCH(ssm_step_norm_kernel, d, a.B, s, a)
    } else {
        PDA_STEP_LAUNCH(ssm_step_kernel, d, a.B, s, a)
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

int check_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* negs, int B,
               int N, int d, float tau, int norm, float reg_div, const float* gU, const float* gI, const int32_t* tagU, const int32_t* tagI,
               int step_tag, int flags) {
    if (!U || !I || !users || !pos || !negs || !gU || !gI || !tagU || !tagI) return PDA_ERR_ARG;
    if (B <= 0 || B > (1 << 28) || !(reg_div > 0.f) || step_tag <= 0 || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (N < 1 || N > PDA_SSM_MAX_NEGS || !(tau > 0.f) || !std::isfinite(tau) || (norm != 0 && norm != 1)) return PDA_ERR_ARG;
    if (flags & ~(PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT)) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    return PDA_OK;
}

SsmStepArgs step_args(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* negs,
                      int B, int N, float tau, float regs, float reg_div, float* gU, float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags,
                      float* loss_acc) {
    return SsmStepArgs{U, I, users, pos, negs, gU, gI, tagU, tagI, loss_acc, (unsigned)n_users, (unsigned)n_items, step_tag, B, N, 1.0f / (float)B,
                       1.0f / tau, regs / reg_div, (flags & PDA_UPD_ANY_ORDER) ? 1 : 0, (flags & PDA_UPD_USERS_DISTINCT) ? 1 : 0};
}

// Both sampler entry points.  counter (pda_ssm_sample_dev): the step is read on the device; else it travels by value and the two are null.
int ssm_sample(bool counter, int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int N, const int64_t* train_indptr,
               const int32_t* train_indices, int neg_lo, int neg_hi, uint64_t seed, uint64_t step, const uint64_t* step_dev, uint64_t* step_next,
               int32_t* pos, int32_t* negs, void* stream) {
    const SsmSampleArgs a{users, user_pool, train_indptr, train_indices, pos, negs, seed, step, B, N, n_pool, gen_users, neg_lo, neg_hi,
                          step_dev, step_next};
    if (!block_sample_ok(a, counter, PDA_SSM_MAX_NEGS)) return PDA_ERR_ARG;
    const size_t n = (size_t)B * (size_t)N;             // <= 2^30: B <= 2^22, N <= 256
    hipLaunchKernelGGL(ssm_sample_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" int pda_ssm_step_logq_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                                     const int32_t* negs, const float* logq, int B, int N, int d, float tau, int norm, float regs, float reg_div,
                                     float* gU, float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags, float* loss_acc, void* stream) {
    const int rc = check_step(U, I, n_users, n_items, users, pos, negs, B, N, d, tau, norm, reg_div, gU, gI, tagU, tagI, step_tag, flags);
    if (rc != PDA_OK) return rc;
    return launch_step(step_args(U, I, n_users, n_items, users, pos, negs, B, N, tau, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags, loss_acc),
                       logq, d, norm, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_ssm_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                                const int32_t* negs, int B, int N, int d, float tau, int norm, float regs, float reg_div, float* gU, float* gI,
                                int32_t* tagU, int32_t* tagI, int step_tag, int flags, float* loss_acc, void* stream) {
    return pda_ssm_step_logq_f32(U, I, n_users, n_items, users, pos, negs, nullptr, B, N, d, tau, norm, regs, reg_div, gU, gI, tagU, tagI, step_tag,
                                 flags, loss_acc, stream);
}

extern "C" int pda_ssm_adam_step_logq_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                          float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* negs,
                                          const float* logq, int B, int N, int d, float tau, int norm, float regs, float reg_div, int step_tag,
                                          float lr_t, float beta1, float beta2, float eps, int flags, int cache_policy, float* loss_acc,
                                          void* stream) {
    if (!mU || !vU || !mI || !vI) return PDA_ERR_ARG;
    if (cache_policy < PDA_ADAM_CACHE_AUTO || cache_policy > PDA_ADAM_CACHE_STREAM) return PDA_ERR_ARG;
    int rc = check_step(U, I, n_users, n_items, users, pos, negs, B, N, d, tau, norm, reg_div, gU, gI, tagU, tagI, step_tag, flags);
    if (rc != PDA_OK) return rc;
    rc = launch_step(step_args(U, I, n_users, n_items, users, pos, negs, B, N, tau, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags, loss_acc),
                     logq, d, norm, reinterpret_cast<hipStream_t>(stream));
    if (rc != PDA_OK) return rc;
    return pda_adam_dense_sweep4_f32(U, mU, vU, gU, n_users, tagU, I, mI, vI, gI, n_items, tagI, d, step_tag, lr_t, beta1, beta2, eps, cache_policy,
                                     stream);
}

extern "C" int pda_ssm_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                     float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* negs, int B,
                                     int N, int d, float tau, int norm, float regs, float reg_div, int step_tag, float lr_t, float beta1,
                                     float beta2, float eps, int flags, int cache_policy, float* loss_acc, void* stream) {
    return pda_ssm_adam_step_logq_f32(U, mU, vU, gU, tagU, n_users, I, mI, vI, gI, tagI, n_items, users, pos, negs, nullptr, B, N, d, tau, norm, regs,
                                      reg_div, step_tag, lr_t, beta1, beta2, eps, flags, cache_policy, loss_acc, stream);
}

extern "C" int pda_ssm_sample(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int N, const int64_t* train_indptr,
                              const int32_t* train_indices, int neg_lo, int neg_hi, uint64_t seed, uint64_t step, int32_t* pos, int32_t* negs,
                              void* stream) {
    return ssm_sample(false, users, gen_users, user_pool, n_pool, B, N, train_indptr, train_indices, neg_lo, neg_hi, seed, step, nullptr, nullptr, pos,
                      negs, stream);
}

extern "C" int pda_ssm_sample_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, int N, const int64_t* train_indptr,
                                  const int32_t* train_indices, int neg_lo, int neg_hi, uint64_t seed, const uint64_t* step_dev,
                                  uint64_t* step_next, int32_t* pos, int32_t* negs, void* stream) {
    return ssm_sample(true, users, gen_users, user_pool, n_pool, B, N, train_indptr, train_indices, neg_lo, neg_hi, seed, 0, step_dev, step_next, pos,
                      negs, stream);
}

extern "C" int pda_ssm_normalize_rows_f32(const float* X, size_t n_rows, int d, float* Y, void* stream) {
    if (!X || !Y || n_rows == 0 || n_rows > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    switch (d) {
        case 32: hipLaunchKernelGGL(ssm_normalize_kernel<32>, dim3((unsigned)((n_rows + 63) / 64)), dim3(512), 0, s, X, n_rows, Y); break;
        case 64: hipLaunchKernelGGL(ssm_normalize_kernel<64>, dim3((unsigned)((n_rows + 31) / 32)), dim3(512), 0, s, X, n_rows, Y); break;
        case 128: hipLaunchKernelGGL(ssm_normalize_kernel<128>, dim3((unsigned)((n_rows + 15) / 16)), dim3(512), 0, s, X, n_rows, Y); break;
        default: hipLaunchKernelGGL(ssm_normalize_kernel<256>, dim3((unsigned)((n_rows + 7) / 8)), dim3(512), 0, s, X, n_rows, Y); break;
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
