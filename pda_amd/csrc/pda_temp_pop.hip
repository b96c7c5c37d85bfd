// BPRMF(t)-pop (MF/model_api.py:300-416) on MI355X (gfx950): the fused gradient step of the four tables and the dense-decay Adam sweep
// over all of them -- two launches per reference step, like pda_adam_step_f32 -- plus the C entry point of the bias-head score kernel
// (the kernel itself is generation 1's template, pda_score_topk.hip).
//
// Step layout: the one of pda_bpr_step.hip (d/4 lanes per triplet, each lane owns one float4 of the three gathered rows, dots by xor-shuffle
// inside the lane group).  The bias terms are four scalars of C and one of bu per triplet: every lane of the group loads them (same address,
// one transaction) and lane 0 of the group scatters their gradients.  Equal positives inside a workgroup are summed by their first
// triplet (the LDS combine of pda_bpr_step.hip's PDA_UPD_ANY_ORDER): a hot item then costs one atomic per element per workgroup, for its
// embedding row and for its init-bias column C[p, T].
#include <cmath>
#include <cstdlib>
#include <cstring>
#include "pda_common.h"
#include "pda_topk_common.h"
#include "pda_train_common.h"
#include "pda_hip_temp_pop.h"

namespace {

struct TPStepArgs {
    const float* U;
    const float* I;
    const float* bu;
    const float* C;
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    const float* temps;
    float* gU;
    float* gI;
    float* gbu;
    float* gC;
    int32_t* tagU;
    int32_t* tagI;
    float* loss_acc;
    int tag;
    int B;
    int T;
    float inv_B;
    float reg_c;   // regs / reg_div
};

template <int D>
__global__ void __launch_bounds__(512) temp_pop_step_kernel(TPStepArgs a) {
    constexpr int L = D / 4;        // lanes per triplet
    constexpr int TPB = 512 / L;    // triplets per block
    __shared__ float red[2][8];
    __shared__ int s_pos[TPB];
    __shared__ float s_gb[TPB];
    __shared__ __attribute__((aligned(16))) float s_dpe[TPB * D];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;
    const bool active = t < a.B;
    const int W = a.T + 1;          // columns of C

    float maxi = 0.f, sq = 0.f;
    int p = -1;
    if (active) {
        const int u = a.users[t], n = a.neg[t];
        p = a.pos[t];
        int ts = (int)a.temps[t];                       // tf.cast(temp, tf.int32): the slot travels as a float (MF/train_new_api.py:575)
        ts = ts < 0 ? 0 : (ts >= a.T ? a.T - 1 : ts);   // (memory safety only: the loaders refuse slots >= T)
        const f32x4 ue = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * D + 4 * e);
        const f32x4 pe = *reinterpret_cast<const f32x4*>(a.I + (size_t)p * D + 4 * e);
        const f32x4 ne = *reinterpret_cast<const f32x4*>(a.I + (size_t)n * D + 4 * e);
        const float cpT = a.C[(size_t)p * W + a.T], cpt = a.C[(size_t)p * W + ts];
        const float cnT = a.C[(size_t)n * W + a.T], cnt = a.C[(size_t)n * W + ts];
        // quirk 1: user_temp_bias_all is [B, 1] and gather_nd reads it at (raw, temp) -- in range only for temp == 0; TF's GPU kernel returns 0
        // out of range and drops the gradient (MF/model_api.py:342-343)
        const float bt = ts == 0 ? a.bu[u] : 0.f;
        float ps, ns;
        triplet_dots<D>(ue, pe, ne, ps, ns);
        sq = triplet_sq(ue, pe, ne);
        // TF's op order (:355-364): ub = b~ + 1, pb = init + temp, s = ub * pb + preference
        const float ub = bt + 1.0f;
        const float pb = cpT + cpt, nb = cnT + cnt;
        const float sp = ub * pb + ps, sn = ub * nb + ns;
        const float gg = bpr_dloss_dx(sp - sn, a.inv_B, e, maxi);  // :367
        f32x4 due, dpe, dne;
        triplet_row_grads(ue, pe, ne, gg, gg, a.reg_c, due, dpe, dne);
        atomic_add4(a.gU + (size_t)u * D + 4 * e, due);
        atomic_add4(a.gI + (size_t)n * D + 4 * e, dne);
        *reinterpret_cast<f32x4*>(s_dpe + g * D + 4 * e) = dpe;
        const float gb = gg * ub;                                 // d loss / d pb;  d loss / d nb = -gb
        if (e == 0) {
            s_gb[g] = gb;
            unsafeAtomicAdd(a.gC + (size_t)p * W + ts, gb);
            unsafeAtomicAdd(a.gC + (size_t)n * W + a.T, -gb);
            unsafeAtomicAdd(a.gC + (size_t)n * W + ts, -gb);
            if (ts == 0) unsafeAtomicAdd(a.gbu + u, gg * pb - gg * nb);
            a.tagU[u] = a.tag;                                    // same value from every writer of a row: plain stores
            a.tagI[p] = a.tag;
            a.tagI[n] = a.tag;
        }
    }
    if (e == 0) s_pos[g] = p;
    __syncthreads();
    if (active) {
        // the first triplet of the workgroup with this positive sums all the workgroup's contributions to its row and to C[p, T]: pos_scatter_any
        // (pda_train_common.h) with the second LDS array summed in the same loop
        bool leader = true;
        for (int k = 0; k < g; ++k) leader = leader && (s_pos[k] != p);
        if (leader) {
            f32x4 sum = *reinterpret_cast<const f32x4*>(s_dpe + g * D + 4 * e);
            float gsum = s_gb[g];
            for (int k = g + 1; k < TPB; ++k)
                if (s_pos[k] == p) {
                    sum += *reinterpret_cast<const f32x4*>(s_dpe + k * D + 4 * e);
                    gsum += s_gb[k];
                }
            atomic_add4(a.gI + (size_t)p * D + 4 * e, sum);
            if (e == 0) unsafeAtomicAdd(a.gC + (size_t)p * W + a.T, gsum);
        }
    }
    block_loss_reduce(maxi, sq, red);
    if (tid == 0 && a.loss_acc) block_loss_add(red, a.inv_B, a.reg_c, a.loss_acc);     // (l2 of the three EMBEDDING rows: the biases take none, :370-373)
}

// TF-1.14 dense-decay Adam over the four tables (adam_elem, pda_train_common.h); g is read only on tagged rows.

struct TPSweepArgs {
    float* x[4];
    float* m[4];
    float* v[4];
    float* g[4];
    const int32_t* tag[4];
    size_t n[4];          // units: float4 chunks (embedding tables), floats (bias tables)
    int row_div[4];       // units per table row
    unsigned blk_end[4];  // workgroups [blk_end[s - 1], blk_end[s]) sweep table s
    int tag_now;
    float lr_t, b1, b2, eps;
};

__global__ void __launch_bounds__(256) temp_pop_sweep_kernel(TPSweepArgs a) {
    int s = 0;
    while (s < 3 && blockIdx.x >= a.blk_end[s]) ++s;
    const unsigned b0 = s == 0 ? 0u : a.blk_end[s - 1];
    const size_t stride = (size_t)(a.blk_end[s] - b0) * blockDim.x;
    float* X = a.x[s];
    float* M = a.m[s];
    float* V = a.v[s];
    float* G = a.g[s];
    const int32_t* tg = a.tag[s];
    const int rd = a.row_div[s];
    const size_t n = a.n[s];
    if (s < 2) {
        for (size_t i = (size_t)(blockIdx.x - b0) * blockDim.x + threadIdx.x; i < n; i += stride) {
            const bool touched = tg[i / (size_t)rd] == a.tag_now;
            f32x4 gg = {0.f, 0.f, 0.f, 0.f};
            if (touched) gg = reinterpret_cast<const f32x4*>(G)[i];
            f32x4 xx = reinterpret_cast<f32x4*>(X)[i], mm = reinterpret_cast<f32x4*>(M)[i], vv = reinterpret_cast<f32x4*>(V)[i];
            adam_elem(xx, mm, vv, gg, a.lr_t, a.b1, a.b2, a.eps);
            reinterpret_cast<f32x4*>(M)[i] = mm;
            reinterpret_cast<f32x4*>(V)[i] = vv;
            reinterpret_cast<f32x4*>(X)[i] = xx;
            if (touched) reinterpret_cast<f32x4*>(G)[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
    } else {
        for (size_t i = (size_t)(blockIdx.x - b0) * blockDim.x + threadIdx.x; i < n; i += stride) {
            const bool touched = tg[i / (size_t)rd] == a.tag_now;
            const float gg = touched ? G[i] : 0.f;
            float xx = X[i], mm = M[i], vv = V[i];
            adam_elem(xx, mm, vv, gg, a.lr_t, a.b1, a.b2, a.eps);
            M[i] = mm;
            V[i] = vv;
            X[i] = xx;
            if (touched) G[i] = 0.f;
        }
    }
}

int launch_temp_pop_step(const TPStepArgs& a, int d, hipStream_t s) {
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    PDA_STEP_LAUNCH(temp_pop_step_kernel, d, a.B, s, a)
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

int launch_temp_pop_sweep(TPSweepArgs& a, hipStream_t s) {
    // workgroups in proportion to the work units of each table (a float4 chunk of U / I, a float of bu / C: one unit per thread and
    // iteration either way; 7 workgroups per CU in all, like pda_adam_step_f32's sweep), at least one per table and no more than it has work
    // for.  (In proportion to BYTES the bias tables got a quarter of that: their threads ran four times as many dependent scalar iterations
    // and the sweep ended on their tail -- 24.3 against 18.3 us for pda_adam_step_f32's sweep at Douban shape, profiles/temp_pop_step.txt.)
    const unsigned total = 256u * 7u;
    double sum = 0.0;
    for (int q = 0; q < 4; ++q) sum += (double)a.n[q];
    unsigned end = 0;
    for (int q = 0; q < 4; ++q) {
        size_t want = (a.n[q] + 255) / 256;
        size_t share = (size_t)((double)total * (double)a.n[q] / sum);
        share = share < 1 ? 1 : share;
        end += (unsigned)(want < share ? want : share);
        a.blk_end[q] = end;
    }
    hipLaunchKernelGGL(temp_pop_sweep_kernel, dim3(end), dim3(256), 0, s, a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" int pda_temp_pop_step_f32(const float* U, const float* I, const float* bu, const float* C, const int32_t* users, const int32_t* pos,
                                     const int32_t* neg, const float* temps, int B, int d, int T, float regs, float reg_div, float* gU, float* gI,
                                     float* gbu, float* gC, int32_t* tagU, int32_t* tagI, int step_tag, float* loss_acc, void* stream) {
    if (!U || !I || !bu || !C || !users || !pos || !neg || !temps || !gU || !gI || !gbu || !gC || !tagU || !tagI) return PDA_ERR_ARG;
    if (B <= 0 || T < 1 || reg_div <= 0.f || step_tag <= 0) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    TPStepArgs a{U, I, bu, C, users, pos, neg, temps, gU, gI, gbu, gC, tagU, tagI, loss_acc, step_tag, B, T, 1.0f / (float)B, regs / reg_div};
    return launch_temp_pop_step(a, d, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_temp_pop_sweep_f32(float* U, float* mU, float* vU, float* gU, const int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                      float* gI, const int32_t* tagI, size_t n_items, float* bu, float* mbu, float* vbu, float* gbu, float* C, float* mC,
                                      float* vC, float* gC, int d, int T, int step_tag, float lr_t, float beta1, float beta2, float eps, void* stream) {
    if (!U || !mU || !vU || !gU || !tagU || !I || !mI || !vI || !gI || !tagI || !bu || !mbu || !vbu || !gbu || !C || !mC || !vC || !gC)
        return PDA_ERR_ARG;
    if (n_users == 0 || n_items == 0 || T < 1 || step_tag <= 0) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    TPSweepArgs a{{U, I, bu, C}, {mU, mI, mbu, mC}, {vU, vI, vbu, vC}, {gU, gI, gbu, gC}, {tagU, tagI, tagU, tagI},
                  {n_users * (size_t)(d / 4), n_items * (size_t)(d / 4), n_users, n_items * (size_t)(T + 1)}, {d / 4, d / 4, 1, T + 1},
                  {0u, 0u, 0u, 0u}, step_tag, lr_t, beta1, beta2, eps};
    return launch_temp_pop_sweep(a, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_temp_pop_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                          float* gI, int32_t* tagI, size_t n_items, float* bu, float* mbu, float* vbu, float* gbu, float* C, float* mC,
                                          float* vC, float* gC, const int32_t* users, const int32_t* pos, const int32_t* neg, const float* temps, int B,
                                          int d, int T, float regs, float reg_div, int step_tag, float lr_t, float beta1, float beta2, float eps,
                                          float* loss_acc, void* stream) {
    if (!mU || !vU || !mI || !vI || !mbu || !vbu || !mC || !vC || n_users == 0 || n_items == 0) return PDA_ERR_ARG;
    const int rc = pda_temp_pop_step_f32(U, I, bu, C, users, pos, neg, temps, B, d, T, regs, reg_div, gU, gI, gbu, gC, tagU, tagI, step_tag,
                                         loss_acc, stream);
    if (rc != PDA_OK) return rc;
    return pda_temp_pop_sweep_f32(U, mU, vU, gU, tagU, n_users, I, mI, vI, gI, tagI, n_items, bu, mbu, vbu, gbu, C, mC, vC, gC, d, T, step_tag, lr_t,
                                  beta1, beta2, eps, stream);
}

extern "C" size_t pda_temp_pop_score_workspace_bytes(int n_users_blk) {
    if (n_users_blk <= 0) return 0;
    const size_t exact = 64 + 4 * (size_t)n_users_blk, pre = pda_score_topk_workspace_bytes(n_users_blk);
    return exact > pre ? exact : pre;
}

// Which kernel serves a call: the pre-filtered one (generation 3: bf16 MFMA filter, candidate ring, exact rescoring) whenever a prep is given and
// it can run (K <= PDA_TOPK_CAP - 4, item ids below 2^27), the exact one (generation 1) otherwise.  PDA_TEMP_POP_KERNEL=exact | prefiltered forces
// one (prefiltered without a prep, or where generation 3 cannot run: PDA_ERR_UNSUPPORTED).  Both return the same keys.
extern "C" int pda_temp_pop_score_topk_f32(const float* U, const float* I_shard, const void* prep, const float* alpha, const float* beta,
                                           const int32_t* users, int n_users_blk, int item_offset, int n_items_local, int d,
                                           const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, int K, int n_splits,
                                           uint64_t* out_keys, void* workspace, void* stream) {
    if (!U || !I_shard || !alpha || !beta || !users || !out_keys || !workspace) return PDA_ERR_ARG;
    if (n_users_blk <= 0 || n_items_local <= 0 || item_offset < 0) return PDA_ERR_ARG;
    if (K < 1 || K > PDA_MAX_K || K > PDA_TOPK_CAP - 1) return PDA_ERR_ARG;
    if (hist_indptr && !hist_indices) return PDA_ERR_ARG;
    if (d != 64 && d != 128 && d != 256) return PDA_ERR_UNSUPPORTED;
    if (n_splits <= 0) n_splits = pda_score_topk_auto_splits(n_users_blk, n_items_local);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const char* env = getenv("PDA_TEMP_POP_KERNEL");
    const bool force_exact = env && strcmp(env, "exact") == 0, force_pre = env && strcmp(env, "prefiltered") == 0;
    if (force_pre && !prep) return PDA_ERR_UNSUPPORTED;
    if (prep && !force_exact) {
        const int rc = pda_topk::run_score_bias_prefiltered(U, I_shard, prep, alpha, beta, users, n_users_blk, item_offset, n_items_local, d,
                                                            hist_indptr, hist_indices, hist_row_mode, K, n_splits, out_keys, workspace, s);
        if (rc != PDA_ERR_UNSUPPORTED || force_pre) return rc;
    }
    // the exact kernel reads alpha from the workspace (generation 1's argument block is shared with the other heads and stays as it is)
    if (hipMemcpyAsync(reinterpret_cast<unsigned char*>(workspace) + 64, alpha, 4 * (size_t)n_users_blk, hipMemcpyDeviceToDevice, s) != hipSuccess)
        return PDA_ERR_LAUNCH;
    pda_topk::ScoreArgs a{U, I_shard, beta, users, hist_indptr, hist_indices, out_keys,
                          n_users_blk, item_offset, n_items_local, hist_row_mode, K, n_splits, reinterpret_cast<const int*>(workspace)};
    return pda_topk::launch_score_bias(a, d, s);
}
