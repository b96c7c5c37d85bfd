// What every training step kernel shares (pda_bpr_step.hip, pda_bpr_plan.hip, pda_temp_pop.hip, pda_dice.hip, pda_ips.hip, pda_macr.hip; pda_gcn.hip
// takes the loss reduction).  The arithmetic: the triplet forward / backward of the reference model, the block reduction of the loss, and the TF-1.14
// Adam element update.  Around it: the id test of a triplet, the precondition of the dense-gradient writes of a tagged step, and the scatter of the
// positives' gradients through LDS.  One definition each: the bit-identity of the sweeps, the lazy replay, --deterministic and the checkpoints
// (tests/test_gpu_bpr_step.py, test_gpu_deterministic.py, test_gpu_temp_pop.py) holds because every kernel compiles THESE expressions, in this
// order, under -ffp-contract=off.
#pragma once
#include "pda_common.h"

__device__ __forceinline__ float dot4(f32x4 a, f32x4 b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2] + a[3] * b[3]; }

__device__ __forceinline__ void atomic_add4(float* p, f32x4 v) {
    unsafeAtomicAdd(p + 0, v[0]);
    unsafeAtomicAdd(p + 1, v[1]);
    unsafeAtomicAdd(p + 2, v[2]);
    unsafeAtomicAdd(p + 3, v[3]);
}

// COH (pda_bpr_train_steps_f32): the value was written by ANOTHER workgroup of this launch at device scope and is read with a device-scope
// load (it misses the caches that are not coherent across the XCDs), so that a grid barrier needs no cache invalidation.
template <bool COH, typename T>
__device__ __forceinline__ T in_load(const T* p) {
    if constexpr (COH) return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else return *p;
}

// ---- the triplet: d/4 lanes, each with one float4 of the three gathered rows ------------------------------------------------------------------
// ps = <u, p>, ns = <u, n>, summed over the D/4 lanes of the group: every lane holds them
template <int D>
__device__ __forceinline__ void triplet_dots(f32x4 ue, f32x4 pe, f32x4 ne, float& ps, float& ns) {
    ps = dot4(ue, pe), ns = dot4(ue, ne);
#pragma unroll
    for (int o = D / 8; o > 0; o >>= 1) {
        ps += __shfl_xor(ps, o, 64);
        ns += __shfl_xor(ns, o, 64);
    }
}
// DICE (pda_dice.hip): a row of W floats is two embeddings of W/2, the lower half of the W/4 lanes holds the first (interest), the upper half
// (upper == true) the second (conformity).  x_lo / x_hi = <u, p> - <u, n> over each half: the ladder above stopped one rung early, then one
// exchange across the halves.  Every lane of the group holds both, bit for bit the same.
template <int W>
__device__ __forceinline__ void triplet_half_dots(f32x4 ue, f32x4 pe, f32x4 ne, bool upper, float& x_lo, float& x_hi) {
    float ps = dot4(ue, pe), ns = dot4(ue, ne);
#pragma unroll
    for (int o = W / 16; o > 0; o >>= 1) {
        ps += __shfl_xor(ps, o, 64);
        ns += __shfl_xor(ns, o, 64);
    }
    const float mine = ps - ns, other = __shfl_xor(mine, W / 8, 64);
    x_lo = upper ? other : mine;
    x_hi = upper ? mine : other;
}
// this lane's share of |u|^2 + |p|^2 + |n|^2 (the L2 term of the loss)
__device__ __forceinline__ float triplet_sq(f32x4 ue, f32x4 pe, f32x4 ne) { return dot4(ue, ue) + dot4(pe, pe) + dot4(ne, ne); }
// x = positive score - negative score  ->  d(mean loss) / dx; lane 0 of the group (e == 0) takes the triplet's log-sigmoid into maxi
__device__ __forceinline__ float bpr_dloss_dx(float x, float inv_B, int e, float& maxi) {
    const float sg = 1.f / (1.f + expf(-x));
    if (e == 0) maxi = logf(sg + 1e-10f);                 // MF/model_api.py:112 / :367 / :702
    return -inv_B * sg * (1.f - sg) / (sg + 1e-10f);
}
// the rows' gradients with the L2 term (c = regs / reg_div): gp = d loss / d(positive score), gn = -d loss / d(negative score)
__device__ __forceinline__ void triplet_row_grads(f32x4 ue, f32x4 pe, f32x4 ne, float gp, float gn, float c, f32x4& due, f32x4& dpe, f32x4& dne) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        due[k] = gp * pe[k] - gn * ne[k] + c * ue[k];
        dpe[k] = gp * ue[k] + c * pe[k];
        dne[k] = -gn * ue[k] + c * ne[k];
    }
}

// PD / PDA and plain BPR-MF (MF/model_api.py:102-121 / :695-705): scores (ELU + 1) * pop where pos_pop is given (pos_pop[t], neg_pop[t]: read
// only then), the raw dots otherwise.
template <int D, bool COH = false>
__device__ __forceinline__ void bpr_triplet(f32x4 ue, f32x4 pe, f32x4 ne, const float* pos_pop, const float* neg_pop, int t, float inv_B, float reg_c,
                                            int e, float& maxi, float& sq, float& gp, float& gn, f32x4& due, f32x4& dpe, f32x4& dne) {
    float ps, ns;
    triplet_dots<D>(ue, pe, ne, ps, ns);
    float ap = 1.f, an = 1.f, psw = ps, nsw = ns;
    if (pos_pop != nullptr) {
        const float qp = in_load<COH>(&pos_pop[t]), qn = in_load<COH>(&neg_pop[t]);
        const float ep = ps > 0.f ? 1.f : expf(ps);   // d(elu+1)/dx  [TF-ext EluGrad]
        const float en = ns > 0.f ? 1.f : expf(ns);
        psw = (ps > 0.f ? ps + 1.f : ep) * qp;        // (elu(ps)+1)*pos_pop   MF/model_api.py:107,109
        nsw = (ns > 0.f ? ns + 1.f : en) * qn;        // :108,110
        ap = qp * ep;
        an = qn * en;
    }
    const float gg = bpr_dloss_dx(psw - nsw, inv_B, e, maxi);
    sq = triplet_sq(ue, pe, ne);      // (behind the score chain: nothing waits for it before the block reduction)
    gp = gg * ap, gn = gg * an;
    triplet_row_grads(ue, pe, ne, gp, gn, reg_c, due, dpe, dne);
}

// ---- around the arithmetic: which triplets count, and where their gradients go -------------------------------------------------------------------
// a triplet whose ids lie outside the tables is skipped (memory safety when the host check is off): it reads and writes nothing
__device__ __forceinline__ bool triplet_ids_ok(int u, int p, int n, unsigned n_users, unsigned n_items) {
    return (unsigned)u < n_users && (unsigned)p < n_items && (unsigned)n < n_items;
}

// The dense-gradient writes of a tagged step (pda_ips.hip, pda_macr.hip, the PDA_UPD_DENSE_GRAD branch of pda_bpr_step.hip): the user row of gU by
// a plain store under users_distinct and by atomics otherwise, the negative's row of gI by atomics, and the step's tag on the three rows by lane 0
// (the same value from every writer of a row: plain stores).  The three kernels keep these ten lines: as a helper -- one of W, the pointers and
// the flag, one of the argument block, or split in two -- the IPS and MACR kernels kept three more addresses in registers (43 -> 46, 60 -> 64
// VGPRs, five instructions fewer) and ran 0.3 us per step slower (profiles/step_scatter_timing.txt).
// PRECONDITION of users_distinct (PDA_UPD_USERS_DISTINCT): the PLAIN STORE is the row's gradient only if gU is zero on every row the batch touches
// and no user occurs twice in the batch.  The sweep behind the step clears the tagged rows of g, so the condition holds from one whole step to
// the next; a call that returns anything but PDA_OK between the step and the sweep leaves g and the tags dirty, and the caller has to zero them
// before the next step (include/pda_hip.h, pda_adam_step_f32).  Without the flag the row takes atomics and needs neither.

// The positives' gradients go through LDS first: positive items are popularity-skewed, one batch holds the hottest item ~170 times, and that many
// float atomics on the same cache lines serialise in L2 (24.8 -> 12.9 us per 2048-triplet step, pda_bpr_step.hip).  The caller has written, for
// every triplet g of the workgroup (TPB of them, W/4 lanes each, lane e owns floats [4 e, 4 e + 4) of a row of W), s_pos[g] -- the positive, -1 for a
// refused or inactive triplet, a distinct dummy where the row does not take part -- and s_dpe[g W ..] for the triplets that do, and passed its own
// barrier.  A triplet that takes part calls ONE of the two with its own p (never a dummy) and the address of its float4 in the target row.  The
// order of the sum -- the triplet's own contribution, then ascending k -- is part of the bit-identity contract.
// Any batch order: the first triplet of the workgroup with this positive sums ALL the workgroup's contributions, adjacent or not: one atomic_add4.
template <int W, int TPB>
__device__ __forceinline__ void pos_scatter_any(const int* s_pos, const float* s_dpe, int g, int e, int p, float* target) {
    bool leader = true;
    for (int k = 0; k < g; ++k) leader = leader && (s_pos[k] != p);
    if (leader) {
        f32x4 sum = *reinterpret_cast<const f32x4*>(s_dpe + g * W + 4 * e);
        for (int k = g + 1; k < TPB; ++k)
            if (s_pos[k] == p) sum += *reinterpret_cast<const f32x4*>(s_dpe + k * W + 4 * e);
        atomic_add4(target, sum);
    }
}
// Grouped batch (equal positives adjacent): is triplet g the first of a run of equal positives? ...
__device__ __forceinline__ bool pos_run_head(const int* s_pos, int g, int p) { return g == 0 || s_pos[g - 1] != p; }
// ... then it sums the run: a refused triplet (-1) inside a run ends it, and the triplet behind it heads the next one.
template <int W, int TPB>
__device__ __forceinline__ void pos_scatter_run(const int* s_pos, const float* s_dpe, int g, int e, int p, float* target) {
    f32x4 sum = *reinterpret_cast<const f32x4*>(s_dpe + g * W + 4 * e);
    for (int k = g + 1; k < TPB && s_pos[k] == p; ++k) sum += *reinterpret_cast<const f32x4*>(s_dpe + k * W + 4 * e);
    atomic_add4(target, sum);
}

// ---- block reduction of sum(log(.)) and of the squared norms (512 threads = 8 waves; red: a __shared__ float[2][8] of the calling kernel) -----
__device__ __forceinline__ void block_loss_reduce(float maxi, float sq, float (&red)[2][8]) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        maxi += __shfl_xor(maxi, o, 64);
        sq += __shfl_xor(sq, o, 64);
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) {
        red[0][wave] = maxi;
        red[1][wave] = sq;
    }
    __syncthreads();
}
// (one thread, behind block_loss_reduce) the block's share of the two loss terms
__device__ __forceinline__ void block_loss_terms(const float (&red)[2][8], float inv_B, float reg_c, float& mf, float& rg) {
    float sm = 0.f, ss = 0.f;
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        sm += red[0][w];
        ss += red[1][w];
    }
    mf = -sm * inv_B;               // -mean(maxi)          MF/model_api.py:114 / :368 / :704
    rg = reg_c * 0.5f * ss;         // regs * l2 / batch    :117-120 / :370-373
}
// (one thread, behind block_loss_reduce) loss_acc[0..2] += (loss, mf, reg) of this block: three atomics per workgroup
__device__ __forceinline__ void block_loss_add(const float (&red)[2][8], float inv_B, float reg_c, float* loss_acc) {
    float mf, rg;
    block_loss_terms(red, inv_B, reg_c, mf, rg);
    unsafeAtomicAdd(loss_acc + 0, mf + rg);
    unsafeAtomicAdd(loss_acc + 1, mf);
    unsafeAtomicAdd(loss_acc + 2, rg);
}

// ---- TF-1.14 Adam with dense decay, one element: lr_t is the bias-corrected rate of the step.  A row the step did not touch takes g = 0 (the
// literal, through these very expressions: that is what makes the sweeps and the exact replay bit-identical) ----------------------------------
__device__ __forceinline__ void adam_moments(float& m, float& v, float g, float b1, float b2) {
    m = b1 * m + (1.f - b1) * g;
    v = b2 * v + (1.f - b2) * g * g;
}
__device__ __forceinline__ void adam_elem(float& x, float& m, float& v, float g, float lr_t, float b1, float b2, float eps) {
    adam_moments(m, v, g, b1, b2);
    x = x - lr_t * m / (sqrtf(v) + eps);
}
// (the four elements of a chunk; a vector element cannot bind to a reference, hence the copies)
__device__ __forceinline__ void adam_moments(f32x4& mm, f32x4& vv, f32x4 gg, float b1, float b2) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float m = mm[k], v = vv[k];
        adam_moments(m, v, gg[k], b1, b2);
        mm[k] = m;
        vv[k] = v;
    }
}
__device__ __forceinline__ void adam_elem(f32x4& xx, f32x4& mm, f32x4& vv, f32x4 gg, float lr_t, float b1, float b2, float eps) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float x = xx[k], m = mm[k], v = vv[k];
        adam_elem(x, m, v, gg[k], lr_t, b1, b2, eps);
        xx[k] = x;
        mm[k] = m;
        vv[k] = v;
    }
}

// ---- the sweeps over both tables of the model in one launch: workgroups [0, blocks_a) take the first table, the rest the second ---------------
struct SweepTable {
    float *var, *m, *v, *g;
    size_t n4;              // 16-byte chunks of the table
};
__device__ __forceinline__ SweepTable sweep_table(bool first, float* var_a, float* m_a, float* v_a, float* g_a, size_t n4_a, float* var_b, float* m_b,
                                                  float* v_b, float* g_b, size_t n4_b) {
    return SweepTable{first ? var_a : var_b, first ? m_a : m_b, first ? v_a : v_b, first ? g_a : g_b, first ? n4_a : n4_b};
}
