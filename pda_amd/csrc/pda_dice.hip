// DICE (include/pda_hip_dice.h) on MI355X (gfx950): the fused gradient step of the two concatenated tables, the L_dis pass over
// the batch's distinct rows, and PNSM, the popularity-margin negative sampler.  The Adam update is pda_adam_dense_sweep4_f32 at row width 2d.
//
// Step layout: the one of pda_bpr_step.hip at row width W = 2d -- W/4 = d/2 lanes per triplet, each lane owns one float4 of the three gathered
// rows.  The lower half of the lane group holds the interest columns, the upper half the conformity columns: the two dots are the xor-shuffle
// ladder of triplet_dots stopped one rung early, and one more exchange hands each half the other half's sum.  Equal positives inside a workgroup
// are summed by their first triplet through LDS (pda_bpr_step.hip's PDA_UPD_ANY_ORDER).
//
// L_dis needs |S_u| and |S_i|, the numbers of distinct rows, which are known only once the whole batch has been seen: the lane group whose
// atomic exchange on a row's tag finds another step's value lists the row (LDS first, one global atomic per workgroup and table reserves the
// range), and dice_dis_kernel walks the lists behind the step kernel.
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_sample.h"
#include "pda_train_common.h"
#include "pda_hip_dice.h"

namespace {

constexpr int kWsHead = 4;      // words in front of the row lists of rows_ws: |S_u|, |S_i|, two spare (the block the memset clears)

struct DiceStepArgs {
    const float* U;
    const float* I;
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    const uint8_t* mask;
    float* gU;
    float* gI;
    int32_t* tagU;
    int32_t* tagI;
    int32_t* ws;
    float* loss_acc;
    unsigned n_users, n_items;
    int tag;
    int B;
    float inv_B;
    float reg_c;   // regs / reg_div
    float w_int, w_con;
};

template <int W>
__global__ void __launch_bounds__(512) dice_step_kernel(DiceStepArgs a) {
    constexpr int L = W / 4;        // lanes per triplet
    constexpr int H = L / 2;        // lanes per embedding
    constexpr int TPB = 512 / L;    // triplets per block
    __shared__ float red[2][8], red2[2][8];
    __shared__ int s_pos[TPB];
    __shared__ int s_rows[3 * TPB];   // rows this workgroup tagged first: users [TPB], items [2 TPB]
    __shared__ int s_n[2], s_base[2];
    __shared__ __attribute__((aligned(16))) float s_dpe[TPB * W];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;
    const bool con = e >= H;
    if (tid < 2) s_n[tid] = 0;
    __syncthreads();

    float l_click = 0.f, l_int = 0.f, l_con = 0.f, sq = 0.f;
    int u = 0, p = -1, n = 0;
    bool active = t < a.B;
    if (active) {
        u = a.users[t], p = a.pos[t], n = a.neg[t];
        active = triplet_ids_ok(u, p, n, a.n_users, a.n_items);
        if (!active) p = -1;
    }
    if (active) {
        const bool m = a.mask[t] != 0;
        const f32x4 ue = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * W + 4 * e);
        const f32x4 pe = *reinterpret_cast<const f32x4*>(a.I + (size_t)p * W + 4 * e);
        const f32x4 ne = *reinterpret_cast<const f32x4*>(a.I + (size_t)n * W + 4 * e);
        float x_int, x_con;
        triplet_half_dots<W>(ue, pe, ne, con, x_int, x_con);
        sq = triplet_sq(ue, pe, ne);
        // d loss / d x_int and d loss / d x_con: the click term feeds both, L_int only the masked triplets, L_con flips its sign with the mask
        float lc, li = 0.f, lk;
        const float g_click = bpr_dloss_dx(x_int + x_con, a.inv_B, 0, lc);
        float g_i = 0.f, g_c;
        if (m) {
            g_i = a.w_int * bpr_dloss_dx(x_int, a.inv_B, 0, li);
            g_c = -a.w_con * bpr_dloss_dx(-x_con, a.inv_B, 0, lk);
        } else {
            g_c = a.w_con * bpr_dloss_dx(x_con, a.inv_B, 0, lk);
        }
        if (e == 0) l_click = lc, l_int = li, l_con = lk;
        const float gx = g_click + (con ? g_c : g_i);
        f32x4 due, dpe, dne;
        triplet_row_grads(ue, pe, ne, gx, gx, a.reg_c, due, dpe, dne);
        atomic_add4(a.gU + (size_t)u * W + 4 * e, due);
        atomic_add4(a.gI + (size_t)n * W + 4 * e, dne);
        *reinterpret_cast<f32x4*>(s_dpe + g * W + 4 * e) = dpe;
        if (e == 0) {
            // the first group to tag a row of this step lists it (an equal pos and neg: the second exchange finds the tag)
            if (atomicExch(&a.tagU[u], a.tag) != a.tag) s_rows[atomicAdd(&s_n[0], 1)] = u;
            if (atomicExch(&a.tagI[p], a.tag) != a.tag) s_rows[TPB + atomicAdd(&s_n[1], 1)] = p;
            if (atomicExch(&a.tagI[n], a.tag) != a.tag) s_rows[TPB + atomicAdd(&s_n[1], 1)] = n;
        }
    }
    if (e == 0) s_pos[g] = p;
    __syncthreads();
    if (tid < 2) s_base[tid] = s_n[tid] > 0 ? atomicAdd(&a.ws[tid], s_n[tid]) : 0;
    if (active) pos_scatter_any<W, TPB>(s_pos, s_dpe, g, e, p, a.gI + (size_t)p * W + 4 * e);
    block_loss_reduce(l_click, sq, red);
    block_loss_reduce(l_int, l_con, red2);      // (its barrier also publishes s_base)
    // distinct users <= B and distinct items <= 2 B: the lists cannot overflow (the counters start at zero in every call)
    if (tid < s_n[0]) a.ws[kWsHead + s_base[0] + tid] = s_rows[tid];
    if (tid < s_n[1]) a.ws[kWsHead + a.B + s_base[1] + tid] = s_rows[TPB + tid];
    if (tid == 0 && a.loss_acc) {
        float mf, rg, si = 0.f, sc = 0.f;
        block_loss_terms(red, a.inv_B, a.reg_c, mf, rg);
#pragma unroll
        for (int w = 0; w < 8; ++w) {
            si += red2[0][w];
            sc += red2[1][w];
        }
        const float Li = -si * a.inv_B, Lc = -sc * a.inv_B;
        mf = mf + a.w_int * Li + a.w_con * Lc;
        unsafeAtomicAdd(a.loss_acc + 0, mf + rg);
        unsafeAtomicAdd(a.loss_acc + 1, mf);
        unsafeAtomicAdd(a.loss_acc + 2, rg);
        unsafeAtomicAdd(a.loss_acc + 3, Li);
        unsafeAtomicAdd(a.loss_acc + 4, Lc);
    }
}

struct DiceDisArgs {
    const float* U;
    const float* I;
    float* gU;
    float* gI;
    const int32_t* ws;
    float* loss_acc;
    unsigned n_users, n_items;
    int B;
    int l2;
    float pen;
};

// W/8 lanes per listed row: a lane holds one float4 of the interest half and the float4 of the conformity half under it.  Every element of
// g has one writer here, and the step kernel's atomics are complete (the launch before this one): plain read-modify-write.
template <int W>
__global__ void __launch_bounds__(256) dice_dis_kernel(DiceDisArgs a) {
    constexpr int H = W / 8, D = W / 2;
    __shared__ float red[4];
    int nU = a.ws[0], nI = a.ws[1];
    nU = nU < 0 ? 0 : (nU > a.B ? a.B : nU);              // (memory safety only)
    nI = nI < 0 ? 0 : (nI > 2 * a.B ? 2 * a.B : nI);
    const float invU = nU > 0 ? 1.f / ((float)nU * (float)D) : 0.f, invI = nI > 0 ? 1.f / ((float)nI * (float)D) : 0.f;
    const int c = threadIdx.x % H;
    float acc = 0.f;
    for (int slot = (int)((blockIdx.x * 256u + threadIdx.x) / H); slot < nU + nI; slot += (int)(gridDim.x * 256u / H)) {
        const bool user = slot < nU;
        const int row = user ? a.ws[kWsHead + slot] : a.ws[kWsHead + a.B + (slot - nU)];
        const float inv = user ? invU : invI;
        if ((unsigned)row >= (user ? a.n_users : a.n_items)) continue;      // (memory safety only: the step kernel lists valid rows)
        const size_t at = (size_t)row * W + 4 * c;
        const float* X = user ? a.U : a.I;
        float* G = user ? a.gU : a.gI;
        const f32x4 xi = *reinterpret_cast<const f32x4*>(X + at), xc = *reinterpret_cast<const f32x4*>(X + at + D);
        f32x4 gi = *reinterpret_cast<const f32x4*>(G + at), gc = *reinterpret_cast<const f32x4*>(G + at + D);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float df = xi[k] - xc[k];
            float dd;       // d dis / d x_int (the conformity element takes the opposite)
            if (a.l2) {
                acc += df * df * inv;
                dd = 2.f * df * inv;
            } else {
                acc += fabsf(df) * inv;
                dd = df > 0.f ? inv : (df < 0.f ? -inv : 0.f);
            }
            gi[k] -= a.pen * dd;
            gc[k] += a.pen * dd;
        }
        *reinterpret_cast<f32x4*>(G + at) = gi;
        *reinterpret_cast<f32x4*>(G + at + D) = gc;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0 && a.loss_acc) {
        const float ld = (red[0] + red[1]) + (red[2] + red[3]);
        if (ld != 0.f) {
            unsafeAtomicAdd(a.loss_acc + 0, -a.pen * ld);
            unsafeAtomicAdd(a.loss_acc + 1, -a.pen * ld);
            unsafeAtomicAdd(a.loss_acc + 5, ld);
        }
    }
}

// ---- PNSM ---------------------------------------------------------------------------------------------------------------------------------
struct DiceSampleArgs {
    int32_t* users;
    const int32_t* user_pool;
    const int64_t* indptr;
    const int32_t* indices;
    const int32_t* order;
    const int32_t* sorted_pop;
    const int32_t* pop;
    int32_t* pos;
    int32_t* neg;
    uint8_t* mask;
    uint64_t seed, step;
    float margin;
    int B, n_pool, gen_users, n_items;
    const float* margin_dev;    // optional: the margin in device memory
    const uint64_t* step_dev;   // optional: a device-resident step counter added to `step`
    uint64_t* step_next;        // optional: receives *step_dev + 1
};

// one thread = one triplet.  The step, the user, the positive and the rejection loop are the pieces sample_one is made of (pda_sample.h; no
// time slots here): a row draws the user and the positive that pda_sample_triplets draws for the same (seed, step, row).  PNSM's own: the two
// ranges of `order` around the positive's popularity, the coin between them, the mask.
__global__ void __launch_bounds__(64) dice_sample_kernel(DiceSampleArgs a) {
    const int r = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (r >= a.B) return;
    a.step = sample_step(a.step, a.step_dev, a.step_next, r == 0);
    const float margin = a.margin_dev ? *a.margin_dev : a.margin;
    int u;
    if (a.gen_users) {
        u = sample_user(a.seed, a.step, r, a.B, a.n_pool, a.user_pool);
        a.users[r] = u;
    } else {
        u = a.users[r];
    }
    const int64_t b = a.indptr[u], e = a.indptr[u + 1];
    const int len = (int)(e - b);
    int p = len == 0 ? 0 : a.indices[b + sample_pos_index(a.seed, a.step, r, len)];
    if ((unsigned)p >= (unsigned)a.n_items) p = 0;      // (memory safety only: the train lists hold ids of the catalogue)
    // H = [hi_at, n_items) and L = [0, lo_end) of `order`, in fp32 like the restatement (tests/dice_ref.py)
    const float P = (float)a.pop[p], above = P + margin, below = P - margin;
    int lo = 0, hi = a.n_items;
    while (lo < hi) {                       // first position with sorted_pop > above
        const int mid = (lo + hi) >> 1;
        if ((float)a.sorted_pop[mid] > above) hi = mid; else lo = mid + 1;
    }
    const int hi_at = lo;
    lo = 0, hi = a.n_items;
    while (lo < hi) {                       // first position with sorted_pop >= below
        const int mid = (lo + hi) >> 1;
        if ((float)a.sorted_pop[mid] < below) lo = mid + 1; else hi = mid;
    }
    const int lo_end = lo, nH = a.n_items - hi_at, nL = lo_end;
    bool fromH = false, whole = false;
    if (nH > 0 && nL > 0) fromH = (draw(a.seed, a.step, r, 2) >> 31) != 0;
    else if (nH > 0) fromH = true;
    else if (nL == 0) whole = true;
    const int start = whole ? 0 : (fromH ? hi_at : 0);
    const uint32_t span = (uint32_t)(whole ? a.n_items : (fromH ? nH : nL));
    const int n = sample_negative(a.seed, a.step, r, kNegDraw, span, a.indices, b, e, [&](uint32_t x) {
        const int at = start + (int)x;
        return whole ? at : a.order[at];
    });
    a.pos[r] = p;
    a.neg[r] = n;
    a.mask[r] = whole ? (uint8_t)(a.pop[n] > a.pop[p]) : (uint8_t)fromH;
}

bool dice_d_ok(int d) { return d == 32 || d == 64 || d == 128; }       // (the width of ONE embedding: rows of 2 d floats)

// Both PNSM entry points.  counter (pda_dice_sample_dev): the step and the margin are read on the device; else both travel by value, the
// three device pointers are null, and the margin is checked here.
int dice_sample(bool counter, int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr,
                const int32_t* train_indices, int n_items, const int32_t* order, const int32_t* sorted_pop, const int32_t* pop, float margin,
                const float* margin_dev, uint64_t seed, uint64_t step, const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* neg,
                uint8_t* mask, void* stream) {
    if (!sample_call_ok(users, train_indptr, train_indices, pos, neg, gen_users, n_pool, counter, step_dev, step_next)) return PDA_ERR_ARG;
    if (!order || !sorted_pop || !pop || !mask || B <= 0 || n_items <= 0) return PDA_ERR_ARG;
    if (counter ? !margin_dev : !(margin >= 0.f)) return PDA_ERR_ARG;
    const DiceSampleArgs a{users, user_pool, train_indptr, train_indices, order, sorted_pop, pop, pos, neg, mask, seed, step, margin, B, n_pool,
                           gen_users, n_items, margin_dev, step_dev, step_next};
    hipLaunchKernelGGL(dice_sample_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" size_t pda_dice_rows_ws_words(int B) { return B > 0 ? (size_t)kWsHead + 3 * (size_t)B : 0; }

extern "C" int pda_dice_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                                 const int32_t* neg, const uint8_t* mask, int B, int d, float w_int, float w_con, float regs, float reg_div,
                                 float* gU, float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int32_t* rows_ws, float* loss_acc,
                                 void* stream) {
    if (!U || !I || !users || !pos || !neg || !mask || !gU || !gI || !tagU || !tagI || !rows_ws) return PDA_ERR_ARG;
    if (B <= 0 || B > (1 << 28) || reg_div <= 0.f || step_tag <= 0 || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (!dice_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (hipMemsetAsync(rows_ws, 0, kWsHead * sizeof(int32_t), s) != hipSuccess) return PDA_ERR_LAUNCH;
    DiceStepArgs a{U, I, users, pos, neg, mask, gU, gI, tagU, tagI, rows_ws, loss_acc, (unsigned)n_users, (unsigned)n_items, step_tag, B,
                   1.0f / (float)B, regs / reg_div, w_int, w_con};
    switch (d) {        // (rows of 2 d floats; no width 32)
        case 32: PDA_STEP_LAUNCH_W(dice_step_kernel, 64, B, s, a); break;
        case 64: PDA_STEP_LAUNCH_W(dice_step_kernel, 128, B, s, a); break;
        default: PDA_STEP_LAUNCH_W(dice_step_kernel, 256, B, s, a); break;
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_dice_dis_f32(const float* U, const float* I, size_t n_users, size_t n_items, int B, int d, int dis_kind, float dis_pen,
                                float* gU, float* gI, const int32_t* rows_ws, float* loss_acc, void* stream) {
    if (!U || !I || !gU || !gI || !rows_ws || B <= 0 || B > (1 << 28)) return PDA_ERR_ARG;
    if (!pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (dis_kind != PDA_DICE_DIS_L1 && dis_kind != PDA_DICE_DIS_L2) return PDA_ERR_ARG;
    if (!dice_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    DiceDisArgs a{U, I, gU, gI, rows_ws, loss_acc, (unsigned)n_users, (unsigned)n_items, B, dis_kind == PDA_DICE_DIS_L2 ? 1 : 0, dis_pen};
    // a thread per float4 pair of the 3 B rows the lists can hold, at most 2 048 workgroups (grid-stride beyond)
    const size_t want = (3 * (size_t)B * (size_t)(d / 4) + 255) / 256;
    const unsigned grid = (unsigned)(want > 2048 ? 2048 : want);
    switch (d) {
        case 32: hipLaunchKernelGGL(dice_dis_kernel<64>, dim3(grid), dim3(256), 0, s, a); break;
        case 64: hipLaunchKernelGGL(dice_dis_kernel<128>, dim3(grid), dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(dice_dis_kernel<256>, dim3(grid), dim3(256), 0, s, a); break;
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_dice_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                      float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                                      const uint8_t* mask, int B, int d, float w_int, float w_con, int dis_kind, float dis_pen, float regs,
                                      float reg_div, int step_tag, float lr_t, float beta1, float beta2, float eps, int cache_policy,
                                      int32_t* rows_ws, float* loss_acc, void* stream) {
    if (!mU || !vU || !mI || !vI) return PDA_ERR_ARG;
    if (dis_kind != PDA_DICE_DIS_L1 && dis_kind != PDA_DICE_DIS_L2) return PDA_ERR_ARG;
    if (cache_policy < PDA_ADAM_CACHE_AUTO || cache_policy > PDA_ADAM_CACHE_STREAM) return PDA_ERR_ARG;
    int rc = pda_dice_step_f32(U, I, n_users, n_items, users, pos, neg, mask, B, d, w_int, w_con, regs, reg_div, gU, gI, tagU, tagI, step_tag,
                               rows_ws, loss_acc, stream);
    if (rc != PDA_OK) return rc;
    rc = pda_dice_dis_f32(U, I, n_users, n_items, B, d, dis_kind, dis_pen, gU, gI, rows_ws, loss_acc, stream);
    if (rc != PDA_OK) return rc;
    return pda_adam_dense_sweep4_f32(U, mU, vU, gU, n_users, tagU, I, mI, vI, gI, n_items, tagI, 2 * d, step_tag, lr_t, beta1, beta2, eps,
                                     cache_policy, stream);
}

extern "C" int pda_dice_sample(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr,
                               const int32_t* train_indices, int n_items, const int32_t* order, const int32_t* sorted_pop, const int32_t* pop,
                               float margin, uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg, uint8_t* mask, void* stream) {
    return dice_sample(false, users, gen_users, user_pool, n_pool, B, train_indptr, train_indices, n_items, order, sorted_pop, pop, margin, nullptr,
                       seed, step, nullptr, nullptr, pos, neg, mask, stream);
}

extern "C" int pda_dice_sample_dev(int32_t* users, int gen_users, const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr,
                                   const int32_t* train_indices, int n_items, const int32_t* order, const int32_t* sorted_pop,
                                   const int32_t* pop, const float* margin_dev, uint64_t seed, const uint64_t* step_dev, uint64_t* step_next,
                                   int32_t* pos, int32_t* neg, uint8_t* mask, void* stream) {
    return dice_sample(true, users, gen_users, user_pool, n_pool, B, train_indptr, train_indices, n_items, order, sorted_pop, pop, 0.f, margin_dev,
                       seed, 0, step_dev, step_next, pos, neg, mask, stream);
}
