// The WARP loss (include/pda_hip_warp.h) on MI355X (gfx950): the draw -- the triplet batch of pda_sample_triplets with the negative
// of a row the FIRST of up to T uniform candidates that violates the margin under the live tables -- and the gradient step of the rank-weighted
// hinge.  The Adam update is pda_adam_dense_sweep4_f32 itself.
//
// The draw: one launch, 512 threads, a workgroup owns R whole rows (R <= 64: a wave lists the open rows with one ballot) and runs ROUNDS over LDS.
// It is the row / draw / score structure of dns_sample_kernel, with a list of ENTRIES per round in place of the fixed R M candidates:
//   rows     thread q < R draws row q's user, positive and slot (the pieces of pda_sample.h, as sample_one composes them);
//   open     wave 0 lists the rows without a violator (ballot + popcount: the list is ascending, no atomics);
//   draw     thread i < n_open C draws candidate j0 + i % C of open row i / C (the body of ssm_sample_kernel); a closed row draws nothing more --
//            a rejection draw is a binary search in the train row.  Round 0 appends the rows' positives to the list: they take the very code
//            path of the candidates, so equal items have equal bits;
//   score    the 512 / (d/4) lane groups share the entries in contiguous runs; a group gathers four item rows per step, ids first, so that eight
//            loads are in flight under every ladder; lane 0 leaves the score in LDS;
//   decide   thread i tests its candidate and lowers the row's first violating column with an LDS integer minimum (order-free), then writes its
//            test outputs; a thread per row writes the row's outputs behind the loop.
// How many candidates a round takes (the outputs do not depend on it: the first violator of a row is what it is).  Round 0: kFirst a row -- early
// in training nearly every row closes on its first candidates, and the round is one gather step of every lane group for R = 4 at every d.  Then
// one gather step of all lane groups (8192 / d entries) shared among the rows still open, doubled with every further round up to 512 entries:
// late in training nearly no row closes, and the four barriers of a round are paid 7 times for T = 256, d = 256, not 32 times.
// LDS: 9 KiB a workgroup; eight waves a workgroup, so the wave slots of a compute unit (four workgroups), not LDS, bound the occupancy.
//
// Step layout: the one of pda_ips.hip -- d/4 lanes per triplet, each lane owns one float4 of the three gathered rows, the dots by the xor-shuffle
// ladder of triplet_dots; one 4-byte load per triplet (coef[t]) is the only traffic beside the rows.
#include <climits>
#include <cmath>
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_sample.h"
#include "pda_hip_warp.h"

namespace {

struct WarpArgs {
    const float* U;
    const float* I;
    SampleArgs s;               // users .. n_slots, step_dev, step_next: what sample_one takes (neg: the first violator)
    const float* wtab;
    int32_t* trials;
    float* coef;
    int32_t* cand;
    float* cand_score;
    float* pos_score;
    unsigned long long* stat;
    unsigned n_users;
    int T;
    float margin;
    int rows_per_block;         // R
};

constexpr int kThreads = 512;
constexpr int kChunk = 4;       // item rows gathered per step of a lane group
constexpr int kFirst = 4;       // candidates of a row in round 0
constexpr int kMaxRows = 64;    // rows of a workgroup: one ballot lists the open ones

template <int D>
__global__ void __launch_bounds__(kThreads) warp_sample_kernel(WarpArgs a) {
    constexpr int L = D / 4;            // lanes per entry
    constexpr int G = kThreads / L;     // lane groups
    __shared__ int64_t s_b[kMaxRows], s_e[kMaxRows];
    __shared__ int s_user[kMaxRows], s_slot[kMaxRows], s_pos[kMaxRows], s_first[kMaxRows], s_neg[kMaxRows], s_last[kMaxRows], s_open[kMaxRows];
    __shared__ float s_ps[kMaxRows];
    __shared__ int s_item[kThreads], s_euser[kThreads];
    __shared__ float s_score[kThreads];
    __shared__ int s_nopen;
    const SampleArgs& s = a.s;
    const int tid = threadIdx.x, T = a.T;
    const int row0 = blockIdx.x * a.rows_per_block;
    const int rows = min(a.rows_per_block, s.B - row0);     // >= 1: the grid is ceil(B / R)
    const uint64_t step = sample_step(s.step, s.step_dev, s.step_next, blockIdx.x == 0 && tid == 0);

    // ---- rows: user, positive, slot (sample_one's, piece by piece)
    if (tid < rows) {
        const int r = row0 + tid;
        int u;
        if (s.gen_users) {
            u = sample_user(s.seed, step, r, s.B, s.n_pool, s.user_pool);
            s.users[r] = u;
        } else {
            u = s.users[r];
        }
        const bool known = (unsigned)u < a.n_users;
        const int64_t b = known ? s.indptr[u] : 0, e = known ? s.indptr[u + 1] : 0;
        const int len = (int)(e - b);
        int p = 0, slot = 0;
        if (len == 0) {
            slot = s.n_slots > 0 ? (int)bounded(draw(s.seed, step, r, 1), s.n_slots) : 0;
        } else {
            const int idx = sample_pos_index(s.seed, step, r, len);
            p = s.indices[b + idx];
            slot = s.slots ? s.slots[b + idx] : 0;
        }
        s.pos[r] = p;
        if (s.pos_pop) s.pos_pop[r] = s.pop[(size_t)p * s.n_slots + slot];
        s_b[tid] = b, s_e[tid] = e;
        s_user[tid] = known ? u : -1;
        s_slot[tid] = slot;
        s_pos[tid] = p;
        s_first[tid] = INT_MAX;
        s_neg[tid] = s_last[tid] = 0;
        s_ps[tid] = 0.f;
    }
    __syncthreads();

    // (wave 0) the rows without a violator, ascending
    auto list_open = [&]() {
        const bool open = tid < rows && s_first[tid] == INT_MAX;
        const unsigned long long m = __ballot(open);
        if (open) s_open[__popcll(m & ((1ull << tid) - 1ull))] = tid;
        if (tid == 0) s_nopen = __popcll(m);
    };
    if (tid < 64) list_open();
    __syncthreads();

    int j0 = 0;                 // the first column of the round
    int cap = kChunk * G;       // entries of a round behind round 0
    for (bool first = true;; first = false) {
        const int n_open = s_nopen;
        if (n_open == 0 || j0 >= T) break;
        int C = first ? kFirst : max(1, cap / n_open);
        C = min(C, T - j0);
        const int n_ent = n_open * C;                           // <= 512: round 0 64 * 4, then max(cap, n_open)
        const int n_tot = n_ent + (first ? rows : 0);           // round 0: the positives behind the candidates (<= 320)

        // ---- draw: entry i is candidate j of open row q, the tries kNegDraw + kRejectTries j + ..
        int q = 0, j = 0, c = 0;
        if (tid < n_ent) {
            q = s_open[tid / C], j = j0 + tid % C;
            c = sample_negative(s.seed, step, row0 + q, kNegDraw + kRejectTries * (uint32_t)j, (uint32_t)(s.neg_hi - s.neg_lo), s.indices, s_b[q],
                                s_e[q], [&](uint32_t x) { return s.neg_lo + (int)x; });
        } else if (tid < n_tot) {
            q = tid - n_ent;
            c = s_pos[q];
        }
        if (tid < n_tot) {
            s_item[tid] = c;
            s_euser[tid] = s_user[q];
            s_score[tid] = 0.f;
        }
        __syncthreads();

        // ---- score: group g takes the entries [g per, (g + 1) per)
        {
            const int g = tid / L, e4 = 4 * (tid % L);
            const int per = (n_tot + G - 1) / G;
            const int end = min(n_tot, (g + 1) * per);
            for (int k0 = g * per; k0 < end; k0 += kChunk) {
                int at[kChunk], id[kChunk], us[kChunk];
                f32x4 ie[kChunk], ue[kChunk];
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    at[k] = min(k0 + k, end - 1);               // (the tail of the last step: the run's last entry again, never stored)
                    id[k] = s_item[at[k]];
                    us[k] = s_euser[at[k]];
                }
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    ie[k] = ue[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (us[k] >= 0) {                           // (an unknown user reads no table row)
                        ie[k] = *reinterpret_cast<const f32x4*>(a.I + (size_t)id[k] * D + e4);
                        ue[k] = *reinterpret_cast<const f32x4*>(a.U + (size_t)us[k] * D + e4);
                    }
                }
#pragma unroll
                for (int k = 0; k < kChunk; ++k) {
                    float x = dot4(ue[k], ie[k]);
#pragma unroll
                    for (int o = L / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
                    if (e4 == 0 && k0 + k < end && us[k] >= 0) s_score[at[k]] = x;
                }
            }
        }
        __syncthreads();

        // ---- decide: the first violating column of a row, an integer minimum
        if (tid < n_ent) {
            const float sp = first ? s_score[n_ent + q] : s_ps[q];
            const float x = sp - s_score[tid];
            if (s_user[q] >= 0 && a.margin - x > 0.f) atomicMin(&s_first[q], j);      // (a NaN compares false: never a violator)
        } else if (tid < n_tot) {
            s_ps[q] = s_score[tid];                             // (round 0 reads s_score, not s_ps)
        }
        __syncthreads();
        if (tid < n_ent) {
            const int f = s_first[q];
            if (j == f) s_neg[q] = c;
            if (j == (s_user[q] >= 0 ? T - 1 : 0)) s_last[q] = c;      // (no violator: candidate T - 1; an unknown user: candidate 0)
            if (j <= f) {
                const size_t at = (size_t)(row0 + q) * T + j;
                if (a.cand) a.cand[at] = c;
                if (a.cand_score) a.cand_score[at] = s_score[tid];
            }
        }
        if (tid < 64) list_open();                              // (every thread has read s_nopen and its s_open entry: three barriers ago)
        __syncthreads();
        j0 += C;
        if (!first) cap = min(2 * cap, kThreads);
    }

    // ---- the rows' outputs, the columns behind a first violator, the workgroup's share of stat
    if (a.cand || a.cand_score) {
        for (int i = tid; i < rows * T; i += kThreads) {
            const int q = i / T, j = i - q * T;
            if (j > s_first[q]) {
                const size_t at = (size_t)(row0 + q) * T + j;
                if (a.cand) a.cand[at] = -1;
                if (a.cand_score) a.cand_score[at] = 0.f;
            }
        }
    }
    if (tid < 64) {
        int sum = 0, none = 0;
        if (tid < rows) {
            const int r = row0 + tid, f = s_first[tid];
            const int N = f == INT_MAX ? 0 : f + 1;
            const int n = N > 0 ? s_neg[tid] : s_last[tid];
            s.neg[r] = n;
            a.trials[r] = N;
            a.coef[r] = N > 0 ? a.wtab[N] : 0.f;
            if (a.pos_score) a.pos_score[r] = s_ps[tid];
            if (s.neg_pop) s.neg_pop[r] = s.pop[(size_t)n * s.n_slots + s_slot[tid]];
            sum = N, none = N == 0 ? 1 : 0;
        }
        if (a.stat) {           // (integer adds: the same bits in any order)
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                sum += __shfl_xor(sum, o, 64);
                none += __shfl_xor(none, o, 64);
            }
            if (tid == 0) {
                atomicAdd(a.stat + 0, (unsigned long long)sum);
                atomicAdd(a.stat + 1, (unsigned long long)none);
            }
        }
    }
}

// (host) R, the rows of a workgroup: four, so that round 0 (4 positives + 16 candidates) is one gather step of the lane groups at every d and a
// batch of 2 048 spreads over 512 workgroups (two on each of 256 compute units).  Only where that leaves more than kResident workgroups do the
// rows of a workgroup double, up to kMaxRows: from there on the fixed part of a workgroup (the rows phase, the barriers of a round) costs more
// than a longer entry list.
constexpr int kResident = 512, kBaseRows = 4;
int rows_per_block(int B) {
    int R = kBaseRows;
    while (R < kMaxRows && (B + R - 1) / R > kResident) R *= 2;
    return R;
}

// Both entry points.  counter (pda_warp_sample_f32_dev): the step is read on the device; else it travels by value and the two are null.
int warp_sample(bool counter, const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
                const int32_t* user_pool, int n_pool, int B, const int64_t* indptr, const int32_t* indices, const int32_t* slots, const float* pop,
                int n_slots, int neg_lo, int neg_hi, int T, float margin, const float* wtab, uint64_t seed, uint64_t step, const uint64_t* step_dev,
                uint64_t* step_next, int32_t* pos, int32_t* neg, int32_t* trials, float* coef, float* pos_pop, float* neg_pop, int32_t* cand,
                float* cand_score, float* pos_score, int64_t* stat, void* stream) {
    if (!U || !I || !wtab || !trials || !coef) return PDA_ERR_ARG;
    if (!sample_call_ok(users, indptr, indices, pos, neg, gen_users, n_pool, counter, step_dev, step_next)) return PDA_ERR_ARG;
    if (B <= 0 || B > (1 << 22) || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (T < 1 || T > PDA_WARP_MAX_TRIALS || margin != margin) return PDA_ERR_ARG;
    if (neg_hi <= neg_lo || neg_lo < 0 || (size_t)neg_hi > n_items) return PDA_ERR_ARG;
    if (pop && n_slots <= 0) return PDA_ERR_ARG;
    if ((pos_pop == nullptr) != (neg_pop == nullptr) || (pos_pop && !pop)) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    WarpArgs a{};
    a.U = U, a.I = I;
    a.s = SampleArgs{users, user_pool, indptr, indices, slots, pop, pos, neg, pos_pop, neg_pop, seed, step, B, n_pool, gen_users, neg_lo, neg_hi,
                     pop ? n_slots : 0, step_dev, step_next};
    a.wtab = wtab, a.trials = trials, a.coef = coef;
    a.cand = cand, a.cand_score = cand_score, a.pos_score = pos_score;
    a.stat = reinterpret_cast<unsigned long long*>(stat);
    a.n_users = (unsigned)n_users;
    a.T = T, a.margin = margin;
    a.rows_per_block = rows_per_block(B);
    const dim3 grid((unsigned)((B + a.rows_per_block - 1) / a.rows_per_block));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (d) {
        case 32: hipLaunchKernelGGL(warp_sample_kernel<32>, grid, dim3(kThreads), 0, st, a); break;
        case 64: hipLaunchKernelGGL(warp_sample_kernel<64>, grid, dim3(kThreads), 0, st, a); break;
        case 128: hipLaunchKernelGGL(warp_sample_kernel<128>, grid, dim3(kThreads), 0, st, a); break;
        default: hipLaunchKernelGGL(warp_sample_kernel<256>, grid, dim3(kThreads), 0, st, a); break;
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

// ---- the step ---------------------------------------------------------------------------------------------------------------------------------
struct WarpStepArgs {
    const float* U;
    const float* I;
    const int32_t* users;
    const int32_t* pos;
    const int32_t* neg;
    const float* coef;
    float* gU;
    float* gI;
    int32_t* tagU;
    int32_t* tagI;
    float* loss_acc;
    unsigned n_users, n_items;
    int tag;
    int B;
    float margin;
    float inv_B;
    float reg_c;            // regs / reg_div
    int any_order;          // PDA_UPD_ANY_ORDER
    int users_distinct;     // PDA_UPD_USERS_DISTINCT
};

template <int D>
__global__ void __launch_bounds__(512) warp_step_kernel(WarpStepArgs a) {
    constexpr int L = D / 4;        // lanes per triplet
    constexpr int TPB = 512 / L;    // triplets per block
    __shared__ float red[2][8];
    __shared__ int s_pos[TPB];
    __shared__ __attribute__((aligned(16))) float s_dpe[TPB * D];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;

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
        const float ct = a.coef[t];
        const f32x4 ue = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * D + 4 * e);
        const f32x4 pe = *reinterpret_cast<const f32x4*>(a.I + (size_t)p * D + 4 * e);
        const f32x4 ne = *reinterpret_cast<const f32x4*>(a.I + (size_t)n * D + 4 * e);
        float ps, ns;
        triplet_dots<D>(ue, pe, ne, ps, ns);
        const float h = a.margin - (ps - ns);
        const bool hinge = ct > 0.f && h > 0.f;                 // (a NaN compares false: an inactive triplet)
        const float gg = hinge ? -ct * a.inv_B : 0.f;           // d mf / dx
        if (e == 0 && hinge) maxi = -(ct * h);                  // the triplet's share of -B mf
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
    if (tid == 0 && a.loss_acc) block_loss_add(red, a.inv_B, a.reg_c, a.loss_acc);
}

int launch_step(const WarpStepArgs& a, int d, hipStream_t s) {
    PDA_STEP_LAUNCH(warp_step_kernel, d, a.B, s, a)
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

int check_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
               const float* coef, float margin, int B, int d, float reg_div, const float* gU, const float* gI, const int32_t* tagU,
               const int32_t* tagI, int step_tag, int flags) {
    if (!U || !I || !users || !pos || !neg || !coef || !gU || !gI || !tagU || !tagI) return PDA_ERR_ARG;
    if (B <= 0 || B > (1 << 28) || !(reg_div > 0.f) || step_tag <= 0 || margin != margin || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (flags & ~(PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT)) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    return PDA_OK;
}

WarpStepArgs step_args(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                       const float* coef, float margin, int B, float regs, float reg_div, float* gU, float* gI, int32_t* tagU, int32_t* tagI,
                       int step_tag, int flags, float* loss_acc) {
    return WarpStepArgs{U, I, users, pos, neg, coef, gU, gI, tagU, tagI, loss_acc, (unsigned)n_users, (unsigned)n_items, step_tag, B, margin,
                        1.0f / (float)B, regs / reg_div, (flags & PDA_UPD_ANY_ORDER) ? 1 : 0, (flags & PDA_UPD_USERS_DISTINCT) ? 1 : 0};
}

}  // namespace

extern "C" int pda_warp_sample_f32(const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
                                   const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr, const int32_t* train_indices,
                                   const int32_t* train_slots, const float* pop, int n_slots, int neg_lo, int neg_hi, int T, float margin,
                                   const float* wtab, uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg, int32_t* trials, float* coef,
                                   float* pos_pop, float* neg_pop, int32_t* cand, float* cand_score, float* pos_score, int64_t* stat, void* stream) {
    return warp_sample(false, U, I, n_users, n_items, d, users, gen_users, user_pool, n_pool, B, train_indptr, train_indices, train_slots, pop,
                       n_slots, neg_lo, neg_hi, T, margin, wtab, seed, step, nullptr, nullptr, pos, neg, trials, coef, pos_pop, neg_pop, cand,
                       cand_score, pos_score, stat, stream);
}

extern "C" int pda_warp_sample_f32_dev(const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
                                       const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr, const int32_t* train_indices,
                                       const int32_t* train_slots, const float* pop, int n_slots, int neg_lo, int neg_hi, int T, float margin,
                                       const float* wtab, uint64_t seed, const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* neg,
                                       int32_t* trials, float* coef, float* pos_pop, float* neg_pop, int32_t* cand, float* cand_score,
                                       float* pos_score, int64_t* stat, void* stream) {
    return warp_sample(true, U, I, n_users, n_items, d, users, gen_users, user_pool, n_pool, B, train_indptr, train_indices, train_slots, pop, n_slots,
                       neg_lo, neg_hi, T, margin, wtab, seed, 0, step_dev, step_next, pos, neg, trials, coef, pos_pop, neg_pop, cand, cand_score,
                       pos_score, stat, stream);
}

extern "C" int pda_warp_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos,
                                 const int32_t* neg, const float* coef, float margin, int B, int d, float regs, float reg_div, float* gU, float* gI,
                                 int32_t* tagU, int32_t* tagI, int step_tag, int flags, float* loss_acc, void* stream) {
    const int rc = check_step(U, I, n_users, n_items, users, pos, neg, coef, margin, B, d, reg_div, gU, gI, tagU, tagI, step_tag, flags);
    if (rc != PDA_OK) return rc;
    return launch_step(step_args(U, I, n_users, n_items, users, pos, neg, coef, margin, B, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags,
                                 loss_acc),
                       d, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_warp_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                      float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, const int32_t* neg,
                                      const float* coef, float margin, int B, int d, float regs, float reg_div, int step_tag, float lr_t,
                                      float beta1, float beta2, float eps, int flags, int cache_policy, float* loss_acc, void* stream) {
    if (!mU || !vU || !mI || !vI) return PDA_ERR_ARG;
    if (cache_policy < PDA_ADAM_CACHE_AUTO || cache_policy > PDA_ADAM_CACHE_STREAM) return PDA_ERR_ARG;
    int rc = check_step(U, I, n_users, n_items, users, pos, neg, coef, margin, B, d, reg_div, gU, gI, tagU, tagI, step_tag, flags);
    if (rc != PDA_OK) return rc;
    rc = launch_step(step_args(U, I, n_users, n_items, users, pos, neg, coef, margin, B, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags, loss_acc),
                     d, reinterpret_cast<hipStream_t>(stream));
    if (rc != PDA_OK) return rc;
    return pda_adam_dense_sweep4_f32(U, mU, vU, gU, n_users, tagU, I, mI, vI, gI, n_items, tagI, d, step_tag, lr_t, beta1, beta2, eps, cache_policy,
                                     stream);
}
