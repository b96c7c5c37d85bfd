// Dynamic hard-negative sampling (include/pda_hip_dns.h) on MI355X (gfx950): the triplet batch of pda_sample_triplets with the
// negative of a row picked among the best-scoring of M uniform candidates under the live tables.
//
// One launch, 512 threads, a workgroup owns R whole rows (R M <= 512 candidates; rows_per_block below: as a rule one round of the score phase,
// 8192 / d candidates, so that every gather of the workgroup is in flight at once) and runs four phases over LDS:
//   rows     thread q < R draws row q's user, positive and slot (the pieces of pda_sample.h, as sample_one composes them) and leaves the user,
//            the slot and the bounds of the train row in LDS;
//   draw     thread i < R M draws candidate i % M of row i / M (the body of ssm_sample_kernel) into LDS;
//   score    the 512 / (d/4) lane groups share the workgroup's candidates in contiguous runs; a group gathers four item rows (and their user
//            rows: the same row for a whole run once M exceeds the run, so L1 hits) per round, ids first, so that eight loads are in flight
//            under every ladder; lane 0 applies the head and leaves the score in LDS;
//   select   thread i counts the candidates of its row that stand before candidate i in the order (<= M LDS reads, the rows of a wave read
//            one address each: broadcasts); the one that counts t writes neg, pick_col and neg_pop.  No sort, no atomics.
// LDS: 16 KiB a workgroup; eight waves a workgroup, so the wave slots of a compute unit (four workgroups), not LDS, bound the occupancy.
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_sample.h"
#include "pda_hip_dns.h"

namespace {

struct DnsArgs {
    const float* U;
    const float* I;
    SampleArgs s;               // users .. n_slots, step_dev, step_next: what sample_one takes (neg: the pick)
    int32_t* cand;
    float* cand_score;
    int32_t* pick_col;
    unsigned n_users;
    int M, topn, head;
    int rows_per_block;         // R
    int score;                  // 0: M == 1 and no cand_score -- nothing depends on a score
};

constexpr int kThreads = 512;
constexpr int kChunk = 4;       // candidates gathered per round of a lane group

// Does candidate (sk, k) stand before candidate (si, j) of the same row?  Score descending, then column ascending; NaNs behind every number.
__device__ __forceinline__ bool dns_before(float sk, int k, float si, int j) {
    const bool nk = sk != sk, ni = si != si;
    if (nk || ni) return nk == ni ? k < j : ni;
    return sk > si || (sk == si && k < j);
}

template <int D>
__global__ void __launch_bounds__(kThreads) dns_sample_kernel(DnsArgs a) {
    constexpr int L = D / 4;            // lanes per candidate
    constexpr int G = kThreads / L;     // lane groups
    __shared__ int64_t s_b[kThreads], s_e[kThreads];
    __shared__ int s_user[kThreads], s_slot[kThreads], s_cand[kThreads];
    __shared__ float s_score[kThreads];
    const SampleArgs& s = a.s;
    const int tid = threadIdx.x, M = a.M;
    const int row0 = blockIdx.x * a.rows_per_block;
    const int rows = min(a.rows_per_block, s.B - row0);     // >= 1: the grid is ceil(B / R)
    const int n_cand = rows * M;                            // <= 512
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
    }
    __syncthreads();

    // ---- draw: candidate j of row q, the tries kNegDraw + kRejectTries j + ..
    const int q = tid / M, j = tid - q * M;
    const bool mine = tid < n_cand;
    int c = 0;
    if (mine) {
        c = sample_negative(s.seed, step, row0 + q, kNegDraw + kRejectTries * (uint32_t)j, (uint32_t)(s.neg_hi - s.neg_lo), s.indices, s_b[q], s_e[q],
                            [&](uint32_t x) { return s.neg_lo + (int)x; });
        s_cand[tid] = c;
        s_score[tid] = 0.f;
    }

    // ---- score: group g takes the candidates [g per, (g + 1) per)
    if (a.score) {
        __syncthreads();
        const int g = tid / L, e4 = 4 * (tid % L);
        const int per = (n_cand + G - 1) / G;
        const int end = min(n_cand, (g + 1) * per);
        for (int k0 = g * per; k0 < end; k0 += kChunk) {
            int at[kChunk], id[kChunk], us[kChunk];
            f32x4 ie[kChunk], ue[kChunk];
            float pw[kChunk];
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                at[k] = min(k0 + k, end - 1);                   // (the tail of the last round: the run's last candidate again, never stored)
                id[k] = s_cand[at[k]];
                us[k] = s_user[at[k] / M];
            }
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                ie[k] = ue[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                pw[k] = 0.f;
                if (us[k] >= 0) {                               // (an unknown user reads no table row)
                    ie[k] = *reinterpret_cast<const f32x4*>(a.I + (size_t)id[k] * D + e4);
                    ue[k] = *reinterpret_cast<const f32x4*>(a.U + (size_t)us[k] * D + e4);
                    // the popularity too, with the rows: a load behind the ladder would put its latency into every candidate's chain
                    if (a.head == PDA_HEAD_POP) pw[k] = s.pop[(size_t)id[k] * s.n_slots + s_slot[at[k] / M]];
                }
            }
#pragma unroll
            for (int k = 0; k < kChunk; ++k) {
                float x = dot4(ue[k], ie[k]);
#pragma unroll
                for (int o = L / 2; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
                if (a.head == PDA_HEAD_POP) x = (x > 0.f ? x + 1.f : expf(x)) * pw[k];
                if (e4 == 0 && k0 + k < end && us[k] >= 0) s_score[at[k]] = x;
            }
        }
    }
    __syncthreads();

    // ---- select: the candidate with t candidates of its row before it is the row's negative
    if (!mine) return;
    const int r = row0 + q;
    const float si = s_score[tid];
    if (a.cand) a.cand[(size_t)r * M + j] = c;
    if (a.cand_score) a.cand_score[(size_t)r * M + j] = si;
    int before = 0;
    if (s_user[q] < 0) {
        before = j;                                             // (an unknown user: candidate 0 is taken)
    } else {
        const float* row_score = s_score + q * M;
        for (int k = 0; k < M; ++k) before += dns_before(row_score[k], k, si, j) ? 1 : 0;
    }
    const int tn = min(a.topn, M);
    const int t = (tn > 1 && s_user[q] >= 0) ? (int)bounded(draw(s.seed, step, r, kPickDraw), (uint32_t)tn) : 0;
    if (before == t) {
        s.neg[r] = c;
        if (a.pick_col) a.pick_col[r] = j;
        if (s.neg_pop) s.neg_pop[r] = s.pop[(size_t)c * s.n_slots + s_slot[q]];
    }
}

// (host) R, the rows of a workgroup.  One round of the score phase is kChunk candidates per lane group, 8192 / d per workgroup: R M is that
// many candidates (as many whole rows as fit; never less than a row, never more than kThreads candidates) -- every gather of the workgroup is
// in flight at once and the call spreads over B M d / 8192 workgroups instead of B M / 512.  Only where that leaves more than kResident
// workgroups (two on each of 256 compute units) do the rows of a workgroup double, up to kThreads / M: from there on the fixed part of a
// workgroup (the rows phase, two barriers) costs more than a further round of gathers.  Measured at B = 2 048 with 128 / 256 / 512 / 1 024
// (profiles/dns_timing.txt): 512 is best or level at every M and d.  Without a score phase (M == 1, no cand_score) a workgroup takes a
// wave's worth of rows.
constexpr int kResident = 512;
int rows_per_block(int B, int M, int d, bool score) {
    const int cap = kThreads / M > 0 ? kThreads / M : 1;
    const int round = score ? kChunk * kThreads / (d / 4) : 64;
    int R = round / M > 0 ? round / M : 1;
    if (R > cap) R = cap;
    while (R < cap && (B + R - 1) / R > kResident) R = 2 * R < cap ? 2 * R : cap;
    return R;
}

// Both entry points.  counter (pda_dns_sample_f32_dev): the step is read on the device; else it travels by value and the two are null.
int dns_sample(bool counter, const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
               const int32_t* user_pool, int n_pool, int B, const int64_t* indptr, const int32_t* indices, const int32_t* slots, const float* pop,
               int n_slots, int neg_lo, int neg_hi, int M, int topn, int head, uint64_t seed, uint64_t step, const uint64_t* step_dev,
               uint64_t* step_next, int32_t* pos, int32_t* neg, float* pos_pop, float* neg_pop, int32_t* cand, float* cand_score, int32_t* pick_col,
               void* stream) {
    if (!U || !I || !sample_call_ok(users, indptr, indices, pos, neg, gen_users, n_pool, counter, step_dev, step_next)) return PDA_ERR_ARG;
    if (B <= 0 || B > (1 << 22) || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (M < 1 || M > PDA_DNS_MAX_CANDIDATES || topn < 1 || topn > M) return PDA_ERR_ARG;
    if (neg_hi <= neg_lo || neg_lo < 0 || (size_t)neg_hi > n_items) return PDA_ERR_ARG;
    if (head != PDA_HEAD_RAW && head != PDA_HEAD_POP) return PDA_ERR_ARG;
    if ((head == PDA_HEAD_POP && !pop) || (pop && n_slots <= 0)) return PDA_ERR_ARG;
    if ((pos_pop == nullptr) != (neg_pop == nullptr) || (pos_pop && !pop)) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    DnsArgs a{};
    a.U = U, a.I = I;
    a.s = SampleArgs{users, user_pool, indptr, indices, slots, pop, pos, neg, pos_pop, neg_pop, seed, step, B, n_pool, gen_users, neg_lo, neg_hi,
                     pop ? n_slots : 0, step_dev, step_next};
    a.cand = cand, a.cand_score = cand_score, a.pick_col = pick_col;
    a.n_users = (unsigned)n_users;
    a.M = M, a.topn = topn, a.head = head;
    a.score = (M > 1 || cand_score) ? 1 : 0;
    a.rows_per_block = rows_per_block(B, M, d, a.score != 0);
    const dim3 grid((unsigned)((B + a.rows_per_block - 1) / a.rows_per_block));
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    switch (d) {
        case 32: hipLaunchKernelGGL(dns_sample_kernel<32>, grid, dim3(kThreads), 0, st, a); break;
        case 64: hipLaunchKernelGGL(dns_sample_kernel<64>, grid, dim3(kThreads), 0, st, a); break;
        case 128: hipLaunchKernelGGL(dns_sample_kernel<128>, grid, dim3(kThreads), 0, st, a); break;
        default: hipLaunchKernelGGL(dns_sample_kernel<256>, grid, dim3(kThreads), 0, st, a); break;
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" int pda_dns_sample_f32(const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
                                  const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr, const int32_t* train_indices,
                                  const int32_t* train_slots, const float* pop, int n_slots, int neg_lo, int neg_hi, int M, int topn, int head,
                                  uint64_t seed, uint64_t step, int32_t* pos, int32_t* neg, float* pos_pop, float* neg_pop, int32_t* cand,
                                  float* cand_score, int32_t* pick_col, void* stream) {
    return dns_sample(false, U, I, n_users, n_items, d, users, gen_users, user_pool, n_pool, B, train_indptr, train_indices, train_slots, pop, n_slots,
                      neg_lo, neg_hi, M, topn, head, seed, step, nullptr, nullptr, pos, neg, pos_pop, neg_pop, cand, cand_score, pick_col, stream);
}

extern "C" int pda_dns_sample_f32_dev(const float* U, const float* I, size_t n_users, size_t n_items, int d, int32_t* users, int gen_users,
                                      const int32_t* user_pool, int n_pool, int B, const int64_t* train_indptr, const int32_t* train_indices,
                                      const int32_t* train_slots, const float* pop, int n_slots, int neg_lo, int neg_hi, int M, int topn, int head,
                                      uint64_t seed, const uint64_t* step_dev, uint64_t* step_next, int32_t* pos, int32_t* neg, float* pos_pop,
                                      float* neg_pop, int32_t* cand, float* cand_score, int32_t* pick_col, void* stream) {
    return dns_sample(true, U, I, n_users, n_items, d, users, gen_users, user_pool, n_pool, B, train_indptr, train_indices, train_slots, pop, n_slots,
                      neg_lo, neg_hi, M, topn, head, seed, 0, step_dev, step_next, pos, neg, pos_pop, neg_pop, cand, cand_score, pick_col, stream);
}
