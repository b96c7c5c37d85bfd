// Calibrated-popularity re-ranking (up to 8 popularity groups) for MI355X (gfx950): include/pda_hip_calib.h, DESIGN.md "5w. Calibrated popularity".
//
// The route without this file is a loop of K steps over [users, N] tensors with G divergences per user and step.  Here one wave owns one row
// (user), four rows per workgroup, in all three kernels:
//   profile    the history row is walked once, 64 entries at a time; an entry counts when it differs from the one before it (the row is
//              sorted), lies inside the catalogue and has a group.  A group's count is a sum of ballots; lane g writes group g.
//   counts     a list is walked 64 columns at a time, one ballot per group; lane 8 j + g counts group g below cut-off j from those ballots.
//   rerank     members    W >= 0 and rounding is monotone, so inside a group the candidates keep their list order at every step: the greedy
//                         selection is a G-way merge of the group sub-lists, and only the first K members of each group can ever be picked.
//                         The candidates are read in chunks of 64 (one dword per lane), the next chunk's loads in flight under the current
//                         chunk's gather of group bytes.  A group's members of a chunk are one ballot, a member's rank a popcount below its
//                         lane.  Members of rank < K go to the wave's LDS slots [group][rank] (value and position); reading stops once every group holds K members
//                         or the valid prefix ends.
//              the end    as in pda_xquad.hip: when the chunks stopped early, the end of the prefix is searched for in two probes of 64 and
//                         at most 13 positions (the invalid suffix is contiguous: a precondition).
//              merge      lane 8 c + g computes term g of the divergence the list would have with one more item of group c: the G^2 <= 64
//                         terms of a step at once, in double.  Lane 8 c adds its group's terms in ascending g (the order is the contract),
//                         puts the sum on the 2^-20 grid and takes x of its group's head member from LDS; the G heads are compared on
//                         (x, position), and lane t keeps step t's pick.  Behind the loop lane t reads its pick's position from LDS and the id at that position: the row's K
//                         outputs are one store per array.
// Nothing is shared between rows: the result does not depend on the geometry.
#include <math.h>

#include "pda_common.h"
#include "pda_hip_calib.h"

namespace {

constexpr int kCbRows = 4;                  // rows (waves) per workgroup
constexpr int kCbG = PDA_CALIB_MAX_G;       // 8: the lane layout 8 c + g below

__device__ __forceinline__ int cb_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// number of leading set bits of a ballot, counted from lane 0
__device__ __forceinline__ int cb_leading(unsigned long long m) { return m == ~0ull ? 64 : __builtin_ctzll(~m); }

__device__ __forceinline__ double cb_shfl(double v, int src_lane) {
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(uint32_t)b);
    const int hi = __builtin_amdgcn_ds_bpermute(src_lane << 2, (int)(uint32_t)((unsigned long long)b >> 32));
    return __longlong_as_double((long long)(((unsigned long long)(uint32_t)hi << 32) | (uint32_t)lo));
}

// ---- the profile ---------------------------------------------------------------------------------------------------------------------------
struct CalibProfileArgs {
    const int32_t* users;
    const int64_t* hist_indptr;
    const int32_t* hist_indices;
    const uint8_t* item_group;
    int32_t* prof;
    int hist_row_mode, n_rows, n_items, G;
};

__global__ void __launch_bounds__(64 * kCbRows) calib_profile_kernel(CalibProfileArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = cb_uniform((int)(threadIdx.x >> 6));
    const int row = blockIdx.x * kCbRows + wave;
    if (row >= a.n_rows) return;
    const int G = a.G;
    int mine = 0;                                  // lane g: the entries of group g
    if (a.hist_indptr != nullptr) {
        const int64_t hr = a.hist_row_mode == PDA_HIST_BY_USER_ID ? (int64_t)a.users[row] : (int64_t)row;
        const int64_t p0 = a.hist_indptr[hr], p1 = a.hist_indptr[hr + 1];
        for (int64_t b = p0; b < p1; b += 64) {
            const int64_t p = b + lane;
            int gb = kCbG;                         // no group
            if (p < p1) {
                const int32_t it = a.hist_indices[p];
                if ((uint32_t)it < (uint32_t)a.n_items && (p == p0 || a.hist_indices[p - 1] != it)) gb = a.item_group[it];
            }
#pragma unroll
            for (int c = 0; c < kCbG; ++c) {
                if (c < G) {
                    const int n = __popcll(__ballot(gb == c));
                    if (lane == c) mine += n;
                }
            }
        }
    }
    if (lane < G) a.prof[(size_t)row * G + lane] = mine;
}

// ---- the group counts of a list -----------------------------------------------------------------------------------------------------------
struct CalibCountArgs {
    const int32_t* idx;
    const uint8_t* item_group;
    int32_t* cnt;
    int n_rows, K, n_items, G, nK, k_max;       // k_max = ks[nK - 1] <= K: columns behind it are not read
    int ks[PDA_CALIB_MAX_KS];
};

__global__ void __launch_bounds__(64 * kCbRows) calib_counts_kernel(CalibCountArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = cb_uniform((int)(threadIdx.x >> 6));
    const int row = blockIdx.x * kCbRows + wave;
    if (row >= a.n_rows) return;
    const int G = a.G, K = a.K;
    const int j = lane >> 3, g = lane & 7;          // lane 8 j + g: group g below cut-off j
    int my_k = 0;
#pragma unroll
    for (int i = 0; i < PDA_CALIB_MAX_KS; ++i)
        if (i == j && i < a.nK) my_k = a.ks[i];
    const int k_max = a.k_max;
    int mine = 0;
    for (int base = 0; base < k_max; base += 64) {
        const int col = base + lane;
        int gb = kCbG;
        if (col < k_max) {
            const int32_t it = a.idx[(size_t)row * K + col];
            if ((uint32_t)it < (uint32_t)a.n_items) gb = a.item_group[it];
        }
        unsigned long long m = 0;
#pragma unroll
        for (int c = 0; c < kCbG; ++c) {
            if (c < G) {
                const unsigned long long mc = __ballot(gb == c);
                if (g == c) m = mc;
            }
        }
        const int below = my_k - base;              // columns of this chunk in front of the lane's cut-off
        if (below > 0) mine += __popcll(below >= 64 ? m : m & ((1ull << below) - 1ull));
    }
    if (j < a.nK && g < G) a.cnt[((size_t)row * a.nK + j) * G + g] = mine;
}

// ---- the selection -------------------------------------------------------------------------------------------------------------------------
struct CalibArgs {
    const int32_t* cand_idx;
    const float* cand_val;
    const int32_t* prof;
    const uint8_t* item_group;
    int32_t* out_idx;
    float* out_val;
    float* out_div;
    double alpha, one_minus_alpha;
    float L, W;
    int n_rows, N, n_items, G, K;
};

template <int VARIANT>
__global__ void __launch_bounds__(64 * kCbRows) calib_rerank_kernel(CalibArgs a) {
    __shared__ float s_val[kCbRows][kCbG][64];      // a member's value, then W p of it
    __shared__ int32_t s_pos[kCbRows][kCbG][64];
    const int lane = threadIdx.x & 63;
    const int wave = cb_uniform((int)(threadIdx.x >> 6));
    const int row = blockIdx.x * kCbRows + wave;
    if (row >= a.n_rows) return;   // (whole waves leave: nothing below synchronises across waves)
    const int N = a.N, K = a.K, G = a.G;
    const int32_t* cidx = a.cand_idx + (size_t)row * N;
    const float* cval = a.cand_val + (size_t)row * N;
    const unsigned long long below = (1ull << lane) - 1ull;
    auto load = [&](int v, int32_t& id, float& x) {   // a position behind the row: id -1
        id = -1;
        x = 0.f;
        if (v < N) {
            id = cidx[v];
            x = cval[v];
        }
    };
    // the group byte of a candidate, kCbG (no group) for an invalid one: valid <=> below G
    auto group_of = [&](int32_t id, float x) -> int {
        int gb = kCbG;
        if ((uint32_t)id < (uint32_t)a.n_items && fabsf(x) < INFINITY) gb = a.item_group[id];
        return gb;
    };

    int32_t idA, idB;
    float xA, xB;
    load(lane, idA, xA);

    // ---- the target: lane 8 c + g holds pi_g ----
    const int c_ = lane >> 3, g_ = lane & 7;
    const bool term_lane = c_ < G && g_ < G;
    const int my_prof = g_ < G ? a.prof[(size_t)row * G + g_] : 0;
    long long H = 0;
#pragma unroll
    for (int g = 0; g < kCbG; ++g)
        if (g < G) H += (long long)__builtin_amdgcn_readlane(my_prof, g);
    const bool no_profile = H == 0;
    const double pi = no_profile ? 0.0 : (double)my_prof / (double)H;

    // ---- the first K members of each group ----
    int cnt[kCbG];
#pragma unroll
    for (int c = 0; c < kCbG; ++c) cnt[c] = 0;
    int n_valid = -1, base = 0;
    const float first = pda_readlane_f32(xA, 0);   // val[0] (used when n_valid > 0)
    float last = 0.f;                              // val[n_valid - 1], once n_valid is known; before: the value at the end of the last chunk
    bool full = false;
    for (;;) {
        load(base + 64 + lane, idB, xB);           // the next chunk, in flight under this one's gather
        const int gb = group_of(idA, xA);
        const int nok = cb_leading(__ballot(gb < G));
        const bool live = lane < nok;
        full = true;
#pragma unroll
        for (int c = 0; c < kCbG; ++c) {
            if (c < G) {
                const unsigned long long m = __ballot(live && gb == c);
                if (live && gb == c) {
                    const int r = cnt[c] + __popcll(m & below);
                    if (r < K) {
                        s_val[wave][c][r] = xA;
                        s_pos[wave][c][r] = base + lane;
                    }
                }
                cnt[c] += __popcll(m);
                full = full && cnt[c] >= K;
            }
        }
        if (nok < 64) {
            n_valid = base + nok;
            if (nok > 0) last = pda_readlane_f32(xA, nok - 1);   // (nok == 0: `last` is the value at the end of the chunk before, or unused)
            break;
        }
        last = pda_readlane_f32(xA, 63);
        base += 64;
        if (full || base >= N) break;
        idA = idB;
        xA = xB;
    }
    int my_cnt = 0;                                // lane 8 c + g: the members kept of group c
#pragma unroll
    for (int c = 0; c < kCbG; ++c) {
        cnt[c] = min(cnt[c], K);
        if (c == c_) my_cnt = cnt[c];
    }

    // ---- the end of the valid prefix, when the chunks stopped before it: the positions below base are valid ----
    if (n_valid < 0) {
        n_valid = N;                              // (base >= N: the chunks covered the row; `last` is val[N - 1])
        if (base < N) {
            const int s = (N - base + 63) >> 6;   // <= 15
            int32_t id1, id2;
            float x1, x2;
            load(base + lane * s, id1, x1);
            const int j = cb_leading(__ballot(group_of(id1, x1) < G));
            if (j == 0) {
                n_valid = base;
            } else {
                const int at = base + (j - 1) * s;   // valid; at + s is not, or lies behind the row
                load(lane < s - 1 ? at + 1 + lane : N, id2, x2);
                const int k = cb_leading(__ballot(group_of(id2, x2) < G));
                n_valid = at + 1 + k;
                last = k > 0 ? pda_readlane_f32(x2, k - 1) : pda_readlane_f32(x1, j - 1);
            }
        }
    }
    n_valid = cb_uniform(n_valid);
    const int steps = min(K, n_valid);

    // ---- relevance: lane r normalises member r of every group ----
    const float lo = last, rng = n_valid > 0 ? first - lo : 0.f;
    const bool flat = !(rng != 0.f && fabsf(rng) < INFINITY);
    pda_wave_sync();
#pragma unroll
    for (int c = 0; c < kCbG; ++c) {
        if (c < G && lane < cnt[c]) s_val[wave][c][lane] = a.W * (flat ? 0.f : (s_val[wave][c][lane] - lo) / rng);
    }
    pda_wave_sync();

    // ---- the merge ----
    int my_ng = 0, my_nc = 0;                      // lane 8 c + g: the picks of group g and of group c so far
    int my_pick = 0, my_n = 0;                     // lane t keeps step t: the group it picked and that group's picks before it
    float my_x = -INFINITY, my_d = -INFINITY;
    for (int t = 0; t < steps; ++t) {
        double term = 0.0;
        if (term_lane && !no_profile) {
            const double q = (double)(my_ng + (g_ == c_ ? 1 : 0)) / (double)(t + 1);
            if (VARIANT == PDA_CALIB_JS) {
                const double m = 0.5 * (pi + q);
                const double ta = pi > 0.0 ? pi * log2(pi / m) : 0.0;
                const double tb = q > 0.0 ? q * log2(q / m) : 0.0;
                term = ta + tb;
            } else {
                const double qs = a.one_minus_alpha * q + a.alpha * pi;
                term = pi > 0.0 ? pi * log(pi / qs) : 0.0;
            }
        }
        double sum = term;                         // lane 8 c: term_0 + term_1 + ... in ascending g
#pragma unroll
        for (int g = 1; g < kCbG; ++g)
            if (g < G) sum += cb_shfl(term, lane + g);
        const double D = VARIANT == PDA_CALIB_JS ? 0.5 * sum : sum;
        const double Dq = fmin(fmax(rint(D * 1048576.0), 0.0), 8388608.0);
        const float d32 = (float)(int)Dq * 9.5367431640625e-07f;   // 2^-20: exact
        float x = -INFINITY;
        int pos = 0x7FFFFFFF;
        if (c_ < G && my_nc < my_cnt) {            // (behind a group's members: x = -inf, an exhausted group never wins)
            x = s_val[wave][c_][my_nc] - a.L * d32;
            pos = s_pos[wave][c_][my_nc];
        }
        int pick = 0;
        float bx = pda_readlane_f32(x, 0);
        int bp = __builtin_amdgcn_readlane(pos, 0);
#pragma unroll
        for (int c = 1; c < kCbG; ++c) {
            if (c < G) {
                const float xc = pda_readlane_f32(x, 8 * c);
                const int pc = __builtin_amdgcn_readlane(pos, 8 * c);
                if (xc > bx || (xc == bx && pc < bp)) {    // (steps <= the members kept: one of the heads is a member)
                    pick = c;
                    bx = xc;
                    bp = pc;
                }
            }
        }
        pick = cb_uniform(pick);
        const float dp = pda_readlane_f32(d32, 8 * pick);
        const int np = __builtin_amdgcn_readlane(my_nc, 8 * pick);
        if (lane == t) {
            my_pick = pick;
            my_n = min(np, 63);                    // (a member's rank; the bound only matters on a list that breaks a precondition)
            my_x = bx;
            my_d = dp;
        }
        my_ng += g_ == pick ? 1 : 0;
        my_nc += c_ == pick ? 1 : 0;
    }
    if (lane < K) {
        int32_t oid = -1;
        if (lane < steps) {
            const int pos = s_pos[wave][my_pick][my_n];          // (the id is read again: 16 KB of LDS per workgroup instead of 24)
            if ((uint32_t)pos < (uint32_t)N) oid = cidx[pos];
        }
        a.out_idx[(size_t)row * K + lane] = oid;
        a.out_val[(size_t)row * K + lane] = my_x;
        if (a.out_div != nullptr) a.out_div[(size_t)row * K + lane] = my_d;
    }
}

bool cb_groups_ok(int G) { return G >= 2 && G <= PDA_CALIB_MAX_G; }

}  // namespace

extern "C" int pda_calib_profile(const int32_t* users, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, int n_rows,
                                 const uint8_t* item_group, int n_items, int G, int32_t* prof, void* stream) {
    if (!item_group || !prof) return PDA_ERR_ARG;
    if (n_rows < 1 || n_items < 1 || !cb_groups_ok(G)) return PDA_ERR_ARG;
    if (hist_indptr) {
        if (!hist_indices || (hist_row_mode != PDA_HIST_BY_BLOCK_ROW && hist_row_mode != PDA_HIST_BY_USER_ID)) return PDA_ERR_ARG;
        if (hist_row_mode == PDA_HIST_BY_USER_ID && !users) return PDA_ERR_ARG;
    }
    CalibProfileArgs a{users, hist_indptr, hist_indices, item_group, prof, hist_row_mode, n_rows, n_items, G};
    hipLaunchKernelGGL(calib_profile_kernel, dim3((unsigned)((n_rows + kCbRows - 1) / kCbRows)), dim3(64 * kCbRows), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_calib_list_counts(const int32_t* idx, int n_rows, int K, const uint8_t* item_group, int n_items, int G, const int32_t* Ks,
                                     int nK, int32_t* cnt, void* stream) {
    if (!idx || !item_group || !Ks || !cnt) return PDA_ERR_ARG;
    if (n_rows < 1 || n_items < 1 || K < 1 || K > PDA_CALIB_MAX_N || !cb_groups_ok(G)) return PDA_ERR_ARG;
    if (nK < 1 || nK > PDA_CALIB_MAX_KS) return PDA_ERR_ARG;
    CalibCountArgs a{idx, item_group, cnt, n_rows, K, n_items, G, nK, 0, {0, 0, 0, 0, 0, 0, 0, 0}};
    for (int j = 0; j < nK; ++j) {
        if (Ks[j] < 1 || Ks[j] > K || (j > 0 && Ks[j] <= Ks[j - 1])) return PDA_ERR_ARG;
        a.ks[j] = Ks[j];
    }
    a.k_max = Ks[nK - 1];
    hipLaunchKernelGGL(calib_counts_kernel, dim3((unsigned)((n_rows + kCbRows - 1) / kCbRows)), dim3(64 * kCbRows), 0,
                       reinterpret_cast<hipStream_t>(stream), a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_calib_rerank(const int32_t* cand_idx, const float* cand_val, int n_rows, int N, const int32_t* prof, const uint8_t* item_group,
                                int n_items, int G, double lambda, int variant, double alpha, int K, int32_t* out_idx, float* out_val,
                                float* out_div, void* stream) {
    if (!cand_idx || !cand_val || !prof || !item_group || !out_idx || !out_val) return PDA_ERR_ARG;
    if (n_rows < 1 || n_items < 1 || N < 1 || N > PDA_CALIB_MAX_N || !cb_groups_ok(G)) return PDA_ERR_ARG;
    if (K < 1 || K > PDA_CALIB_MAX_K || K > N) return PDA_ERR_ARG;
    if (!(lambda >= 0.0 && lambda <= 1.0)) return PDA_ERR_ARG;   // (NaN fails both)
    if (variant != PDA_CALIB_JS && variant != PDA_CALIB_KL) return PDA_ERR_ARG;
    if (variant == PDA_CALIB_KL && !(alpha > 0.0 && alpha < 1.0)) return PDA_ERR_ARG;
    if (variant == PDA_CALIB_JS) alpha = 0.0;                    // (not read)
    CalibArgs a{cand_idx, cand_val, prof, item_group, out_idx, out_val, out_div, alpha, 1.0 - alpha, (float)lambda, (float)(1.0 - lambda),
                n_rows, N, n_items, G, K};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n_rows + kCbRows - 1) / kCbRows));
    if (variant == PDA_CALIB_JS)
        hipLaunchKernelGGL(calib_rerank_kernel<PDA_CALIB_JS>, grid, dim3(64 * kCbRows), 0, s, a);
    else
        hipLaunchKernelGGL(calib_rerank_kernel<PDA_CALIB_KL>, grid, dim3(64 * kCbRows), 0, s, a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
