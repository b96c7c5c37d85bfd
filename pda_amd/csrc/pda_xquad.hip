// xQuAD (personalised popularity re-ranking, two categories) for MI355X (gfx950): include/pda_hip_xquad.h, DESIGN.md "5e. xQuAD".
//
// The route without this file is a loop of K steps over [users, N] tensors.  Here one wave owns one row (user), four rows per workgroup:
//   profile    the history row is walked once, 64 entries at a time; an entry counts when it differs from the one before it (the row is
//              sorted) and lies inside the catalogue.  H and H1 are sums of two ballots.
//   members    W >= 0 and rounding is monotone, so inside a category the candidates keep their list order at every step: the greedy selection
//              is a merge of the two category sub-lists, and only the first K members of each category can ever be picked.  The candidates
//              are read in chunks of 64 (one dword per lane, 256 contiguous bytes per load whatever the row's alignment), two chunks per
//              trip so that their loads and their category gathers are in flight together; the first trip's loads are issued ahead of the
//              profile.  (Four chunks per trip measured slower: a gather of 64 category bytes from 64 cache lines is the kernel's most
//              expensive instruction, about 0.08 ms per 262 144 rows, and two of the four were often not needed)  The categories of a chunk are one ballot, a member's rank in its category a popcount below its lane.  Members of
//              rank < K go to the wave's LDS slots [category][rank]; reading stops once both categories hold K members or the valid prefix ends.
//   the end    the normalisation needs n_valid and val[n_valid - 1].  When the chunks stopped early, the end of the prefix is searched for
//              in two probes of 64 and at most 13 positions (the invalid suffix is contiguous: a precondition); the value comes from the lane
//              that probed it.
//   merge      lane i holds x of member i of both categories as it would be with n_c = i; a step fetches the two lanes n_0 and n_1
//              (ds_bpermute), compares, and lane t keeps step t's category and count.  The smooth variant renews the lanes' x at every
//              step (one division per step, in all lanes at once); the binary one computes them once.  Behind the loop lane t reads its
//              pick's id from LDS and computes its x again: the row's K outputs are one store per array.
// Nothing is shared between rows: the result does not depend on the geometry.
#include <math.h>

#include "pda_common.h"
#include "pda_hip_xquad.h"

namespace {

constexpr int kXqRows = 4;   // rows (waves) per workgroup

struct XquadArgs {
    const int32_t* cand_idx;
    const float* cand_val;
    const uint8_t* is_head;
    const int32_t* users;
    const int64_t* hist_indptr;
    const int32_t* hist_indices;
    int32_t* out_idx;
    float* out_val;
    float L, W;
    int n_rows, N, n_items, hist_row_mode, K;
};

__device__ __forceinline__ int xq_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

// number of leading set bits of a ballot, counted from lane 0
__device__ __forceinline__ int xq_leading(unsigned long long m) { return m == ~0ull ? 64 : __builtin_ctzll(~m); }

template <int VARIANT>
__device__ __forceinline__ float xq_cov(int n, int t) {
    if (VARIANT == PDA_XQUAD_BINARY) return n == 0 ? 1.f : 0.f;
    return t == 0 ? 1.f : 1.f - (float)n / (float)t;
}

template <int VARIANT>
__global__ void __launch_bounds__(64 * kXqRows) xquad_rerank_kernel(XquadArgs a) {
    __shared__ float s_val[kXqRows][2][64];      // a member's value, then W p of it
    __shared__ int32_t s_id[kXqRows][2][64];
    __shared__ int32_t s_pos[kXqRows][2][64];
    const int lane = threadIdx.x & 63;
    const int wave = xq_uniform((int)(threadIdx.x >> 6));
    const int row = blockIdx.x * kXqRows + wave;
    if (row >= a.n_rows) return;   // (whole waves leave: nothing below synchronises across waves)
    const int N = a.N, K = a.K;
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
    auto valid = [&](int32_t id, float x) -> bool { return (uint32_t)id < (uint32_t)a.n_items && fabsf(x) < INFINITY; };

    int32_t idA, idB;
    float xA, xB;
    load(lane, idA, xA);
    load(64 + lane, idB, xB);

    // ---- the profile ----
    float q0 = 0.f, q1 = 0.f;
    if (a.hist_indptr != nullptr) {
        const int64_t hr = a.hist_row_mode == PDA_HIST_BY_USER_ID ? (int64_t)a.users[row] : (int64_t)row;
        const int64_t p0 = a.hist_indptr[hr], p1 = a.hist_indptr[hr + 1];
        int H = 0, H1 = 0;
        for (int64_t b = p0; b < p1; b += 64) {
            const int64_t p = b + lane;
            bool ok = false, hd = false;
            if (p < p1) {
                const int32_t it = a.hist_indices[p];
                ok = (uint32_t)it < (uint32_t)a.n_items && (p == p0 || a.hist_indices[p - 1] != it);
                if (ok) hd = a.is_head[it] != 0;
            }
            H += __popcll(__ballot(ok));
            H1 += __popcll(__ballot(hd));
        }
        if (H > 0) {
            q1 = (float)H1 / (float)H;
            q0 = (float)(H - H1) / (float)H;
        }
    }

    // ---- the first K members of each category ----
    int cnt0 = 0, cnt1 = 0, n_valid = -1, base = 0;
    const float first = pda_readlane_f32(xA, 0);   // val[0] (used when n_valid > 0)
    float last = 0.f;                              // val[n_valid - 1], once n_valid is known; before: the value at the end of the last chunk
    bool full = false;
    auto commit = [&](int at, int32_t id, float x, bool hd, int nok) {   // the members of the chunk at `at`, whose first nok positions are valid
        const bool live = lane < nok;
        const unsigned long long hm = __ballot(hd), tm = __ballot(live && !hd);
        if (live) {
            const int c = hd ? 1 : 0;
            const int r = hd ? cnt1 + __popcll(hm & below) : cnt0 + __popcll(tm & below);
            if (r < K) {
                s_val[wave][c][r] = x;
                s_id[wave][c][r] = id;
                s_pos[wave][c][r] = at + lane;
            }
        }
        cnt1 += __popcll(hm);
        cnt0 += __popcll(tm);
        full = cnt0 >= K && cnt1 >= K;
    };
    for (;;) {
        const int nokA = xq_leading(__ballot(valid(idA, xA))), nokB = xq_leading(__ballot(valid(idB, xB)));
        const bool hdA = lane < nokA && a.is_head[idA] != 0;
        const bool hdB = lane < nokB && a.is_head[idB] != 0;
        commit(base, idA, xA, hdA, nokA);
        if (nokA < 64) {
            n_valid = base + nokA;
            if (nokA > 0) last = pda_readlane_f32(xA, nokA - 1);
            break;
        }
        if (!full) commit(base + 64, idB, xB, hdB, nokB);
        if (nokB < 64) {
            n_valid = base + 64 + nokB;
            last = pda_readlane_f32(nokB > 0 ? xB : xA, nokB > 0 ? nokB - 1 : 63);
            break;
        }
        last = pda_readlane_f32(xB, 63);
        base += 128;
        if (full || base >= N) break;
        load(base + lane, idA, xA);
        load(base + 64 + lane, idB, xB);
    }
    cnt0 = min(cnt0, K);
    cnt1 = min(cnt1, K);

    // ---- the end of the valid prefix, when the chunks stopped before it: the positions below base are valid ----
    if (n_valid < 0) {
        n_valid = N;                              // (base >= N: the chunks covered the row; `last` is val[N - 1])
        if (base < N) {
            const int s = (N - base + 63) >> 6;   // <= 14
            int32_t id1, id2;
            float x1, x2;
            load(base + lane * s, id1, x1);
            const int j = xq_leading(__ballot(valid(id1, x1)));
            if (j == 0) {
                n_valid = base;
            } else {
                const int at = base + (j - 1) * s;   // valid; at + s is not, or lies behind the row
                load(lane < s - 1 ? at + 1 + lane : N, id2, x2);
                const int k = xq_leading(__ballot(valid(id2, x2)));
                n_valid = at + 1 + k;
                last = k > 0 ? pda_readlane_f32(x2, k - 1) : pda_readlane_f32(x1, j - 1);
            }
        }
    }
    n_valid = xq_uniform(n_valid);
    const int steps = min(K, n_valid);

    // ---- relevance: lane r normalises member r of both categories ----
    const float lo = last, rng = n_valid > 0 ? first - lo : 0.f;
    const bool flat = !(rng != 0.f && fabsf(rng) < INFINITY);
    pda_wave_sync();
    float wp0 = -INFINITY, wp1 = -INFINITY;   // (behind a list's members: x = -inf, an exhausted list never wins)
    int32_t pos0 = 0, pos1 = 0;
    if (lane < cnt0) {
        wp0 = a.W * (flat ? 0.f : (s_val[wave][0][lane] - lo) / rng);
        pos0 = s_pos[wave][0][lane];
        s_val[wave][0][lane] = wp0;
    }
    if (lane < cnt1) {
        wp1 = a.W * (flat ? 0.f : (s_val[wave][1][lane] - lo) / rng);
        pos1 = s_pos[wave][1][lane];
        s_val[wave][1][lane] = wp1;
    }
    pda_wave_sync();

    // ---- the merge: lane i holds x of member i of each category for n_c = i; a step fetches the lanes n_0 and n_1 (ds_bpermute: the
    // counts stay in vector registers, the same in every lane -- the CU's one scalar unit is what a loop on read lanes waits for) ----
    int a0 = 0, a1 = 0;               // 4 n_0, 4 n_1: the byte addresses ds_bpermute takes
    int my_n1 = 0, my_pick = 0;       // lane t keeps step t: n_1 before it and the category it picked
    float x0v = wp0 + a.L * (q0 * xq_cov<PDA_XQUAD_BINARY>(lane, 0)), x1v = wp1 + a.L * (q1 * xq_cov<PDA_XQUAD_BINARY>(lane, 0));
    for (int t = 0; t < steps; ++t) {
        if (VARIANT == PDA_XQUAD_SMOOTH) {
            const float cov = xq_cov<PDA_XQUAD_SMOOTH>(lane, t);
            x0v = wp0 + a.L * (q0 * cov);
            x1v = wp1 + a.L * (q1 * cov);
        }
        const float x0 = __int_as_float(__builtin_amdgcn_ds_bpermute(a0, __float_as_int(x0v)));
        const float x1 = __int_as_float(__builtin_amdgcn_ds_bpermute(a1, __float_as_int(x1v)));
        const int p0 = __builtin_amdgcn_ds_bpermute(a0, pos0), p1 = __builtin_amdgcn_ds_bpermute(a1, pos1);
        const int pick = (x1 > x0 || (x1 == x0 && p1 < p0)) ? 1 : 0;      // (steps <= the members kept: one of the two is a member)
        if (lane == t) {
            my_n1 = a1;
            my_pick = pick;
        }
        a1 += 4 * pick;
        a0 += 4 - 4 * pick;
    }
    if (lane < K) {
        int32_t oid = -1;
        float ox = -INFINITY;
        if (lane < steps) {
            const int c = my_pick, n1t = my_n1 >> 2;
            const int n = c ? n1t : lane - n1t;              // the picks of category c before step `lane`: the member it picked
            ox = s_val[wave][c][n] + a.L * ((c ? q1 : q0) * xq_cov<VARIANT>(n, lane));
            oid = s_id[wave][c][n];
        }
        a.out_idx[(size_t)row * K + lane] = oid;
        a.out_val[(size_t)row * K + lane] = ox;
    }
}

}  // namespace

extern "C" int pda_xquad_rerank(const int32_t* cand_idx, const float* cand_val, int n_rows, int N, const uint8_t* item_is_head, int n_items,
                                const int32_t* users, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, double lambda,
                                int variant, int K, int32_t* out_idx, float* out_val, void* stream) {
    if (!cand_idx || !cand_val || !item_is_head || !out_idx || !out_val) return PDA_ERR_ARG;
    if (n_rows < 1 || n_items < 1 || N < 1 || N > PDA_XQUAD_MAX_N) return PDA_ERR_ARG;
    if (K < 1 || K > PDA_XQUAD_MAX_K || K > N) return PDA_ERR_ARG;
    if (!(lambda >= 0.0 && lambda <= 1.0)) return PDA_ERR_ARG;   // (NaN fails both)
    if (variant != PDA_XQUAD_BINARY && variant != PDA_XQUAD_SMOOTH) return PDA_ERR_ARG;
    if (hist_indptr) {
        if (!hist_indices || (hist_row_mode != PDA_HIST_BY_BLOCK_ROW && hist_row_mode != PDA_HIST_BY_USER_ID)) return PDA_ERR_ARG;
        if (hist_row_mode == PDA_HIST_BY_USER_ID && !users) return PDA_ERR_ARG;
    }
    XquadArgs a{cand_idx, cand_val, item_is_head, users, hist_indptr, hist_indices, out_idx, out_val, (float)lambda, (float)(1.0 - lambda),
                n_rows, N, n_items, hist_row_mode, K};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n_rows + kXqRows - 1) / kXqRows));
    if (variant == PDA_XQUAD_BINARY)
        hipLaunchKernelGGL(xquad_rerank_kernel<PDA_XQUAD_BINARY>, grid, dim3(64 * kXqRows), 0, s, a);
    else
        hipLaunchKernelGGL(xquad_rerank_kernel<PDA_XQUAD_SMOOTH>, grid, dim3(64 * kXqRows), 0, s, a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
