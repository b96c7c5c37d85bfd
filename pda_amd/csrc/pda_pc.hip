// BPR-PC (popularity-compensated re-ranking, Zhu et al., WSDM'21) for MI355X (gfx950): include/pda_hip_pc.h.
//
// The reference builds, per 2 048-user block, the [B, I] rating matrix and four more [B, I] tensors, then calls top_k
// (MF/BPR_PC.py:684-713).  Here:
//   item moments   G = sum v v^T, H = sum p^2 v v^T, h = sum p^2 v, P = sum p^2 (float64, once per (I, pop)): a tall-skinny reduction
//   user stats     A_u = u^T G u + history corrections, Bc_u = b^2 u^T H u + 2 b w u^T h + w^2 P + history corrections -> U_n, U_c, k_u:
//                  O(d^2 + |hist| d) per user instead of a second full-catalogue sweep
//   sweep          generation 1's exact fp32 MFMA kernel with the PC head (pda_score_topk.hip): ranks by r, keeps K' = min(K + 8, 54)
//                  candidates per row and writes the per-row minimum of r of each item split
//   finish         merge the splits (pda_topk_merge), m per group of rows_per_min rows, g of the candidates, a stable sort by (g, id),
//                  and a completeness test; the rows it cannot settle are swept again ranked by g (kHeadPcG) -- only those rows.
#include "pda_topk_common.h"
#include "pda_hip_pc.h"

namespace {

using namespace pda_topk;

__device__ __forceinline__ float pc_p(float pop) { return 1.0f / pop; }   // p_i = RN32(1 / pop_i) (correctly rounded fp32 division)

// ---- item moments ---------------------------------------------------------------------------------------------------------------
// One workgroup per (64 x 64 output tile, item chunk); thread (rr, cc) owns rows 4 rr .. 4 rr + 3 and columns 4 cc .. 4 cc + 3 of the tile
// in G and H.  Tiles in the first column also sum h, tile (0, 0) sums P.  Partial sums per chunk, then a fixed-order reduction.
constexpr int kMomItems = 32;

__host__ __device__ constexpr size_t mom_size(int d) { return 2 * (size_t)d * d + d + 1; }

int mom_chunks(int n_items, int d) {
    const int tiles = (d / 64) * (d / 64);
    int c = (n_items + 255) / 256;
    const int cap = 256 / tiles > 1 ? 256 / tiles : 1;
    return c < 1 ? 1 : (c > cap ? cap : c);
}

template <int D>
__global__ void __launch_bounds__(256) pc_moments_kernel(const float* __restrict__ I, const float* __restrict__ pop, int n, int chunk_items,
                                                         double* __restrict__ part) {
    constexpr int T1 = D / 64;
    __shared__ __attribute__((aligned(16))) float srow[kMomItems][64];
    __shared__ __attribute__((aligned(16))) float scol[kMomItems][64];
    __shared__ double sw[kMomItems];
    const int tile = blockIdx.x % (T1 * T1), chunk = blockIdx.x / (T1 * T1);
    const int ty = tile / T1, tx = tile % T1;
    const int tid = threadIdx.x, rr = tid >> 4, cc = tid & 15;
    const bool do_h = tx == 0 && cc == 0, do_p = tile == 0 && tid == 0;
    double g[4][4], hh[4][4], hv[4] = {0.0, 0.0, 0.0, 0.0}, P = 0.0;
#pragma unroll
    for (int x = 0; x < 4; ++x)
#pragma unroll
        for (int y = 0; y < 4; ++y) g[x][y] = hh[x][y] = 0.0;
    const int i0 = chunk * chunk_items, i1 = min(n, i0 + chunk_items);
    for (int b = i0; b < i1; b += kMomItems) {
        for (int q = tid; q < kMomItems * 16; q += 256) {
            const int it = q >> 4, ch = q & 15, item = b + it;
            f32x4 vr = {0.f, 0.f, 0.f, 0.f}, vc = vr;
            if (item < i1) {
                vr = *reinterpret_cast<const f32x4*>(I + (size_t)item * D + ty * 64 + 4 * ch);
                vc = *reinterpret_cast<const f32x4*>(I + (size_t)item * D + tx * 64 + 4 * ch);
            }
            *reinterpret_cast<f32x4*>(&srow[it][4 * ch]) = vr;
            *reinterpret_cast<f32x4*>(&scol[it][4 * ch]) = vc;
        }
        if (tid < kMomItems) {
            const int item = b + tid;
            const double p = item < i1 ? (double)pc_p(pop[item]) : 0.0;
            sw[tid] = p * p;
        }
        __syncthreads();
        const int nb = min(kMomItems, i1 - b);
        for (int it = 0; it < nb; ++it) {
            const f32x4 va = *reinterpret_cast<const f32x4*>(&srow[it][4 * rr]);
            const f32x4 vc = *reinterpret_cast<const f32x4*>(&scol[it][4 * cc]);
            const double w = sw[it];
#pragma unroll
            for (int x = 0; x < 4; ++x) {
                const double ax = (double)va[x], wa = w * ax;
#pragma unroll
                for (int y = 0; y < 4; ++y) {
                    g[x][y] = fma(ax, (double)vc[y], g[x][y]);
                    hh[x][y] = fma(wa, (double)vc[y], hh[x][y]);
                }
                if (do_h) hv[x] += wa;
            }
            if (do_p) P += w;
        }
        __syncthreads();
    }
    double* out = part + (size_t)chunk * mom_size(D);
#pragma unroll
    for (int x = 0; x < 4; ++x) {
        const int row = ty * 64 + 4 * rr + x;
#pragma unroll
        for (int y = 0; y < 4; ++y) {
            const int col = tx * 64 + 4 * cc + y;
            out[(size_t)row * D + col] = g[x][y];
            out[(size_t)D * D + (size_t)row * D + col] = hh[x][y];
        }
        if (do_h) out[2 * (size_t)D * D + row] = hv[x];
    }
    if (do_p) out[2 * (size_t)D * D + D] = P;
}

__global__ void __launch_bounds__(256) pc_moments_reduce_kernel(const double* __restrict__ part, int chunks, size_t S, double* __restrict__ out) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= S) return;
    double s = 0.0;
    for (int c = 0; c < chunks; ++c) s += part[(size_t)c * S + e];
    out[e] = s;
}

// ---- per-user statistics -----------------------------------------------------------------------------------------------------------
// 64 users per workgroup, one per lane; wave w owns the columns [w d/4, (w + 1) d/4) of the quadratic forms (G and H are read wave-uniformly)
// and every fourth run of equal items of the history.  Everything in float64.
struct StatsArgs {
    const float* U;
    const float* I;
    const float* pop;
    const double* mom;
    const int32_t* users;
    const int64_t* hist_indptr;
    const int32_t* hist_indices;
    float* Un;
    float* Uc;
    float* k;
    double b, w;
    int n, n_items, hist_row_mode;
};

template <int D>
__global__ void __launch_bounds__(256) pc_user_stats_kernel(StatsArgs a) {
    constexpr int UB = 64, J = D / 4;
    __shared__ float su[UB][D + 1];
    __shared__ double red[4][4][UB];
    __shared__ long long cnt[4][UB];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row0 = blockIdx.x * UB;
    for (int q = tid; q < UB * (D / 4); q += 256) {
        const int r = q / (D / 4), c = q % (D / 4);
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row0 + r < a.n) v = *reinterpret_cast<const f32x4*>(a.U + (size_t)a.users[row0 + r] * D + 4 * c);
#pragma unroll
        for (int x = 0; x < 4; ++x) su[r][4 * c + x] = v[x];
    }
    __syncthreads();
    const int row = row0 + lane;
    const bool ok = row < a.n;

    double uj[J];
#pragma unroll
    for (int j = 0; j < J; ++j) uj[j] = (double)su[lane][wave * J + j];
    const double* G = a.mom + wave * J;
    const double* H = a.mom + (size_t)D * D + wave * J;
    double accG = 0.0, accH = 0.0;
    for (int k = 0; k < D; ++k) {
        double gs = 0.0, hs = 0.0;
#pragma unroll
        for (int j = 0; j < J; ++j) {
            gs = fma(G[(size_t)k * D + j], uj[j], gs);
            hs = fma(H[(size_t)k * D + j], uj[j], hs);
        }
        const double uk = (double)su[lane][k];
        accG = fma(uk, gs, accG);
        accH = fma(uk, hs, accH);
    }

    // history: a run of c equal items is worth ((1 - c)^2 - 1) s^2 (and C^2) more than the moments count for it
    double cA = 0.0, cB = 0.0;
    long long ncl = 0;
    if (ok && a.hist_indptr != nullptr) {
        const int64_t hr = a.hist_row_mode == PDA_HIST_BY_USER_ID ? (int64_t)a.users[row] : (int64_t)row;
        const int64_t p0 = a.hist_indptr[hr], p1 = a.hist_indptr[hr + 1];
        int runs = 0;
        for (int64_t p = p0; p < p1;) {
            const int it = a.hist_indices[p];
            int64_t q = p + 1;
            while (q < p1 && a.hist_indices[q] == it) ++q;
            const int c = (int)(q - p);
            if ((runs & 3) == wave) {
                const float* v = a.I + (size_t)it * D;
                double s = 0.0;
                for (int kk = 0; kk < D / 4; ++kk) {
                    const f32x4 vv = *reinterpret_cast<const f32x4*>(v + 4 * kk);
#pragma unroll
                    for (int x = 0; x < 4; ++x) s = fma((double)su[lane][4 * kk + x], (double)vv[x], s);
                }
                const double C = (a.b * s + a.w) * (double)pc_p(a.pop[it]);
                const double f = (double)((1 - c) * (1 - c) - 1);
                cA += f * s * s;
                cB += f * C * C;
                ncl += c;
            }
            ++runs;
            p = q;
        }
    }
    red[wave][0][lane] = accG;
    red[wave][1][lane] = accH;
    red[wave][2][lane] = cA;
    red[wave][3][lane] = cB;
    cnt[wave][lane] = ncl;
    __syncthreads();
    if (wave != 0 || !ok) return;
    double sG = 0.0, sH = 0.0, sA = 0.0, sB = 0.0;
    long long nc = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        sG += red[q][0][lane];
        sH += red[q][1][lane];
        sA += red[q][2][lane];
        sB += red[q][3][lane];
        nc += cnt[q][lane];
    }
    const double* hvec = a.mom + 2 * (size_t)D * D;
    double uh = 0.0;
    for (int k = 0; k < D; ++k) uh = fma(hvec[k], (double)su[lane][k], uh);
    const double P = hvec[D];
    const double A = sG + sA;
    const double Bc = a.b * a.b * sH + 2.0 * a.b * a.w * uh + a.w * a.w * P + sB;
    const long long nu = (long long)a.n_items - nc;
    float Un = 0.f, Uc = 0.f, kk = 0.f;
    if (nu != 0) {   // n_u = 0: U_n = U_c = k_u = 0 (the reference divides by zero).  Duplicates can make n_u negative: the norm of
                     // x / n_u is |1 / n_u| times that of x
        const float inv = fabsf(1.0f / (float)nu);
        Un = (float)((double)inv * sqrt(fmax(A, 0.0)));
        Uc = (float)((double)inv * sqrt(fmax(Bc, 0.0)));
        if (Uc > 0.f && Uc < INFINITY) kk = Un * (1.0f / Uc);   // U_c = 0: k_u = 0 (the reference: inf / NaN)
    }
    a.Un[row] = Un;
    a.Uc[row] = Uc;
    a.k[row] = kk;
}

// ---- the score call ----------------------------------------------------------------------------------------------------------------
struct PcLayout {
    size_t blk1, blk2, p, keys, merged, gmin, map, users_c, U_c, total;
};

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// Candidates the sweep keeps per row: K + 8, but never more than PDA_TOPK_CAP - 6.  The generation-1 list holds PDA_TOPK_CAP = 60 keys
// and compacts when it fills: at K' = 58 it compacted every second candidate (the bias-head kernel itself: 166 against 132 ms at C3 for
// K = 58 against 50); six free slots keep that cost near the bias head's.
int pc_kprime(int K) { return K + 8 < PDA_TOPK_CAP - 6 ? K + 8 : PDA_TOPK_CAP - 6; }

PcLayout pc_layout(int n, int n_items, int d, int K, int S) {
    PcLayout L;
    const size_t Kp = (size_t)pc_kprime(K);
    size_t o = 0;
    L.blk1 = o;    o = al256(o + kPcBlockHdr + 4 * (size_t)n * (2 + S));
    L.blk2 = o;    o = al256(o + kPcBlockHdr + 8 * (size_t)n);
    L.p = o;       o = al256(o + 4 * (size_t)n_items);
    L.keys = o;    o = al256(o + 8 * (size_t)S * n * Kp);
    L.merged = o;  o = al256(o + 8 * (size_t)n * Kp);
    L.gmin = o;    o = al256(o + 4 * (size_t)n);
    L.map = o;     o = al256(o + 4 * (size_t)n);
    L.users_c = o; o = al256(o + 4 * (size_t)n);
    L.U_c = o;     o = al256(o + 4 * (size_t)n * d);
    L.total = o;
    return L;
}

// both sweep blocks' headers, k_u of every row into the first, p_i of every item
__global__ void __launch_bounds__(256) pc_setup_kernel(unsigned char* blk1, unsigned char* blk2, const float* __restrict__ scale, int n,
                                                       const float* __restrict__ pop, float* __restrict__ p, int n_items, float ca, float cb,
                                                       float cw, float ce) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < 2) {
        unsigned char* hb = i == 0 ? blk1 : blk2;
        *reinterpret_cast<int*>(hb + 20) = 0;
        float* cst = reinterpret_cast<float*>(hb + 32);
        cst[0] = ca;
        cst[1] = cb;
        cst[2] = cw;
        cst[3] = ce;
        *reinterpret_cast<int*>(hb + 48) = n;
    }
    if (i < n) reinterpret_cast<float*>(blk1 + kPcBlockHdr)[i] = scale[i];
    if (i < n_items) p[i] = pc_p(pop[i]);
}

// m of each group of rows_per_min rows: the minimum over its rows and every split
__global__ void __launch_bounds__(256) pc_group_min_kernel(const float* __restrict__ rowmin, int n, int S, int rpm, float* __restrict__ gmin) {
    __shared__ float red[4];
    const int g = blockIdx.x;
    const int r0 = g * rpm, r1 = (int)min((long long)n, (long long)r0 + rpm);
    float v = INFINITY;
    for (int s = 0; s < S; ++s)
        for (int r = r0 + (int)threadIdx.x; r < r1; r += 256) v = fminf(v, rowmin[(size_t)s * n + r]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) gmin[g] = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
}

// the exact fp32 chain of every top-K kernel (oracle/pda_oracle.c:dot_chain; pda_aux.hip's score_dense_kernel)
template <int D>
__device__ float pc_chain(const float* u, const float* v) {
    float acc[2] = {0.f, 0.f};
#pragma unroll 4
    for (int c = 0; c < D / 8; ++c) {
        const f32x4 ua = *reinterpret_cast<const f32x4*>(u + 8 * c), ub = *reinterpret_cast<const f32x4*>(u + 8 * c + 4);
        const f32x4 va = *reinterpret_cast<const f32x4*>(v + 8 * c), vb = *reinterpret_cast<const f32x4*>(v + 8 * c + 4);
#pragma unroll
        for (int s2 = 0; s2 < 4; ++s2) {
            acc[c & 1] = fmaf(ua[s2], va[s2], acc[c & 1]);
            acc[c & 1] = fmaf(ub[s2], vb[s2], acc[c & 1]);
        }
    }
    return acc[0] + acc[1];
}

struct FinishArgs {
    const uint64_t* merged;   // [n][Kp], by r
    const float* gmin;
    const float* k;
    const float* p;
    const int32_t* users;
    const int64_t* hist_indptr;
    const int32_t* hist_indices;
    const float* U;
    const float* I;
    int32_t* out_idx;
    float* out_val;
    int* counter;
    int32_t* map;
    float a, b, w, e;
    int n, Kp, K, rpm, hist_row_mode;
};

// One wave per row: g of the K' candidates by r, a stable sort by (g descending, id ascending), the completeness test, the output
// -- or the row goes to the fallback list.  Rows with fewer than K unmasked items are filled with the listed ones in the reference's order:
// value 0 (listed once) by id, then value g - c g (listed c >= 2 times, r from the exact chain) descending, ties by id.
template <int D>
__global__ void __launch_bounds__(256) pc_finish_kernel(FinishArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.n) return;
    const uint64_t key = lane < a.Kp ? a.merged[(size_t)row * a.Kp + lane] : 0ull;
    const bool real = key != 0ull;
    const int nc = __popcll(__ballot(real));   // the merged list is sorted: its keys sit in lanes 0 .. nc - 1
    const float m = a.gmin[row / a.rpm];
    const float r = real ? pda_key_val(key) : 0.f;
    const int32_t it = real ? pda_key_item(key) : 0;
    const float g = (r - m) + a.e;
    const uint64_t gk = real ? pda_pack_key(g, (uint32_t)it) : 0ull;
    int rank = 0;
    for (int q = 0; q < nc; ++q) rank += pda_readlane_u64(gk, q) > gk ? 1 : 0;
    if (nc == a.Kp) {
        // every item not kept has r <= r_last, so g <= g(r_last): the list is settled when the K-th g beats g(r_last) strictly
        const float r_last = pda_readlane_f32(r, a.Kp - 1);
        const float g_last = (r_last - m) + a.e;
        const uint64_t mk = __ballot(real && rank == a.K - 1);
        const float gK = pda_readlane_f32(g, __builtin_ctzll(mk));
        if (!(gK > g_last)) {
            if (lane == 0) a.map[atomicAdd(a.counter, 1)] = row;
            return;
        }
    }
    if (real && rank < a.K) {
        a.out_idx[(size_t)row * a.K + rank] = it;
        a.out_val[(size_t)row * a.K + rank] = g;
    }
    if (nc >= a.K || a.hist_indptr == nullptr) return;
    const int64_t hr = a.hist_row_mode == PDA_HIST_BY_USER_ID ? (int64_t)a.users[row] : (int64_t)row;
    const int64_t p0 = a.hist_indptr[hr], p1 = a.hist_indptr[hr + 1];
    int fill = nc;
    if (lane == 0) {   // listed once: value fl(g - g) = 0, lowest id first
        for (int64_t p = p0; p < p1 && fill < a.K;) {
            const int item = a.hist_indices[p];
            int64_t q = p + 1;
            while (q < p1 && a.hist_indices[q] == item) ++q;
            if (q - p == 1) {
                a.out_idx[(size_t)row * a.K + fill] = item;
                a.out_val[(size_t)row * a.K + fill] = 0.0f;
                ++fill;
            }
            p = q;
        }
    }
    fill = __builtin_amdgcn_readfirstlane(fill);
    // listed c >= 2 times: -(c - 1) g (c subtractions of g in turn), by selection rounds -- rows this short are rare
    const float* urow = a.U + (size_t)a.users[row] * D;
    const float kr = a.k[row];
    uint64_t bound = ~0ull;
    for (; fill < a.K; ++fill) {
        uint64_t best = 0ull;
        for (int64_t p = p0 + lane; p < p1; p += 64) {
            const int item = a.hist_indices[p];
            if (p > p0 && a.hist_indices[p - 1] == item) continue;   // not the start of a run
            int64_t q = p + 1;
            while (q < p1 && a.hist_indices[q] == item) ++q;
            const int c = (int)(q - p);
            if (c < 2) continue;
            const float s = pc_chain<D>(urow, a.I + (size_t)item * D);
            const float C = (s * a.b + a.w) * a.p[item];
            const float rr = s + a.a * (C * kr);
            const float gg = (rr - m) + a.e;
            float v = gg;
            for (int t = 0; t < c; ++t) v = v - gg;
            const uint64_t vk = pda_pack_key(v, (uint32_t)item);
            if (vk < bound && vk > best) best = vk;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint64_t other = (uint64_t)__shfl_xor((unsigned long long)best, o, 64);
            best = other > best ? other : best;
        }
        if (best == 0ull) break;
        if (lane == 0) {
            a.out_idx[(size_t)row * a.K + fill] = pda_key_item(best);
            a.out_val[(size_t)row * a.K + fill] = pda_key_val(best);
        }
        bound = best;
    }
}

// the fallback rows' arguments for the second sweep (ranked by g): row ids (user-id histories) or block rows (block-row histories, whose
// rows then read a copy of their user's embedding at U_c[row]: the block's own CSR serves the sweep as a by-row-id history), k_u and m
__global__ void __launch_bounds__(256) pc_fallback_prep_kernel(const int32_t* __restrict__ map, const int32_t* __restrict__ users, int by_user,
                                                               const float* __restrict__ gmin, int rpm, const float* __restrict__ k1,
                                                               unsigned char* blk2, int cap, int32_t* __restrict__ users_c, const float* __restrict__ U,
                                                               float* __restrict__ U_c, int d) {
    const int slot = blockIdx.x;
    const int row = map[slot];
    if (threadIdx.x == 0) {
        users_c[slot] = by_user ? users[row] : row;
        float* k2 = reinterpret_cast<float*>(blk2 + kPcBlockHdr);
        k2[slot] = k1[row];
        k2[cap + slot] = gmin[row / rpm];
    }
    if (!by_user)
        for (int q = threadIdx.x; q < d; q += 256) U_c[(size_t)row * d + q] = U[(size_t)users[row] * d + q];
}

__global__ void __launch_bounds__(256) pc_fallback_write_kernel(const uint64_t* __restrict__ merged, const int32_t* __restrict__ map, int nf, int K,
                                                                int32_t* __restrict__ out_idx, float* __restrict__ out_val) {
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (size_t)nf * K) return;
    const int slot = (int)(e / K), q = (int)(e % K);
    const uint64_t key = merged[e];
    const size_t o = (size_t)map[slot] * K + q;
    out_idx[o] = key ? pda_key_item(key) : -1;
    out_val[o] = key ? pda_key_val(key) : -INFINITY;
}

bool pc_d_ok(int d) { return d == 64 || d == 128 || d == 256; }

}  // namespace

extern "C" size_t pda_pc_moments_workspace_bytes(int n_items, int d) {
    if (n_items <= 0 || !pc_d_ok(d)) return 0;
    return (size_t)mom_chunks(n_items, d) * mom_size(d) * sizeof(double);
}

extern "C" int pda_pc_item_moments_f32(const float* I, const float* pop, int n_items, int d, double* moments, void* workspace, void* stream) {
    if (!I || !pop || !moments || !workspace || n_items <= 0) return PDA_ERR_ARG;
    if (!pc_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int chunks = mom_chunks(n_items, d), tiles = (d / 64) * (d / 64);
    const int per = (n_items + chunks - 1) / chunks;
    double* part = reinterpret_cast<double*>(workspace);
    const dim3 grid((unsigned)(chunks * tiles));
    switch (d) {
        case 64: hipLaunchKernelGGL(pc_moments_kernel<64>, grid, dim3(256), 0, s, I, pop, n_items, per, part); break;
        case 128: hipLaunchKernelGGL(pc_moments_kernel<128>, grid, dim3(256), 0, s, I, pop, n_items, per, part); break;
        default: hipLaunchKernelGGL(pc_moments_kernel<256>, grid, dim3(256), 0, s, I, pop, n_items, per, part); break;
    }
    PDA_CHECK_LAUNCH();
    const size_t S = mom_size(d);
    hipLaunchKernelGGL(pc_moments_reduce_kernel, dim3((unsigned)((S + 255) / 256)), dim3(256), 0, s, part, chunks, S, moments);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_pc_user_stats_f32(const float* U, const float* I, const float* pop, const double* moments, const int32_t* users, int n_users_blk,
                                     int n_items, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, double beta,
                                     float* U_n, float* U_c, float* scale, void* stream) {
    if (!U || !I || !pop || !moments || !users || !U_n || !U_c || !scale) return PDA_ERR_ARG;
    if (n_users_blk <= 0 || n_items <= 0 || !(fabs(beta) < INFINITY)) return PDA_ERR_ARG;
    if (hist_indptr && (!hist_indices || (hist_row_mode != PDA_HIST_BY_BLOCK_ROW && hist_row_mode != PDA_HIST_BY_USER_ID))) return PDA_ERR_ARG;
    if (!pc_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    const float b = (float)beta, w = (float)(1.0 - beta);
    StatsArgs a{U, I, pop, moments, users, hist_indptr, hist_indices, U_n, U_c, scale, (double)b, (double)w, n_users_blk, n_items, hist_row_mode};
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((n_users_blk + 63) / 64));
    switch (d) {
        case 64: hipLaunchKernelGGL(pc_user_stats_kernel<64>, grid, dim3(256), 0, s, a); break;
        case 128: hipLaunchKernelGGL(pc_user_stats_kernel<128>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(pc_user_stats_kernel<256>, grid, dim3(256), 0, s, a); break;
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" size_t pda_pc_score_workspace_bytes(int n_users_blk, int n_items, int d, int K) {
    if (n_users_blk <= 0 || n_items <= 0 || !pc_d_ok(d) || K < 1 || K > PDA_PC_MAX_K) return 0;
    return pc_layout(n_users_blk, n_items, d, K, pda_score_topk_auto_splits(n_users_blk, n_items)).total;
}

extern "C" int pda_pc_score_topk_f32(const float* U, const float* I, const float* pop, const float* scale, const int32_t* users, int n_users_blk,
                                     int n_items, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, double alpha,
                                     double beta, int rows_per_min, int K, int32_t* out_idx, float* out_val, void* workspace, void* stream) {
    if (!U || !I || !pop || !scale || !users || !out_idx || !out_val || !workspace) return PDA_ERR_ARG;
    if (n_users_blk <= 0 || n_items <= 0 || rows_per_min < 1) return PDA_ERR_ARG;
    if (K < 1 || K > PDA_PC_MAX_K || K > n_items) return PDA_ERR_ARG;
    if (!(fabs(alpha) < INFINITY) || !(fabs(beta) < INFINITY)) return PDA_ERR_ARG;
    if (hist_indptr && (!hist_indices || (hist_row_mode != PDA_HIST_BY_BLOCK_ROW && hist_row_mode != PDA_HIST_BY_USER_ID))) return PDA_ERR_ARG;
    if (!pc_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return PDA_ERR_WORKSPACE;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int n = n_users_blk, S = pda_score_topk_auto_splits(n, n_items), Kp = pc_kprime(K);
    const PcLayout L = pc_layout(n, n_items, d, K, S);
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    unsigned char* blk1 = ws + L.blk1;
    unsigned char* blk2 = ws + L.blk2;
    float* p = reinterpret_cast<float*>(ws + L.p);
    uint64_t* keys = reinterpret_cast<uint64_t*>(ws + L.keys);
    uint64_t* merged = reinterpret_cast<uint64_t*>(ws + L.merged);
    float* gmin = reinterpret_cast<float*>(ws + L.gmin);
    int32_t* map = reinterpret_cast<int32_t*>(ws + L.map);
    int32_t* users_c = reinterpret_cast<int32_t*>(ws + L.users_c);
    float* Uc = reinterpret_cast<float*>(ws + L.U_c);
    const float ca = (float)alpha, cb = (float)beta, cw = (float)(1.0 - beta), ce = 0.01f;

    const int nmax = n > n_items ? n : n_items;
    hipLaunchKernelGGL(pc_setup_kernel, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, s, blk1, blk2, scale, n, pop, p, n_items, ca, cb, cw, ce);
    PDA_CHECK_LAUNCH();
    // 1. the sweep, ranked by r, K' candidates per row; the per-row minimum of r of each split
    ScoreArgs sa{U, I, p, users, hist_indptr, hist_indices, keys, n, 0, n_items, hist_row_mode, Kp, S, reinterpret_cast<const int*>(blk1)};
    int rc = pda_topk::launch_score_pc(sa, d, false, s);
    if (rc != PDA_OK) return rc;
    // 2. m per group of rows
    const int ngroups = (int)(((long long)n + rows_per_min - 1) / rows_per_min);
    hipLaunchKernelGGL(pc_group_min_kernel, dim3((unsigned)ngroups), dim3(256), 0, s,
                       reinterpret_cast<const float*>(blk1 + kPcBlockHdr) + 2 * (size_t)n, n, S, rows_per_min, gmin);
    PDA_CHECK_LAUNCH();
    // 3. the splits' lists merged (by r), then g, the sort by (g, id), the completeness test and the output
    rc = pda_topk_merge(keys, S, n, Kp, merged, nullptr, nullptr, users, nullptr, nullptr, 0, stream);
    if (rc != PDA_OK) return rc;
    int* counter = reinterpret_cast<int*>(blk1 + 20);
    FinishArgs fa{merged, gmin, reinterpret_cast<const float*>(blk1 + kPcBlockHdr), p, users, hist_indptr, hist_indices, U, I, out_idx, out_val,
                  counter, map, ca, cb, cw, ce, n, Kp, K, rows_per_min, hist_row_mode};
    const dim3 fgrid((unsigned)((n + 3) / 4));
    switch (d) {
        case 64: hipLaunchKernelGGL(pc_finish_kernel<64>, fgrid, dim3(256), 0, s, fa); break;
        case 128: hipLaunchKernelGGL(pc_finish_kernel<128>, fgrid, dim3(256), 0, s, fa); break;
        default: hipLaunchKernelGGL(pc_finish_kernel<256>, fgrid, dim3(256), 0, s, fa); break;
    }
    PDA_CHECK_LAUNCH();
    int nf = 0;
    if (hipMemcpyAsync(&nf, counter, sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess)
        return PDA_ERR_LAUNCH;
    if (nf <= 0) return PDA_OK;
    // 4. the rows the ranking by r could not settle, swept again ranked by g (their cost follows their number)
    const bool by_user = hist_indptr == nullptr || hist_row_mode == PDA_HIST_BY_USER_ID;
    hipLaunchKernelGGL(pc_fallback_prep_kernel, dim3((unsigned)nf), dim3(256), 0, s, map, users, by_user ? 1 : 0, gmin, rows_per_min,
                       reinterpret_cast<const float*>(blk1 + kPcBlockHdr), blk2, n, users_c, U, Uc, d);
    PDA_CHECK_LAUNCH();
    int S2 = pda_score_topk_auto_splits(nf, n_items);
    const long long room = (long long)S * n * Kp / ((long long)nf * K);   // the second sweep's keys reuse the first's buffer
    if (S2 > room) S2 = (int)room;
    if (S2 < 1) S2 = 1;
    ScoreArgs sb{by_user ? U : Uc, I, p, users_c, hist_indptr, hist_indices, keys, nf, 0, n_items, PDA_HIST_BY_USER_ID, K, S2,
                 reinterpret_cast<const int*>(blk2)};
    rc = pda_topk::launch_score_pc(sb, d, true, s);
    if (rc != PDA_OK) return rc;
    rc = pda_topk_merge(keys, S2, nf, K, merged, nullptr, nullptr, users_c, nullptr, nullptr, 0, stream);
    if (rc != PDA_OK) return rc;
    hipLaunchKernelGGL(pc_fallback_write_kernel, dim3((unsigned)(((size_t)nf * K + 255) / 256)), dim3(256), 0, s, merged, map, nf, K, out_idx, out_val);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
