// iALS++ (include/pda_hip_ialspp.h) on MI355X (gfx950): the prediction cache, one pass of one coordinate block over a work list,
// the Gram matrix and the objective's per-row terms at the four embedding sizes.
//
// Block pass layout: ONE workgroup per entry of the work list, as in pda_ials.hip, but a workgroup gathers only the k-float slice
// Z[c, p0 .. p0 + k) of each partner row and the pair's cached prediction e: 4 k + 4 bytes per pair instead of 4 d.  The slices are staged in
// LDS in blocks of 32 (the next block's 16-byte loads in flight in registers); sum z z^T lives in the accumulators of
// v_mfma_f32_32x32x2_f32 (lower triangle of 32 x 32 tiles, dealt round-robin to the waves) and sum (e - 1) z in one register of k lanes.  The
// tail adds alpha0 G[pi, pi], alpha0 G[pi, :] x_r and the lam_row terms, factorises the k x k matrix in place (stride k + 1), substitutes
// twice, stores x_{r,pi} and walks the row's pairs once more to update e.  Cut rows: partial (H, g) to slots, one workgroup per cut row sums
// and solves and leaves delta once per slot, the chunks gather again for their e.
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_hip_ialspp.h"
#include "pda_hip_ials_itemw.h"

namespace {

constexpr int kKB = 32;         // pairs per staged block
constexpr int kMaxD = 256;

template <int K>
struct Cfg {
    static constexpr int NT = K == 32 ? 64 : 256;           // lanes per workgroup
    static constexpr int NW = NT / 64;
    static constexpr int TN = K / 32;
    static constexpr int NTILES = TN * (TN + 1) / 2;        // lower triangle of 32 x 32 tiles
    static constexpr int MAXT = (NTILES + NW - 1) / NW;     // tiles per wave
    static constexpr int LD = K + 1;
    static constexpr int G = K / 4;                         // lanes per gathered slice
    static constexpr int RPP = NT / G;                      // slices per gather pass
    static constexpr int NP = kKB / RPP;
    static constexpr int Q = NT / K;                        // parts of the G[pi, :] x product
    static constexpr size_t SLOT = (size_t)K * K + K;
    // H, g, y, delta, the row x_r, the parts of G x, the staged e - 1, the failed-pivot flag
    static constexpr size_t LDS_FLOATS = (size_t)K * LD + 3 * K + kMaxD + (size_t)Q * K + kKB + 4;
    static constexpr size_t LDS_BYTES = LDS_FLOATS * sizeof(float);
};

struct PpArgs {
    const int64_t* indptr;
    const int32_t* indices;
    const int64_t* perm;        // [nnz] position in this CSR -> position in e; nullptr: the identity
    const int64_t* work;        // [n_work, 4]: row, first pair, end pair, slot
    const int64_t* long_rows;   // [n_long, 3]: row, first slot, chunks
    const float* Z;
    const float* G;
    const float* lam_row;
    float* X;
    float* e;
    int32_t* fail;
    float* dbg;
    float* slots;               // [n_slots, k * k + k]
    float* delta_ws;            // [n_slots, k]
    size_t n_rows, nnz, n_slots;
    unsigned n_z;
    int d, p0;
    float alpha0;
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }
__device__ __forceinline__ float hsum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}
// the position in e of the pair at position kk of the CSR; -1 when the permutation points outside e (skipped)
__device__ __forceinline__ int64_t e_pos(const PpArgs& a, int64_t kk) {
    const int64_t p = a.perm != nullptr ? a.perm[kk] : kk;
    return (uint64_t)p < a.nnz ? p : -1;
}

template <int K>
struct Lds {
    using C = Cfg<K>;
    float *sA, *sb, *sy, *sx, *sxr, *sp, *se;
    int* sflag;
    __device__ __forceinline__ explicit Lds(float* sm) {
        sA = sm;
        sb = sA + K * C::LD;
        sy = sb + K;
        sx = sy + K;
        sxr = sx + K;
        sp = sxr + kMaxD;
        se = sp + C::Q * K;
        sflag = reinterpret_cast<int*>(se + kKB);
    }
};

// sum z z^T (symmetric, stride LD) and sum (e - 1) z over the pairs k0 .. k1 of the CSR, z the slice [p0, p0 + K) of a partner row, into
// sA [K, LD] and sb [K].  Every lane of the workgroup calls it; it ends behind a barrier.
template <int K>
__device__ __forceinline__ void pp_accumulate(const PpArgs& a, int64_t k0, int64_t k1, float* sm) {
    using C = Cfg<K>;
    const Lds<K> L(sm);
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 31, h = lane >> 5;
    const int el = tid % C::G, rr = tid / C::G;
    const int bcol = tid - (C::NT - K);         // the last K lanes sum g: the waves with the fewest tiles
    f32x16 acc[C::MAXT];
    int ti[C::MAXT], tj[C::MAXT];
#pragma unroll
    for (int s = 0; s < C::MAXT; ++s) {
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
        const int t = wv + s * C::NW;
        ti[s] = t >= 6 ? 3 : t >= 3 ? 2 : t >= 1 ? 1 : 0;
        tj[s] = t - ti[s] * (ti[s] + 1) / 2;
    }
    float gsum = 0.f, prew = 0.f;
    f32x4 pre[C::NP];
    auto fetch = [&](int64_t base) {
#pragma unroll
        for (int p = 0; p < C::NP; ++p) {
            const int64_t kk = base + p * C::RPP + rr;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (kk < k1) {
                const unsigned c = (unsigned)a.indices[kk];
                if (c < a.n_z) v = ld4(a.Z + (size_t)c * a.d + a.p0 + 4 * el);
            }
            pre[p] = v;
        }
        if (tid < kKB) {
            float w = 0.f;
            if (base + tid < k1) {
                const int64_t pos = e_pos(a, base + tid);
                if (pos >= 0) w = a.e[pos] - 1.f;
            }
            prew = w;
        }
    };
    if (k0 < k1) fetch(k0);
    for (int64_t base = k0; base < k1; base += kKB) {
#pragma unroll
        for (int p = 0; p < C::NP; ++p) st4(sm + (p * C::RPP + rr) * K + 4 * el, pre[p]);
        if (tid < kKB) L.se[tid] = prew;
        __syncthreads();
        if (base + kKB < k1) fetch(base + kKB);
#pragma unroll
        for (int kp = 0; kp < kKB / 2; ++kp) {
#pragma unroll
            for (int s = 0; s < C::MAXT; ++s) {
                if (wv + s * C::NW < C::NTILES) {
                    const float av = sm[(2 * kp + h) * K + 32 * ti[s] + i];
                    const float bv = sm[(2 * kp + h) * K + 32 * tj[s] + i];
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[s], 0, 0, 0);
                }
            }
        }
        if (bcol >= 0) {
#pragma unroll 8
            for (int k = 0; k < kKB; ++k) gsum = fmaf(L.se[k], sm[k * K + bcol], gsum);
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < C::MAXT; ++s) {
        if (wv + s * C::NW < C::NTILES) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = acc_row(reg, h);
                L.sA[(32 * ti[s] + r) * C::LD + 32 * tj[s] + i] = acc[s][reg];
                if (ti[s] != tj[s]) L.sA[(32 * tj[s] + i) * C::LD + 32 * ti[s] + r] = acc[s][reg];
            }
        }
    }
    if (bcol >= 0) L.sb[bcol] = gsum;
    __syncthreads();
}

// The tail of a row whose sums stand in sm: the G and lam_row terms, H = L L^T in place, the two substitutions, x_{r,pi} -= delta.
// Leaves delta in sx (NaN after a failed pivot), behind a barrier.  alpha is a.alpha0, or with ROWALPHA the row's own alpha_row[row]
// (pda_hip_ials_itemw.h).
template <int K, bool ROWALPHA = false>
__device__ __forceinline__ void pp_finish_solve(const PpArgs& a, int64_t row, float* sm, const float* alpha_row = nullptr) {
    using C = Cfg<K>;
    const Lds<K> L(sm);
    const int tid = threadIdx.x, d = a.d, p0 = a.p0;
    const float lam = a.lam_row[row];
    float ar = 0.f;
    if constexpr (ROWALPHA) ar = alpha_row[row];
    float* dbg = a.dbg != nullptr ? a.dbg + (size_t)row * C::SLOT : nullptr;
    if (tid == 0) *L.sflag = 0;
    for (int q = tid; q < d; q += C::NT) L.sxr[q] = a.X[(size_t)row * d + q];
    for (int q = tid; q < K * K; q += C::NT) {
        const int i = q / K, j = q % K;
        float v = L.sA[i * C::LD + j] + (ROWALPHA ? ar : a.alpha0) * a.G[(size_t)(p0 + i) * d + p0 + j];
        if (i == j) v = v + lam;
        L.sA[i * C::LD + j] = v;
        if (dbg != nullptr) dbg[q] = v;
    }
    __syncthreads();
    {   // t = G[:, pi]^T x_r in Q parts of d / Q columns
        const int part = tid / K, i = tid % K, seg = d / C::Q;
        float t = 0.f;
        for (int j = part * seg; j < (part + 1) * seg; ++j) t = fmaf(a.G[(size_t)j * d + p0 + i], L.sxr[j], t);
        L.sp[part * K + i] = t;
    }
    __syncthreads();
    if (tid < K) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < C::Q; ++q) t = t + L.sp[q * K + tid];
        const float g = (L.sb[tid] + (ROWALPHA ? ar : a.alpha0) * t) + lam * L.sxr[p0 + tid];
        L.sb[tid] = g;
        if (dbg != nullptr) dbg[K * K + tid] = g;
    }
    __syncthreads();
    float* sA = L.sA;
    float* sb = L.sb;
    float* sy = L.sy;
    float* sx = L.sx;
    for (int j = 0; j < K; ++j) {
        float s = 0.f;
        if (tid >= j && tid < K) {
            const float* ri = sA + tid * C::LD;
            const float* rj = sA + j * C::LD;
            s = ri[j];
            for (int k = 0; k < j; ++k) s = fmaf(-ri[k], rj[k], s);
            if (tid == j) {
                if (!(s > 0.f) || !(s < INFINITY)) *L.sflag = 1;
                sA[j * C::LD + j] = sqrtf(s);
            }
        }
        __syncthreads();
        if (tid > j && tid < K) sA[tid * C::LD + j] = s / sA[j * C::LD + j];
        __syncthreads();
    }
    for (int j = 0; j < K; ++j) {
        if (tid >= j && tid < K) {
            const float yj = sb[j] / sA[j * C::LD + j];
            if (tid == j) sy[j] = yj;
            else sb[tid] = fmaf(-sA[tid * C::LD + j], yj, sb[tid]);
        }
        __syncthreads();
    }
    for (int j = K - 1; j >= 0; --j) {
        if (tid <= j) {
            const float xj = sy[j] / sA[j * C::LD + j];
            if (tid == j) sx[j] = xj;
            else sy[tid] = fmaf(-sA[j * C::LD + tid], xj, sy[tid]);
        }
        __syncthreads();
    }
    const bool bad = *L.sflag != 0;
    if (tid < K) {
        const float dl = bad ? NAN : sx[tid];
        sx[tid] = dl;
        a.X[(size_t)row * d + p0 + tid] = bad ? NAN : L.sxr[p0 + tid] - dl;
    }
    if (bad && tid == 0 && a.fail != nullptr) atomicAdd(a.fail, 1);
    __syncthreads();
}

// e_c -= z_{c,pi} . delta over the pairs k0 .. k1, delta [K] in LDS
template <int K>
__device__ __forceinline__ void pp_update_e(const PpArgs& a, int64_t k0, int64_t k1, const float* sdelta) {
    using C = Cfg<K>;
    const int l = threadIdx.x % C::G, grp = threadIdx.x / C::G;
    const f32x4 dl = {sdelta[4 * l], sdelta[4 * l + 1], sdelta[4 * l + 2], sdelta[4 * l + 3]};
    for (int64_t kk = k0 + grp; kk < k1; kk += C::RPP) {     // (uniform over the lane group)
        const unsigned c = (unsigned)a.indices[kk];
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (c < a.n_z) z = ld4(a.Z + (size_t)c * a.d + a.p0 + 4 * l);
        const float dot = group_sum<C::G>(hsum4(z * dl));
        if (l == 0) {
            const int64_t pos = e_pos(a, kk);
            if (pos >= 0) a.e[pos] = a.e[pos] - dot;
        }
    }
}

__device__ __forceinline__ bool pp_entry_ok(const PpArgs& a, int64_t row, int64_t k0, int64_t k1, int64_t slot) {
    return !(row < 0 || (uint64_t)row >= a.n_rows || k0 < 0 || k1 < k0 || (uint64_t)k1 > a.nnz || slot >= (int64_t)a.n_slots);
}

template <int K>
__global__ __launch_bounds__(Cfg<K>::NT) void pp_rows_kernel(PpArgs a) {
    using C = Cfg<K>;
    extern __shared__ __attribute__((aligned(16))) unsigned char pp_smem[];
    float* sm = reinterpret_cast<float*>(pp_smem);
    const int64_t* wk = a.work + 4 * (size_t)blockIdx.x;
    const int64_t row = wk[0], k0 = wk[1], k1 = wk[2], slot = wk[3];
    if (!pp_entry_ok(a, row, k0, k1, slot)) return;     // (uniform)
    pp_accumulate<K>(a, k0, k1, sm);
    if (slot >= 0) {
        float* dst = a.slots + (size_t)slot * C::SLOT;
        for (int q = threadIdx.x; q < K * K; q += C::NT) dst[q] = sm[(q / K) * C::LD + q % K];
        if (threadIdx.x < K) dst[K * K + threadIdx.x] = sm[K * C::LD + threadIdx.x];
        return;
    }
    pp_finish_solve<K>(a, row, sm);
    pp_update_e<K>(a, k0, k1, Lds<K>(sm).sx);
}

// the cut rows: the slots of a row in chunk order onto zero, the same tail, delta once per slot of the row
template <int K>
__global__ __launch_bounds__(Cfg<K>::NT) void pp_long_rows_kernel(PpArgs a) {
    using C = Cfg<K>;
    extern __shared__ __attribute__((aligned(16))) unsigned char pp_smem[];
    float* sm = reinterpret_cast<float*>(pp_smem);
    const int64_t* lr = a.long_rows + 3 * (size_t)blockIdx.x;
    const int64_t row = lr[0], s0 = lr[1], n = lr[2];
    if (row < 0 || (uint64_t)row >= a.n_rows || s0 < 0 || n < 0 || (uint64_t)s0 + (uint64_t)n > a.n_slots) return;   // (uniform)
    const float* src = a.slots + (size_t)s0 * C::SLOT;
    for (int q = threadIdx.x; q < K * K; q += C::NT) {
        float v = 0.f;
        for (int64_t j = 0; j < n; ++j) v = v + src[(size_t)j * C::SLOT + q];
        sm[(q / K) * C::LD + q % K] = v;
    }
    if (threadIdx.x < K) {
        float v = 0.f;
        for (int64_t j = 0; j < n; ++j) v = v + src[(size_t)j * C::SLOT + K * K + threadIdx.x];
        sm[K * C::LD + threadIdx.x] = v;
    }
    __syncthreads();
    pp_finish_solve<K>(a, row, sm);
    if (threadIdx.x < K) {
        const float dl = Lds<K>(sm).sx[threadIdx.x];
        for (int64_t j = 0; j < n; ++j) a.delta_ws[(size_t)(s0 + j) * K + threadIdx.x] = dl;
    }
}

// The same two kernels with alpha_row (pda_ialspp_block_pass_rowalpha_f32): their text is that of the two above with the tail's ROWALPHA flag
// set.  They are kernels of their own, with their own argument struct, so that the two above keep their argument layout and their
// instructions (a body shared through a function of both reordered theirs); a.alpha0 is not read here.  pp_chunk_update_kernel reads no
// alpha: it serves both.
struct PpRowAlphaArgs {
    PpArgs a;
    const float* alpha_row;     // [n_rows]
};

template <int K>
__global__ __launch_bounds__(Cfg<K>::NT) void pp_rows_rowalpha_kernel(PpRowAlphaArgs ra) {
    using C = Cfg<K>;
    extern __shared__ __attribute__((aligned(16))) unsigned char pp_smem[];
    float* sm = reinterpret_cast<float*>(pp_smem);
    const PpArgs& a = ra.a;
    const int64_t* wk = a.work + 4 * (size_t)blockIdx.x;
    const int64_t row = wk[0], k0 = wk[1], k1 = wk[2], slot = wk[3];
    if (!pp_entry_ok(a, row, k0, k1, slot)) return;     // (uniform)
    pp_accumulate<K>(a, k0, k1, sm);
    if (slot >= 0) {
        float* dst = a.slots + (size_t)slot * C::SLOT;
        for (int q = threadIdx.x; q < K * K; q += C::NT) dst[q] = sm[(q / K) * C::LD + q % K];
        if (threadIdx.x < K) dst[K * K + threadIdx.x] = sm[K * C::LD + threadIdx.x];
        return;
    }
    pp_finish_solve<K, true>(a, row, sm, ra.alpha_row);
    pp_update_e<K>(a, k0, k1, Lds<K>(sm).sx);
}

template <int K>
__global__ __launch_bounds__(Cfg<K>::NT) void pp_long_rows_rowalpha_kernel(PpRowAlphaArgs ra) {
    using C = Cfg<K>;
    extern __shared__ __attribute__((aligned(16))) unsigned char pp_smem[];
    float* sm = reinterpret_cast<float*>(pp_smem);
    const PpArgs& a = ra.a;
    const int64_t* lr = a.long_rows + 3 * (size_t)blockIdx.x;
    const int64_t row = lr[0], s0 = lr[1], n = lr[2];
    if (row < 0 || (uint64_t)row >= a.n_rows || s0 < 0 || n < 0 || (uint64_t)s0 + (uint64_t)n > a.n_slots) return;   // (uniform)
    const float* src = a.slots + (size_t)s0 * C::SLOT;
    for (int q = threadIdx.x; q < K * K; q += C::NT) {
        float v = 0.f;
        for (int64_t j = 0; j < n; ++j) v = v + src[(size_t)j * C::SLOT + q];
        sm[(q / K) * C::LD + q % K] = v;
    }
    if (threadIdx.x < K) {
        float v = 0.f;
        for (int64_t j = 0; j < n; ++j) v = v + src[(size_t)j * C::SLOT + K * K + threadIdx.x];
        sm[K * C::LD + threadIdx.x] = v;
    }
    __syncthreads();
    pp_finish_solve<K, true>(a, row, sm, ra.alpha_row);
    if (threadIdx.x < K) {
        const float dl = Lds<K>(sm).sx[threadIdx.x];
        for (int64_t j = 0; j < n; ++j) a.delta_ws[(size_t)(s0 + j) * K + threadIdx.x] = dl;
    }
}

// the chunks of the cut rows once more: their e
template <int K>
__global__ __launch_bounds__(Cfg<K>::NT) void pp_chunk_update_kernel(PpArgs a) {
    __shared__ __attribute__((aligned(16))) float sdelta[K];
    const int64_t* wk = a.work + 4 * (size_t)blockIdx.x;
    const int64_t row = wk[0], k0 = wk[1], k1 = wk[2], slot = wk[3];
    if (slot < 0 || !pp_entry_ok(a, row, k0, k1, slot)) return;     // (uniform)
    if (threadIdx.x < K) sdelta[threadIdx.x] = a.delta_ws[(size_t)slot * K + threadIdx.x];
    __syncthreads();
    pp_update_e<K>(a, k0, k1, sdelta);
}

// ---- prediction cache ------------------------------------------------------------------------------------------------------------------
struct PredictArgs {
    const int64_t* indptr;
    const int32_t* indices;
    const float* X;
    const float* Z;
    float* e;
    size_t n_rows, nnz;
    unsigned n_z;
};

template <int D>
__global__ __launch_bounds__(256) void pp_predict_kernel(PredictArgs a) {
    constexpr int G = D / 4, PER = 256 / G;
    const int l = threadIdx.x % G, grp = threadIdx.x / G;
    const size_t row = blockIdx.x;
    const int64_t k0 = a.indptr[row], k1 = a.indptr[row + 1];
    if (k0 < 0 || k1 < k0 || (uint64_t)k1 > a.nnz) return;      // (uniform)
    const f32x4 x = ld4(a.X + row * D + 4 * l);
    for (int64_t kk = k0 + grp; kk < k1; kk += PER) {           // (uniform over the lane group)
        const unsigned c = (unsigned)a.indices[kk];
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (c < a.n_z) z = ld4(a.Z + (size_t)c * D + 4 * l);
        const float s = group_sum<G>(hsum4(x * z));
        if (l == 0) a.e[kk] = s;
    }
}

// ---- Gram matrix at d = 256 ----------------------------------------------------------------------------------------------------------------
struct GramArgs {
    const float* Z;
    float* G;
    float* partials;        // [n_blocks, d * d + d]; the d * d part is used
    size_t n_rows, n_blocks;
};

// one wave per (block of PDA_IALS_GRAM_ROWS rows, lower-triangle 32 x 32 tile): the operands come straight from global memory
template <int D>
__global__ __launch_bounds__(64) void pp_gram_tiles_kernel(GramArgs a) {
    constexpr size_t SLOT = (size_t)D * D + D;
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int t = blockIdx.y;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    const size_t r0 = (size_t)blockIdx.x * PDA_IALS_GRAM_ROWS;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
    for (int kp = 0; kp < PDA_IALS_GRAM_ROWS / 2; ++kp) {
        const size_t r = r0 + 2 * kp + h;
        float av = 0.f, bv = 0.f;
        if (r < a.n_rows) {
            av = a.Z[r * D + 32 * ti + i];
            bv = a.Z[r * D + 32 * tj + i];
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    float* dst = a.partials + (size_t)blockIdx.x * SLOT;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int r = acc_row(reg, h);
        dst[(size_t)(32 * ti + r) * D + 32 * tj + i] = acc[reg];
        if (ti != tj) dst[(size_t)(32 * tj + i) * D + 32 * ti + r] = acc[reg];
    }
}

// pda_ials_gram_scaled_f32 at d = 256 (pda_hip_ials_itemw.h): the kernel above with the row r entering as fl(scale[r] z_r[j]), one more
// 4-byte load per row fetch.  A kernel of its own for the reason given at pp_rows_rowalpha_kernel.
struct GramScaledArgs {
    GramArgs g;
    const float* scale;     // [n_rows]
};

template <int D>
__global__ __launch_bounds__(64) void pp_gram_tiles_scaled_kernel(GramScaledArgs sa) {
    constexpr size_t SLOT = (size_t)D * D + D;
    const GramArgs& a = sa.g;
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int t = blockIdx.y;
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= t) ++ti;
    const int tj = t - ti * (ti + 1) / 2;
    const size_t r0 = (size_t)blockIdx.x * PDA_IALS_GRAM_ROWS;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
    for (int kp = 0; kp < PDA_IALS_GRAM_ROWS / 2; ++kp) {
        const size_t r = r0 + 2 * kp + h;
        float av = 0.f, bv = 0.f;
        if (r < a.n_rows) {
            const float sc = sa.scale[r];
            av = a.Z[r * D + 32 * ti + i] * sc;
            bv = a.Z[r * D + 32 * tj + i] * sc;
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    float* dst = a.partials + (size_t)blockIdx.x * SLOT;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int r = acc_row(reg, h);
        dst[(size_t)(32 * ti + r) * D + 32 * tj + i] = acc[reg];
        if (ti != tj) dst[(size_t)(32 * tj + i) * D + 32 * ti + r] = acc[reg];
    }
}

template <int D>
__global__ __launch_bounds__(256) void pp_gram_sum_kernel(GramArgs a) {
    constexpr size_t SLOT = (size_t)D * D + D;
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= D * D) return;
    float v = 0.f;
    for (size_t c = 0; c < a.n_blocks; ++c) v = v + a.partials[c * SLOT + q];
    a.G[q] = v;
}

// ---- the objective's per-row terms at d = 256 (the kernel of pda_ials.hip at one more width) -----------------------------------------------
struct LossArgs {
    const int64_t* indptr;
    const int32_t* indices;
    const float* X;
    const float* Z;
    const float* G;
    const float* lam_row;
    float* out;
    size_t n_rows, nnz;
    unsigned n_z;
};

template <int D>
__global__ __launch_bounds__(256) void pp_loss_kernel(LossArgs a) {
    constexpr int G = D / 4, PER = 256 / G;
    __shared__ __attribute__((aligned(16))) float sx[PER * D];
    const int el = threadIdx.x % G, rl = threadIdx.x / G;
    const size_t row = (size_t)blockIdx.x * PER + rl;
    const bool valid = row < a.n_rows;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (valid) x = ld4(a.X + row * D + 4 * el);
    st4(sx + rl * D + 4 * el, x);
    __syncthreads();
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < D; ++i) t = t + ld4(a.G + (size_t)i * D + 4 * el) * sx[rl * D + i];
    const float q = group_sum<G>(hsum4(t * x));
    const float nn = group_sum<G>(hsum4(x * x));
    int64_t k0 = 0, k1 = 0;
    if (valid) {
        k0 = a.indptr[row];
        k1 = a.indptr[row + 1];
        if (k0 < 0 || k1 < k0 || (uint64_t)k1 > a.nnz) k0 = k1 = 0;
    }
    float fit = 0.f;
    for (int64_t k = k0; k < k1; ++k) {     // (uniform over the lane group)
        const unsigned c = (unsigned)a.indices[k];
        f32x4 z = {0.f, 0.f, 0.f, 0.f};
        if (c < a.n_z) z = ld4(a.Z + (size_t)c * D + 4 * el);
        const float r = group_sum<G>(hsum4(x * z)) - 1.f;
        fit = fit + r * r;
    }
    if (valid && el == 0) {
        a.out[row * 3 + 0] = fit;
        a.out[row * 3 + 1] = q;
        a.out[row * 3 + 2] = a.lam_row[row] * nn;
    }
}

inline bool pp_d_ok(int d) { return d == 32 || d == 64 || d == 128 || d == 256; }
inline bool pp_k_ok(int k) { return k == 32 || k == 64 || k == 128; }

template <typename Kn>
bool pp_lds(Kn kernel, size_t bytes, int* done) {
    if (*done) return true;     // idempotent attribute; benign if raced
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    *done = 1;
    return true;
}

template <int K>
int launch_block_pass(const PpArgs& a, size_t n_work, size_t n_long, hipStream_t s) {
    using C = Cfg<K>;
    static int set_rows = 0, set_long = 0;
    if (!pp_lds(&pp_rows_kernel<K>, C::LDS_BYTES, &set_rows) || !pp_lds(&pp_long_rows_kernel<K>, C::LDS_BYTES, &set_long)) return PDA_ERR_LAUNCH;
    hipLaunchKernelGGL(pp_rows_kernel<K>, dim3((unsigned)n_work), dim3(C::NT), C::LDS_BYTES, s, a);
    if (n_long != 0) {
        hipLaunchKernelGGL(pp_long_rows_kernel<K>, dim3((unsigned)n_long), dim3(C::NT), C::LDS_BYTES, s, a);
        hipLaunchKernelGGL(pp_chunk_update_kernel<K>, dim3((unsigned)n_work), dim3(C::NT), 0, s, a);
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

template <int K>
int launch_block_pass_rowalpha(const PpRowAlphaArgs& ra, size_t n_work, size_t n_long, hipStream_t s) {
    using C = Cfg<K>;
    static int set_rows = 0, set_long = 0;
    if (!pp_lds(&pp_rows_rowalpha_kernel<K>, C::LDS_BYTES, &set_rows) || !pp_lds(&pp_long_rows_rowalpha_kernel<K>, C::LDS_BYTES, &set_long))
        return PDA_ERR_LAUNCH;
    hipLaunchKernelGGL(pp_rows_rowalpha_kernel<K>, dim3((unsigned)n_work), dim3(C::NT), C::LDS_BYTES, s, ra);
    if (n_long != 0) {
        hipLaunchKernelGGL(pp_long_rows_rowalpha_kernel<K>, dim3((unsigned)n_long), dim3(C::NT), C::LDS_BYTES, s, ra);
        hipLaunchKernelGGL(pp_chunk_update_kernel<K>, dim3((unsigned)n_work), dim3(C::NT), 0, s, ra.a);
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" int pda_ialspp_predict_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const float* X, const float* Z,
                                      size_t n_z, int d, float* e, void* stream) {
    if (!indptr || !X || !Z) return PDA_ERR_ARG;
    if (nnz != 0 && (!indices || !e)) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu || n_z == 0 || n_z > 0x7FFFFFFFu || nnz > ((size_t)1 << 40)) return PDA_ERR_ARG;
    if (!pp_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (nnz == 0) return PDA_OK;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const PredictArgs a{indptr, indices, X, Z, e, n_rows, nnz, (unsigned)n_z};
    const dim3 grid((unsigned)n_rows);
    switch (d) {
        case 32: hipLaunchKernelGGL(pp_predict_kernel<32>, grid, dim3(256), 0, s, a); break;
        case 64: hipLaunchKernelGGL(pp_predict_kernel<64>, grid, dim3(256), 0, s, a); break;
        case 128: hipLaunchKernelGGL(pp_predict_kernel<128>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(pp_predict_kernel<256>, grid, dim3(256), 0, s, a); break;
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_ialspp_block_pass_f32(const int64_t* indptr, const int32_t* indices, const int64_t* pair_perm, size_t n_rows, size_t nnz,
                                         const int64_t* work, size_t n_work, const int64_t* long_rows, size_t n_long, size_t n_slots,
                                         const float* Z, size_t n_z, const float* G, int d, int k, int p0, float alpha0, const float* lam_row,
                                         float* X, float* e, int32_t* fail_count, float* dbg, float* slots, size_t slot_floats, float* delta_ws,
                                         size_t delta_floats, void* stream) {
    if (!indptr || !work || !Z || !G || !lam_row || !X || !fail_count) return PDA_ERR_ARG;
    if (nnz != 0 && (!indices || !e)) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu || n_z == 0 || n_z > 0x7FFFFFFFu || nnz > ((size_t)1 << 40)) return PDA_ERR_ARG;
    if (n_work == 0 || n_work > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (!(alpha0 >= 0.f) || !std::isfinite(alpha0)) return PDA_ERR_ARG;
    if (X == Z || X == G || (e != nullptr && (e == X || e == Z || e == G))) return PDA_ERR_ARG;
    if (n_long > n_rows || (n_long != 0 && (!long_rows || n_slots < 2 * n_long)) || (n_long == 0 && n_slots != 0)) return PDA_ERR_ARG;
    if (n_work < n_slots || n_slots > 0x7FFFFFFFu) return PDA_ERR_ARG;      // one entry per chunk of a cut row, at least
    if (p0 < 0) return PDA_ERR_ARG;
    if (!pp_d_ok(d) || !pp_k_ok(k)) return PDA_ERR_UNSUPPORTED;
    if (d % k != 0 || p0 % k != 0 || p0 >= d) return PDA_ERR_ARG;
    if (n_slots != 0 && (!slots || !delta_ws || slot_floats < n_slots * PDA_IALSPP_SLOT_FLOATS(k) ||
                         delta_floats < PDA_IALSPP_DELTA_FLOATS(n_slots, k))) return PDA_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const PpArgs a{indptr, indices, pair_perm, work, long_rows, Z, G, lam_row, X, e, fail_count, dbg, slots, delta_ws,
                   n_rows, nnz, n_slots, (unsigned)n_z, d, p0, alpha0};
    switch (k) {
        case 32: return launch_block_pass<32>(a, n_work, n_long, s);
        case 64: return launch_block_pass<64>(a, n_work, n_long, s);
        default: return launch_block_pass<128>(a, n_work, n_long, s);
    }
}

extern "C" int pda_ialspp_block_pass_rowalpha_f32(const int64_t* indptr, const int32_t* indices, const int64_t* pair_perm, size_t n_rows, size_t nnz,
                                                  const int64_t* work, size_t n_work, const int64_t* long_rows, size_t n_long, size_t n_slots,
                                                  const float* Z, size_t n_z, const float* G, int d, int k, int p0, const float* alpha_row,
                                                  const float* lam_row, float* X, float* e, int32_t* fail_count, float* dbg, float* slots,
                                                  size_t slot_floats, float* delta_ws, size_t delta_floats, void* stream) {
    if (!indptr || !work || !Z || !G || !alpha_row || !lam_row || !X || !fail_count) return PDA_ERR_ARG;
    if (nnz != 0 && (!indices || !e)) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu || n_z == 0 || n_z > 0x7FFFFFFFu || nnz > ((size_t)1 << 40)) return PDA_ERR_ARG;
    if (n_work == 0 || n_work > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (X == Z || X == G || X == alpha_row || (e != nullptr && (e == X || e == Z || e == G || e == alpha_row))) return PDA_ERR_ARG;
    if (n_long > n_rows || (n_long != 0 && (!long_rows || n_slots < 2 * n_long)) || (n_long == 0 && n_slots != 0)) return PDA_ERR_ARG;
    if (n_work < n_slots || n_slots > 0x7FFFFFFFu) return PDA_ERR_ARG;      // one entry per chunk of a cut row, at least
    if (p0 < 0) return PDA_ERR_ARG;
    if (!pp_d_ok(d) || !pp_k_ok(k)) return PDA_ERR_UNSUPPORTED;
    if (d % k != 0 || p0 % k != 0 || p0 >= d) return PDA_ERR_ARG;
    if (n_slots != 0 && (!slots || !delta_ws || slot_floats < n_slots * PDA_IALSPP_SLOT_FLOATS(k) ||
                         delta_floats < PDA_IALSPP_DELTA_FLOATS(n_slots, k))) return PDA_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const PpRowAlphaArgs ra{PpArgs{indptr, indices, pair_perm, work, long_rows, Z, G, lam_row, X, e, fail_count, dbg, slots, delta_ws,
                                   n_rows, nnz, n_slots, (unsigned)n_z, d, p0, 0.f},
                            alpha_row};
    switch (k) {
        case 32: return launch_block_pass_rowalpha<32>(ra, n_work, n_long, s);
        case 64: return launch_block_pass_rowalpha<64>(ra, n_work, n_long, s);
        default: return launch_block_pass_rowalpha<128>(ra, n_work, n_long, s);
    }
}

extern "C" int pda_ialspp_gram256_scaled_f32(const float* Z, const float* scale_row, size_t n_rows, float* G, float* workspace, size_t workspace_floats,
                                             void* stream) {
    if (!Z || !scale_row || !G || !workspace) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (G == Z || G == scale_row) return PDA_ERR_ARG;
    if (workspace_floats < PDA_IALSPP_GRAM_WS_FLOATS(n_rows, 256)) return PDA_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t n_blocks = (n_rows + PDA_IALS_GRAM_ROWS - 1) / PDA_IALS_GRAM_ROWS;
    const GramScaledArgs sa{GramArgs{Z, G, workspace, n_rows, n_blocks}, scale_row};
    constexpr int TN = 256 / 32;
    hipLaunchKernelGGL(pp_gram_tiles_scaled_kernel<256>, dim3((unsigned)n_blocks, TN * (TN + 1) / 2), dim3(64), 0, s, sa);
    hipLaunchKernelGGL(pp_gram_sum_kernel<256>, dim3(256 * 256 / 256), dim3(256), 0, s, sa.g);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_ialspp_gram_f32(const float* Z, size_t n_rows, int d, float* G, float* workspace, size_t workspace_floats, void* stream) {
    if (!Z || !G || !workspace) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (!pp_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (workspace_floats < PDA_IALSPP_GRAM_WS_FLOATS(n_rows, d)) return PDA_ERR_ARG;
    if (d != 256) return pda_ials_gram_f32(Z, n_rows, d, G, workspace, workspace_floats * sizeof(float), stream);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const size_t n_blocks = (n_rows + PDA_IALS_GRAM_ROWS - 1) / PDA_IALS_GRAM_ROWS;
    const GramArgs a{Z, G, workspace, n_rows, n_blocks};
    constexpr int TN = 256 / 32;
    hipLaunchKernelGGL(pp_gram_tiles_kernel<256>, dim3((unsigned)n_blocks, TN * (TN + 1) / 2), dim3(64), 0, s, a);
    hipLaunchKernelGGL(pp_gram_sum_kernel<256>, dim3(256 * 256 / 256), dim3(256), 0, s, a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" int pda_ialspp_loss_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const float* X, const float* Z,
                                   size_t n_z, const float* G, int d, const float* lam_row, float* out, void* stream) {
    if (!indptr || !X || !Z || !G || !lam_row || !out) return PDA_ERR_ARG;
    if (nnz != 0 && !indices) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu || n_z == 0 || n_z > 0x7FFFFFFFu || nnz > ((size_t)1 << 40)) return PDA_ERR_ARG;
    if (!pp_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (d != 256) return pda_ials_loss_f32(indptr, indices, n_rows, nnz, X, Z, n_z, G, d, lam_row, out, stream);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const LossArgs a{indptr, indices, X, Z, G, lam_row, out, n_rows, nnz, (unsigned)n_z};
    constexpr int per = 256 / (256 / 4);
    hipLaunchKernelGGL(pp_loss_kernel<256>, dim3((unsigned)((n_rows + per - 1) / per)), dim3(256), 0, s, a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
