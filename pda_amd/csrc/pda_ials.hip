// The iALS baseline (include/pda_hip_ials.h) on MI355X (gfx950): the Gram matrix of a table, the exact row-wise half-sweep and
// the per-row terms of the objective.
//
// Half-sweep layout: ONE workgroup per entry of the work list (a whole row of at most PDA_IALS_CHUNK pairs, or one chunk of a longer row).
// The gathered rows of Z are staged in LDS in blocks of 32 (16-byte loads, the next block's loads in flight in registers while the current one
// is consumed); sum z z^T lives in the accumulators of v_mfma_f32_32x32x2_f32 -- only the lower triangle of 32 x 32 tiles, dealt round-robin to
// the waves -- and sum z in one register of d lanes.  The staged block and the matrix share the same LDS: the tiles are written out (mirrored to
// the upper triangle) only after the last block.  A chunk stores its partial (A, b) to its workspace slot; a whole row adds alpha0 G + lambda_r I,
// factorises in place (stride d + 1: a column walk over the lanes is conflict-free) and substitutes twice.  A second launch sums the slots of
// the cut rows in chunk order and runs the same tail.  The Gram matrix of the whole table is the same accumulation over consecutive rows.
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_hip_ials.h"
#include "pda_hip_ials_itemw.h"

namespace {

constexpr int kKB = 32;     // rows per staged block

template <int D>
struct Cfg {
    static constexpr int NT = D == 32 ? 64 : 256;           // lanes per workgroup
    static constexpr int NW = NT / 64;
    static constexpr int TN = D / 32;
    static constexpr int NTILES = TN * (TN + 1) / 2;        // lower triangle of 32 x 32 tiles
    static constexpr int MAXT = (NTILES + NW - 1) / NW;     // tiles per wave
    static constexpr int LD = D + 1;
    static constexpr int G = D / 4;                         // lanes per gathered row
    static constexpr int RPP = NT / G;                      // rows per gather pass
    static constexpr int NP = kKB / RPP;
    static constexpr size_t SLOT = (size_t)D * D + D;
    static constexpr size_t LDS_BYTES = ((size_t)D * LD + 3 * D + 4) * sizeof(float);     // A, b, y, x, the failed-pivot flag
};

struct IalsArgs {
    const int64_t* indptr;
    const int32_t* indices;
    const int64_t* work;        // [n_work, 4]: row, first pair, end pair, slot
    const int64_t* long_rows;   // [n_long, 3]: row, first slot, chunks
    const float* Z;
    const float* G;
    const float* lam_row;
    float* X_out;
    int32_t* fail;
    float* dbg;
    float* partials;            // [n_slots, d * d + d]
    size_t n_rows, nnz, n_slots;
    unsigned n_z;
    float alpha0;
};

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

// sum z z^T (symmetric, stride LD) and sum z over the rows k0 .. k1 of the list (GATHER: Z[idx[k]]; otherwise Z[k] itself), into sm as
// sA [D, LD] and sb [D].  Every lane of the workgroup calls it; it ends behind a barrier.  SCALED (pda_hip_ials_itemw.h): the row c enters as
// fl(scale[c] z_c[j]), the product fused into the row fetch -- one more 4-byte load and four multiplications per lane, no scaled copy of Z.
template <int D, bool GATHER, bool SCALED = false>
__device__ __forceinline__ void ials_accumulate(const int32_t* idx, const float* Z, unsigned n_z, int64_t k0, int64_t k1, float* sm,
                                                const float* scale = nullptr) {
    using C = Cfg<D>;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, i = lane & 31, h = lane >> 5;
    const int e = tid % C::G, rr = tid / C::G;
    const int bcol = tid - (C::NT - D);         // the last D lanes sum b: the waves with the fewest tiles
    float* sA = sm;
    float* sb = sm + D * C::LD;
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
    float bsum = 0.f;
    f32x4 pre[C::NP];
    auto fetch = [&](int64_t base) {
#pragma unroll
        for (int p = 0; p < C::NP; ++p) {
            const int64_t kk = base + p * C::RPP + rr;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (kk < k1) {
                const unsigned c = GATHER ? (unsigned)idx[kk] : (unsigned)kk;
                if (c < n_z) {
                    v = ld4(Z + (size_t)c * D + 4 * e);
                    if constexpr (SCALED) v = v * scale[c];
                }
            }
            pre[p] = v;
        }
    };
    if (k0 < k1) fetch(k0);
    for (int64_t base = k0; base < k1; base += kKB) {
#pragma unroll
        for (int p = 0; p < C::NP; ++p) st4(sm + (p * C::RPP + rr) * D + 4 * e, pre[p]);
        __syncthreads();
        if (base + kKB < k1) fetch(base + kKB);
#pragma unroll
        for (int kp = 0; kp < kKB / 2; ++kp) {
#pragma unroll
            for (int s = 0; s < C::MAXT; ++s) {
                if (wv + s * C::NW < C::NTILES) {
                    const float a = sm[(2 * kp + h) * D + 32 * ti[s] + i];
                    const float b = sm[(2 * kp + h) * D + 32 * tj[s] + i];
                    acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc[s], 0, 0, 0);
                }
            }
        }
        if (bcol >= 0) {
#pragma unroll 8
            for (int k = 0; k < kKB; ++k) bsum = bsum + sm[k * D + bcol];
        }
        __syncthreads();
    }
#pragma unroll
    for (int s = 0; s < C::MAXT; ++s) {
        if (wv + s * C::NW < C::NTILES) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int r = acc_row(reg, h);
                sA[(32 * ti[s] + r) * C::LD + 32 * tj[s] + i] = acc[s][reg];
                if (ti[s] != tj[s]) sA[(32 * tj[s] + i) * C::LD + 32 * ti[s] + r] = acc[s][reg];
            }
        }
    }
    if (bcol >= 0) sb[bcol] = bsum;
    __syncthreads();
}

// The tail of a row whose sums stand in sm: A += alpha G + lambda_r I, A = L L^T in place, L y = b, L^T x = y, the 16-byte store.  alpha is
// a.alpha0, or with
// ROWALPHA the row's own alpha_row[row] (pda_hip_ials_itemw.h).
template <int D, bool ROWALPHA = false>
__device__ __forceinline__ void ials_finish_solve(const IalsArgs& a, int64_t row, float* sm, const float* alpha_row = nullptr) {
    using C = Cfg<D>;
    const int tid = threadIdx.x;
    float* sA = sm;
    float* sb = sm + D * C::LD;
    float* sy = sb + D;
    float* sx = sy + D;
    int* sflag = reinterpret_cast<int*>(sx + D);
    const float lam = a.lam_row[row];
    float ar = 0.f;
    if constexpr (ROWALPHA) ar = alpha_row[row];
    float* dbg = a.dbg != nullptr ? a.dbg + (size_t)row * C::SLOT : nullptr;
    if (tid == 0) *sflag = 0;
    for (int q = tid; q < D * D; q += C::NT) {
        const int i = q / D, j = q % D;
        float v = sA[i * C::LD + j] + (ROWALPHA ? ar : a.alpha0) * a.G[q];
        if (i == j) v = v + lam;
        sA[i * C::LD + j] = v;
        if (dbg != nullptr) dbg[q] = v;
    }
    if (dbg != nullptr && tid < D) dbg[D * D + tid] = sb[tid];
    __syncthreads();
    for (int j = 0; j < D; ++j) {
        float s = 0.f;
        if (tid >= j && tid < D) {
            const float* ri = sA + tid * C::LD;
            const float* rj = sA + j * C::LD;
            s = ri[j];
            for (int k = 0; k < j; ++k) s = fmaf(-ri[k], rj[k], s);
            if (tid == j) {
                if (!(s > 0.f) || !(s < INFINITY)) *sflag = 1;
                sA[j * C::LD + j] = sqrtf(s);
            }
        }
        __syncthreads();
        if (tid > j && tid < D) sA[tid * C::LD + j] = s / sA[j * C::LD + j];
        __syncthreads();
    }
    for (int j = 0; j < D; ++j) {
        if (tid >= j && tid < D) {
            const float yj = sb[j] / sA[j * C::LD + j];
            if (tid == j) sy[j] = yj;
            else sb[tid] = fmaf(-sA[tid * C::LD + j], yj, sb[tid]);
        }
        __syncthreads();
    }
    for (int j = D - 1; j >= 0; --j) {
        if (tid <= j) {
            const float xj = sy[j] / sA[j * C::LD + j];
            if (tid == j) sx[j] = xj;
            else sy[tid] = fmaf(-sA[j * C::LD + tid], xj, sy[tid]);
        }
        __syncthreads();
    }
    const bool bad = *sflag != 0;
    if (tid < D / 4) {
        f32x4 v = {sx[4 * tid], sx[4 * tid + 1], sx[4 * tid + 2], sx[4 * tid + 3]};
        if (bad) v = f32x4{NAN, NAN, NAN, NAN};
        st4(a.X_out + (size_t)row * D + 4 * tid, v);
    }
    if (bad && tid == 0 && a.fail != nullptr) atomicAdd(a.fail, 1);
}

template <int D>
__global__ __launch_bounds__(Cfg<D>::NT) void ials_rows_kernel(IalsArgs a) {
    using C = Cfg<D>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ials_smem[];
    float* sm = reinterpret_cast<float*>(ials_smem);
    const int64_t* wk = a.work + 4 * (size_t)blockIdx.x;
    const int64_t row = wk[0], k0 = wk[1], k1 = wk[2], slot = wk[3];
    if (row < 0 || (uint64_t)row >= a.n_rows || k0 < 0 || k1 < k0 || (uint64_t)k1 > a.nnz || slot >= (int64_t)a.n_slots) return;   // (uniform)
    ials_accumulate<D, true>(a.indices, a.Z, a.n_z, k0, k1, sm);
    if (slot >= 0) {
        float* dst = a.partials + (size_t)slot * C::SLOT;
        for (int q = threadIdx.x; q < D * D; q += C::NT) dst[q] = sm[(q / D) * C::LD + q % D];
        if (threadIdx.x < D) dst[D * D + threadIdx.x] = sm[D * C::LD + threadIdx.x];
        return;
    }
    ials_finish_solve<D>(a, row, sm);
}

// the cut rows: the slots of a row in chunk order onto zero, then the same tail
template <int D>
__global__ __launch_bounds__(Cfg<D>::NT) void ials_long_rows_kernel(IalsArgs a) {
    using C = Cfg<D>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ials_smem[];
    float* sm = reinterpret_cast<float*>(ials_smem);
    const int64_t* lr = a.long_rows + 3 * (size_t)blockIdx.x;
    const int64_t row = lr[0], s0 = lr[1], n = lr[2];
    if (row < 0 || (uint64_t)row >= a.n_rows || s0 < 0 || n < 0 || (uint64_t)s0 + (uint64_t)n > a.n_slots) return;   // (uniform)
    const float* src = a.partials + (size_t)s0 * C::SLOT;
    for (int q = threadIdx.x; q < D * D; q += C::NT) {
        float v = 0.f;
        for (int64_t j = 0; j < n; ++j) v = v + src[(size_t)j * C::SLOT + q];
        sm[(q / D) * C::LD + q % D] = v;
    }
    if (threadIdx.x < D) {
        float v = 0.f;
        for (int64_t j = 0; j < n; ++j) v = v + src[(size_t)j * C::SLOT + D * D + threadIdx.x];
        sm[D * C::LD + threadIdx.x] = v;
    }
    __syncthreads();
    ials_finish_solve<D>(a, row, sm);
}

// The same two kernels with alpha_row (pda_ials_half_sweep_rowalpha_f32): their text is that of the two above with the tail's ROWALPHA flag
// set.  They are kernels of their own, with their own argument struct, so that the two above keep their argument layout and their
// instructions (a body shared through a function of both reordered the instructions of ials_rows_kernel); a.alpha0 is not read here.
struct IalsRowAlphaArgs {
    IalsArgs a;
    const float* alpha_row;     // [n_rows]
};

template <int D>
__global__ __launch_bounds__(Cfg<D>::NT) void ials_rows_rowalpha_kernel(IalsRowAlphaArgs ra) {
    using C = Cfg<D>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ials_smem[];
    float* sm = reinterpret_cast<float*>(ials_smem);
    const IalsArgs& a = ra.a;
    const int64_t* wk = a.work + 4 * (size_t)blockIdx.x;
    const int64_t row = wk[0], k0 = wk[1], k1 = wk[2], slot = wk[3];
    if (row < 0 || (uint64_t)row >= a.n_rows || k0 < 0 || k1 < k0 || (uint64_t)k1 > a.nnz || slot >= (int64_t)a.n_slots) return;   // (uniform)
    ials_accumulate<D, true>(a.indices, a.Z, a.n_z, k0, k1, sm);
    if (slot >= 0) {
        float* dst = a.partials + (size_t)slot * C::SLOT;
        for (int q = threadIdx.x; q < D * D; q += C::NT) dst[q] = sm[(q / D) * C::LD + q % D];
        if (threadIdx.x < D) dst[D * D + threadIdx.x] = sm[D * C::LD + threadIdx.x];
        return;
    }
    ials_finish_solve<D, true>(a, row, sm, ra.alpha_row);
}

template <int D>
__global__ __launch_bounds__(Cfg<D>::NT) void ials_long_rows_rowalpha_kernel(IalsRowAlphaArgs ra) {
    using C = Cfg<D>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ials_smem[];
    float* sm = reinterpret_cast<float*>(ials_smem);
    const IalsArgs& a = ra.a;
    const int64_t* lr = a.long_rows + 3 * (size_t)blockIdx.x;
    const int64_t row = lr[0], s0 = lr[1], n = lr[2];
    if (row < 0 || (uint64_t)row >= a.n_rows || s0 < 0 || n < 0 || (uint64_t)s0 + (uint64_t)n > a.n_slots) return;   // (uniform)
    const float* src = a.partials + (size_t)s0 * C::SLOT;
    for (int q = threadIdx.x; q < D * D; q += C::NT) {
        float v = 0.f;
        for (int64_t j = 0; j < n; ++j) v = v + src[(size_t)j * C::SLOT + q];
        sm[(q / D) * C::LD + q % D] = v;
    }
    if (threadIdx.x < D) {
        float v = 0.f;
        for (int64_t j = 0; j < n; ++j) v = v + src[(size_t)j * C::SLOT + D * D + threadIdx.x];
        sm[D * C::LD + threadIdx.x] = v;
    }
    __syncthreads();
    ials_finish_solve<D, true>(a, row, sm, ra.alpha_row);
}

struct GramArgs {
    const float* Z;
    float* G;
    float* partials;        // [n_blocks, d * d + d]; the d * d part is used
    size_t n_rows, n_blocks;
};

template <int D>
__global__ __launch_bounds__(Cfg<D>::NT) void ials_gram_blocks_kernel(GramArgs a) {
    using C = Cfg<D>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ials_smem[];
    float* sm = reinterpret_cast<float*>(ials_smem);
    const int64_t k0 = (int64_t)blockIdx.x * PDA_IALS_GRAM_ROWS;
    const int64_t k1 = k0 + PDA_IALS_GRAM_ROWS < (int64_t)a.n_rows ? k0 + PDA_IALS_GRAM_ROWS : (int64_t)a.n_rows;
    ials_accumulate<D, false>(nullptr, a.Z, (unsigned)a.n_rows, k0, k1, sm);
    float* dst = a.partials + (size_t)blockIdx.x * C::SLOT;
    for (int q = threadIdx.x; q < D * D; q += C::NT) dst[q] = sm[(q / D) * C::LD + q % D];
}

// G_w = sum_c (s_c z_c)(s_c z_c)^T: the same blocks with the scale fused into the row fetch (pda_ials_gram_scaled_f32); the blocks are added by
// ials_gram_sum_kernel as they are.
struct GramScaledArgs {
    GramArgs g;
    const float* scale;     // [n_rows]
};

template <int D>
__global__ __launch_bounds__(Cfg<D>::NT) void ials_gram_scaled_blocks_kernel(GramScaledArgs sa) {
    using C = Cfg<D>;
    extern __shared__ __attribute__((aligned(16))) unsigned char ials_smem[];
    float* sm = reinterpret_cast<float*>(ials_smem);
    const GramArgs& a = sa.g;
    const int64_t k0 = (int64_t)blockIdx.x * PDA_IALS_GRAM_ROWS;
    const int64_t k1 = k0 + PDA_IALS_GRAM_ROWS < (int64_t)a.n_rows ? k0 + PDA_IALS_GRAM_ROWS : (int64_t)a.n_rows;
    ials_accumulate<D, false, true>(nullptr, a.Z, (unsigned)a.n_rows, k0, k1, sm, sa.scale);
    float* dst = a.partials + (size_t)blockIdx.x * C::SLOT;
    for (int q = threadIdx.x; q < D * D; q += C::NT) dst[q] = sm[(q / D) * C::LD + q % D];
}

template <int D>
__global__ __launch_bounds__(256) void ials_gram_sum_kernel(GramArgs a) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= D * D) return;
    float v = 0.f;
    for (size_t c = 0; c < a.n_blocks; ++c) v = v + a.partials[c * Cfg<D>::SLOT + q];
    a.G[q] = v;
}

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

__device__ __forceinline__ float hsum4(f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }
template <int G>
__device__ __forceinline__ float group_sum(float v) {
#pragma unroll
    for (int off = G / 2; off >= 1; off >>= 1) v = v + __shfl_xor(v, off);
    return v;
}

template <int D>
__global__ __launch_bounds__(256) void ials_loss_kernel(LossArgs a) {
    constexpr int G = D / 4, PER = 256 / G;
    __shared__ __attribute__((aligned(16))) float sx[PER * D];
    const int e = threadIdx.x % G, rl = threadIdx.x / G;
    const size_t row = (size_t)blockIdx.x * PER + rl;
    const bool valid = row < a.n_rows;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (valid) x = ld4(a.X + row * D + 4 * e);
    st4(sx + rl * D + 4 * e, x);
    __syncthreads();
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    for (int i = 0; i < D; ++i) t = t + ld4(a.G + (size_t)i * D + 4 * e) * sx[rl * D + i];
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
        if (c < a.n_z) z = ld4(a.Z + (size_t)c * D + 4 * e);
        const float r = group_sum<G>(hsum4(x * z)) - 1.f;
        fit = fit + r * r;
    }
    if (valid && e == 0) {
        a.out[row * 3 + 0] = fit;
        a.out[row * 3 + 1] = q;
        a.out[row * 3 + 2] = a.lam_row[row] * nn;
    }
}

inline bool ials_d_ok(int d) { return d == 32 || d == 64 || d == 128; }

template <typename K>
bool ials_lds(K kernel, size_t bytes, int* done) {
    if (*done) return true;     // idempotent attribute; benign if raced
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) != hipSuccess) return false;
    *done = 1;
    return true;
}

template <int D>
int launch_half_sweep(const IalsArgs& a, size_t n_work, size_t n_long, hipStream_t s) {
    using C = Cfg<D>;
    static int set_rows = 0, set_long = 0;
    if (!ials_lds(&ials_rows_kernel<D>, C::LDS_BYTES, &set_rows) || !ials_lds(&ials_long_rows_kernel<D>, C::LDS_BYTES, &set_long)) return PDA_ERR_LAUNCH;
    hipLaunchKernelGGL(ials_rows_kernel<D>, dim3((unsigned)n_work), dim3(C::NT), C::LDS_BYTES, s, a);
    if (n_long != 0) hipLaunchKernelGGL(ials_long_rows_kernel<D>, dim3((unsigned)n_long), dim3(C::NT), C::LDS_BYTES, s, a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

template <int D>
int launch_half_sweep_rowalpha(const IalsRowAlphaArgs& ra, size_t n_work, size_t n_long, hipStream_t s) {
    using C = Cfg<D>;
    static int set_rows = 0, set_long = 0;
    if (!ials_lds(&ials_rows_rowalpha_kernel<D>, C::LDS_BYTES, &set_rows) || !ials_lds(&ials_long_rows_rowalpha_kernel<D>, C::LDS_BYTES, &set_long))
        return PDA_ERR_LAUNCH;
    hipLaunchKernelGGL(ials_rows_rowalpha_kernel<D>, dim3((unsigned)n_work), dim3(C::NT), C::LDS_BYTES, s, ra);
    if (n_long != 0) hipLaunchKernelGGL(ials_long_rows_rowalpha_kernel<D>, dim3((unsigned)n_long), dim3(C::NT), C::LDS_BYTES, s, ra);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

template <int D>
int launch_gram_scaled(const GramScaledArgs& sa, hipStream_t s) {
    using C = Cfg<D>;
    static int set_gram = 0;
    if (!ials_lds(&ials_gram_scaled_blocks_kernel<D>, C::LDS_BYTES, &set_gram)) return PDA_ERR_LAUNCH;
    hipLaunchKernelGGL(ials_gram_scaled_blocks_kernel<D>, dim3((unsigned)sa.g.n_blocks), dim3(C::NT), C::LDS_BYTES, s, sa);
    hipLaunchKernelGGL(ials_gram_sum_kernel<D>, dim3((unsigned)((D * D + 255) / 256)), dim3(256), 0, s, sa.g);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

template <int D>
int launch_gram(const GramArgs& a, hipStream_t s) {
    using C = Cfg<D>;
    static int set_gram = 0;
    if (!ials_lds(&ials_gram_blocks_kernel<D>, C::LDS_BYTES, &set_gram)) return PDA_ERR_LAUNCH;
    hipLaunchKernelGGL(ials_gram_blocks_kernel<D>, dim3((unsigned)a.n_blocks), dim3(C::NT), C::LDS_BYTES, s, a);
    hipLaunchKernelGGL(ials_gram_sum_kernel<D>, dim3((unsigned)((D * D + 255) / 256)), dim3(256), 0, s, a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" size_t pda_ials_workspace_bytes(size_t n_slots, int d) {
    if (!ials_d_ok(d)) return 0;
    return n_slots * ((size_t)d * d + d) * sizeof(float);
}

extern "C" int pda_ials_gram_f32(const float* Z, size_t n_rows, int d, float* G, void* workspace, size_t workspace_bytes, void* stream) {
    if (!Z || !G || !workspace) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (!ials_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    const size_t n_blocks = (n_rows + PDA_IALS_GRAM_ROWS - 1) / PDA_IALS_GRAM_ROWS;
    if (workspace_bytes < pda_ials_workspace_bytes(n_blocks, d)) return PDA_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const GramArgs a{Z, G, reinterpret_cast<float*>(workspace), n_rows, n_blocks};
    switch (d) {
        case 32: return launch_gram<32>(a, s);
        case 64: return launch_gram<64>(a, s);
        default: return launch_gram<128>(a, s);
    }
}

extern "C" int pda_ials_half_sweep_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const int64_t* work, size_t n_work,
                                       const int64_t* long_rows, size_t n_long, size_t n_slots, const float* Z, size_t n_z, const float* G, int d,
                                       float alpha0, const float* lam_row, float* X_out, int32_t* fail_count, float* dbg_normal, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    if (!indptr || !work || !Z || !G || !lam_row || !X_out || !fail_count) return PDA_ERR_ARG;
    if (nnz != 0 && !indices) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu || n_z == 0 || n_z > 0x7FFFFFFFu || nnz > ((size_t)1 << 40)) return PDA_ERR_ARG;
    if (n_work == 0 || n_work > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (!(alpha0 >= 0.f) || !std::isfinite(alpha0)) return PDA_ERR_ARG;
    if (X_out == Z || X_out == G) return PDA_ERR_ARG;
    if (n_long > n_rows || (n_long != 0 && (!long_rows || n_slots < 2 * n_long)) || (n_long == 0 && n_slots != 0)) return PDA_ERR_ARG;
    if (n_work < n_slots || n_slots > 0x7FFFFFFFu) return PDA_ERR_ARG;      // one entry per chunk of a cut row, at least
    if (!ials_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (n_slots != 0 && (!workspace || workspace_bytes < pda_ials_workspace_bytes(n_slots, d))) return PDA_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const IalsArgs a{indptr, indices, work, long_rows, Z, G, lam_row, X_out, fail_count, dbg_normal, reinterpret_cast<float*>(workspace),
                     n_rows, nnz, n_slots, (unsigned)n_z, alpha0};
    switch (d) {
        case 32: return launch_half_sweep<32>(a, n_work, n_long, s);
        case 64: return launch_half_sweep<64>(a, n_work, n_long, s);
        default: return launch_half_sweep<128>(a, n_work, n_long, s);
    }
}

extern "C" int pda_ials_gram_scaled_f32(const float* Z, const float* scale_row, size_t n_rows, int d, float* G, float* workspace,
                                        size_t workspace_floats, void* stream) {
    if (!Z || !scale_row || !G || !workspace) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (G == Z || G == scale_row) return PDA_ERR_ARG;
    if (!ials_d_ok(d) && d != 256) return PDA_ERR_UNSUPPORTED;
    const size_t n_blocks = (n_rows + PDA_IALS_GRAM_ROWS - 1) / PDA_IALS_GRAM_ROWS;
    if (workspace_floats < n_blocks * ((size_t)d * d + d)) return PDA_ERR_ARG;
    if (d == 256) return pda_ialspp_gram256_scaled_f32(Z, scale_row, n_rows, G, workspace, workspace_floats, stream);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const GramScaledArgs sa{GramArgs{Z, G, workspace, n_rows, n_blocks}, scale_row};
    switch (d) {
        case 32: return launch_gram_scaled<32>(sa, s);
        case 64: return launch_gram_scaled<64>(sa, s);
        default: return launch_gram_scaled<128>(sa, s);
    }
}

extern "C" int pda_ials_half_sweep_rowalpha_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const int64_t* work,
                                                size_t n_work, const int64_t* long_rows, size_t n_long, size_t n_slots, const float* Z, size_t n_z,
                                                const float* G, int d, const float* alpha_row, const float* lam_row, float* X_out,
                                                int32_t* fail_count, float* dbg_normal, void* workspace, size_t workspace_bytes, void* stream) {
    if (!indptr || !work || !Z || !G || !alpha_row || !lam_row || !X_out || !fail_count) return PDA_ERR_ARG;
    if (nnz != 0 && !indices) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu || n_z == 0 || n_z > 0x7FFFFFFFu || nnz > ((size_t)1 << 40)) return PDA_ERR_ARG;
    if (n_work == 0 || n_work > 0x7FFFFFFFu) return PDA_ERR_ARG;
    if (X_out == Z || X_out == G || X_out == alpha_row) return PDA_ERR_ARG;
    if (n_long > n_rows || (n_long != 0 && (!long_rows || n_slots < 2 * n_long)) || (n_long == 0 && n_slots != 0)) return PDA_ERR_ARG;
    if (n_work < n_slots || n_slots > 0x7FFFFFFFu) return PDA_ERR_ARG;      // one entry per chunk of a cut row, at least
    if (!ials_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (n_slots != 0 && (!workspace || workspace_bytes < pda_ials_workspace_bytes(n_slots, d))) return PDA_ERR_ARG;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const IalsRowAlphaArgs ra{IalsArgs{indptr, indices, work, long_rows, Z, G, lam_row, X_out, fail_count, dbg_normal,
                                       reinterpret_cast<float*>(workspace), n_rows, nnz, n_slots, (unsigned)n_z, 0.f},
                              alpha_row};
    switch (d) {
        case 32: return launch_half_sweep_rowalpha<32>(ra, n_work, n_long, s);
        case 64: return launch_half_sweep_rowalpha<64>(ra, n_work, n_long, s);
        default: return launch_half_sweep_rowalpha<128>(ra, n_work, n_long, s);
    }
}

extern "C" int pda_ials_loss_f32(const int64_t* indptr, const int32_t* indices, size_t n_rows, size_t nnz, const float* X, const float* Z, size_t n_z,
                                 const float* G, int d, const float* lam_row, float* out, void* stream) {
    if (!indptr || !X || !Z || !G || !lam_row || !out) return PDA_ERR_ARG;
    if (nnz != 0 && !indices) return PDA_ERR_ARG;
    if (n_rows == 0 || n_rows > 0x7FFFFFFFu || n_z == 0 || n_z > 0x7FFFFFFFu || nnz > ((size_t)1 << 40)) return PDA_ERR_ARG;
    if (!ials_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const LossArgs a{indptr, indices, X, Z, G, lam_row, out, n_rows, nnz, (unsigned)n_z};
    const int per = 256 / (d / 4);
    const dim3 grid((unsigned)((n_rows + per - 1) / per));
    switch (d) {
        case 32: hipLaunchKernelGGL(ials_loss_kernel<32>, grid, dim3(256), 0, s, a); break;
        case 64: hipLaunchKernelGGL(ials_loss_kernel<64>, grid, dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL(ials_loss_kernel<128>, grid, dim3(256), 0, s, a); break;
    }
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
