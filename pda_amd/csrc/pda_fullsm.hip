// The full-catalogue softmax loss (include/pda_hip_fullsm.h) on MI355X (gfx950): the columns of the [B, n_items] logit matrix are
// ALL items.  The matrix exists only as 32 x 32 tiles in the accumulators of v_mfma_f32_32x32x2_f32 (exact f32), the tile loop of pda_inbatch.hip
// with the item table itself as the column side.  Three passes over the tiles, no float atomic and no partial sum of the item side in memory:
//   pack    the B user rows gathered once into an image in the workspace (u^ under norm, the raw rows otherwise) with 1 / max(|u|, 1e-12), |u|^2
//           and the validated positive beside it.
//   inv     (norm) 1 / max(|i_c|, 1e-12) of every item: the tile loads scale the rows of I by it, no normalised image of I is kept.
//   bits    (train graph) the exclusion mask, B x ceil(n_items / 32) words: one thread per word, a binary search for the word's first item in
//           the sorted train row, then the row's items inside the word.  One writer per word; the passes read 32 words per tile.
//   stats   workgroup (row tile, column split): the logit tiles of the split, each lane's running (m, se) over its 16 rows, merged over the 32
//           lanes of a row at the end -> (m, se) per (split, row); the tile that holds a row's positive also stores S_{r,pos[r]}.
//   merge   one thread per row: (m, se) over the splits in split order -> m, 1 / se, log se (and row_stats).
//   gradu   workgroup (row tile, column split): the same tiles recomputed by the same code (bit for bit the logits the statistics saw), C for
//           the tile, C I^ with the tile transposed through LDS, summed over the split's column tiles in accumulators -> the split's partial g_r.
//   gradi   workgroup = ONE column tile, which it owns: the tiles of ALL row tiles in ascending order, C^T U^ straight from the accumulator
//           layout summed in accumulators over the whole batch, then the projection, n_c c_reg i_c, gI and tagI of its 32 items.
//   tail    d / 4 lanes per row: the partial g_r added in split order, the projection, c_reg u_r, gU, tagU and the block's loss terms through
//           the shared pieces of pda_train_common.h.
//   loss    one wave: the blocks' loss terms summed in a fixed order into loss_acc.
// A workgroup of the three tile passes is ONE wave: nothing but the wave's own LDS traffic orders it.  Each pass fetches its next tile into
// registers before it computes on the current one (TileRegs), so the loads run under the MFMAs.
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_softmax_tiles.h"
#include "pda_hip_fullsm.h"

namespace {

constexpr int kTargetGroups = 1024;     // workgroups of one wave the split passes aim at: one per SIMD of the chip
static_assert(PDA_FULLSM_ROW_TILE == kT && PDA_FULLSM_COL_TILE == kT, "the tile passes are written for 32 x 32 tiles");

// ---- the workspace ------------------------------------------------------------------------------------------------------------------------------
struct Ws {
    float* P;           // [Bp, d]   the user rows (u^ under norm)
    float* inv_u;       // [Bp]      1 / max(|u|, 1e-12)
    float* sq_u;        // [Bp]      |u|^2
    float* diag;        // [Bp]      S_{r,pos[r]}
    float* rm;          // [Bp]      m_r           (-inf for a dropped row)
    float* rinv;        // [Bp]      1 / se_r      (0 for a dropped row)
    float* rlog;        // [Bp]      log se_r
    int32_t* vpos;      // [Bp]      pos[r], -1 for an invalid row
    float* part;        // [splits, Bp, 2]  (m, se)
    float* lossp;       // [tail blocks, 2] (mf, reg) of the block
    float* inv_i;       // [n_items] 1 / max(|i_c|, 1e-12)
    float* GU;          // [splits, Bp, d]  the split's sum_c C_rc i^_c
    uint32_t* bits;     // [B, W]    bit c % 32 of word [r, c / 32]: item c is a train item of users[r]
    size_t bytes;
};

inline int tiles_of(size_t n) { return (int)((n + kT - 1) / kT); }
// column tiles per split, and the number of splits that leaves
inline int tiles_per_split(size_t n_items, int B) {
    const int nr = tiles_of((size_t)B), nc = tiles_of(n_items);
    int want = (kTargetGroups + nr - 1) / nr;       // splits that would give kTargetGroups workgroups
    if (want > nc) want = nc;
    return (nc + want - 1) / want;
}
inline int col_splits(size_t n_items, int B) {
    const int nc = tiles_of(n_items), tps = tiles_per_split(n_items, B);
    return (nc + tps - 1) / tps;
}
inline int tail_blocks(int B, int d) { return (B + 512 / (d / 4) - 1) / (512 / (d / 4)); }

inline bool sizes_ok(int B, size_t n_items) { return B >= 1 && B <= PDA_FULLSM_MAX_B && n_items >= 1 && n_items <= 0x7FFFFFFFu; }

Ws carve(void* base, int B, size_t n_items, int d) {
    const size_t Bp = (size_t)tiles_of((size_t)B) * kT, S = (size_t)col_splits(n_items, B), W = (size_t)tiles_of(n_items);
    char* p = reinterpret_cast<char*>(base);
    Ws w;
    size_t off = 0;
    auto take = [&](size_t n_words) {
        char* at = p + off;
        off += ((n_words * 4 + 15) / 16) * 16;
        return at;
    };
    w.P = reinterpret_cast<float*>(take(Bp * d));
    w.inv_u = reinterpret_cast<float*>(take(Bp));
    w.sq_u = reinterpret_cast<float*>(take(Bp));
    w.diag = reinterpret_cast<float*>(take(Bp));
    w.rm = reinterpret_cast<float*>(take(Bp));
    w.rinv = reinterpret_cast<float*>(take(Bp));
    w.rlog = reinterpret_cast<float*>(take(Bp));
    w.vpos = reinterpret_cast<int32_t*>(take(Bp));
    w.part = reinterpret_cast<float*>(take(S * Bp * 2));
    w.lossp = reinterpret_cast<float*>(take((size_t)tail_blocks(B, d) * 2));
    w.inv_i = reinterpret_cast<float*>(take(n_items));
    w.GU = reinterpret_cast<float*>(take(S * Bp * d));
    w.bits = reinterpret_cast<uint32_t*>(take((size_t)B * W));
    w.bytes = off;
    return w;
}

struct FullsmArgs {
    const float* U;
    const float* I;
    const int32_t* users;
    const int32_t* pos;
    const int64_t* indptr;      // null: no mask
    const int32_t* indices;
    float* gU;
    float* gI;
    int32_t* tagU;
    int32_t* tagI;
    float* loss_acc;
    float* row_stats;
    Ws ws;
    unsigned n_users, n_items;
    int tag;
    int B, Bp, W;               // W: column tiles = words per mask row
    int tps, splits;            // column tiles per split, splits
    int n_tail;                 // workgroups of the tail
    float inv_B, inv_tau, reg_c;
    int users_distinct;
};

// ---- pack: d / 4 lanes per row, B user rows ---------------------------------------------------------------------------------------------------------
template <int D, bool NORM>
__device__ __forceinline__ void pack_body(const FullsmArgs& a) {
    constexpr int L = D / 4, TPB = 512 / L;
    const int g = threadIdx.x / L, e = threadIdx.x % L;
    const int r = blockIdx.x * TPB + g;
    if (r >= a.B) return;                           // (whole lane groups leave)
    const int u = a.users[r], p = a.pos[r];
    const bool ok = (unsigned)u < a.n_users && (unsigned)p < a.n_items;
    f32x4 x = {0.f, 0.f, 0.f, 0.f};
    if (ok) x = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * D + 4 * e);
    const float sq = group_sum<D>(dot4(x, x));
    const float inv = 1.f / fmaxf(sqrtf(sq), kNormFloor);
    if constexpr (NORM) x = x * inv;
    *reinterpret_cast<f32x4*>(a.ws.P + (size_t)r * D + 4 * e) = x;
    if (e == 0) {
        a.ws.inv_u[r] = inv;
        a.ws.sq_u[r] = sq;
        a.ws.vpos[r] = ok ? p : -1;
        a.ws.diag[r] = 0.f;
    }
}
template <int D>
__global__ void __launch_bounds__(512) fullsm_pack_kernel(FullsmArgs a) { pack_body<D, false>(a); }
template <int D>
__global__ void __launch_bounds__(512) fullsm_pack_norm_kernel(FullsmArgs a) { pack_body<D, true>(a); }

// ---- inv: d / 4 lanes per item ------------------------------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(512) fullsm_inv_kernel(FullsmArgs a) {
    constexpr int L = D / 4, TPB = 512 / L;
    const int g = threadIdx.x / L, e = threadIdx.x % L;
    const size_t c = (size_t)blockIdx.x * TPB + g;
    if (c >= a.n_items) return;                     // (whole lane groups leave)
    const f32x4 x = *reinterpret_cast<const f32x4*>(a.I + c * D + 4 * e);
    const float sq = group_sum<D>(dot4(x, x));
    if (e == 0) a.ws.inv_i[c] = 1.f / fmaxf(sqrtf(sq), kNormFloor);
}

// ---- bits: one thread per word of the exclusion mask, grid (ceil(W / 256), B) --------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fullsm_bits_kernel(FullsmArgs a) {
    const int w = blockIdx.x * 256 + threadIdx.x, r = blockIdx.y;
    if (w >= a.W) return;
    uint32_t word = 0u;
    const int u = a.users[r];
    if ((unsigned)u < a.n_users) {
        int64_t lo = a.indptr[u];
        const int64_t end = a.indptr[u + 1];
        const int64_t first = (int64_t)w * 32;      // the word's items: [first, first + 32)
        int64_t hi = end;
        while (lo < hi) {                           // the first entry of the row that is >= first
            const int64_t mid = lo + (hi - lo) / 2;
            if ((int64_t)a.indices[mid] < first) lo = mid + 1;
            else hi = mid;
        }
        for (; lo < end; ++lo) {
            const int64_t off = (int64_t)a.indices[lo] - first;
            if (off >= 32) break;
            word |= 1u << (unsigned)off;
        }
    }
    a.ws.bits[(size_t)r * a.W + w] = word;
}

// ---- the tile passes (the tile itself: pda_softmax_tiles.h) --------------------------------------------------------------------------------------------------------------------------------
// A tile on its way from global memory to its LDS image (the layout of load_tile, pda_softmax_tiles.h): every pass fetches the NEXT tile
// into registers before it computes on the current one and stores it behind the barrier, so the loads' latency runs under the MFMAs.  Rows at
// and past rows_end are zero (rows_end <= row0: nothing is loaded).  scale (or null): row r is multiplied by scale[r] on its way to the LDS
// (an item row becomes i^).
template <int D>
struct TileRegs {
    static constexpr int N = kT * (D / 4) / 64;     // float4 per lane
    f32x4 v[N];
    float sc[N];
};
template <int D>
__device__ __forceinline__ void fetch_tile(TileRegs<D>& t, const float* P, int row0, int rows_end, const float* scale) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int k = 0; k < TileRegs<D>::N; ++k) {
        const int idx = threadIdx.x + 64 * k, row = idx / Q, q = idx % Q;
        const bool in = row < rows_end - row0;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        t.v[k] = in ? *reinterpret_cast<const f32x4*>(P + (size_t)(row0 + row) * D + 4 * q) : zero;
        t.sc[k] = (in && scale) ? scale[row0 + row] : 1.f;
    }
}
template <int D, bool SCALED>
__device__ __forceinline__ void store_tile(float* s, const TileRegs<D>& t) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int k = 0; k < TileRegs<D>::N; ++k) {
        const int idx = threadIdx.x + 64 * k, row = idx / Q, q = idx % Q;
        *reinterpret_cast<f32x4*>(s + row * (D + 4) + 4 * q) = SCALED ? t.v[k] * t.sc[k] : t.v[k];
    }
}

// is item c in E_r?  (pos_r: vpos of row r, -1 for a row that is dropped or past B; word: the row's mask word of this column tile)
__device__ __forceinline__ bool admitted(int pos_r, int c, unsigned n_items, uint32_t word) {
    if (pos_r < 0 || (unsigned)c >= n_items) return false;
    return c == pos_r || ((word >> (threadIdx.x & 31)) & 1u) == 0u;
}
__device__ __forceinline__ uint32_t mask_word(const FullsmArgs& a, int r, int ct) {
    return (a.indptr && r < a.B) ? a.ws.bits[(size_t)r * a.W + ct] : 0u;
}

template <int D, bool NORM>
__device__ __forceinline__ void stats_body(const FullsmArgs& a) {
    __shared__ __attribute__((aligned(16))) float sU[kT * (D + 4)];
    __shared__ __attribute__((aligned(16))) float sI[kT * (D + 4)];
    const int lane = threadIdx.x, h = lane >> 5;
    const int r0 = blockIdx.x * kT, split = blockIdx.y;
    const int ct0 = split * a.tps, ct1 = min(ct0 + a.tps, a.W);
    load_tile<D>(sU, a.ws.P, r0, a.B);
    float m[16], se[16];
    int pos_r[16];
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int r = r0 + acc_row(reg, h);
        m[reg] = -INFINITY, se[reg] = 0.f;
        pos_r[reg] = r < a.B ? a.ws.vpos[r] : -1;
    }
    TileRegs<D> nxt;
    fetch_tile<D>(nxt, a.I, ct0 * kT, (int)a.n_items, NORM ? a.ws.inv_i : nullptr);
    for (int ct = ct0; ct < ct1; ++ct) {
        const int c0 = ct * kT, c = c0 + (lane & 31);
        __syncthreads();                            // (the previous tile's reads of sI)
        store_tile<D, NORM>(sI, nxt);
        __syncthreads();
        const bool more = ct + 1 < ct1;
        fetch_tile<D>(nxt, a.I, more ? c0 + kT : 0, more ? (int)a.n_items : 0, NORM ? a.ws.inv_i : nullptr);
        const f32x16 dots = tile_dots<D>(sU, sI);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int r = r0 + acc_row(reg, h);
            if (!admitted(pos_r[reg], c, a.n_items, mask_word(a, r, ct))) continue;
            const float s = dots[reg] * a.inv_tau;
            if (c == pos_r[reg]) a.ws.diag[r] = s;
            // one exp per logit: the smaller of (m, s) is the one rescaled.  m == -inf: dlt = +inf, e = 0, se = 1.
            const float dlt = s - m[reg], e = expf(-fabsf(dlt));
            se[reg] = dlt <= 0.f ? se[reg] + e : se[reg] * e + 1.f;
            m[reg] = fmaxf(m[reg], s);
        }
    }
    // the 32 lanes of a half hold the same 16 rows: merge them
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const float m2 = __shfl_xor(m[reg], o, 64), se2 = __shfl_xor(se[reg], o, 64);
            merge_stats(m[reg], se[reg], m2, se2);
        }
        const int r = r0 + acc_row(reg, h);
        if ((lane & 31) == 0 && r < a.B) {
            float* out = a.ws.part + ((size_t)split * a.Bp + r) * 2;
            out[0] = m[reg], out[1] = se[reg];
        }
    }
}
template <int D>
__global__ void __launch_bounds__(64) fullsm_stats_kernel(FullsmArgs a) { stats_body<D, false>(a); }
template <int D>
__global__ void __launch_bounds__(64) fullsm_stats_norm_kernel(FullsmArgs a) { stats_body<D, true>(a); }

// ---- merge: one thread per row, the splits in split order ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) fullsm_merge_kernel(FullsmArgs a) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= a.B) return;
    float m = -INFINITY, se = 0.f;
    for (int s = 0; s < a.splits; ++s) {
        const float* in = a.ws.part + ((size_t)s * a.Bp + r) * 2;
        merge_stats(m, se, in[0], in[1]);
    }
    const bool any = se > 0.f;                      // (a valid row admits its positive at least)
    const float lg = any ? logf(se) : 0.f;
    a.ws.rm[r] = m;
    a.ws.rinv[r] = any ? 1.f / se : 0.f;
    a.ws.rlog[r] = lg;
    if (a.row_stats) {
        a.row_stats[2 * (size_t)r] = any ? m : 0.f;
        a.row_stats[2 * (size_t)r + 1] = lg;
    }
}

// C of the lane's 16 rows of one tile (rows r0 + acc_row(reg, h), column c): sM / sInv / sPos hold m_r, 1 / se_r and vpos of the tile's 32 rows
__device__ __forceinline__ void tile_coeffs(const FullsmArgs& a, const f32x16& dots, int r0, int ct, int c, const float* sM, const float* sInv,
                                            const int* sPos, float cscale, float (&C)[16]) {
    const int h = threadIdx.x >> 5;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int rr = acc_row(reg, h);
        const int pos_r = sPos[rr];
        float cf = 0.f;
        if (admitted(pos_r, c, a.n_items, mask_word(a, r0 + rr, ct))) {
            const float s = dots[reg] * a.inv_tau;
            const float p = expf(s - sM[rr]) * sInv[rr];
            cf = (c == pos_r ? p - 1.f : p) * cscale;
        }
        C[reg] = cf;
    }
}
// the statistics of the 32 rows from r0 on (lanes 0 .. 31): fetched into registers, stored to LDS in front of the caller's barrier; rows at and
// past B are dropped rows
struct RowRegs {
    float m, inv;
    int pos;
};
__device__ __forceinline__ void fetch_row_stats(RowRegs& t, const FullsmArgs& a, int r0) {
    const int r = r0 + (threadIdx.x & 31);
    const bool in = threadIdx.x < kT && r < a.B;
    t.m = in ? a.ws.rm[r] : -INFINITY;
    t.inv = in ? a.ws.rinv[r] : 0.f;
    t.pos = in ? a.ws.vpos[r] : -1;
}
__device__ __forceinline__ void store_row_stats(const RowRegs& t, float* sM, float* sInv, int* sPos) {
    const int lane = threadIdx.x;
    if (lane < kT) sM[lane] = t.m, sInv[lane] = t.inv, sPos[lane] = t.pos;
}

// ---- gradu: workgroup (row tile, column split) -> GU[split] ----------------------------------------------------------------------------------------
template <int D, bool NORM>
__device__ __forceinline__ void gradu_body(const FullsmArgs& a) {
    constexpr int NC = D / 32;                      // 32-wide chunks of the embedding
    __shared__ __attribute__((aligned(16))) float sU[kT * (D + 4)];
    __shared__ __attribute__((aligned(16))) float sI[kT * (D + 4)];
    __shared__ float sC[kT * (kT + 1)];
    __shared__ float sM[kT], sInv[kT];
    __shared__ int sPos[kT];
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * kT, split = blockIdx.y;
    const int ct0 = split * a.tps, ct1 = min(ct0 + a.tps, a.W);
    load_tile<D>(sU, a.ws.P, r0, a.B);
    RowRegs row;
    fetch_row_stats(row, a, r0);
    store_row_stats(row, sM, sInv, sPos);
    const float cscale = a.inv_tau * a.inv_B;
    f32x16 accG[NC];                                // sum_c C_rc i^_c of the split's columns: rows in the registers, 32 floats of d on the lanes
#pragma unroll
    for (int k = 0; k < NC; ++k) accG[k] = f32x16{0.f};
    TileRegs<D> nxt;
    fetch_tile<D>(nxt, a.I, ct0 * kT, (int)a.n_items, NORM ? a.ws.inv_i : nullptr);
    for (int ct = ct0; ct < ct1; ++ct) {
        const int c0 = ct * kT;
        __syncthreads();                            // (the previous tile's reads of sI and sC; the first time: sM, sInv, sPos)
        store_tile<D, NORM>(sI, nxt);
        __syncthreads();
        const bool more = ct + 1 < ct1;
        fetch_tile<D>(nxt, a.I, more ? c0 + kT : 0, more ? (int)a.n_items : 0, NORM ? a.ws.inv_i : nullptr);
        const f32x16 dots = tile_dots<D>(sU, sI);
        float C[16];
        tile_coeffs(a, dots, r0, ct, c0 + i, sM, sInv, sPos, cscale, C);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) sC[acc_row(reg, h) * (kT + 1) + i] = C[reg];
        // C I^ for the row block: it sums over the column (lane) index, so the tile goes through LDS: A[row][k = col] = sC[row][col]
        __syncthreads();
        float ca[16];
#pragma unroll
        for (int s = 0; s < 16; ++s) ca[s] = sC[i * (kT + 1) + 2 * s + h];
#pragma unroll
        for (int k = 0; k < NC; ++k) {
#pragma unroll
            for (int s = 0; s < 16; ++s)
                accG[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(ca[s], sI[(2 * s + h) * (D + 4) + 32 * k + i], accG[k], 0, 0, 0);
        }
    }
    // every (split, row < B) of GU has this one writer: plain stores, nothing to zero
    float* out = a.ws.GU + (size_t)split * a.Bp * D;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int r = r0 + acc_row(reg, h);
            if (r < a.B) out[(size_t)r * D + 32 * k + i] = accG[k][reg];
        }
    }
}
template <int D>
__global__ void __launch_bounds__(64) fullsm_gradu_kernel(FullsmArgs a) { gradu_body<D, false>(a); }
template <int D>
__global__ void __launch_bounds__(64) fullsm_gradu_norm_kernel(FullsmArgs a) { gradu_body<D, true>(a); }

// ---- gradi: the workgroup owns column tile blockIdx.x ---------------------------------------------------------------------------------------------------
template <int D, bool NORM>
__device__ __forceinline__ void gradi_body(const FullsmArgs& a) {
    constexpr int NC = D / 32;
    __shared__ __attribute__((aligned(16))) float sU[kT * (D + 4)];
    __shared__ __attribute__((aligned(16))) float sI[kT * (D + 4)];
    __shared__ float sM[kT], sInv[kT];
    __shared__ int sPos[kT];
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int ct = blockIdx.x, c0 = ct * kT, c = c0 + i;
    TileRegs<D> nxt;
    fetch_tile<D>(nxt, a.I, c0, (int)a.n_items, NORM ? a.ws.inv_i : nullptr);
    store_tile<D, NORM>(sI, nxt);
    RowRegs nrow;
    fetch_tile<D>(nxt, a.ws.P, 0, a.B, nullptr);
    fetch_row_stats(nrow, a, 0);
    const float cscale = a.inv_tau * a.inv_B;
    f32x16 accH[NC];                                // sum_r C_rc u^_r over the whole batch: the tile's columns in the registers, 32 floats of d on the lanes
#pragma unroll
    for (int k = 0; k < NC; ++k) accH[k] = f32x16{0.f};
    int n_own = 0;                                  // valid rows whose positive is this lane's column, among the lane's 16 rows of every row tile
    for (int r0 = 0; r0 < a.Bp; r0 += kT) {         // ascending row tiles: the order of the sum is fixed
        __syncthreads();                            // (the previous tile's reads of sU, sM, sInv, sPos)
        store_tile<D, false>(sU, nxt);
        store_row_stats(nrow, sM, sInv, sPos);
        __syncthreads();
        fetch_tile<D>(nxt, a.ws.P, r0 + kT, r0 + kT < a.Bp ? a.B : 0, nullptr);
        fetch_row_stats(nrow, a, r0 + kT);
        const f32x16 dots = tile_dots<D>(sU, sI);
        float C[16];
        tile_coeffs(a, dots, r0, ct, c, sM, sInv, sPos, cscale, C);
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) n_own += (sPos[acc_row(reg, h)] == c) ? 1 : 0;
        // C^T U^: it sums over the tile's ROW index -- the accumulator registers themselves are the A operand (A[col][k = row]), the B operand is
        // row acc_row(reg, h) of sU.  One chunk of 32 floats of d per accumulator.
#pragma unroll
        for (int k = 0; k < NC; ++k) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                accH[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(C[reg], sU[acc_row(reg, h) * (D + 4) + 32 * k + i], accH[k], 0, 0, 0);
        }
    }
    n_own += __shfl_xor(n_own, 32, 64);             // both halves: all 32 rows of every tile; lane (i, .) holds n_c of column c0 + i
    // the epilogue: register reg of lane (i, h) is column cc = c0 + acc_row(reg, h), floats 32 k + i of its row
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int cl = acc_row(reg, h), cc = c0 + cl;
        const int n_c = __shfl(n_own, cl, 64);      // (every lane takes part)
        float pi = 0.f;
        if constexpr (NORM) {
#pragma unroll
            for (int k = 0; k < NC; ++k) pi += accH[k][reg] * sI[cl * (D + 4) + 32 * k + i];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) pi += __shfl_xor(pi, o, 64);           // i^_c . h_c: over the 32 lanes of the half
        }
        if ((unsigned)cc >= a.n_items) continue;    // (behind the shuffles)
        const float inv = NORM ? a.ws.inv_i[cc] : 1.f;
        const float reg_n = a.reg_c * (float)n_c;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const size_t at = (size_t)cc * D + 32 * k + i;
            float g = accH[k][reg];
            if constexpr (NORM) g = inv * (g - pi * sI[cl * (D + 4) + 32 * k + i]);
            if (n_c > 0) g += reg_n * a.I[at];
            a.gI[at] += g;                          // the column's only writer
        }
        if (i == 0) a.tagI[cc] = a.tag;
    }
}
template <int D>
__global__ void __launch_bounds__(64) fullsm_gradi_kernel(FullsmArgs a) { gradi_body<D, false>(a); }
template <int D>
__global__ void __launch_bounds__(64) fullsm_gradi_norm_kernel(FullsmArgs a) { gradi_body<D, true>(a); }

// ---- the tail: d / 4 lanes per row, the layout of the other step kernels ----------------------------------------------------------------------------
template <int D, bool NORM>
__device__ __forceinline__ void tail_body(const FullsmArgs& a) {
    constexpr int L = D / 4, TPB = 512 / L;
    __shared__ float red[2][8];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;
    float maxi = 0.f, sq = 0.f;
    int p = -1;
    if (t < a.B) p = a.ws.vpos[t];
    if (p >= 0) {
        const int u = a.users[t];
        const f32x4 uq = *reinterpret_cast<const f32x4*>(a.ws.P + (size_t)t * D + 4 * e);
        const f32x4 iq = *reinterpret_cast<const f32x4*>(a.I + (size_t)p * D + 4 * e);
        f32x4 gq = {0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s < a.splits; ++s)          // split order
            gq += *reinterpret_cast<const f32x4*>(a.ws.GU + ((size_t)s * a.Bp + t) * D + 4 * e);
        const float sq_i = group_sum<D>(dot4(iq, iq));
        f32x4 due;
        if constexpr (NORM) {
            // the image holds u^ = u inv: the raw row is u^ max(|u|, 1e-12) to a rounding
            const float inv_u = a.ws.inv_u[t], nu = fmaxf(sqrtf(a.ws.sq_u[t]), kNormFloor);
            const float pu = group_sum<D>(dot4(uq, gq));
            due = inv_u * (gq - pu * uq) + (a.reg_c * nu) * uq;
        } else {
            due = gq + a.reg_c * uq;
        }
        if (e == 0) {
            maxi = -((a.ws.rm[t] - a.ws.diag[t]) + a.ws.rlog[t]);               // block_loss_terms takes -sum(maxi) / B
            sq = a.ws.sq_u[t] + sq_i;
            a.tagU[u] = a.tag;                                                  // same value from every writer of a row: plain stores
        }
        // (the dense-gradient writes of a tagged step: pda_train_common.h has the precondition of the plain store)
        if (a.users_distinct) *reinterpret_cast<f32x4*>(a.gU + (size_t)u * D + 4 * e) = due;
        else atomic_add4(a.gU + (size_t)u * D + 4 * e, due);
    }
    block_loss_reduce(maxi, sq, red);
    if (tid == 0) block_loss_terms(red, a.inv_B, a.reg_c, a.ws.lossp[2 * blockIdx.x], a.ws.lossp[2 * blockIdx.x + 1]);       // (mf, reg) of the block
}
template <int D>
__global__ void __launch_bounds__(512) fullsm_tail_kernel(FullsmArgs a) { tail_body<D, false>(a); }
template <int D>
__global__ void __launch_bounds__(512) fullsm_tail_norm_kernel(FullsmArgs a) { tail_body<D, true>(a); }

// ---- loss: one wave, the tail's blocks in a fixed order (lane l takes blocks l, l + 64, ..., then the ladder of block_loss_reduce) ----------------------
__global__ void __launch_bounds__(64) fullsm_loss_kernel(FullsmArgs a) {
    float mf = 0.f, rg = 0.f;
    for (int b = threadIdx.x; b < a.n_tail; b += 64) mf += a.ws.lossp[2 * b], rg += a.ws.lossp[2 * b + 1];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mf += __shfl_xor(mf, o, 64);
        rg += __shfl_xor(rg, o, 64);
    }
    if (threadIdx.x == 0) {
        a.loss_acc[0] += mf + rg;
        a.loss_acc[1] += mf;
        a.loss_acc[2] += rg;
    }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------
int check_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float tau,
               int norm, const int64_t* indptr, const int32_t* indices, float reg_div, const float* gU, const float* gI, const int32_t* tagU,
               const int32_t* tagI, int step_tag, int flags, const void* ws, size_t ws_bytes) {
    if (!U || !I || !users || !pos || !gU || !gI || !tagU || !tagI || !ws) return PDA_ERR_ARG;
    if ((indptr == nullptr) != (indices == nullptr)) return PDA_ERR_ARG;
    if (B < 1 || B > PDA_FULLSM_MAX_B || !(reg_div > 0.f) || step_tag <= 0 || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (!(tau > 0.f) || !std::isfinite(tau) || (norm != 0 && norm != 1)) return PDA_ERR_ARG;
    if (flags & ~(PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT)) return PDA_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) & 15u) != 0) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (ws_bytes < pda_fullsm_workspace_bytes(B, n_items, d)) return PDA_ERR_ARG;
    return PDA_OK;
}

#define FULLSM_TILE_LAUNCH(KERNEL, W, GRID, STREAM, ARGS)                                       \
    switch (W) {                                                                                \
        case 32: hipLaunchKernelGGL(KERNEL<32>, GRID, dim3(64), 0, STREAM, ARGS); break;        \
        case 64: hipLaunchKernelGGL(KERNEL<64>, GRID, dim3(64), 0, STREAM, ARGS); break;        \
        case 128: hipLaunchKernelGGL(KERNEL<128>, GRID, dim3(64), 0, STREAM, ARGS); break;      \
        default: hipLaunchKernelGGL(KERNEL<256>, GRID, dim3(64), 0, STREAM, ARGS); break;       \
    }
#define FULLSM_LAUNCH2(PLAIN, NORMED, MACRO, ...)   \
    if (norm) {                                     \
        MACRO(NORMED, __VA_ARGS__)                  \
    } else {                                        \
        MACRO(PLAIN, __VA_ARGS__)                   \
    }                                               \
    PDA_CHECK_LAUNCH();

// (arguments checked by the callers)
int launch_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float tau,
                int norm, const int64_t* indptr, const int32_t* indices, float regs, float reg_div, float* gU, float* gI, int32_t* tagU,
                int32_t* tagI, int step_tag, int flags, void* ws, float* loss_acc, float* row_stats, hipStream_t s) {
    FullsmArgs a{U, I, users, pos, indptr, indices, gU, gI, tagU, tagI, loss_acc, row_stats, carve(ws, B, n_items, d), (unsigned)n_users,
                 (unsigned)n_items, step_tag, B, tiles_of((size_t)B) * kT, tiles_of(n_items), tiles_per_split(n_items, B), col_splits(n_items, B),
                 tail_blocks(B, d), 1.0f / (float)B, 1.0f / tau, regs / reg_div, (flags & PDA_UPD_USERS_DISTINCT) ? 1 : 0};
    const dim3 tiles((unsigned)tiles_of((size_t)B), (unsigned)a.splits), owners((unsigned)a.W);
    FULLSM_LAUNCH2(fullsm_pack_kernel, fullsm_pack_norm_kernel, PDA_STEP_LAUNCH, d, B, s, a)
    if (norm) {
        PDA_STEP_LAUNCH(fullsm_inv_kernel, d, n_items, s, a)
        PDA_CHECK_LAUNCH();
    }
    if (indptr) {
        hipLaunchKernelGGL(fullsm_bits_kernel, dim3((unsigned)((a.W + 255) / 256), (unsigned)B), dim3(256), 0, s, a);
        PDA_CHECK_LAUNCH();
    }
    FULLSM_LAUNCH2(fullsm_stats_kernel, fullsm_stats_norm_kernel, FULLSM_TILE_LAUNCH, d, tiles, s, a)
    hipLaunchKernelGGL(fullsm_merge_kernel, dim3((unsigned)((B + 255) / 256)), dim3(256), 0, s, a);
    PDA_CHECK_LAUNCH();
    FULLSM_LAUNCH2(fullsm_gradu_kernel, fullsm_gradu_norm_kernel, FULLSM_TILE_LAUNCH, d, tiles, s, a)
    FULLSM_LAUNCH2(fullsm_gradi_kernel, fullsm_gradi_norm_kernel, FULLSM_TILE_LAUNCH, d, owners, s, a)
    FULLSM_LAUNCH2(fullsm_tail_kernel, fullsm_tail_norm_kernel, PDA_STEP_LAUNCH, d, B, s, a)
    if (loss_acc) {
        hipLaunchKernelGGL(fullsm_loss_kernel, dim3(1), dim3(64), 0, s, a);
        PDA_CHECK_LAUNCH();
    }
    return PDA_OK;
}

}  // namespace

extern "C" int pda_fullsm_col_splits(size_t n_items, int B) { return sizes_ok(B, n_items) ? col_splits(n_items, B) : 0; }

extern "C" size_t pda_fullsm_workspace_bytes(int B, size_t n_items, int d) {
    if (!sizes_ok(B, n_items) || !pda_d_ok(d)) return 0;
    return carve(nullptr, B, n_items, d).bytes;
}

extern "C" int pda_fullsm_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B,
                                   int d, float tau, int norm, const int64_t* train_indptr, const int32_t* train_indices, float regs, float reg_div,
                                   float* gU, float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags, void* ws, size_t ws_bytes,
                                   float* loss_acc, float* row_stats, void* stream) {
    const int rc = check_step(U, I, n_users, n_items, users, pos, B, d, tau, norm, train_indptr, train_indices, reg_div, gU, gI, tagU, tagI, step_tag,
                              flags, ws, ws_bytes);
    if (rc != PDA_OK) return rc;
    return launch_step(U, I, n_users, n_items, users, pos, B, d, tau, norm, train_indptr, train_indices, regs, reg_div, gU, gI, tagU, tagI, step_tag,
                       flags, ws, loss_acc, row_stats, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_fullsm_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                        float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float tau,
                                        int norm, const int64_t* train_indptr, const int32_t* train_indices, float regs, float reg_div, int step_tag,
                                        float lr_t, float beta1, float beta2, float eps, int flags, int cache_policy, void* ws, size_t ws_bytes,
                                        float* loss_acc, float* row_stats, void* stream) {
    if (!mU || !vU || !mI || !vI) return PDA_ERR_ARG;
    if (cache_policy < PDA_ADAM_CACHE_AUTO || cache_policy > PDA_ADAM_CACHE_STREAM) return PDA_ERR_ARG;
    int rc = check_step(U, I, n_users, n_items, users, pos, B, d, tau, norm, train_indptr, train_indices, reg_div, gU, gI, tagU, tagI, step_tag, flags,
                        ws, ws_bytes);
    if (rc != PDA_OK) return rc;
    rc = launch_step(U, I, n_users, n_items, users, pos, B, d, tau, norm, train_indptr, train_indices, regs, reg_div, gU, gI, tagU, tagI, step_tag,
                     flags, ws, loss_acc, row_stats, reinterpret_cast<hipStream_t>(stream));
    if (rc != PDA_OK) return rc;
    return pda_adam_dense_sweep4_f32(U, mU, vU, gU, n_users, tagU, I, mI, vI, gI, n_items, tagI, d, step_tag, lr_t, beta1, beta2, eps, cache_policy,
                                     stream);
}
