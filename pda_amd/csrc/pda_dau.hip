// The DirectAU loss (include/pda_hip_dau.h) on MI355X (gfx950): alignment of a user with its positive, and uniformity of the batch's
// user rows and of its item rows on the unit sphere.  The two [B, B] Gram matrices U^ U^T and I^ I^T exist only as 32 x 32 tiles in the
// accumulators of v_mfma_f32_32x32x2_f32 (exact f32).
//
// Four launches:
//   pack    d / 4 lanes per row: u^_r and i^_r gathered and normalised once into an image in the workspace, with 1 / max(|x|, 1e-12), |x|^2, |x^|^2,
//           the validated ids and the row's alignment term |u^_r - i^_r|^2 beside it.
//   tiles   workgroup (row tile, column split, side) = ONE wave.  It OWNS 32 rows a and walks the column tiles b of its split.  The exponent is
//           never positive, so there is no running maximum, no rescale and no second pass: r_a, n_a and G_a = sum_b e_ab x^_b are accumulated
//           directly.  The tile is taken TRANSPOSED (the walked rows b on the accumulator's row index, the owned rows a on the lanes): e_ab is
//           symmetric, and G_a then sums over the accumulator's row index, which sits in the registers -- the E X product needs no trip through
//           LDS.  The next column tile is fetched into registers under the arithmetic of the current one (a workgroup is the only wave of its
//           SIMD: nothing else hides the latency of the loads).  Each (side, split, row) has one writer: plain stores, no float atomics; the
//           workgroup also leaves the sum of its 32 r_a and n_a (a wave ladder: a fixed order), which is all S and P need.
//   reduce  ONE workgroup: S (float64) and P (int64) from the workgroups' partial sums, the alignment sum and the squared norms, in a fixed
//           order (thread-strided, wave ladder, waves in order); uni_U, uni_I, the two coefficients (gamma / 2)(-2 t / S) for the tail, loss_acc
//           and stat.
//   tail    d / 4 lanes per row: r and G of the row added in split order, the coefficient, the projection of the normalisation, c_reg x, the
//           scatter to gU / gI through the shared pieces of pda_train_common.h (the tail of pda_inbatch.hip), the tags.
#include <cmath>
#include <cstdlib>
#include "pda_common.h"
#include "pda_train_common.h"
#include "pda_softmax_tiles.h"
#include "pda_hip_dau.h"

namespace {

constexpr int kTargetGroups = 1024;     // workgroups of one wave the tile pass aims at over both sides: one per SIMD of the chip
static_assert(PDA_DAU_TILE == kT, "the tile pass is written for 32 x 32 tiles");

// ---- the workspace ------------------------------------------------------------------------------------------------------------------------------
struct Ws {
    float* P;           // [2 Bp, d]: rows [0, B) u^, rows [Bp, Bp + B) i^ (zero for a dropped row)
    float* G;           // [2, splits, Bp, d]   sum_b e_ab x^_b over the split's columns
    float* r;           // [2, splits, Bp]      sum_b e_ab
    float* wr;          // [2, splits, Bp / 32] sum of r over the 32 rows of a workgroup
    int32_t* wn;        // [2, splits, Bp / 32] sum of n_a = #{b : adm(a, b)} over the 32 rows of a workgroup
    float* inv;         // [2 Bp]    1 / max(|x|, 1e-12)
    float* sq;          // [2 Bp]    |x|^2
    float* nsq;         // [2 Bp]    |x^|^2 (1 to a rounding; 0 for a zero row)
    int32_t* vid;       // [2 Bp]    users[r] / pos[r], -1 for a dropped row
    float* al;          // [Bp]      |u^_r - i^_r|^2
    float* coef;        // [4]       (gamma / 2)(-2 t / S) per side, 0 if P = 0
    size_t bytes;
};

inline int tiles_of(int B) { return (B + kT - 1) / kT; }
// column tiles per split, and the number of splits that leaves
inline int tiles_per_split(int B) {
    const int nt = tiles_of(B);
    int want = (kTargetGroups / 2 + nt - 1) / nt;   // splits that would give kTargetGroups workgroups over the two sides
    if (want > nt) want = nt;
    return (nt + want - 1) / want;
}
inline int col_splits(int B) {
    const int nt = tiles_of(B), tps = tiles_per_split(B);
    return (nt + tps - 1) / tps;
}

Ws carve(void* base, int B, int d) {
    const size_t Bp = (size_t)tiles_of(B) * kT, S = (size_t)col_splits(B);
    char* p = reinterpret_cast<char*>(base);
    Ws w;
    size_t off = 0;
    auto take = [&](size_t n_words) {
        char* at = p + off;
        off += ((n_words * 4 + 15) / 16) * 16;
        return at;
    };
    w.P = reinterpret_cast<float*>(take(2 * Bp * d));
    w.G = reinterpret_cast<float*>(take(2 * S * Bp * d));
    w.r = reinterpret_cast<float*>(take(2 * S * Bp));
    w.wr = reinterpret_cast<float*>(take(2 * S * (Bp / kT)));
    w.wn = reinterpret_cast<int32_t*>(take(2 * S * (Bp / kT)));
    w.inv = reinterpret_cast<float*>(take(2 * Bp));
    w.sq = reinterpret_cast<float*>(take(2 * Bp));
    w.nsq = reinterpret_cast<float*>(take(2 * Bp));
    w.vid = reinterpret_cast<int32_t*>(take(2 * Bp));
    w.al = reinterpret_cast<float*>(take(Bp));
    w.coef = reinterpret_cast<float*>(take(4));
    w.bytes = off;
    return w;
}

struct DauArgs {
    const float* U;
    const float* I;
    const int32_t* users;
    const int32_t* pos;
    float* gU;
    float* gI;
    int32_t* tagU;
    int32_t* tagI;
    float* stat;
    float* loss_acc;
    Ws ws;
    unsigned n_users, n_items;
    int tag;
    int B, Bp;
    int tps, splits;        // column tiles per split, splits
    float t, gamma, inv_B, reg_c;
    int drop_same, any_order, users_distinct;
};

// ---- pack: d / 4 lanes per row r, both of its rows ------------------------------------------------------------------------------------------------
template <int D>
__global__ void __launch_bounds__(512) dau_pack_kernel(DauArgs a) {
    constexpr int L = D / 4, TPB = 512 / L;
    const int g = threadIdx.x / L, e = threadIdx.x % L;
    const int r = blockIdx.x * TPB + g;
    if (r >= a.B) return;                           // (whole lane groups leave)
    const int u = a.users[r], p = a.pos[r];
    const bool ok = (unsigned)u < a.n_users && (unsigned)p < a.n_items;
    f32x4 x = {0.f, 0.f, 0.f, 0.f}, y = {0.f, 0.f, 0.f, 0.f};
    if (ok) {
        x = *reinterpret_cast<const f32x4*>(a.U + (size_t)u * D + 4 * e);
        y = *reinterpret_cast<const f32x4*>(a.I + (size_t)p * D + 4 * e);
    }
    const float squ = group_sum<D>(dot4(x, x)), sqi = group_sum<D>(dot4(y, y));
    const float invu = 1.f / fmaxf(sqrtf(squ), kNormFloor), invi = 1.f / fmaxf(sqrtf(sqi), kNormFloor);
    x = x * invu;
    y = y * invi;
    const float nsqu = group_sum<D>(dot4(x, x)), nsqi = group_sum<D>(dot4(y, y));
    const f32x4 df = x - y;
    const float al = group_sum<D>(dot4(df, df));
    const size_t ru = (size_t)r, ri = (size_t)a.Bp + r;
    *reinterpret_cast<f32x4*>(a.ws.P + ru * D + 4 * e) = x;
    *reinterpret_cast<f32x4*>(a.ws.P + ri * D + 4 * e) = y;
    if (e == 0) {
        a.ws.inv[ru] = invu, a.ws.inv[ri] = invi;
        a.ws.sq[ru] = squ, a.ws.sq[ri] = sqi;
        a.ws.nsq[ru] = nsqu, a.ws.nsq[ri] = nsqi;
        a.ws.vid[ru] = ok ? u : -1, a.ws.vid[ri] = ok ? p : -1;
        a.ws.al[r] = al;
    }
}

// ---- the pass over the Gram tiles (the tile itself: pda_softmax_tiles.h) ------------------------------------------------------------------------------
// load_tile in two halves: the 32 rows into registers (D / 8 float4 per lane), and from there into the LDS image
template <int D>
__device__ __forceinline__ void fetch_tile(f32x4 (&v)[D / 8], const float* P, int row0, int rows_end) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int j = 0; j < D / 8; ++j) {
        const int idx = threadIdx.x + 64 * j, row = idx / Q, q = idx % Q;
        v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (row0 + row < rows_end) v[j] = *reinterpret_cast<const f32x4*>(P + (size_t)(row0 + row) * D + 4 * q);
    }
}
template <int D>
__device__ __forceinline__ void store_tile(float* s, const f32x4 (&v)[D / 8]) {
    constexpr int Q = D / 4;
#pragma unroll
    for (int j = 0; j < D / 8; ++j) {
        const int idx = threadIdx.x + 64 * j, row = idx / Q, q = idx % Q;
        *reinterpret_cast<f32x4*>(s + row * (D + 4) + 4 * q) = v[j];
    }
}

template <int D>
__global__ void __launch_bounds__(64) dau_tiles_kernel(DauArgs a) {
    constexpr int NC = D / 32;                      // 32-wide chunks of the embedding
    __shared__ __attribute__((aligned(16))) float sOwn[kT * (D + 4)];
    __shared__ __attribute__((aligned(16))) float sWalk[kT * (D + 4)];
    __shared__ int sId[kT];
    __shared__ float sNsq[kT];
    const int lane = threadIdx.x, i = lane & 31, h = lane >> 5;
    const int r0 = blockIdx.x * kT, split = blockIdx.y, side = blockIdx.z;
    const int ct0 = split * a.tps, ct1 = min(ct0 + a.tps, a.Bp / kT);
    const float* P = a.ws.P + (size_t)side * a.Bp * D;
    const int32_t* vid = a.ws.vid + (size_t)side * a.Bp;
    const float* nsq = a.ws.nsq + (size_t)side * a.Bp;
    load_tile<D>(sOwn, P, r0, a.B);
    // the owned row of this lane: a = r0 + (lane & 31), on both halves of the wave
    const int ra = r0 + i;
    const int id_a = ra < a.B ? vid[ra] : -1;
    const float nsq_a = ra < a.B ? nsq[ra] : 0.f;
    float rsum = 0.f;
    int ncnt = 0;
    f32x16 accG[NC];                                // G of the owned rows: rows on the accumulator's row index, 32 floats of d on the lanes
#pragma unroll
    for (int k = 0; k < NC; ++k) accG[k] = f32x16{0.f};
    // the walked tile, its ids and |x^|^2, one tile ahead in registers
    f32x4 pre[D / 8];
    int pre_id = -1;
    float pre_nsq = 0.f;
    auto fetch = [&](int c0) {
        fetch_tile<D>(pre, P, c0, a.B);
        const int c = c0 + i;
        pre_id = c < a.B ? vid[c] : -1;
        pre_nsq = c < a.B ? nsq[c] : 0.f;
    };
    fetch(ct0 * kT);
    for (int ct = ct0; ct < ct1; ++ct) {
        const int c0 = ct * kT;
        __syncthreads();                            // (the previous tile's reads of sWalk, sId, sNsq)
        store_tile<D>(sWalk, pre);
        if (lane < kT) {
            sId[lane] = pre_id;
            sNsq[lane] = pre_nsq;
        }
        __syncthreads();
        if (ct + 1 < ct1) fetch(c0 + kT);           // (in flight under this tile's arithmetic)
        // dots[reg] = x^_b . x^_a, b = c0 + acc_row(reg, h) the walked row, a the lane's owned row: the transposed tile
        const f32x16 dots = tile_dots<D>(sWalk, sOwn);
        float E[16];
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int rr = acc_row(reg, h), rb = c0 + rr;
            const int id_b = sId[rr];
            float ev = 0.f;
            if (id_a >= 0 && id_b >= 0 && rb != ra && !(a.drop_same && id_b == id_a)) {
                // the same id is the same table row: distance 0, not what the rounded products leave of it
                const float dist = id_b == id_a ? 0.f : fmaxf(nsq_a + sNsq[rr] - 2.f * dots[reg], 0.f);
                ev = expf(-a.t * dist);
                rsum += ev;
                ncnt += 1;
            }
            E[reg] = ev;
        }
        // G_a += sum_b e_ab x^_b: the sum runs over the accumulator's row index -- the registers themselves are the A operand (A[a][k = b]), the B
        // operand is row acc_row(reg, h) of the walked tile.  One chunk of 32 floats of d per accumulator.
#pragma unroll
        for (int k = 0; k < NC; ++k) {
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                accG[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(E[reg], sWalk[acc_row(reg, h) * (D + 4) + 32 * k + i], accG[k], 0, 0, 0);
        }
    }
    // the two halves of the wave hold the two halves of the walked rows of the same owned row
    rsum += __shfl_xor(rsum, 32, 64);
    ncnt += __shfl_xor(ncnt, 32, 64);
    const size_t slice = ((size_t)side * a.splits + split) * a.Bp;
    if (h == 0 && ra < a.B) a.ws.r[slice + ra] = rsum;
    // the workgroup's share of S and P (a row past B or a dropped row holds 0)
#pragma unroll
    for (int o = 16; o > 0; o >>= 1) {
        rsum += __shfl_xor(rsum, o, 64);
        ncnt += __shfl_xor(ncnt, o, 64);
    }
    if (lane == 0) {
        const size_t wg = ((size_t)side * a.splits + split) * (a.Bp / kT) + blockIdx.x;
        a.ws.wr[wg] = rsum;
        a.ws.wn[wg] = ncnt;
    }
#pragma unroll
    for (int k = 0; k < NC; ++k) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int r = r0 + acc_row(reg, h);
            if (r < a.B) a.ws.G[(slice + r) * D + 32 * k + i] = accG[k][reg];
        }
    }
}

// ---- the reduction: ONE workgroup, a fixed order -------------------------------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ long long wave_sum(long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
// r of (side, row) over the splits, in split order: the tail takes the same bits
__device__ __forceinline__ float row_r(const DauArgs& a, int side, int row) {
    float r = 0.f;
    for (int s = 0; s < a.splits; ++s) r += a.ws.r[((size_t)side * a.splits + s) * a.Bp + row];
    return r;
}

__global__ void __launch_bounds__(1024) dau_reduce_kernel(DauArgs a) {
    __shared__ double sD[4][16];
    __shared__ long long sN[2][16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double S[2] = {0.0, 0.0}, al = 0.0, sq = 0.0;
    long long N[2] = {0, 0};
    const int n_wg = a.splits * (a.Bp / kT);        // workgroups of the tile pass per side
    for (int wg = tid; wg < n_wg; wg += 1024) {
        S[0] += (double)a.ws.wr[wg], S[1] += (double)a.ws.wr[n_wg + wg];
        N[0] += a.ws.wn[wg], N[1] += a.ws.wn[n_wg + wg];
    }
    for (int row = tid; row < a.B; row += 1024) {   // (a dropped row holds zeros)
        al += (double)a.ws.al[row];
        sq += (double)a.ws.sq[row] + (double)a.ws.sq[a.Bp + row];
    }
    S[0] = wave_sum(S[0]), S[1] = wave_sum(S[1]), al = wave_sum(al), sq = wave_sum(sq);
    N[0] = wave_sum(N[0]), N[1] = wave_sum(N[1]);
    if (lane == 0) {
        sD[0][wave] = S[0], sD[1][wave] = S[1], sD[2][wave] = al, sD[3][wave] = sq;
        sN[0][wave] = N[0], sN[1][wave] = N[1];
    }
    __syncthreads();
    if (tid != 0) return;
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    long long cnt[2] = {0, 0};
    for (int w = 0; w < 16; ++w) {
#pragma unroll
        for (int k = 0; k < 4; ++k) tot[k] += sD[k][w];
        cnt[0] += sN[0][w], cnt[1] += sN[1][w];
    }
    float uni[2];
    for (int side = 0; side < 2; ++side) {
        const double Sx = 0.5 * tot[side], Px = 0.5 * (double)cnt[side];
        const bool any = cnt[side] > 0 && Sx > 0.0;
        uni[side] = any ? (float)log(Sx / Px) : 0.f;
        a.ws.coef[side] = any ? (float)(-(double)a.gamma * (double)a.t / Sx) : 0.f;      // (gamma / 2)(-2 t / S)
    }
    const float align = (float)(tot[2] * (double)a.inv_B);
    const float mf = (float)((double)align + 0.5 * (double)a.gamma * ((double)uni[0] + (double)uni[1]));
    const float rg = (float)((double)a.reg_c * 0.5 * tot[3]);
    if (a.loss_acc) {                               // (one writer per call: plain read-modify-write)
        a.loss_acc[0] += mf + rg;
        a.loss_acc[1] += mf;
        a.loss_acc[2] += rg;
    }
    if (a.stat) {
        a.stat[0] += align;
        a.stat[1] += uni[0];
        a.stat[2] += uni[1];
        a.stat[3] += 1.f;
    }
}

// ---- the tail: d / 4 lanes per row, the layout of the other step kernels ----------------------------------------------------------------------------
// g = c_al (x^ - y^) + coef (r x^ - G): the gradient on the unit row x^ of `side`, y^ the row's other side
template <int D>
__device__ __forceinline__ f32x4 unit_grad(const DauArgs& a, int side, int row, int e, f32x4 xq, f32x4 yq, float c_al) {
    // G of the row over the splits, in split order; four loads in flight at a time (64 workgroups of the tail are all that hide their latency)
    f32x4 G = {0.f, 0.f, 0.f, 0.f};
    const float* g0 = a.ws.G + ((size_t)side * a.splits * a.Bp + row) * D + 4 * e;
    const size_t stride = (size_t)a.Bp * D;
    int s = 0;
    for (; s + 4 <= a.splits; s += 4) {
        const f32x4 v0 = *reinterpret_cast<const f32x4*>(g0 + (s + 0) * stride), v1 = *reinterpret_cast<const f32x4*>(g0 + (s + 1) * stride);
        const f32x4 v2 = *reinterpret_cast<const f32x4*>(g0 + (s + 2) * stride), v3 = *reinterpret_cast<const f32x4*>(g0 + (s + 3) * stride);
        G += v0;
        G += v1;
        G += v2;
        G += v3;
    }
    for (; s < a.splits; ++s) G += *reinterpret_cast<const f32x4*>(g0 + s * stride);
    const float r = row_r(a, side, row), coef = a.ws.coef[side];
    return c_al * (xq - yq) + coef * (r * xq - G);
}

template <int D>
__global__ void __launch_bounds__(512) dau_tail_kernel(DauArgs a) {
    constexpr int L = D / 4, TPB = 512 / L;
    __shared__ int s_pos[TPB];
    __shared__ __attribute__((aligned(16))) float s_dpe[TPB * D];
    const int tid = threadIdx.x, g = tid / L, e = tid % L;
    const int t = blockIdx.x * TPB + g;
    int p = -1;
    if (t < a.B) p = a.ws.vid[a.Bp + t];
    const bool active = p >= 0;
    float* ptarget = nullptr;
    if (active) {
        const int u = a.ws.vid[t];
        const f32x4 uq = *reinterpret_cast<const f32x4*>(a.ws.P + (size_t)t * D + 4 * e);
        const f32x4 iq = *reinterpret_cast<const f32x4*>(a.ws.P + (size_t)(a.Bp + t) * D + 4 * e);
        const float c_al = 2.f * a.inv_B;
        const f32x4 gq = unit_grad<D>(a, 0, t, e, uq, iq, c_al);
        const f32x4 hq = unit_grad<D>(a, 1, t, e, iq, uq, c_al);
        // the image holds x^ = x inv: the raw row is x^ max(|x|, 1e-12) to a rounding
        const float inv_u = a.ws.inv[t], inv_i = a.ws.inv[a.Bp + t];
        const float nu = fmaxf(sqrtf(a.ws.sq[t]), kNormFloor), ni = fmaxf(sqrtf(a.ws.sq[a.Bp + t]), kNormFloor);
        const float pu = group_sum<D>(dot4(uq, gq)), pi = group_sum<D>(dot4(iq, hq));
        const f32x4 due = inv_u * (gq - pu * uq) + (a.reg_c * nu) * uq;
        const f32x4 die = inv_i * (hq - pi * iq) + (a.reg_c * ni) * iq;
        if (e == 0) {
            a.tagU[u] = a.tag;                                  // same value from every writer of a row: plain stores
            a.tagI[p] = a.tag;
        }
        // (the dense-gradient writes of a tagged step: pda_train_common.h has the precondition of the plain store)
        if (a.users_distinct) *reinterpret_cast<f32x4*>(a.gU + (size_t)u * D + 4 * e) = due;
        else atomic_add4(a.gU + (size_t)u * D + 4 * e, due);
        *reinterpret_cast<f32x4*>(s_dpe + g * D + 4 * e) = die;
        ptarget = a.gI + (size_t)p * D + 4 * e;
    }
    if (e == 0) s_pos[g] = p;
    __syncthreads();
    if (active && a.any_order) pos_scatter_any<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);
    else if (active && pos_run_head(s_pos, g, p)) pos_scatter_run<D, TPB>(s_pos, s_dpe, g, e, p, ptarget);     // (grouped batch)
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------
int check_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float t,
               float gamma, int same, float reg_div, const float* gU, const float* gI, const int32_t* tagU, const int32_t* tagI, int step_tag,
               int flags, const void* ws, size_t ws_bytes) {
    if (!U || !I || !users || !pos || !gU || !gI || !tagU || !tagI || !ws) return PDA_ERR_ARG;
    if (B < 1 || B > PDA_DAU_MAX_B || !(reg_div > 0.f) || step_tag <= 0 || !pda_tables_ok(n_users, n_items)) return PDA_ERR_ARG;
    if (!(t > 0.f) || !(t <= PDA_DAU_MAX_T) || !(gamma >= 0.f) || !std::isfinite(gamma)) return PDA_ERR_ARG;
    if (same != PDA_DAU_SAME_KEEP && same != PDA_DAU_SAME_DROP) return PDA_ERR_ARG;
    if (flags & ~(PDA_UPD_ANY_ORDER | PDA_UPD_USERS_DISTINCT)) return PDA_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(ws) & 15u) != 0) return PDA_ERR_ARG;
    if (!pda_d_ok(d)) return PDA_ERR_UNSUPPORTED;
    if (ws_bytes < pda_dau_workspace_bytes(B, d)) return PDA_ERR_ARG;
    return PDA_OK;
}

#define DAU_TILE_LAUNCH(KERNEL, W, GRID, STREAM, ARGS)                                          \
    switch (W) {                                                                                \
        case 32: hipLaunchKernelGGL(KERNEL<32>, GRID, dim3(64), 0, STREAM, ARGS); break;        \
        case 64: hipLaunchKernelGGL(KERNEL<64>, GRID, dim3(64), 0, STREAM, ARGS); break;        \
        case 128: hipLaunchKernelGGL(KERNEL<128>, GRID, dim3(64), 0, STREAM, ARGS); break;      \
        default: hipLaunchKernelGGL(KERNEL<256>, GRID, dim3(64), 0, STREAM, ARGS); break;       \
    }

// (arguments checked by the callers)
int launch_step(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float t,
                float gamma, int same, float regs, float reg_div, float* gU, float* gI, int32_t* tagU, int32_t* tagI, int step_tag, int flags,
                void* ws, float* stat, float* loss_acc, hipStream_t s) {
    DauArgs a{U, I, users, pos, gU, gI, tagU, tagI, stat, loss_acc, carve(ws, B, d), (unsigned)n_users, (unsigned)n_items, step_tag, B,
              tiles_of(B) * kT, tiles_per_split(B), col_splits(B), t, gamma, 1.0f / (float)B, regs / reg_div, same == PDA_DAU_SAME_DROP ? 1 : 0,
              (flags & PDA_UPD_ANY_ORDER) ? 1 : 0, (flags & PDA_UPD_USERS_DISTINCT) ? 1 : 0};
    PDA_STEP_LAUNCH(dau_pack_kernel, d, B, s, a)
    PDA_CHECK_LAUNCH();
    const dim3 tiles((unsigned)tiles_of(B), (unsigned)a.splits, 2u);
    DAU_TILE_LAUNCH(dau_tiles_kernel, d, tiles, s, a)
    PDA_CHECK_LAUNCH();
    hipLaunchKernelGGL(dau_reduce_kernel, dim3(1), dim3(1024), 0, s, a);
    PDA_CHECK_LAUNCH();
    PDA_STEP_LAUNCH(dau_tail_kernel, d, B, s, a)
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

}  // namespace

extern "C" int pda_dau_col_splits(int B) { return (B < 1 || B > PDA_DAU_MAX_B) ? 0 : col_splits(B); }

extern "C" size_t pda_dau_workspace_bytes(int B, int d) {
    if (B < 1 || B > PDA_DAU_MAX_B || !pda_d_ok(d)) return 0;
    return carve(nullptr, B, d).bytes;
}

extern "C" int pda_dau_step_f32(const float* U, const float* I, size_t n_users, size_t n_items, const int32_t* users, const int32_t* pos, int B,
                                int d, float t, float gamma, int same, float regs, float reg_div, float* gU, float* gI, int32_t* tagU,
                                int32_t* tagI, int step_tag, int flags, void* ws, size_t ws_bytes, float* stat, float* loss_acc, void* stream) {
    const int rc = check_step(U, I, n_users, n_items, users, pos, B, d, t, gamma, same, reg_div, gU, gI, tagU, tagI, step_tag, flags, ws, ws_bytes);
    if (rc != PDA_OK) return rc;
    return launch_step(U, I, n_users, n_items, users, pos, B, d, t, gamma, same, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags, ws, stat,
                       loss_acc, reinterpret_cast<hipStream_t>(stream));
}

extern "C" int pda_dau_adam_step_f32(float* U, float* mU, float* vU, float* gU, int32_t* tagU, size_t n_users, float* I, float* mI, float* vI,
                                     float* gI, int32_t* tagI, size_t n_items, const int32_t* users, const int32_t* pos, int B, int d, float t,
                                     float gamma, int same, float regs, float reg_div, int step_tag, float lr_t, float beta1, float beta2,
                                     float eps, int flags, int cache_policy, void* ws, size_t ws_bytes, float* stat, float* loss_acc,
                                     void* stream) {
    if (!mU || !vU || !mI || !vI) return PDA_ERR_ARG;
    if (cache_policy < PDA_ADAM_CACHE_AUTO || cache_policy > PDA_ADAM_CACHE_STREAM) return PDA_ERR_ARG;
    int rc = check_step(U, I, n_users, n_items, users, pos, B, d, t, gamma, same, reg_div, gU, gI, tagU, tagI, step_tag, flags, ws, ws_bytes);
    if (rc != PDA_OK) return rc;
    rc = launch_step(U, I, n_users, n_items, users, pos, B, d, t, gamma, same, regs, reg_div, gU, gI, tagU, tagI, step_tag, flags, ws, stat, loss_acc,
                     reinterpret_cast<hipStream_t>(stream));
    if (rc != PDA_OK) return rc;
    return pda_adam_dense_sweep4_f32(U, mU, vU, gU, n_users, tagU, I, mI, vI, gI, n_items, tagI, d, step_tag, lr_t, beta1, beta2, eps, cache_policy,
                                     stream);
}
