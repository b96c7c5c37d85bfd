// Exact full-catalogue ranks of chosen (user, item) pairs (include/pda_hip_rank.h) on MI355X (gfx950): where a held-out item stands in the
// user's masked ranking of all items, without the [users, items] rating matrix and without a list.
//
//   rank_keys_kernel   the packed key of every target entry.  One wave per 32 users, the users' rows as MFMA A operands in registers; for
//                      slot s the B operand's row j is the s-th target of user j (gathered from HBM, id clamped); one full 32 x 32 product per
//                      slot, of which the diagonal is kept.  An output element of the MFMA depends on its own row and column only, so the
//                      value is the sweep's to the bit.  Cost: (longest target row of the wave) products per 32 users.
//   rank_count_kernel  how many ranking items stand above each key.  Front end = deep_sweep_kernel's (pda_deep_topk.hip), copied: 256 threads =
//                      4 waves per 128 users, 32 user rows per wave as A operands, 32-item tiles staged in LDS with clamped loads
//                      (XOR-swizzled), k = 8c + 4h + s from lane-half h, two v_mfma_f32_32x32x2_f32 chains added once, the history cursor,
//                      valid_mask, accumulator layout row = (r & 3) + 8 (r >> 2) + 4 h.  Back end = counting instead of selecting:
//                        chunk    a row's next PDA_RANK_TCHUNK target keys are loaded into LDS and sorted descending per row (zeros last);
//                                 T = the row's non-zero keys of the chunk
//                        buckets  one i32 per (row, slot).  A finished score's key finds c = the number of the row's keys >= it (a linear
//                                 count up to kRankLinear keys, a binary search above) and, if c < T, increments bucket[row][c] (LDS atomic):
//                                 the item stands above the keys c, c + 1, ... of the row
//                        flush    at the end of the workgroup's item range: above[entry of slot i] += bucket[row][0] + ... + bucket[row][i],
//                                 one global integer atomic per slot; n_ranked[row] += the row's ranking items (first chunk only)
//                      Rows with more targets than a chunk take further launches (`pass`); a workgroup whose 128 rows hold no key in the pass
//                      returns before it loads anything.  Integers only: the result does not depend on the geometry.
#include "pda_topk_common.h"
#include "pda_hip_rank.h"

namespace {

using namespace pda_topk;

constexpr int kTC = PDA_RANK_TCHUNK;      // target keys of a row per pass
constexpr int kRankLinear = 8;            // rows with at most this many keys in the pass count linearly
constexpr int kRankMaxSplits = 32;
static_assert(kTC == 32 && kUserTile * kTC == 16 * kThreads, "the chunk sort deals 16 (row, slot) pairs to every thread");

struct RankArgs {
    const void* U;
    const void* I;
    const float* pop;
    const int32_t* users;
    const int64_t* hist_indptr;
    const int32_t* hist_indices;
    const int64_t* tgt_indptr;
    const int32_t* tgt_indices;   // keys call
    uint64_t* tgt_keys;           // keys call: written; count call: read
    int32_t* above;
    int32_t* n_ranked;
    int n_users_blk, item_offset, n_items_local, hist_row_mode, n_splits, pass;
};

template <int HEAD>
__device__ __forceinline__ float rank_head(float x, float popv) {
    if constexpr (HEAD == PDA_HEAD_POP) return (x > 0.0f ? x + 1.0f : __expf(x)) * popv;
    return x;
}

// ------------------------------------------------------------------------------------------------
// Keys of the target entries.
// ------------------------------------------------------------------------------------------------
template <int D, int HEAD, bool BF>
__global__ void __launch_bounds__(kThreads) rank_keys_kernel(RankArgs a) {
    constexpr int NC = D / 8;             // k-chunks of 8 (even: two accumulator chains)
    static_assert(NC % 2 == 0, "embed dim must be a multiple of 16");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;

    const int row_blk = blockIdx.x * kUserTile + wave * 32 + j;
    const bool row_ok = row_blk < a.n_users_blk;
    const int uid = row_ok ? a.users[row_blk] : 0;

    int64_t tb = 0, te = 0;
    if (row_ok) {
        tb = a.tgt_indptr[row_blk];
        te = a.tgt_indptr[row_blk + 1];
    }
    const int64_t len = te > tb ? te - tb : 0;
    int64_t maxlen = len;                 // the wave's longest row: every lane takes part in every product
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t other = __shfl_xor(maxlen, o, 64);
        maxlen = other > maxlen ? other : maxlen;
    }
    if (maxlen == 0) return;              // (wave-uniform)

    f32x4 areg[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row_ok) v = pda_load4<BF>(a.U, (size_t)uid * D + 4 * h + 8 * c);
        areg[c] = v;
    }

    int64_t hb = 0, he = 0;
    if (a.hist_indptr != nullptr && row_ok) {
        const int64_t hr = a.hist_row_mode == PDA_HIST_BY_USER_ID ? (int64_t)uid : (int64_t)row_blk;
        hb = a.hist_indptr[hr];
        he = a.hist_indptr[hr + 1];
    }

    // the diagonal element (row j, column j) lives in the lane half h = (j >> 2) & 1, register (j & 3) + 4 (j >> 3)
    const bool mine = h == ((j >> 2) & 1);
    const int rsel = (j & 3) + 4 * (j >> 3);

    for (int64_t s = 0; s < maxlen; ++s) {
        const bool has = s < len;
        const int id = has ? a.tgt_indices[tb + s] : a.item_offset;
        const bool in_shard = has && id >= a.item_offset && (int64_t)id < (int64_t)a.item_offset + a.n_items_local;
        const int loc = in_shard ? id - a.item_offset : 0;    // clamped: a row of the shard whatever the entry holds

        f32x16 acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        f32x16 acc1 = acc0;
#pragma unroll
        for (int c = 0; c < NC; c += 2) {
            const f32x4 b0 = pda_load4<BF>(a.I, (size_t)loc * D + 4 * h + 8 * c);
            const f32x4 b1 = pda_load4<BF>(a.I, (size_t)loc * D + 4 * h + 8 * (c + 1));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[c][q], b0[q], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[c + 1][q], b1[q], acc1, 0, 0, 0);
            }
        }
        const f32x16 acc = acc0 + acc1;
        float v = acc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) v = rsel == r ? acc[r] : v;

        if (mine && in_shard) {
            float popv = 1.0f;
            if constexpr (HEAD == PDA_HEAD_POP) popv = a.pop[loc];
            const float tt = rank_head<HEAD>(v, popv);
            int64_t lo = hb, hi = he;     // lower_bound(id) in the history row
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (a.hist_indices[mid] < id) lo = mid + 1; else hi = mid;
            }
            const bool listed = lo < he && a.hist_indices[lo] == id;
            a.tgt_keys[tb + s] = (!listed && tt > -INFINITY) ? pda_pack_key(tt, (uint32_t)id) : 0ull;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Counts.  LDS: item tile f32 [32][D] swizzled | keys u64 [128][kTC] | buckets i32 [128][kTC] | T i32 [128] | slot of a sorted key u8 [128][kTC]
// ------------------------------------------------------------------------------------------------
template <int D>
constexpr size_t rank_count_smem() {
    return 32 * D * sizeof(float) + (size_t)kUserTile * kTC * (sizeof(uint64_t) + sizeof(int) + 1) + kUserTile * sizeof(int);
}

template <int D, int HEAD, bool BF>
__global__ void __launch_bounds__(kThreads, (D <= 128 ? 2 : 1)) rank_count_kernel(RankArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Bt = reinterpret_cast<float*>(smem);                                     // [32][D] swizzled
    uint64_t* tkl = reinterpret_cast<uint64_t*>(smem + 32 * D * sizeof(float));     // [128][kTC] the rows' keys of this pass, descending
    int* bkt = reinterpret_cast<int*>(tkl + kUserTile * kTC);                       // [128][kTC]
    int* tnl = bkt + kUserTile * kTC;                                               // [128] non-zero keys of the row in this pass
    unsigned char* slotl = reinterpret_cast<unsigned char*>(tnl + kUserTile);       // [128][kTC] sorted position -> slot of the chunk

    constexpr int CPR = D / 4;            // 16-B chunks per item row
    constexpr int NLD = (32 * CPR) / kThreads;  // float4 loads / thread / tile (D >= 32)
    static_assert(NLD >= 1, "embed dim too small for the 256-thread staging pattern");
    constexpr int NC = D / 8;             // k-chunks of 8 (even: two accumulator chains)
    static_assert(NC % 2 == 0, "embed dim must be a multiple of 16");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int split = blockIdx.x % a.n_splits, utile = blockIdx.x / a.n_splits;

    const int tiles_total = (a.n_items_local + 31) >> 5;
    const int tiles_per = (tiles_total + a.n_splits - 1) / a.n_splits;
    const int t0 = split * tiles_per;
    const int t1 = min(t0 + tiles_per, tiles_total);

    // ---- this pass's chunk of every row: keys -> LDS, sorted descending per row.  Thread t owns the slots 16 (t & 1) .. + 16 of row t >> 1 ----
    {
        const int row = tid >> 1, s0 = (tid & 1) * 16;
        const int rb = utile * kUserTile + row;
        int64_t tb = 0, te = 0;
        if (rb < a.n_users_blk) {
            tb = a.tgt_indptr[rb] + (int64_t)a.pass * kTC;
            te = a.tgt_indptr[rb + 1];
        }
        // (workgroup-uniform) none of these 128 rows reaches into this chunk: nothing to count, and n_ranked was the first pass's
        if (a.pass > 0 && !__syncthreads_or(tb < te)) return;
        uint64_t mykey[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int64_t e = tb + s0 + q;
            mykey[q] = e < te ? a.tgt_keys[e] : 0ull;
            tkl[row * kTC + s0 + q] = mykey[q];
            bkt[row * kTC + s0 + q] = 0;
        }
        __syncthreads();
        int rank[16];
#pragma unroll
        for (int q = 0; q < 16; ++q) rank[q] = 0;
        for (int m = 0; m < kTC; ++m) {                 // position = the keys above mine, equal keys in slot order
            const uint64_t km = tkl[row * kTC + m];
#pragma unroll
            for (int q = 0; q < 16; ++q) rank[q] += (km > mykey[q] || (km == mykey[q] && m < s0 + q)) ? 1 : 0;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            tkl[row * kTC + rank[q]] = mykey[q];
            slotl[row * kTC + rank[q]] = (unsigned char)(s0 + q);
        }
        int nz = 0;
#pragma unroll
        for (int q = 0; q < 16; ++q) nz += mykey[q] != 0ull;
        nz += __shfl_xor(nz, 1, 64);                    // (the row's two threads are neighbours in one wave)
        if ((tid & 1) == 0) tnl[row] = nz;
    }

    // ---- this lane's user row (rows are indexed by lane&31 in both halves) -------------------
    const int row_blk = utile * kUserTile + wave * 32 + j;
    const bool row_ok = row_blk < a.n_users_blk;
    const int uid = row_ok ? a.users[row_blk] : 0;

    f32x4 areg[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (row_ok) v = pda_load4<BF>(a.U, (size_t)uid * D + 4 * h + 8 * c);
        areg[c] = v;
    }

    // ---- history cursor: head `nxt`, look-ahead `nxt2`, and one refill load in flight (`pend_v`) -- pda_score_topk.hip ---
    int64_t hp = 0, he = 0;
    int nxt = 0x7fffffff, nxt2 = 0x7fffffff, pend_v = 0x7fffffff;
    bool pend_flag = false, pend_ok = false;
    const bool hist_on = a.hist_indptr != nullptr;
    if (hist_on && row_ok) {
        const int64_t hr = a.hist_row_mode == PDA_HIST_BY_USER_ID ? (int64_t)uid : (int64_t)row_blk;
        hp = a.hist_indptr[hr];
        he = a.hist_indptr[hr + 1];
        const int lo_item = a.item_offset + t0 * 32;
        int64_t lo = hp, hi = he;  // lower_bound(lo_item)
        while (lo < hi) {
            int64_t mid = (lo + hi) >> 1;
            if (a.hist_indices[mid] < lo_item) lo = mid + 1; else hi = mid;
        }
        hp = lo;
        if (hp < he) nxt = a.hist_indices[hp];
        if (hp + 1 < he) nxt2 = a.hist_indices[hp + 1];
    }

    // ---- item tile staging -------------------------------------------------------------------
    f32x4 pre[NLD];
    // Unconditional loads (row index clamped, never predicated); rows past the end of the shard produce garbage scores that `vmask` discards.
    auto tile_load = [&](int t) {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int id = tid + kThreads * q;
            const int jj = id / CPR, ch = id % CPR;
            const int it = min(t * 32 + jj, a.n_items_local - 1);
            pre[q] = pda_load4<BF>(a.I, (size_t)it * D + 4 * ch);
        }
    };
    auto tile_store = [&]() {
#pragma unroll
        for (int q = 0; q < NLD; ++q) {
            const int id = tid + kThreads * q;
            const int jj = id / CPR, ch = id % CPR;
            *reinterpret_cast<f32x4*>(Bt + jj * D + 4 * (ch ^ swz<D>(jj))) = pre[q];
        }
    };
    auto pop_load = [&](int t) -> float {
        if constexpr (HEAD == PDA_HEAD_POP) return a.pop[min(t * 32 + j, a.n_items_local - 1)];
        return 1.0f;
    };
    // History bits of tile t for my row (branch-free for at most one listed item of the row inside the tile).
    auto hist_bits = [&](int t) -> uint32_t {
        if (!hist_on) return 0u;                                   // wave-uniform
        const int jg0 = a.item_offset + t * 32, jg1 = jg0 + 32;
        nxt2 = pend_flag ? (pend_ok ? pend_v : 0x7fffffff) : nxt2; // value loaded one tile ago: no stall
        const bool adv = nxt < jg1;
        uint32_t hb = adv ? (1u << ((nxt - jg0) & 31)) : 0u;
        hp += adv ? 1 : 0;
        nxt = adv ? nxt2 : nxt;
        const int64_t idx = hp + 1;
        pend_ok = idx < he;
        pend_flag = adv;
        const int64_t idc = adv ? max((int64_t)0, min(idx, he - 1)) : (int64_t)0;
        pend_v = a.hist_indices[idc];
        if (__builtin_expect(__any(nxt < jg1), 0)) {               // rare: several listed items in one tile
            do {
                if (nxt < jg1) {
                    const int nn2 = pend_flag ? (pend_ok ? pend_v : 0x7fffffff) : nxt2;
                    hb |= 1u << ((nxt - jg0) & 31);
                    ++hp;
                    nxt = nn2;
                    nxt2 = (hp + 1 < he) ? a.hist_indices[hp + 1] : 0x7fffffff;
                    pend_flag = false;
                }
            } while (__any(nxt < jg1));
        }
        return hb;
    };
    auto valid_mask = [&](int t) -> uint64_t {
        const int nvalid = min(32, a.n_items_local - t * 32);
        return nvalid >= 32 ? ~0ull : (((1ull << nvalid) - 1ull) * 0x100000001ull);
    };

    const float* brow = Bt + j * D;
    const int bswz = swz<D>(j);

    // ---- the back end: one finished tile -> the buckets of the rows.  Register r of lane (j, h) is the pair (row (r & 3) + 8 (r >> 2) + 4 h of
    // the wave, item jg0 + j): the 32 lanes of a half share the row, so its keys are read as LDS broadcasts. ----
    int ranked[16];                       // ranking items of the rows of my registers, my column only
#pragma unroll
    for (int r = 0; r < 16; ++r) ranked[r] = 0;
    auto count_tile = [&](const f32x16& accv, float popv, uint64_t vmask, uint32_t hb, int jg0) {
        const uint32_t my_item = (uint32_t)(jg0 + j);
        const bool lane_ok = (vmask >> lane) & 1ull;
        const bool any_hb = __any(hb != 0);   // some row of this wave has listed items inside the tile
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float tt = rank_head<HEAD>(accv[r], popv);
            bool p = lane_ok && (tt > -INFINITY);
            const int rowb = (r & 3) + 8 * (r >> 2);
            if (any_hb) {   // listed items never rank
                const uint32_t h0 = (uint32_t)__builtin_amdgcn_readlane((int)hb, rowb);
                const uint32_t h1 = (uint32_t)__builtin_amdgcn_readlane((int)hb, rowb + 4);
                if (((h ? h1 : h0) >> j) & 1u) p = false;
            }
            ranked[r] += p ? 1 : 0;
            const int row = wave * 32 + rowb + 4 * h;
            const int T = tnl[row];
            if (p && T > 0) {
                const uint64_t key = pda_pack_key(tt, my_item);
                const uint64_t* tk = tkl + row * kTC;
                int c = 0;
                if (T <= kRankLinear) {
                    for (int i = 0; i < T; ++i) c += tk[i] >= key ? 1 : 0;
                } else {
                    int hi = T;           // the first position whose key is below mine
                    while (c < hi) {
                        const int mid = (c + hi) >> 1;
                        if (tk[mid] >= key) c = mid + 1; else hi = mid;
                    }
                }
                if (c < T) atomicAdd(&bkt[row * kTC + c], 1);   // (c == T: below every key of the row -- no bucket)
            }
        }
    };

    // Software pipeline of pda_score_topk.hip.  Iteration t: issue the global loads of tile t+1; MFMA chain of tile t; barrier; stage tile t+1
    // into LDS; advance the history cursor to tile t+1; count tile t-1; barrier (next tile visible in Bt).
    f32x16 acc_prev = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    uint64_t vmask_prev = 0, vmask_cur = 0;
    uint32_t hb_prev = 0, hb_cur = 0;
    float popj_prev = 0.f, popj_cur = 0.f;

    if (t0 < t1) {
        tile_load(t0);
        popj_cur = pop_load(t0);
        tile_store();
        hb_cur = hist_bits(t0);
        vmask_cur = valid_mask(t0);
    }
    __syncthreads();   // (also: the sorted keys, T and the zeroed buckets are visible)

    for (int t = t0; t < t1; ++t) {
        const bool has_next = (t + 1) < t1;
        const int tn = has_next ? t + 1 : t;          // last iteration re-loads its own tile: keeps the loads unconditional
        tile_load(tn);
        const float popj_next = pop_load(tn);
        __builtin_amdgcn_sched_barrier(0);   // pin the prefetch ahead of the MFMA chain

        f32x16 acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        f32x16 acc1 = acc0;
#pragma unroll
        for (int c = 0; c < NC; c += 2) {
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(brow + 4 * ((2 * c + h) ^ bswz));
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(brow + 4 * ((2 * c + 2 + h) ^ bswz));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[c][q], b0[q], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[c + 1][q], b1[q], acc1, 0, 0, 0);
            }
        }
        const f32x16 acc = acc0 + acc1;

        __syncthreads();  // every wave is done reading Bt
        uint32_t hb_next = 0;
        if (has_next) {
            tile_store();
            hb_next = hist_bits(t + 1);
        }
        if (t > t0) count_tile(acc_prev, popj_prev, vmask_prev, hb_prev, a.item_offset + (t - 1) * 32);
        __syncthreads();  // next tile visible in Bt

        acc_prev = acc;
        vmask_prev = vmask_cur;
        hb_prev = hb_cur;
        popj_prev = popj_cur;
        vmask_cur = has_next ? valid_mask(t + 1) : 0ull;
        hb_cur = hb_next;
        popj_cur = popj_next;
    }
    if (t0 < t1) count_tile(acc_prev, popj_prev, vmask_prev, hb_prev, a.item_offset + (t1 - 1) * 32);   // drain: the last tile

    // ---- flush: n_ranked (first pass), then the buckets' prefix sums ----
    if (a.pass == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            int v = ranked[r];
#pragma unroll
            for (int o = 16; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);   // over the 32 columns of my half
            const int rb = utile * kUserTile + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
            if (j == 0 && rb < a.n_users_blk && v != 0) atomicAdd(&a.n_ranked[rb], v);
        }
    }
    __syncthreads();
    if (tid < kUserTile) {
        const int rb = utile * kUserTile + tid;
        const int T = tnl[tid];
        if (rb < a.n_users_blk && T > 0) {
            const int64_t tb = a.tgt_indptr[rb] + (int64_t)a.pass * kTC;
            int run = 0;
            for (int i = 0; i < T; ++i) {
                run += bkt[tid * kTC + i];
                if (run != 0) atomicAdd(&a.above[tb + slotl[tid * kTC + i]], run);
            }
        }
    }
}

template <int D, int HEAD, bool BF>
int launch_rank_keys(const RankArgs& a, hipStream_t stream) {
    const int utiles = (a.n_users_blk + kUserTile - 1) / kUserTile;
    hipLaunchKernelGGL((rank_keys_kernel<D, HEAD, BF>), dim3((unsigned)utiles), dim3(kThreads), 0, stream, a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

// Item-range splits per user tile: enough workgroups for the chip while a split still sweeps at least 16 tiles.
inline int rank_splits(int n_users_blk, int n_items_local, int want_wgs) {
    const int utiles = (n_users_blk + kUserTile - 1) / kUserTile;
    const int tiles = (n_items_local + 31) / 32;
    int s = 1;
    while ((long long)utiles * s < want_wgs && s < kRankMaxSplits && tiles / (2 * s) >= 16) s *= 2;
    return s;
}

template <int D, int HEAD, bool BF>
int launch_rank_count(RankArgs a, int max_tgt_row, int n_splits, hipStream_t stream) {
    constexpr size_t smem = rank_count_smem<D>();
    static int attr_set = 0;  // idempotent attribute; benign if raced
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&rank_count_kernel<D, HEAD, BF>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)smem) != hipSuccess)
            return PDA_ERR_LAUNCH;
        attr_set = 1;
    }
    const int utiles = (a.n_users_blk + kUserTile - 1) / kUserTile;
    const int passes = max_tgt_row > 0 ? (max_tgt_row + kTC - 1) / kTC : 1;
    for (int pass = 0; pass < passes; ++pass) {
        a.pass = pass;
        // the first pass sweeps for every row; behind it only the few workgroups with a long row work, so their item range is cut finer
        a.n_splits = n_splits > 0 ? n_splits : rank_splits(a.n_users_blk, a.n_items_local, pass == 0 ? 512 : 0x7fffffff);
        hipLaunchKernelGGL((rank_count_kernel<D, HEAD, BF>), dim3((unsigned)utiles * (unsigned)a.n_splits), dim3(kThreads), smem, stream, a);
        PDA_CHECK_LAUNCH();
    }
    return PDA_OK;
}

#define PDA_RANK_DISPATCH(FN, DD, ...) \
    case DD:                           \
        return head == PDA_HEAD_POP ? FN<DD, PDA_HEAD_POP, BF>(__VA_ARGS__) : FN<DD, PDA_HEAD_RAW, BF>(__VA_ARGS__);

int rank_common_checks(const void* U, const void* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk, int item_offset,
                       int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode,
                       const int64_t* tgt_indptr, int head) {
    if (!U || !I_shard || !users || !tgt_indptr) return PDA_ERR_ARG;
    if (n_users_blk <= 0 || n_items_local <= 0 || item_offset < 0) return PDA_ERR_ARG;
    if (head != PDA_HEAD_RAW && head != PDA_HEAD_POP) return PDA_ERR_ARG;
    if (head == PDA_HEAD_POP && !pop_shard) return PDA_ERR_ARG;
    if (hist_indptr && !hist_indices) return PDA_ERR_ARG;
    if (hist_indptr && hist_row_mode != PDA_HIST_BY_BLOCK_ROW && hist_row_mode != PDA_HIST_BY_USER_ID) return PDA_ERR_ARG;
    if (d != 32 && d != 64 && d != 128 && d != 256) return PDA_ERR_UNSUPPORTED;
    return PDA_OK;
}

template <bool BF>
int rank_keys(const void* U, const void* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk, int item_offset,
              int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, const int64_t* tgt_indptr,
              const int32_t* tgt_indices, int head, uint64_t* tgt_keys, void* stream) {
    if (!tgt_indices || !tgt_keys) return PDA_ERR_ARG;
    const int rc = rank_common_checks(U, I_shard, pop_shard, users, n_users_blk, item_offset, n_items_local, d, hist_indptr, hist_indices,
                                      hist_row_mode, tgt_indptr, head);
    if (rc != PDA_OK) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const RankArgs a{U, I_shard, pop_shard, users, hist_indptr, hist_indices, tgt_indptr, tgt_indices, tgt_keys, nullptr, nullptr,
                     n_users_blk, item_offset, n_items_local, hist_row_mode, 1, 0};
    switch (d) {
        PDA_RANK_DISPATCH(launch_rank_keys, 32, a, s)
        PDA_RANK_DISPATCH(launch_rank_keys, 64, a, s)
        PDA_RANK_DISPATCH(launch_rank_keys, 128, a, s)
        PDA_RANK_DISPATCH(launch_rank_keys, 256, a, s)
        default:
            return PDA_ERR_UNSUPPORTED;
    }
}

template <bool BF>
int rank_count(const void* U, const void* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk, int item_offset,
               int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, const int64_t* tgt_indptr,
               const uint64_t* tgt_keys, int max_tgt_row, int head, int n_splits, int32_t* above, int32_t* n_ranked, void* stream) {
    if (!above || !n_ranked || n_splits < 0 || max_tgt_row < 0) return PDA_ERR_ARG;
    if (max_tgt_row > 0 && !tgt_keys) return PDA_ERR_ARG;
    const int rc = rank_common_checks(U, I_shard, pop_shard, users, n_users_blk, item_offset, n_items_local, d, hist_indptr, hist_indices,
                                      hist_row_mode, tgt_indptr, head);
    if (rc != PDA_OK) return rc;
    const int tiles = (n_items_local + 31) / 32;
    if (n_splits > tiles) n_splits = tiles;               // (a split without a tile would only idle)
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const RankArgs a{U, I_shard, pop_shard, users, hist_indptr, hist_indices, tgt_indptr, nullptr, const_cast<uint64_t*>(tgt_keys), above, n_ranked,
                     n_users_blk, item_offset, n_items_local, hist_row_mode, 1, 0};
    switch (d) {
        PDA_RANK_DISPATCH(launch_rank_count, 32, a, max_tgt_row, n_splits, s)
        PDA_RANK_DISPATCH(launch_rank_count, 64, a, max_tgt_row, n_splits, s)
        PDA_RANK_DISPATCH(launch_rank_count, 128, a, max_tgt_row, n_splits, s)
        PDA_RANK_DISPATCH(launch_rank_count, 256, a, max_tgt_row, n_splits, s)
        default:
            return PDA_ERR_UNSUPPORTED;
    }
}
#undef PDA_RANK_DISPATCH

}  // namespace

extern "C" int pda_rank_keys_f32(const float* U, const float* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk,
                                 int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices,
                                 int hist_row_mode, const int64_t* tgt_indptr, const int32_t* tgt_indices, int head, uint64_t* tgt_keys,
                                 void* stream) {
    return rank_keys<false>(U, I_shard, pop_shard, users, n_users_blk, item_offset, n_items_local, d, hist_indptr, hist_indices, hist_row_mode,
                            tgt_indptr, tgt_indices, head, tgt_keys, stream);
}

extern "C" int pda_rank_keys_bf16(const uint16_t* U, const uint16_t* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk,
                                  int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices,
                                  int hist_row_mode, const int64_t* tgt_indptr, const int32_t* tgt_indices, int head, uint64_t* tgt_keys,
                                  void* stream) {
    return rank_keys<true>(U, I_shard, pop_shard, users, n_users_blk, item_offset, n_items_local, d, hist_indptr, hist_indices, hist_row_mode,
                           tgt_indptr, tgt_indices, head, tgt_keys, stream);
}

extern "C" int pda_rank_count_f32(const float* U, const float* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk,
                                  int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices,
                                  int hist_row_mode, const int64_t* tgt_indptr, const uint64_t* tgt_keys, int max_tgt_row, int head,
                                  int n_splits, int32_t* above, int32_t* n_ranked, void* stream) {
    return rank_count<false>(U, I_shard, pop_shard, users, n_users_blk, item_offset, n_items_local, d, hist_indptr, hist_indices, hist_row_mode,
                             tgt_indptr, tgt_keys, max_tgt_row, head, n_splits, above, n_ranked, stream);
}

extern "C" int pda_rank_count_bf16(const uint16_t* U, const uint16_t* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk,
                                   int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices,
                                   int hist_row_mode, const int64_t* tgt_indptr, const uint64_t* tgt_keys, int max_tgt_row, int head,
                                   int n_splits, int32_t* above, int32_t* n_ranked, void* stream) {
    return rank_count<true>(U, I_shard, pop_shard, users, n_users_blk, item_offset, n_items_local, d, hist_indptr, hist_indices, hist_row_mode,
                            tgt_indptr, tgt_keys, max_tgt_row, head, n_splits, above, n_ranked, stream);
}
