// Deep lists (include/pda_hip_deep.h): full-catalogue score + history mask + top-K for K up to 1 024 on MI355X (gfx950), without the
// [users, items] rating matrix.
//
// This is generation 1's algorithm (pda_score_topk.hip) with the candidate lists moved off chip:
//   front end  = that kernel's: 256 threads = 4 waves per 128 users, 32 user rows per wave as MFMA A operands in registers, 32-item tiles
//                staged in LDS (XOR-swizzled), k = 8c + 4h + s from lane-half h, two v_mfma_f32_32x32x2_f32 chains added once; the history
//                cursor; one v_cmp per accumulator against the row's running threshold and a wave ballot, interleaved with the next tile's
//                MFMAs.  The arithmetic is that kernel's to the bit.
//   lists      = per (split, row) an append buffer of `cap` packed keys in the workspace, cap = the power of two >= max(2 K, 128).  A
//                passing lane takes a slot with an LDS atomic on the row's counter and stores its key; the counters and thresholds of the
//                128 rows stay in LDS.
//   compaction = when a row's buffer is full the WORKGROUP sorts it (a bitonic sort of cap u64 in 16 KB of LDS, 256 threads), keeps the
//                best K at the front and raises the row's threshold to the K-th value.  The decision is taken at the barrier the loop has
//                anyway (__syncthreads_or), so every wave enters it; the lanes whose append found the buffer full retry behind it (K + 32
//                <= cap: the retry cannot fail).  Items are visited in natural order, so a row accepts about K ln(n / K) candidates in all.
//   last pass  = deep_final_kernel, one workgroup per row: gathers the row's buffers of every split, sorts them best first, writes K keys /
//                ids / values and completes a short row with its listed items.
//   shards     = deep_merge_kernel (pda_deep_merge): the sorted lists of R item shards -> one list per user, by ranks, without a sort.
#include "pda_topk_common.h"
#include "pda_hip_deep.h"

namespace {

using namespace pda_topk;

constexpr int kDeepHdr = 256;             // workspace: header (identity word at +16) | counts i32 [kDeepMaxSplits][rows_pad] | lists u64 [splits][rows_pad][cap]
constexpr unsigned kDeepGeneration = 8u;  // identity word: generation tag of the deep path
constexpr int kDeepMaxSplits = 4;         // the last pass sorts splits * cap <= 8 192 keys in 64 KB of LDS

struct DeepArgs {
    const void* U;
    const void* I;
    const float* pop;
    const int32_t* users;
    const int64_t* hist_indptr;
    const int32_t* hist_indices;
    uint64_t* lists;
    int* counts;
    unsigned* ident;
    int n_users_blk, item_offset, n_items_local, hist_row_mode, K, n_splits, cap, rows_pad;
};

__host__ __device__ inline int deep_cap(int K) {
    int c = 128;
    while (c < 2 * K) c <<= 1;
    return c;
}

// Item-range splits per user tile: enough workgroups for the chip while every split still sees many times its buffer.
inline int deep_splits(int n_users_blk, int n_items_local, int K) {
    const int utiles = (n_users_blk + kUserTile - 1) / kUserTile;
    const int cap = deep_cap(K);
    int s = 1;
    while (utiles * s < 512 && s < kDeepMaxSplits && n_items_local / (2 * s) >= 8 * cap) s *= 2;
    return s;
}

// Bitonic sort of n (a power of two) keys in LDS, descending, by NT threads of one workgroup; ends behind a barrier.
template <int NT>
__device__ __forceinline__ void bitonic_desc(uint64_t* s, int n, int tid) {
    for (int k = 2; k <= n; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < (n >> 1); p += NT) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1));
                const int l = i | j;
                const uint64_t a = s[i], b = s[l];
                const bool desc = (i & k) == 0;
                if ((a < b) == desc) {
                    s[i] = b;
                    s[l] = a;
                }
            }
            __syncthreads();
        }
    }
}

template <int D, int HEAD, bool BF>
__global__ void __launch_bounds__(kThreads, (D <= 128 ? 2 : 1)) deep_sweep_kernel(DeepArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* Bt = reinterpret_cast<float*>(smem);                                    // [32][D] swizzled
    uint64_t* sbuf = reinterpret_cast<uint64_t*>(smem + 32 * D * sizeof(float));   // [cap] the compaction's sort buffer
    const int cap = a.cap;
    int* cntl = reinterpret_cast<int*>(sbuf + cap);                                // [128]
    float* taul = reinterpret_cast<float*>(cntl + kUserTile);                      // [128]

    constexpr int CPR = D / 4;            // 16-B chunks per item row
    constexpr int NLD = (32 * CPR) / kThreads;  // float4 loads / thread / tile (D >= 32)
    static_assert(NLD >= 1, "embed dim too small for the 256-thread staging pattern");
    constexpr int NC = D / 8;             // k-chunks of 8 (even: two accumulator chains)
    static_assert(NC % 2 == 0, "embed dim must be a multiple of 16");

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 31, h = lane >> 5;
    const int split = blockIdx.x % a.n_splits, utile = blockIdx.x / a.n_splits;
    const int K = a.K;

    const int tiles_total = (a.n_items_local + 31) >> 5;
    const int tiles_per = (tiles_total + a.n_splits - 1) / a.n_splits;
    const int t0 = split * tiles_per;
    const int t1 = min(t0 + tiles_per, tiles_total);

    if (blockIdx.x == 0 && tid == 0) *a.ident = (kDeepGeneration << 28) | ((BF ? 1u : 0u) << 14) | ((unsigned)HEAD << 13) | (unsigned)(D >> 6);

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

    // ---- per-row running state in LDS: candidate count + threshold ------
    if (lane < 32) {
        cntl[wave * 32 + lane] = 0;
        taul[wave * 32 + lane] = row_ok ? -INFINITY : INFINITY;  // rows past the end never accept anything
    }
    pda_wave_sync();
    f32x16 thr;
    auto refresh_thr = [&]() {
        int hv = h;
        asm volatile("" : "+v"(hv));   // opaque: keeps the 16 LDS addresses from being hoisted into live registers
#pragma unroll
        for (int r = 0; r < 16; ++r) thr[r] = taul[wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * hv];
    };
    refresh_thr();

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

    uint64_t* wg_lists = a.lists + ((size_t)split * a.rows_pad + (size_t)utile * kUserTile) * cap;   // this workgroup's 128 buffers
    const float* brow = Bt + j * D;
    const int bswz = swz<D>(j);

    // One append pass over a finished tile.  `rm`: accumulator registers to look at; `still`: per lane, the registers it may (still) append.
    // A passing lane takes a slot of its row's buffer (LDS atomic) and stores its key; a lane that finds the buffer full is noted in
    // `next_still`.  Returns the registers in which some lane of the wave was turned away (0: everything is in).
    auto append_pass = [&](uint32_t rm, uint32_t still, uint32_t& next_still, const f32x16& accv, float popv, uint64_t vmask, uint32_t hb,
                           int jg0) -> uint32_t {
        const uint32_t my_item = (uint32_t)(jg0 + j);
        const bool lane_ok = (vmask >> lane) & 1ull;
        const bool any_hb = __any(hb != 0);   // some row of this wave has listed items inside the tile
        uint32_t ovf_regs = 0;
        next_still = 0;
#pragma nounroll
        while (rm) {
            const int r = __builtin_ctz(rm);
            rm &= rm - 1u;
            float tt = accv[r];   // exact head value (the fast test only saw an upper bound)
            if constexpr (HEAD == PDA_HEAD_POP) tt = (tt > 0.0f ? tt + 1.0f : __expf(tt)) * popv;
            bool p = lane_ok && ((still >> r) & 1u) && (tt > thr[r]);
            const int rowb = (r & 3) + 8 * (r >> 2);
            if (any_hb) {   // listed items never enter
                const uint32_t h0 = (uint32_t)__builtin_amdgcn_readlane((int)hb, rowb);
                const uint32_t h1 = (uint32_t)__builtin_amdgcn_readlane((int)hb, rowb + 4);
                if (((h ? h1 : h0) >> j) & 1u) p = false;
            }
            bool ov = false;
            if (p) {
                const int row = wave * 32 + rowb + 4 * h;
                const int slot = atomicAdd(&cntl[row], 1);   // ds_add_rtn_u32: distinct slots for concurrent lanes
                if (slot < cap) wg_lists[(size_t)row * cap + slot] = pda_pack_key(tt, my_item);
                else ov = true;
            }
            if (ov) next_still |= 1u << r;
            if (__any(ov)) ovf_regs |= 1u << r;
        }
        return ovf_regs;
    };

    // Whole-workgroup compaction of every full buffer (entered by all four waves behind a barrier): best K to the front, sorted; the row's
    // count becomes K and its threshold the K-th value.
    auto wg_compact = [&]() {
        for (int row = 0; row < kUserTile; ++row) {
            if (cntl[row] < cap) continue;                    // (workgroup-uniform: LDS is only written behind the barriers below)
            uint64_t* gl = wg_lists + (size_t)row * cap;
            for (int i = tid; i < cap; i += kThreads) sbuf[i] = gl[i];
            __syncthreads();
            bitonic_desc<kThreads>(sbuf, cap, tid);
            for (int i = tid; i < K; i += kThreads) gl[i] = sbuf[i];
            if (tid == 0) {
                cntl[row] = K;
                taul[row] = pda_key_val(sbuf[K - 1]);
            }
            __syncthreads();
        }
    };

    // Slow path of one finished tile, around the barrier that publishes the next tile: append; if any wave of the workgroup was turned
    // away, compact together and let the lanes that were turned away retry (K + 32 <= cap: they get in).
    auto slow_path = [&](uint32_t regmask, const f32x16& accv, float popv, uint64_t vmask, uint32_t hb, int jg0) {
        uint32_t still = 0, ovf = 0;
        if (regmask) ovf = append_pass(regmask, 0xFFFFu, still, accv, popv, vmask, hb, jg0);
        if (__syncthreads_or(ovf != 0)) {
            wg_compact();
            refresh_thr();
            if (ovf) {
                uint32_t dummy;
                append_pass(ovf, still, dummy, accv, popv, vmask, hb, jg0);
            }
        }
    };

    // Threshold test on an UPPER BOUND of the head: ub = (max(s,0)+1)*pop equals the exact (elu(s)+1)*pop for s > 0 (bitwise) and is >= it
    // for s <= 0, so no candidate is missed and the exp is only paid on the slow path.
    auto head_ub = [&](float sc, float popv) -> float {
        if constexpr (HEAD == PDA_HEAD_POP) return (fmaxf(sc, 0.0f) + 1.0f) * popv;
        return sc;
    };

    // Software pipeline of pda_score_topk.hip.  Iteration t: issue the global loads of tile t+1; MFMA chain of tile t with the threshold test
    // of tile t-1 interleaved; barrier; stage tile t+1 into LDS; advance the history cursor to tile t+1; slow path of t-1 (which holds the
    // iteration's second barrier).
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
    __syncthreads();

    for (int t = t0; t < t1; ++t) {
        const bool has_next = (t + 1) < t1;
        const int tn = has_next ? t + 1 : t;          // last iteration re-loads its own tile: keeps the loads unconditional
        tile_load(tn);
        const float popj_next = pop_load(tn);
        __builtin_amdgcn_sched_barrier(0);   // pin the prefetch ahead of the MFMA chain

        f32x16 acc0 = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        f32x16 acc1 = acc0;
        uint32_t regmask = 0;
#pragma unroll
        for (int c = 0; c < NC; c += 2) {
            const f32x4 b0 = *reinterpret_cast<const f32x4*>(brow + 4 * ((2 * c + h) ^ bswz));
            const f32x4 b1 = *reinterpret_cast<const f32x4*>(brow + 4 * ((2 * c + 2 + h) ^ bswz));
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[c][q], b0[q], acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(areg[c + 1][q], b1[q], acc1, 0, 0, 0);
            }
#pragma unroll
            for (int r = (16 * c) / NC; r < (16 * (c + 2)) / NC; ++r)
                regmask |= (__ballot(head_ub(acc_prev[r], popj_prev) > thr[r]) & vmask_prev) ? (1u << r) : 0u;
        }
        // Scheduling recipe for the block above: B fragments ahead of their MFMAs, the test spread over the gaps.
        __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, (HEAD == PDA_HEAD_RAW ? 16 : 64) / (4 * NC) + 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x004, 1, 0);
            }
            __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
        }
        const f32x16 acc = acc0 + acc1;

        __syncthreads();  // every wave is done reading Bt
        uint32_t hb_next = 0;
        if (has_next) {
            tile_store();
            hb_next = hist_bits(t + 1);
        }
        slow_path(regmask, acc_prev, popj_prev, vmask_prev, hb_prev, a.item_offset + (t - 1) * 32);   // (its barrier: next tile visible in Bt)

        acc_prev = acc;
        vmask_prev = vmask_cur;
        hb_prev = hb_cur;
        popj_prev = popj_cur;
        vmask_cur = has_next ? valid_mask(t + 1) : 0ull;
        hb_cur = hb_next;
        popj_cur = popj_next;
    }
    if (t0 < t1) {   // drain: threshold test + slow path of the last tile
        uint32_t regmask = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) regmask |= (__ballot(head_ub(acc_prev[r], popj_prev) > thr[r]) & vmask_prev) ? (1u << r) : 0u;
        slow_path(regmask, acc_prev, popj_prev, vmask_prev, hb_prev, a.item_offset + (t1 - 1) * 32);
    }

    // ---- hand the buffers to the last pass: how many keys each holds ----
    __syncthreads();
    if (tid < kUserTile) a.counts[(size_t)split * a.rows_pad + (size_t)utile * kUserTile + tid] = min(cntl[tid], cap);
}

// ------------------------------------------------------------------------------------------------
// Last pass: one workgroup per row.  The row's buffers of every split -> LDS, one bitonic sort, K keys / ids / values out.  A row with
// fewer than K keys is completed by thread 0: its listed items of this shard, lowest id first (value -inf, key 0), then -1.
// ------------------------------------------------------------------------------------------------
struct DeepFinalArgs {
    const uint64_t* lists;
    const int* counts;
    const int32_t* users;
    const int64_t* hist_indptr;
    const int32_t* hist_indices;
    uint64_t* out_keys;
    int32_t* out_idx;
    float* out_val;
    int n_users_blk, item_offset, n_items_local, hist_row_mode, K, n_splits, cap, rows_pad;
};

__global__ void __launch_bounds__(256) deep_final_kernel(DeepFinalArgs f) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    uint64_t* sbuf = reinterpret_cast<uint64_t*>(smem);   // [n_splits * cap]
    const int tid = threadIdx.x, K = f.K;
    const size_t row = blockIdx.x;
    int total = 0;
    for (int s = 0; s < f.n_splits; ++s) {
        const int c = min(f.counts[(size_t)s * f.rows_pad + row], f.cap);
        const uint64_t* gl = f.lists + ((size_t)s * f.rows_pad + row) * f.cap;
        for (int i = tid; i < c; i += 256) sbuf[total + i] = gl[i];
        total += c;
    }
    int n = 2;
    while (n < total) n <<= 1;                             // (<= n_splits * cap: a power of two)
    for (int i = total + tid; i < n; i += 256) sbuf[i] = 0ull;
    __syncthreads();
    bitonic_desc<256>(sbuf, n, tid);
    const int nreal = min(total, K);
    const bool fill = nreal < K && f.out_idx != nullptr;
    for (int i = tid; i < K; i += 256) {
        const uint64_t k = i < nreal ? sbuf[i] : 0ull;
        const size_t o = row * (size_t)K + i;
        if (f.out_keys) f.out_keys[o] = k;
        if (f.out_val) f.out_val[o] = k ? pda_key_val(k) : -INFINITY;
        if (f.out_idx && i < nreal) f.out_idx[o] = pda_key_item(k);
    }
    if (fill && tid == 0) {
        int32_t* orow = f.out_idx + row * (size_t)K;
        int at = nreal;
        if (f.hist_indptr) {
            const int64_t hr = f.hist_row_mode == PDA_HIST_BY_USER_ID ? (int64_t)f.users[row] : (int64_t)row;
            int prev = -1;
            for (int64_t p = f.hist_indptr[hr]; p < f.hist_indptr[hr + 1] && at < K; ++p) {
                const int it = f.hist_indices[p];
                if (it != prev && it >= f.item_offset && it < f.item_offset + f.n_items_local) orow[at++] = it;
                prev = it;
            }
        }
        for (; at < K; ++at) orow[at] = -1;
    }
}

template <int D, int HEAD, bool BF>
int launch_deep(const DeepArgs& a, hipStream_t stream) {
    const size_t smem = 32 * D * sizeof(float) + (size_t)a.cap * sizeof(uint64_t) + (size_t)kUserTile * 8;
    static int attr_set = 0;  // idempotent attribute; benign if raced
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&deep_sweep_kernel<D, HEAD, BF>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(32 * D * sizeof(float) + 2 * PDA_DEEP_MAX_K * sizeof(uint64_t) + kUserTile * 8)) != hipSuccess)
            return PDA_ERR_LAUNCH;
        attr_set = 1;
    }
    const int utiles = (a.n_users_blk + kUserTile - 1) / kUserTile;
    hipLaunchKernelGGL((deep_sweep_kernel<D, HEAD, BF>), dim3((unsigned)(utiles * a.n_splits)), dim3(kThreads), smem, stream, a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

template <bool BF>
int dispatch_deep(const DeepArgs& a, int d, int head, hipStream_t s) {
#define PDA_DEEP_DISPATCH(DD) \
    case DD:                  \
        return head == PDA_HEAD_POP ? launch_deep<DD, PDA_HEAD_POP, BF>(a, s) : launch_deep<DD, PDA_HEAD_RAW, BF>(a, s);
    switch (d) {
        PDA_DEEP_DISPATCH(32)
        PDA_DEEP_DISPATCH(64)
        PDA_DEEP_DISPATCH(128)
        PDA_DEEP_DISPATCH(256)
        default:
            return PDA_ERR_UNSUPPORTED;
    }
#undef PDA_DEEP_DISPATCH
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

template <bool BF>
int deep_topk(const void* U, const void* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk, int item_offset,
              int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, int K, int head,
              uint64_t* out_keys, int32_t* out_idx, float* out_val, void* workspace, size_t workspace_bytes, void* stream) {
    if (!U || !I_shard || !users || !workspace) return PDA_ERR_ARG;
    if (!out_keys && !out_idx && !out_val) return PDA_ERR_ARG;
    if (n_users_blk <= 0 || n_items_local <= 0 || item_offset < 0) return PDA_ERR_ARG;
    if (K < 1 || K > PDA_DEEP_MAX_K || K > n_items_local) return PDA_ERR_ARG;
    if (head != PDA_HEAD_RAW && head != PDA_HEAD_POP) return PDA_ERR_ARG;
    if (head == PDA_HEAD_POP && !pop_shard) return PDA_ERR_ARG;
    if (hist_indptr && !hist_indices) return PDA_ERR_ARG;
    if (hist_indptr && hist_row_mode != PDA_HIST_BY_BLOCK_ROW && hist_row_mode != PDA_HIST_BY_USER_ID) return PDA_ERR_ARG;
    if (d != 32 && d != 64 && d != 128 && d != 256) return PDA_ERR_UNSUPPORTED;
    if (workspace_bytes < pda_deep_topk_workspace_bytes(n_users_blk, n_items_local, d, K)) return PDA_ERR_WORKSPACE;
    if (reinterpret_cast<uintptr_t>(workspace) & 15u) return PDA_ERR_ARG;

    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const int cap = deep_cap(K), n_splits = deep_splits(n_users_blk, n_items_local, K);
    const int rows_pad = (n_users_blk + kUserTile - 1) / kUserTile * kUserTile;
    unsigned char* ws = reinterpret_cast<unsigned char*>(workspace);
    // the header: cleared here, stream-ordered, so that a caller hands over any memory (the identity word at +16 is written by the sweep; the
    // other header words read as zero afterwards).  counts and lists are written by the sweep before the final kernel reads them.
    if (hipMemsetAsync(ws, 0, kDeepHdr, s) != hipSuccess) return PDA_ERR_LAUNCH;
    int* counts = reinterpret_cast<int*>(ws + kDeepHdr);
    uint64_t* lists = reinterpret_cast<uint64_t*>(ws + kDeepHdr + align256((size_t)kDeepMaxSplits * rows_pad * sizeof(int)));
    DeepArgs a{U, I_shard, pop_shard, users, hist_indptr, hist_indices, lists, counts, reinterpret_cast<unsigned*>(ws + 16),
               n_users_blk, item_offset, n_items_local, hist_row_mode, K, n_splits, cap, rows_pad};
    const int rc = dispatch_deep<BF>(a, d, head, s);
    if (rc != PDA_OK) return rc;

    static int attr_set = 0;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&deep_final_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)(kDeepMaxSplits * 2 * PDA_DEEP_MAX_K * sizeof(uint64_t))) != hipSuccess)
            return PDA_ERR_LAUNCH;
        attr_set = 1;
    }
    DeepFinalArgs f{lists, counts, users, hist_indptr, hist_indices, out_keys, out_idx, out_val,
                    n_users_blk, item_offset, n_items_local, hist_row_mode, K, n_splits, cap, rows_pad};
    hipLaunchKernelGGL(deep_final_kernel, dim3((unsigned)n_users_blk), dim3(256), (size_t)n_splits * cap * sizeof(uint64_t), s, f);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

// ------------------------------------------------------------------------------------------------
// Merge of R sorted lists of K <= 1 024 keys per row (pda_deep_merge): the item shards' lists of a user -> the user's list.  One workgroup
// per row, the row's R * K keys in LDS.  The lists are sorted, so nothing is sorted here:
//   floor     the K-th key of the union is at least (a) the largest K-th key of any list and (b) the smallest ceil(K / R)-th key of the lists
//             (every list holds that many keys at or above it: R ceil(K / R) >= K of them).  Equal shards put (b) near the answer.
//   cut       per list, how many of its keys reach the floor (one binary search): only those can rank, and only those need to be searched.
//   rank      the survivors are dealt to the threads evenly (a prefix sum of the cuts); a survivor's place in the result is the number of
//             keys above it = the sum of its lower bounds in the lists' survivors (its own list gives its own position: the keys of a row are
//             distinct).  Four lists are searched at a time, so that four LDS reads are in flight per step.
// The keys are integers and every result slot is written by the one key whose rank it is: the result does not depend on the geometry.
// ------------------------------------------------------------------------------------------------
struct DeepMergeArgs {
    const uint64_t* in_keys;
    uint64_t* out_keys;
    int32_t* out_idx;
    float* out_val;
    const int32_t* users;
    const int64_t* hist_indptr;
    const int32_t* hist_indices;
    int hist_row_mode, R, n_users_blk, K;
    int vec;   // every array starts on a 16-byte boundary: 16-byte loads and stores
};

constexpr int kMergeThreads = 256;
constexpr int kMergeLoads = 8;     // 16-byte loads a thread has in flight while it stages a row

// LDS of a row: keys u64 [R K] | merged u64 [K] | floors u64 [2] | ids i32 [K] | cut i32 [R] | prefix i32 [R + 1] | partial sums i32 [256]
inline size_t deep_merge_smem(int R, int K) {
    return ((size_t)R * K + K + 2) * sizeof(uint64_t) + ((size_t)K + 2 * (size_t)R + 1 + kMergeThreads) * sizeof(int);
}

__global__ void __launch_bounds__(kMergeThreads) deep_merge_kernel(DeepMergeArgs a) {
    typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));
    typedef int32_t i32x4 __attribute__((ext_vector_type(4)));
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, R = a.R, K = a.K, n = R * K;
    uint64_t* keys = reinterpret_cast<uint64_t*>(smem);
    uint64_t* outl = keys + n;
    unsigned long long* floors = reinterpret_cast<unsigned long long*>(outl + K);
    int* ids = reinterpret_cast<int*>(floors + 2);
    int* cut = ids + K;
    int* pre = cut + R;
    int* part = pre + R + 1;
    const size_t u = blockIdx.x;

    // ---- the row's lists -> LDS.  A list starts on an 8-byte boundary: 16-byte chunks counted from the 16-byte boundary at or below it.
    // kMergeLoads chunks per thread are loaded before the first is written: 64 KB in flight per CU at two workgroups (measured against a
    // chunk at a time: 4.0 - 4.1 instead of 4.4 ms at R = 8, K = 1 000 and 65 536 rows) ----
    const int P = (K + 2) >> 1;   // chunks that cover a list wherever it starts
    const int W = R * P;
    for (int w0 = tid; w0 < W; w0 += kMergeThreads * kMergeLoads) {
        u64x2 v[kMergeLoads];
        int at[kMergeLoads];      // LDS index of the chunk's first key; -1: that key is not the list's
        bool second[kMergeLoads];
#pragma unroll
        for (int q = 0; q < kMergeLoads; ++q) {
            const int w = w0 + q * kMergeThreads;
            const bool in = w < W;
            const int r = in ? w / P : 0, c = in ? w - r * P : 0;
            const size_t e0 = ((size_t)r * a.n_users_blk + u) * K;
            const uint64_t* g = a.in_keys + e0;
            const int p0 = 2 * c - (int)(e0 & 1);
            const bool k0 = in && p0 >= 0 && p0 < K, k1 = in && p0 + 1 < K;
            if (a.vec && k0 && k1) {
                v[q] = *reinterpret_cast<const u64x2*>(g + p0);
            } else {
                v[q][0] = k0 ? g[p0] : 0ull;
                v[q][1] = k1 ? g[p0 + 1] : 0ull;
            }
            at[q] = k0 ? r * K + p0 : -1;
            second[q] = k1;
            if (!k0 && k1) at[q] = -(r * K + p0 + 1) - 2;   // (only the chunk's second key is the list's: its index, folded below -1)
        }
#pragma unroll
        for (int q = 0; q < kMergeLoads; ++q) {
            if (at[q] >= 0) {
                keys[at[q]] = v[q][0];
                if (second[q]) keys[at[q] + 1] = v[q][1];
            } else if (at[q] < -1) {
                keys[-(at[q] + 2)] = v[q][1];
            }
        }
    }
    for (int i = tid; i < K; i += kMergeThreads) outl[i] = 0ull;
    if (tid == 0) {
        floors[0] = 0ull;
        floors[1] = ~0ull;
    }
    __syncthreads();

    // ---- the floor ----
    const int t = (K + R - 1) / R;
    for (int r = tid; r < R; r += kMergeThreads) {
        atomicMax(&floors[0], (unsigned long long)keys[r * K + K - 1]);   // (LDS, integers)
        atomicMin(&floors[1], (unsigned long long)keys[r * K + t - 1]);
    }
    __syncthreads();
    uint64_t fl = floors[0] > floors[1] ? floors[0] : floors[1];
    fl = fl ? fl : 1ull;          // an empty slot never ranks

    // ---- cuts and their prefix sums: thread q owns the lists [q chunk, (q + 1) chunk) ----
    const int chunk = (R + kMergeThreads - 1) / kMergeThreads;
    const int r_lo = min(tid * chunk, R), r_hi = min(r_lo + chunk, R);
    int mine = 0;
    for (int r = r_lo; r < r_hi; ++r) {
        const uint64_t* l = keys + r * K;
        int lo = 0, hi = K;       // first position whose key is below the floor
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (l[mid] >= fl) lo = mid + 1; else hi = mid;
        }
        cut[r] = lo;
        mine += lo;
    }
    part[tid] = mine;
    __syncthreads();
    if (r_lo < r_hi) {
        int base = 0;
        for (int q = 0; q < tid; ++q) base += part[q];
        for (int r = r_lo; r < r_hi; ++r) {
            pre[r] = base;
            base += cut[r];
        }
        if (r_hi == R) pre[R] = base;
    }
    __syncthreads();

    // ---- every survivor's rank ----
    const int S = pre[R];
    for (int s = tid; s < S; s += kMergeThreads) {
        int lo = 0, hi = R - 1;   // the survivor's list: the last one that starts at or before s
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (pre[mid] <= s) lo = mid; else hi = mid - 1;
        }
        const uint64_t key = keys[lo * K + (s - pre[lo])];
        int rank = 0, r2 = 0;
        for (; r2 + 4 <= R; r2 += 4) {
            const uint64_t *b0 = keys + r2 * K, *b1 = b0 + K, *b2 = b1 + K, *b3 = b2 + K;
            int l0 = 0, l1 = 0, l2 = 0, l3 = 0, h0 = cut[r2], h1 = cut[r2 + 1], h2 = cut[r2 + 2], h3 = cut[r2 + 3];
            while ((l0 < h0) | (l1 < h1) | (l2 < h2) | (l3 < h3)) {
                // (a finished search reads the slot at its bound again -- at most b[K], still this row's LDS -- and ignores it)
                const int m0 = (l0 + h0) >> 1, m1 = (l1 + h1) >> 1, m2 = (l2 + h2) >> 1, m3 = (l3 + h3) >> 1;
                const uint64_t k0 = b0[m0], k1 = b1[m1], k2 = b2[m2], k3 = b3[m3];
                if (l0 < h0) { if (k0 > key) l0 = m0 + 1; else h0 = m0; }
                if (l1 < h1) { if (k1 > key) l1 = m1 + 1; else h1 = m1; }
                if (l2 < h2) { if (k2 > key) l2 = m2 + 1; else h2 = m2; }
                if (l3 < h3) { if (k3 > key) l3 = m3 + 1; else h3 = m3; }
            }
            rank += l0 + l1 + l2 + l3;
        }
        for (; r2 < R; ++r2) {
            const uint64_t* b = keys + r2 * K;
            int l0 = 0, h0 = cut[r2];
            while (l0 < h0) {
                const int m0 = (l0 + h0) >> 1;
                if (b[m0] > key) l0 = m0 + 1; else h0 = m0;
            }
            rank += l0;
        }
        if (rank < K) outl[rank] = key;
    }
    __syncthreads();

    // ---- how many slots are filled (the ranks 0 .. nreal - 1 are all taken), the ids, a short row's listed items ----
    int nreal = 0;
    {
        int hi = K;
        while (nreal < hi) {
            const int mid = (nreal + hi) >> 1;
            if (outl[mid] != 0ull) nreal = mid + 1; else hi = mid;
        }
    }
    if (a.out_idx) {
        for (int i = tid; i < K; i += kMergeThreads) {
            const uint64_t k = outl[i];
            ids[i] = k ? pda_key_item(k) : -1;
        }
        if (nreal < K && a.hist_indptr) {   // (the same in every thread)
            __syncthreads();
            if (tid == 0) {
                const int64_t hr = a.hist_row_mode == PDA_HIST_BY_USER_ID ? (int64_t)a.users[u] : (int64_t)u;
                int at = nreal, prev = -1;
                for (int64_t p = a.hist_indptr[hr]; p < a.hist_indptr[hr + 1] && at < K; ++p) {
                    const int it = a.hist_indices[p];
                    if (it != prev) ids[at++] = it;
                    prev = it;
                }
            }
        }
        __syncthreads();
    }

    // ---- out: 16-byte stores counted from the 16-byte boundary at or below the row's start, single words at the row's ends ----
    const size_t o0 = u * (size_t)K;
    if (a.out_keys) {
        uint64_t* g = a.out_keys + o0;
        const int a0 = (int)(o0 & 1);
        for (int c = tid; c < (a0 + K + 1) >> 1; c += kMergeThreads) {
            const int p0 = 2 * c - a0;
            if (a.vec && p0 >= 0 && p0 + 1 < K) {
                const u64x2 v = {outl[p0], outl[p0 + 1]};
                *reinterpret_cast<u64x2*>(g + p0) = v;
            } else {
                if (p0 >= 0) g[p0] = outl[p0];
                if (p0 + 1 < K) g[p0 + 1] = outl[p0 + 1];
            }
        }
    }
    if (a.out_idx || a.out_val) {
        const int a0 = (int)(o0 & 3);
        for (int c = tid; c < (a0 + K + 3) >> 2; c += kMergeThreads) {
            const int p0 = 4 * c - a0;
            if (a.vec && p0 >= 0 && p0 + 3 < K) {
                if (a.out_idx) {
                    const i32x4 v = {ids[p0], ids[p0 + 1], ids[p0 + 2], ids[p0 + 3]};
                    *reinterpret_cast<i32x4*>(a.out_idx + o0 + p0) = v;
                }
                if (a.out_val) {
                    f32x4 v;
#pragma unroll
                    for (int q = 0; q < 4; ++q) v[q] = p0 + q < nreal ? pda_key_val(outl[p0 + q]) : -INFINITY;
                    *reinterpret_cast<f32x4*>(a.out_val + o0 + p0) = v;
                }
            } else {
                for (int p = max(p0, 0); p < min(p0 + 4, K); ++p) {
                    if (a.out_idx) a.out_idx[o0 + p] = ids[p];
                    if (a.out_val) a.out_val[o0 + p] = p < nreal ? pda_key_val(outl[p]) : -INFINITY;
                }
            }
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Metrics on deep lists: one thread per user row, the row walked once per K (no 64-bit hit mask).  Same sums and the same two reductions
// as pda_metrics / pda_metrics_ordered (pda_aux.hip).
// ------------------------------------------------------------------------------------------------
template <bool ORDERED>
__global__ void __launch_bounds__(256) metrics_deep_kernel(const int32_t* topk, int n_rows, int k_cols, const int64_t* tgt_indptr,
                                                           const int32_t* tgt_indices, const int32_t* Ks, int n_ks, double* sums) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    int64_t b = 0, e = 0;
    if (r < n_rows) {
        b = tgt_indptr[r];
        e = tgt_indptr[r + 1];
    }
    const int npos = (int)(e - b);
    for (int q = 0; q < n_ks; ++q) {
        const int K = Ks[q];
        const int kk = K < k_cols ? K : k_cols;   // r[:K] on a k_cols-long vector
        double prec = 0, rec = 0, ndcg = 0, hit = 0;
        if (r < n_rows && npos > 0) {
            int hits = 0;
            double dcg = 0, idcg = 0;
            for (int k = 0; k < kk; ++k) {
                const int it = topk[(size_t)r * k_cols + k];
                bool h = false;
                for (int64_t p = b; p < e; ++p) h |= (tgt_indices[p] == it);
                const double w = 1.0 / log2((double)k + 2.0);
                if (h) {
                    ++hits;
                    dcg += w;
                }
                if (k < npos) idcg += w;
            }
            prec = (double)hits / kk;
            rec = (double)hits / npos;
            ndcg = idcg > 0 ? dcg / idcg : 0.0;
            hit = hits > 0 ? 1.0 : 0.0;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            prec += __shfl_xor(prec, o, 64);
            rec += __shfl_xor(rec, o, 64);
            ndcg += __shfl_xor(ndcg, o, 64);
            hit += __shfl_xor(hit, o, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if constexpr (ORDERED) {
                const size_t n_waves = (size_t)gridDim.x * (blockDim.x / 64), w = (size_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6);
                sums[(size_t)(0 * n_ks + q) * n_waves + w] = prec;
                sums[(size_t)(1 * n_ks + q) * n_waves + w] = rec;
                sums[(size_t)(2 * n_ks + q) * n_waves + w] = ndcg;
                sums[(size_t)(3 * n_ks + q) * n_waves + w] = hit;
            } else {
                atomicAdd(sums + 0 * n_ks + q, prec);
                atomicAdd(sums + 1 * n_ks + q, rec);
                atomicAdd(sums + 2 * n_ks + q, ndcg);
                atomicAdd(sums + 3 * n_ks + q, hit);
            }
        }
    }
}

// One workgroup per sum: thread t adds the waves t, t + 256, ... in that order, thread 0 the 256 partial sums in thread order.
__global__ void __launch_bounds__(256) metrics_deep_sum_kernel(const double* __restrict__ partial, int n_waves, double* __restrict__ sums) {
    __shared__ double s_acc[256];
    const int jx = (int)blockIdx.x, tid = threadIdx.x;
    const double* p = partial + (size_t)jx * n_waves;
    double acc = 0;
    for (int w = tid; w < n_waves; w += 256) acc += p[w];
    s_acc[tid] = acc;
    __syncthreads();
    if (tid == 0) {
        double tot = 0;
        for (int t = 0; t < 256; ++t) tot += s_acc[t];
        sums[jx] += tot;
    }
}

}  // namespace

extern "C" size_t pda_deep_topk_workspace_bytes(int n_users_blk, int n_items_local, int d, int K) {
    if (n_users_blk <= 0 || n_items_local <= 0 || K < 1 || K > PDA_DEEP_MAX_K) return 0;
    (void)d;
    // buffers = user tiles x splits.  More users can mean fewer splits (below 512 workgroups), so the size is that of the largest block of
    // at most this many users: non-decreasing in n_users_blk (and in K: a split never shrinks faster than cap grows)
    const int utiles = (n_users_blk + kUserTile - 1) / kUserTile;
    size_t bufs = (size_t)utiles * deep_splits(n_users_blk, n_items_local, K);
    for (int u = 1; u < utiles && u < 512; ++u) {
        const size_t b = (size_t)u * deep_splits(u * kUserTile, n_items_local, K);
        bufs = b > bufs ? b : bufs;
    }
    return kDeepHdr + align256((size_t)kDeepMaxSplits * utiles * kUserTile * sizeof(int)) + bufs * kUserTile * (size_t)deep_cap(K) * sizeof(uint64_t);
}

extern "C" int pda_deep_topk_f32(const float* U, const float* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk,
                                 int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices,
                                 int hist_row_mode, int K, int head, uint64_t* out_keys, int32_t* out_idx, float* out_val, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    return deep_topk<false>(U, I_shard, pop_shard, users, n_users_blk, item_offset, n_items_local, d, hist_indptr, hist_indices, hist_row_mode,
                            K, head, out_keys, out_idx, out_val, workspace, workspace_bytes, stream);
}

extern "C" int pda_deep_topk_bf16(const uint16_t* U, const uint16_t* I_shard, const float* pop_shard, const int32_t* users, int n_users_blk,
                                  int item_offset, int n_items_local, int d, const int64_t* hist_indptr, const int32_t* hist_indices,
                                  int hist_row_mode, int K, int head, uint64_t* out_keys, int32_t* out_idx, float* out_val, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    return deep_topk<true>(U, I_shard, pop_shard, users, n_users_blk, item_offset, n_items_local, d, hist_indptr, hist_indices, hist_row_mode,
                           K, head, out_keys, out_idx, out_val, workspace, workspace_bytes, stream);
}

extern "C" int pda_deep_merge(const uint64_t* in_keys, int R, int n_users_blk, int K, uint64_t* out_keys, int32_t* out_idx, float* out_val,
                              const int32_t* users, const int64_t* hist_indptr, const int32_t* hist_indices, int hist_row_mode, void* stream) {
    if (!in_keys || R < 1 || n_users_blk <= 0 || K < 1 || K > PDA_DEEP_MAX_K) return PDA_ERR_ARG;
    if (!out_keys && !out_idx) return PDA_ERR_ARG;
    if (hist_indptr && !hist_indices) return PDA_ERR_ARG;
    if (hist_indptr && hist_row_mode != PDA_HIST_BY_BLOCK_ROW && hist_row_mode != PDA_HIST_BY_USER_ID) return PDA_ERR_ARG;
    if (hist_indptr && hist_row_mode == PDA_HIST_BY_USER_ID && !users) return PDA_ERR_ARG;
    if ((long long)R * K > PDA_DEEP_MERGE_MAX_KEYS) return PDA_ERR_UNSUPPORTED;
    const size_t smem = deep_merge_smem(R, K);
    if (smem > 160 * 1024) return PDA_ERR_UNSUPPORTED;   // (not reached: 132 KB at R = 8 192, K = 1)
    static int attr_set = 0;
    if (!attr_set) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(&deep_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) !=
            hipSuccess)
            return PDA_ERR_LAUNCH;
        attr_set = 1;
    }
    const int vec = ((reinterpret_cast<uintptr_t>(in_keys) | reinterpret_cast<uintptr_t>(out_keys) | reinterpret_cast<uintptr_t>(out_idx) |
                      reinterpret_cast<uintptr_t>(out_val)) & 15u) == 0;
    DeepMergeArgs a{in_keys, out_keys, out_idx, out_val, users, hist_indptr, hist_indices, hist_row_mode, R, n_users_blk, K, vec};
    hipLaunchKernelGGL(deep_merge_kernel, dim3((unsigned)n_users_blk), dim3(kMergeThreads), smem, reinterpret_cast<hipStream_t>(stream), a);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}

extern "C" size_t pda_metrics_deep_workspace_bytes(int n_rows, int n_ks) {
    return (n_rows > 0 && n_ks > 0) ? (size_t)4 * n_ks * (size_t)((n_rows + 255) / 256) * 4 * sizeof(double) : 0;
}

extern "C" int pda_metrics_deep(const int32_t* topk, int n_rows, int k_cols, const int64_t* tgt_indptr, const int32_t* tgt_indices,
                                const int32_t* Ks, int n_ks, double* sums, void* workspace, void* stream) {
    if (!topk || !tgt_indptr || !tgt_indices || !Ks || !sums || n_rows <= 0 || n_ks <= 0) return PDA_ERR_ARG;
    if (k_cols < 1 || k_cols > PDA_DEEP_MAX_K) return PDA_ERR_ARG;
    const int n_blocks = (n_rows + 255) / 256;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (!workspace) {
        hipLaunchKernelGGL(metrics_deep_kernel<false>, dim3((unsigned)n_blocks), dim3(256), 0, s, topk, n_rows, k_cols, tgt_indptr, tgt_indices, Ks,
                           n_ks, sums);
        PDA_CHECK_LAUNCH();
        return PDA_OK;
    }
    double* partial = reinterpret_cast<double*>(workspace);
    hipLaunchKernelGGL(metrics_deep_kernel<true>, dim3((unsigned)n_blocks), dim3(256), 0, s, topk, n_rows, k_cols, tgt_indptr, tgt_indices, Ks,
                       n_ks, partial);
    PDA_CHECK_LAUNCH();
    hipLaunchKernelGGL(metrics_deep_sum_kernel, dim3((unsigned)(4 * n_ks)), dim3(256), 0, s, partial, 4 * n_blocks, sums);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
