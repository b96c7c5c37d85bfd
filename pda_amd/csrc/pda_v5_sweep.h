// The "huge" geometry of the sweep (round 4): sweep5_kernel -- included by pda_score_topk_v4.hip behind the shared device pieces.
//
// What generation 4's wide geometry is bound by: the chip is power-limited on the block loop, and what the MFMAs are fed
// from decides the clock -- one ds_read_b128 per two MFMAs 1 500 TFLOP/s executed, register operands 2 050.  And 1/9 of the MFMAs it
// executes (1/5 at d = 64) are the folded threshold test.  This geometry removes both (tools/ubench/mfma_struct5.hip measured the
// mapping first: 1 777 TFLOP/s, all of it algorithmic, against 1 364 algorithmic for the wide mapping on the same box):
//   * FOUR waves per workgroup, one per SIMD, 512 registers each; a wave owns 256 users, whose bf16 rows sit in AGPRs as eight MFMA
//     operands of 32 users (re-loaded from the user image at every entry of the asm loop: the
//     compiler spills into AGPRs between the statements) -- every item fragment read from the LDS feeds EIGHT MFMAs, and a 32-item half-tile is DMA-ed into the LDS
//     once per 1 024 users;
//   * the product is TRANSPOSED (A = item fragment, B = user fragment): an accumulator lane holds 16 items of ONE user, so the test
//     "could this pair reach the user's threshold" is a per-lane compare of the lane's maximum (VALU in the MFMA shadow) -- no test k-step;
//   * the item image is PRE-SCALED by the popularity: i' = pop * i, so that for s > 0 the head (s + 1) pop = u . i' + pop, and the
//     per-item terms (pop, the bf16 error bound eps ||u|| ||i'||) are replaced by their maxima over the 32-item half-tile (pmax, nmax:
//     8 bytes of meta per half-tile; in visiting order the popularities of a half-tile are all but equal):
//         flag  <=>  max(max_i s~'(u, i) + pmax + eps_w nmax, pmax) > thr'(u)         (eps_w = eps x the wave's largest ||u||)
//     which is implied by "some pair of the half-tile has an exact head >= the user's K-th value" (s <= 0: the head is <= pop <= pmax);
//   * no loader and no rescoring waves: the MFMA waves issue the LDS-DMA themselves (two 1 KiB pieces per wave and half-tile at
//     d = 128) and run in step, one s_barrier per half-tile; when a half-tile raised a flag in any of them, all four leave their asm
//     loop together, score that half-tile (and the one behind it) again with compiler-visible MFMAs, rescore the candidates exactly
//     (the fp32 chain of the oracle, generation 4's lists and compaction) and re-enter.  In a dense sweep in visiting order that is a
//     fraction of a candidate per user behind the exact warm-up.
//   * TWO loop bodies (tools/gen_v6_loop_asm.py): the tested one above, and a TEST-FREE one (Loop6Free::run) for the half-tiles behind
//     the workgroup's DECIDED half-tile -- the first from which the suffix bound of the visiting order (Args4::tailA / tailB: the maxima
//     of |pop| and |pop| ||i|| over everything at or behind a 64-item tile) lies below every threshold of the workgroup:
//         fmaf(nw, tailB[T], tailA[T]) * 1.000002f < tw      (nw: the largest padded norm, tw: the lowest lowered threshold of its rows)
//     -- the criterion that ENDS generation 4's early-terminating sweeps.  Behind it the outcome of every threshold test is known to be
//     "no flag"; a dense sweep goes on scoring (the same LDS-DMA pieces, fragment reads, barrier per half-tile and MFMAs on the same
//     operands: tiles_scored counts them as before) without the maxima, compares, clamp, publish, flag word, meta entry and ct.  The
//     decided half-tile is worked out at every (re-)entry from the thresholds as they are then (they only rise); the tested body gets it as
//     its end, so every flag below it has been acted on when it returns, and Loop6Free::run takes over from there to the end of the split.
//     In config 3 that is 94 % of the half-tiles (workspace + 28 counts them: stats["huge_free_halftiles"]).  -DPDA_V5_NO_FREE: never.
//     The test-free range is run at the END of the kernel, behind the workgroup's rows, in chunks claimed from a record that the other
//     workgroups claim from as well once they have nothing left of their own (pda_tail_share.h; the comment at next_chunk below).
// Everything else is generation 4's: warm4_kernel's exact lists (handed over through the workspace), the packed keys, the epilogue.
// Popularity head, d = 64 / 128, dense sweeps (no early termination); selected by the caller's hint PDA_SWEEP_HUGE.
#pragma once
#ifdef PDA_V6_LOOP_HEADER
#include PDA_V6_LOOP_HEADER
#else
#include "pda_v6_loop_asm.h"           // the loop, on v_mfma_f32_16x16x32_bf16 (tools/gen_v6_loop_asm.py)
#endif
#include "pda_v6_free_asm.h"           // its test-free bodies (tools/gen_v6_loop_asm.py --free: made by the Makefile, not kept in the repository)
#include "pda_tail_share.h"            // the shared test-free tail: claim / publish over one atomic word per workgroup (host-compilable)

#ifdef PDA_V5_EXITPROF
// profiling build (tools/build_variant.sh exitprof -DPDA_V5_EXITPROF; read by tools/time_huge_exits.py): what a wave spends OUTSIDE its asm loops,
// in ticks of the constant 100 MHz wall clock -- per (workgroup, wave): [0] in extract, [1] in rescore_ring behind the extracts, [2] from the end
// of an exit's work to the next call of a loop body (thresholds, the decided half-tile, the barrier; the AGPR reload and the restart of the DMA
// pipeline happen inside the asm statement and are not separable here), [3] everything between a loop's return and the next loop's call,
// [4] exits (returns with a flag), [5] the whole kernel (work for other workgroups included), [6] before the first entry, [7] sort and emit,
// [8] the workgroup's decided half-tile (the half-tile at which it went test-free), [9] the wall clock, from the kernel's start, at which it
// entered the test-free body, [10] half-tiles run for other workgroups, [11] the half-tiles of its split.  No code in the product build.
// pda_v5_tail_pieces (pda_debug_v5_tail_pieces): n > 0 -- every workgroup runs its own test-free range in n equal pieces, nobody shares.
constexpr int kXpMaxWg = 4096, kXpWords = 12;
__device__ unsigned long long pda_v5_exitprof[kXpMaxWg * 4 * kXpWords];
__device__ int pda_v5_tail_pieces;
#define XP(...) __VA_ARGS__
#else
#define XP(...)
#endif
constexpr int kRing5 = 192;           // candidate ring entries per wave (u64 each); a push needs 64 free



// UPW users per wave: 256 -- one 1 024-user workgroup per CU, 512 registers per wave; d = 256: 128 (the rows of 128 users fill the 256 AGPRs).
// With one wave per SIMD nothing overlaps the wave's own VALU tests, LDS reads and scalar work with its MFMAs (PMC: matrix pipe 77 % busy at
// 2.03 GHz, 87 % without the tests).  Round 4 measured the two obvious alternatives and round 5 removed them (profiles/round4_huge_variants.txt,
// profiles/README.md): two 512-user workgroups per CU at d <= 128 -- the pipe 82 % busy, but at 1.86 GHz: twice the LDS reads and LDS-DMA per
// MFMA cost more clock than the overlap buys (8.38 vs 8.18 ms) -- and the loop on v_mfma_f32_32x32x16_bf16 (9.16 ms).
template <int D, bool BF, bool S16, int UPW>
__global__ void __launch_bounds__(256, 1) sweep5_kernel(Args4 g) {
    static_assert(slot_bytes5(D) == Loop6<D, 8>::kSlotBytes, "one LDS image for all loops");
    static_assert(S16, "the loop on v_mfma_f32_32x32x16_bf16 (round 4's first form: 9.16 against 8.07 ms, profiles/README.md) left with round 5; the parameter keeps the kernel's name");
    static_assert((D <= 128 && UPW == 256) || (D == 256 && UPW == 128), "users per wave: 256, or (d = 256) 128 -- 8 blocks x 8 k-steps = 256 AGPRs, one 512-user workgroup per CU");
    // NK k-steps per product, NU user blocks of UBW = 16 users per wave (16 x 16 x 32 MFMAs)
    constexpr int NK = D / 32, UBW = 16, NU = UPW / UBW;
    constexpr int SS = slot_bytes5(D), UT = 4 * UPW, CAPL = kCap4, RB4 = row_bytes(D);
    constexpr int LPC = D / 32, CPP = 64 / LPC;                          // lanes per candidate, candidates per rescoring pass
    constexpr float kEps5 = BF ? 4.0234375e-3f : 8.046875e-3f;           // 2^-8 x 1.03 (only the scaled items are rounded: one unit roundoff of bf16)  |  2^-7 x 1.03 (both sides)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* tiles = smem;                                         // kNSlot5 x SS (at LDS address 0: the loop XORs fragment offsets into slot addresses)
    int* cntl = reinterpret_cast<int*>(smem + kNSlot5 * SS);            // [UT]
    float* taul = reinterpret_cast<float*>(cntl + UT);                   // [UT]
    uint64_t* crings = reinterpret_cast<uint64_t*>(taul + UT);           // [4][kRing5]  (user row of the wave << 32 | visiting position)
    unsigned* sync = reinterpret_cast<unsigned*>(crings + 4 * kRing5);   // [2] the shared flag words, one per half-tile parity (pda_v5_loop_asm.h)
    unsigned* s_uns = sync + 8;                                          // [32] one bit per user row: its list came in unsorted
    unsigned* touched = sync + 40;                                       // [32] one bit per user row: the sweep appended to its list
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int split = blockIdx.x % g.n_splits, utile = blockIdx.x / g.n_splits;
    XP(unsigned long long xp[kXpWords] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; const unsigned long long xp_k0 = wall_clock64(); unsigned long long xp_out = 0, xp_re = 0;)
    // the exact lists: the hand-over rows of the warm-up IN PLACE (a one-call sweep; the rows of the workgroup's padding do not exist
    // and are never touched: no candidate, no output), else the workgroup's rows of the workspace
    uint64_t* lists = g.handover != nullptr ? g.handover + ((size_t)split * g.n_users_blk + (size_t)utile * UT) * kCap4
                                            : g.lists_ws + (size_t)blockIdx.x * UT * CAPL;
    const int K = g.K;
    const int nt = split_tiles(g.n_tiles, split, g.n_splits);
    const int wt = warm_tiles_of(g, split);                              // the split's tiles the warm-up has scored
    const bool starts_empty = g.lists_empty || (g.warm_shared && split > 0);   // shared warm-up: its lists went to split 0; this split has the seed and empty lists
    const bool warm_final = g.warm_final && !starts_empty;               // (an empty split writes every row of its out_keys itself)
    const int n_it = max(0, nt - wt);                                    // 64-item tiles behind the warm-up
    const unsigned hend = 2u * (unsigned)n_it;                           // 32-item half-tiles
    // (words 0, 1: the shared flag words; 8 .. 39: every list comes in unsorted -- unless the warm-up sorted them: warm_final; 40 .. 71: no row touched)
    if (tid < 72) sync[tid] = (tid < 8 || tid >= 40 || warm_final || starts_empty) ? 0u : 0xFFFFFFFFu;
    // kernel identity (workspace + 16): generation 4 | geometry (4: the 16 x 16 x 32 loop, one 1 024-user workgroup per CU; 6: the same, two 512-user workgroups; 5: the 32 x 32 x 16 loop) << 8 | head << 13 | bf16 tables << 14 | d / 64
    if (tid == 0 && blockIdx.x == 0) g.stats[4] = (4u << 28) | (4u << 8) | (1u << 13) | ((BF ? 1u : 0u) << 14) | (unsigned)(D >> 6);
    // ---- the counts and K-th values of the warm-up's lists -> LDS (all waves); without a hand-over buffer the lists themselves -> the workspace
    if (starts_empty) {
        for (int rr = tid; rr < UT; rr += 256) {
            cntl[rr] = 0;
            taul[rr] = utile * UT + rr < g.n_users_blk ? -INFINITY : INFINITY;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    } else if (warm_final && g.kth_ws != nullptr) {
        // sorted rows of at most K keys in out_keys (warm4_kernel) and their K-th values, read as one run of floats: a LANE per row -- the value
        // says everything (-inf: fewer than K keys, or K keys down to -inf; count them).  A row reaches the list slots when it is appended to.
        for (int rr = tid; rr < UT; rr += 256) {
            const int rb = utile * UT + rr;
            int c = 0;
            float tau = INFINITY;
            if (rb < g.n_users_blk) {
                tau = g.kth_ws[(size_t)split * g.n_users_blk + rb];
                c = K;
                if (tau == -INFINITY) {
                    const uint64_t* row = g.out_keys + ((size_t)split * g.n_users_blk + rb) * K;
                    for (c = 0; c < K && row[c] != 0ull; ++c) {}
                }
            }
            cntl[rr] = c;
            taul[rr] = tau;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    } else if (warm_final) {
        // sorted lists of at most K keys (warm4_kernel): a LANE per row -- its K-th key says everything (0: fewer than K keys; count them)
        for (int rr = tid; rr < UT; rr += 256) {
            const int rb = utile * UT + rr;
            int c = 0;
            float tau = INFINITY;
            if (rb < g.n_users_blk) {
                const uint64_t kl = lists[(size_t)rr * CAPL + (K - 1)];
                c = K;
                tau = pda_unordf((uint32_t)(kl >> 32));
                if (kl == 0ull) {
                    tau = -INFINITY;
                    for (c = 0; c < K - 1 && lists[(size_t)rr * CAPL + c] != 0ull; ++c) {}
                }
            }
            cntl[rr] = c;
            taul[rr] = tau;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    } else
    {
        constexpr int NW = 4, PB = 8;
        for (int r0 = wave; r0 < UT; r0 += PB * NW) {
            uint64_t keyv[PB];
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                const int rr = r0 + q * NW, rb = utile * UT + rr;
                keyv[q] = (rr >= UT || rb >= g.n_users_blk) ? 0ull
                          : g.handover != nullptr ? (lane < kCap4 ? g.handover[((size_t)split * g.n_users_blk + rb) * kCap4 + lane] : 0ull)
                          : (lane < K ? g.out_keys[((size_t)split * g.n_users_blk + rb) * K + lane] : 0ull);
            }
#pragma unroll
            for (int q = 0; q < PB; ++q) {
                const int rr = r0 + q * NW;
                if (rr >= UT) break;
                const int rb = utile * UT + rr;
                const uint64_t key = keyv[q];
                const int c = __popcll(__ballot(key != 0ull));
                if (g.handover == nullptr && lane < K) lists[(size_t)rr * CAPL + lane] = key;
                uint32_t mn = key != 0ull ? (uint32_t)(key >> 32) : 0xFFFFFFFFu;
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) mn = min(mn, (uint32_t)__shfl_xor((int)mn, o, 64));
                if (lane == 0) {
                    cntl[rr] = c;
                    taul[rr] = rb < g.n_users_blk ? (c >= K ? pda_unordf(mn) : -INFINITY) : INFINITY;
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    }
    __syncthreads();

    // ---- the shared test-free tail (pda_tail_share.h).  Behind a workgroup's decided half-tile the loop only scores: no
    // accumulator is read, nothing is written, and the operands are the item image and the workgroup's user image -- WHICH CU runs such a
    // half-tile changes no result -- nor does WHEN: a workgroup that reaches its test-free part publishes the range in its record, rescores
    // what its rings hold and emits its rows, and only then claims the range back chunk by chunk; when its own record is exhausted it claims
    // chunks from the record with the most left and runs them on the victim's user image and tile sequence.  (One place, at the end of the
    // kernel, runs every test-free half-tile: nothing of the tested part is live there.)  Nobody waits for anybody: no spin, no barrier
    // across workgroups; the owner finishes whatever nobody took.
    unsigned* bcast = sync + 80;                                         // [3] a claim, from wave 0 to all four: they must run the same chunk
    uint64_t* const my_rec = g.tail_rec != nullptr ? g.tail_rec + blockIdx.x : nullptr;
    const unsigned lane16 = (unsigned)lane * 16u;
    const unsigned ring_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)tiles;
    unsigned tail_fixed = 0;                                             // (profiling build: the size of a piece)
    unsigned own_a = 0, own_b = 0;                                       // the workgroup's decided range [own_a, own_b) of local half-tiles; empty: none
    // the next chunk: own = from this workgroup's record (first: its first claim), else from the other record with the most left.
    // One thread claims; false: nothing left there.
    auto next_chunk = [&](bool own, bool first, unsigned& vb, unsigned& a, unsigned& b) __attribute__((always_inline)) -> bool {
        if (wave == 0) {
            unsigned ca = 0, cb = 0, cv = blockIdx.x;
            if (own) {
                if (lane == 0 && !pda_ts_claim(my_rec, first, g.tail_min, tail_fixed, ca, cb)) ca = cb = 0;
            } else {
                // (a record seen with something left and found exhausted by the claim stays exhausted: at most one failure per record)
                for (;;) {
                    unsigned long long key = pda_ts_pick(g.tail_rec, gridDim.x, blockIdx.x, (unsigned)lane, 64u);
#pragma unroll
                    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long k2 = __shfl_xor(key, o, 64); key = k2 > key ? k2 : key; }
                    if ((key >> 32) == 0ull) break;
                    bool ok = false;
                    if (lane == 0) ok = pda_ts_steal(g.tail_rec, key, g.tail_min, cv, ca, cb);
                    if (__any(ok)) break;
                    ca = cb = 0;
                }
            }
            if (lane == 0) { bcast[0] = ca; bcast[1] = cb; bcast[2] = cv; }
        }
        __syncthreads();
        a = (unsigned)__builtin_amdgcn_readfirstlane((int)bcast[0]);
        b = (unsigned)__builtin_amdgcn_readfirstlane((int)bcast[1]);
        vb = (unsigned)__builtin_amdgcn_readfirstlane((int)bcast[2]);
        __syncthreads();
        return a < b;
    };

    unsigned n_cand = 0;
    if (hend > 0) {
        const int row0 = wave * UPW;                                     // this wave's user rows of the workgroup
        const int j = lane & (UBW - 1), hh = lane / UBW;               // the lane's user of a block; its 8-element group of a fragment's k-range
        const unsigned char* my_ufrag = g.ufrag + ((size_t)utile * 4 + wave) * (size_t)(NU * NK * 1024);
        // the wave's largest padded ||u||, the external seeds and the history bounds of the lane's users (block u: row UBW u + j)
        float eu = 0.f, seedv[NU];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const int rb = utile * UT + row0 + UBW * u + j;
            eu = fmaxf(eu, rb < g.n_users_blk ? g.unorm[rb] : 0.f);
            seedv[u] = (g.seed != nullptr && rb < g.n_users_blk) ? g.seed[rb] : -INFINITY;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) eu = fmaxf(eu, __shfl_xor(eu, o, 64));
        const float numax = eu;                                          // the wave's largest padded ||u|| (the decided half-tile)
        eu = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(eu * (kEps5 * 1.001f))));       // eps x the wave's largest ||u||, wave-uniform
        const unsigned flags_lds = (unsigned)(size_t)(__attribute__((address_space(3))) unsigned char*)reinterpret_cast<unsigned char*>(sync);
        uint64_t* my_ring = crings + wave * kRing5;
        unsigned ring_n = 0;                                             // wave-uniform: entries in my_ring
        const unsigned t0 = (unsigned)(split + wt * g.n_splits);
        const size_t img = (size_t)g.rows5, meta = (size_t)g.meta5;
        const bool hist_on = g.hist_indptr != nullptr;
        const bool lazy_rows = warm_final && g.kth_ws != nullptr;

        // the lowered threshold of the lane's user of block u: strictly below the exact K-th value (ties must pass) and below the fp32
        // roundings between the bound and the rescored head; +-1e30 stand for +-inf
        auto thr_of = [&](int u) __attribute__((always_inline)) -> float {
            const float tq = fmaxf(taul[row0 + UBW * u + j], seedv[u]);
            float tf = (tq == INFINITY || tq == -INFINITY) ? tq : tq - fabsf(tq) * 1.52587890625e-5f - 1e-30f;
            return fminf(fmaxf(tf, -1.0e30f), 1.0e30f);
        };
        // ---- exact rescoring of the ring's candidates: the fp32 chain of the oracle (oracle/pda_oracle.c dot_chain; sweep4_kernel's
        // interleaved row loads), the train-item check, the append.  CPP candidates per pass, LPC lanes each.
        auto rescore_ring = [&]() __attribute__((always_inline)) {
            const int q = lane % LPC, ci = lane / LPC;
            for (unsigned base = 0; base < ring_n; base += CPP) {
                const bool have = base + (unsigned)ci < ring_n;
                const uint64_t e = have ? my_ring[base + ci] : 0ull;
                const int row = (int)(e >> 32);
                const unsigned pos = (unsigned)e;
                bool valid = have && pos < (unsigned)g.n_items_local;
                const unsigned char* tail = g.rows + (size_t)(valid ? pos : 0u) * RB4 + 2 * D + 32;
                const float pv = *reinterpret_cast<const float*>(tail);
                const int loc = *reinterpret_cast<const int*>(tail + 4);
                const int rb = utile * UT + row0 + row;
                valid = valid && rb < g.n_users_blk;
                const int uid = valid ? g.users[rb] : 0;
                const float c_sd = (g.seed != nullptr && valid) ? g.seed[rb] : -INFINITY;
                const float c_tau = taul[row0 + (valid ? row : 0)];
                f32x4 uu[8], ii[8];
                // d <= 128: lane q holds chunks LPC cq + q (interleaved: a cache line per candidate and load); d = 256: its 32 consecutive elements
                const size_t ub = (size_t)uid * D + q * (LPC == 8 ? 32 : 8), ib = (size_t)(valid ? loc : 0) * D + q * (LPC == 8 ? 32 : 8);
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const int off = LPC == 8 ? 4 * c : 8 * LPC * (c >> 1) + 4 * (c & 1);
                    uu[c] = pda_load4<BF>(g.U, ub + off);
                    ii[c] = pda_load4<BF>(g.I, ib + off);
                }
                long long hb = 0, he = 0;
                if (hist_on && valid) {
                    const int64_t hr = g.hist_row_mode == PDA_HIST_BY_USER_ID ? (int64_t)uid : (int64_t)rb;
                    hb = g.hist_indptr[hr];
                    he = g.hist_indptr[hr + 1];
                }
                auto fma8 = [&](float acc, int cq) __attribute__((always_inline)) -> float {
#pragma unroll
                    for (int sidx = 0; sidx < 4; ++sidx) {
                        acc = __builtin_fmaf(uu[2 * cq][sidx], ii[2 * cq][sidx], acc);
                        acc = __builtin_fmaf(uu[2 * cq + 1][sidx], ii[2 * cq + 1][sidx], acc);
                    }
                    return acc;
                };
                float o = 0.f, o_other = 0.f;
                if constexpr (LPC == 8) {
                    // d = 256: chunk x = 4 q + cc of the row feeds chain x & 1, the chunks of a chain in ascending order: the two chains
                    // travel from lane to lane (sweep4_kernel's rows that are not interleaved)
                    float c0 = 0.f, c1 = 0.f, o0 = 0.f, o1 = 0.f;
#pragma unroll
                    for (int ph = 0; ph < LPC; ++ph) {
                        o0 = c0;
                        o1 = c1;
#pragma unroll
                        for (int cc = 0; cc < 4; ++cc) {
#pragma unroll
                            for (int sidx = 0; sidx < 4; ++sidx) {
                                if (cc & 1) {
                                    o1 = __builtin_fmaf(uu[2 * cc][sidx], ii[2 * cc][sidx], o1);
                                    o1 = __builtin_fmaf(uu[2 * cc + 1][sidx], ii[2 * cc + 1][sidx], o1);
                                } else {
                                    o0 = __builtin_fmaf(uu[2 * cc][sidx], ii[2 * cc][sidx], o0);
                                    o0 = __builtin_fmaf(uu[2 * cc + 1][sidx], ii[2 * cc + 1][sidx], o0);
                                }
                            }
                        }
                        if (ph < LPC - 1) {
                            const float r0 = __shfl_up(o0, 1, 64), r1 = __shfl_up(o1, 1, 64);
                            if (q == ph + 1) {
                                c0 = r0;
                                c1 = r1;
                            }
                        }
                    }
                    o = o1;
                    o_other = o0;
                } else if constexpr (LPC == 4) {
                    const bool hi = q >= 2;
                    auto swap2 = [](float x) __attribute__((always_inline)) -> float {
                        return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(x), 0x4E, 0xF, 0xF, true));  // quad_perm [2,3,0,1]
                    };
#pragma unroll
                    for (int cq = 0; cq < 4; ++cq) {
                        const float a = fma8(o, cq);
                        const float a_sw = swap2(a);
                        const float b = fma8(hi ? a_sw : o, cq);
                        const float b_sw = swap2(b);
                        o = hi ? b : b_sw;
                    }
                } else {
                    static_assert(LPC == 2, "d = 64");
#pragma unroll
                    for (int cq = 0; cq < 4; ++cq) o = fma8(o, cq);
                }
                const float o0 = LPC == 8 ? o_other : __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(o), 0xB1, 0xF, 0xF, true));            // quad_perm [1,0,3,2]
                float sc = o0 + o;                                  // meaningful on the candidate's last lane
                sc = (sc > 0.0f ? sc + 1.0f : __expf(sc)) * pv;
                const float tt = (valid && q == LPC - 1) ? sc : -INFINITY;
                const int item = g.item_offset + loc;
                bool p = valid && q == LPC - 1 && (tt >= fmaxf(c_tau, c_sd));
                if (hist_on && p) {                                 // train items are masked here: a binary search in the row's id-sorted history
                    long long lo = hb, hi2 = he;
                    while (lo < hi2) {
                        const long long mid = (lo + hi2) >> 1;
                        if (g.hist_indices[mid] < item) lo = mid + 1; else hi2 = mid;
                    }
                    if (lo < he && g.hist_indices[lo] == item) p = false;
                }
                const uint64_t key = pda_pack_key(tt, (uint32_t)item);
                bool first = false;                                 // this lane's append is the first to its row
                if (p) first = (atomicOr(&touched[(row0 + row) >> 5], 1u << ((row0 + row) & 31)) & (1u << ((row0 + row) & 31))) == 0u;
                if (lazy_rows) {
                    // the warm-up's row still sits in out_keys only: into the row's list slots before the first append (rows belong to one wave;
                    // of several lanes on one untouched row the atomic names one)
                    uint64_t need = __ballot(first);
                    if (need != 0ull) {
                        while (need != 0ull) {
                            const int lr = row0 + __builtin_amdgcn_readlane(row, __builtin_ctzll(need));
                            need &= need - 1ull;
                            const int c_r = cntl[lr];
                            if (lane < c_r) lists[(size_t)lr * CAPL + lane] = g.out_keys[((size_t)split * g.n_users_blk + (size_t)(utile * UT + lr)) * K + lane];
                        }
                        list_sync<true>();
                    }
                }
                append_keys<CAPL, true>(p, row0 + row, tt, key, lists, cntl, taul, row0, UPW, K, lane, s_uns);
            }
            n_cand += ring_n;
            ring_n = 0;
        };
        // ---- the two half-tiles behind an exit at half-tile hx (hx - 2 raised the flag, the flags of hx - 1 were still being worked out), scored
        // again with compiler-visible MFMAs in ONE pass over the user blocks: every pair whose bound reaches the user's threshold -> the ring.
        // With one wave per SIMD nothing hides a round trip to the user image (the rows cannot stay in AGPRs across the asm statements), and a pass
        // per half-tile over one block at a time was 2 NU exposed round trips per exit: here both half-tiles' item fragments are read from their LDS
        // slots once (d >= 128: once per batch), a block's user fragments are loaded once for both, and the blocks come in batches of BU whose loads are all in flight together
        // (64 VGPRs of fragments), the next batch requested behind the last MFMA of the current one, over its pushes -- NU / BU waits.
        // (Two batches in flight -- the next one requested BEFORE the current one's MFMAs -- cost 120 - 430 bytes of scratch per lane at d >= 128;
        // with a batch's MFMAs at a quarter of a round trip, more loads per wait beat the overlap anyway.)  The thresholds are read once per batch:
        // a rescoring inside the batch may have raised one since, which only sends a pair to the exact rescoring that the old path would have
        // dropped (keys cannot change).  A batch's masks travel as one 64-bit word per lane to a rolled loop of pushes: one copy of the push code
        // (and of rescore_ring) instead of one per block.
        auto extract2 = [&](unsigned hx, unsigned hl) __attribute__((always_inline)) {     // hl: hlim, the end handed to the tested body
            // (below hl: what the tested body scored behind its end are copies of half-tile hl - 1)
            const bool on0 = hx >= 2u && hx - 2u < hl, on1 = hx >= 1u && hx - 1u < hl;
            if (!on0 && !on1) return;
            constexpr int NR = 8, BU = D == 256 ? 2 : 4, NB = NU / BU, NF = BU * NK;
            static_assert(NU % BU == 0 && 2 * BU * NR <= 64, "the masks of a batch: one 64-bit word per lane");
            // an absent half-tile is stood in for by the present one (valid addresses; its masks are dropped)
            const unsigned f0 = on0 ? hx - 2u : hx - 1u, f1 = on1 ? hx - 1u : hx - 2u;
            // accumulator register r of the lane <-> item of the half-tile (r = 4 ib + register of chain ib)
            auto item_of = [&](int r) __attribute__((always_inline)) -> unsigned {
                return 16u * (r >> 2) + 4u * hh + (r & 3);
            };
            unsigned pos00 = 0, pos01 = 0;                               // visiting position of each half-tile's first item
            float ctv[2], pmx[2];
            const unsigned char* tbv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const unsigned ft = t ? f1 : f0;
                const unsigned T = t0 + (ft >> 1) * (unsigned)g.n_splits;                   // its 64-item tile
                if (t) pos01 = T * 64u + (ft & 1u) * 32u; else pos00 = T * 64u + (ft & 1u) * 32u;
                const float2 mt = *reinterpret_cast<const float2*>(g.meta5 + 4 * (size_t)(2u * T + (ft & 1u)));
                ctv[t] = __builtin_fmaf(eu, mt.y, mt.x);
                pmx[t] = mt.x;
                tbv[t] = tiles + (ft & (kNSlot5 - 1)) * SS + j * (2 * D);
            }
            // a half-tile's item fragments: 8 NK VGPRs.  d = 64: both half-tiles' stay in registers for the whole pass; d >= 128 (32 / 64 VGPRs
            // each): one at a time, read from its LDS slot again for every batch (a fraction of the batch's round trip to the user image) -- both
            // at once cost sweep5_kernel<128> 120 bytes of scratch per lane
            constexpr bool AF_ONCE = D == 64;
            u32x4 af[AF_ONCE ? 2 : 1][2 * NK];
            auto load_af = [&](int t) __attribute__((always_inline)) {
#pragma unroll
                for (int ib = 0; ib < 2; ++ib)
#pragma unroll
                    for (int k = 0; k < NK; ++k)
                        af[AF_ONCE ? t : 0][ib * NK + k] = *reinterpret_cast<const u32x4*>(tbv[t] + ib * 16 * (2 * D) + (((4 * k + hh) ^ swz5<D>(j)) << 4));
            };
            // the fragments of batch b: blocks BU b .. BU b + BU - 1, NK k-steps each -- NF consecutive 1 KiB fragments of the wave's image
            // (addresses: a uniform base per batch, the lane's 32-bit offset per 4 KiB and an immediate.  The offset passes through an empty asm
            // statement: formed from the loop-invariant lane16 alone, the 14 per-lane 64-bit addresses were hoisted out of the sweep's loop, over
            // the asm loops, and spilled -- 112 bytes of scratch per lane)
            unsigned l16 = lane16;
            asm volatile("" : "+v"(l16));
            u32x4 cur[NF];
            auto load_cur = [&](int b) __attribute__((always_inline)) {
                const unsigned char* pb = my_ufrag + (size_t)b * (NF * 1024);
#pragma unroll
                for (int i = 0; i < NF; ++i) cur[i] = *reinterpret_cast<const u32x4*>(pb + (size_t)(l16 + (unsigned)(i >> 2) * 4096u) + (i & 3) * 1024);
            };
            if constexpr (AF_ONCE) {
                load_af(0);
                load_af(1);
            }
            load_cur(0);
#pragma unroll 1
            for (int b = 0; b < NB; ++b) {
                float tlv[BU];
#pragma unroll
                for (int ub = 0; ub < BU; ++ub) tlv[ub] = thr_of(b * BU + ub);
                uint64_t mm = 0ull;
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    if constexpr (!AF_ONCE) load_af(t);
#pragma unroll
                    for (int ub = 0; ub < BU; ++ub) {
                        const float tl = tlv[ub];
                        const bool clampy = pmx[t] > tl;
                        uint32_t m = 0;
#pragma unroll
                        for (int ib = 0; ib < 2; ++ib) {
                            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                            for (int k = 0; k < NK; ++k)
                                acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[AF_ONCE ? t : 0][ib * NK + k]), __builtin_bit_cast(bf16x8, cur[ub * NK + k]), acc, 0, 0, 0);
#pragma unroll
                            for (int r = 0; r < 4; ++r) m |= (acc[r] + ctv[t] > tl) ? (1u << (4 * ib + r)) : 0u;
                        }
                        if (__any(clampy)) {
                            // (rare: a user whose threshold lies below a popularity of this half-tile -- a head pop x exp(s), s <= 0, may qualify)
#pragma unroll
                            for (int r = 0; r < NR; ++r) {
                                const unsigned pp = (t ? pos01 : pos00) + item_of(r);
                                const float pi = clampy ? *reinterpret_cast<const float*>(g.rows + (size_t)pp * RB4 + 2 * D + 32) : 0.f;
                                m |= (clampy && pi > tl) ? (1u << r) : 0u;
                            }
                        }
                        if (!(t ? on1 : on0)) m = 0u;
                        mm |= (uint64_t)m << (NR * (2 * ub + t));
                    }
                }
                // (the fragments are consumed: the next batch's loads travel over the pushes below)
                const int bn = min(b + 1, NB - 1);
                if (b + 1 < NB) load_cur(bn);
                if (__any(mm != 0ull)) {
#pragma unroll 1
                    for (int q = 0; q < 2 * BU; ++q) {                   // (block q >> 1 of the batch, half-tile q & 1)
                        uint32_t m = (uint32_t)(mm >> (NR * q)) & ((1u << NR) - 1u);
                        const int u = b * BU + (q >> 1);
                        const unsigned pos0 = (q & 1) ? pos01 : pos00;
                        while (__any(m != 0u)) {
                            if (ring_n + 64u > (unsigned)kRing5) {
                                // (a full ring in mid-pass, rare: the fragments are not carried across the rescoring -- 64 VGPRs of table rows -- but
                                // read again behind it)
                                rescore_ring();
                                if constexpr (AF_ONCE) {
                                    load_af(0);
                                    load_af(1);
                                }
                                load_cur(bn);
                            }
                            const bool act = m != 0u;
                            const int r = __builtin_ctz(m | 0x10000u);
                            m &= ~(1u << r);
                            const uint64_t pm = __ballot(act);
                            const unsigned slot = ring_n + (unsigned)__builtin_amdgcn_mbcnt_hi((uint32_t)(pm >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)pm, 0));
                            if (act) my_ring[slot] = ((uint64_t)(unsigned)(UBW * u + j) << 32) | (uint64_t)(pos0 + item_of(r));
                            ring_n += (unsigned)__popcll(pm);
                        }
                    }
                }
            }
        };

        // ---- the workgroup's DECIDED half-tile: the first local half-tile from which no pair of the rest of the split can reach ANY row's
        // threshold -- the criterion that ends generation 4's early-terminating sweeps (stop_predict4_kernel, the votes of sweep4_kernel),
        //     fmaf(nu, tailB[T], tailA[T]) * 1.000002f < tau        (T: the 64-item tile of the whole visiting order, conservative for a split)
        // taken once per workgroup on (nw: the largest padded norm of its rows, tw: its lowest LOWERED threshold -- below the exact one,
        // +1e30 for the rows of the padding, -1e30 while a list is shorter than K: never).  The suffix maxima fall along the order: a binary
        // search.  Every operand is workgroup-uniform, so the four waves agree; thresholds only rise, so a value stays valid and a later
        // one is at most as large.
        auto decided = [&](float tw, float nw, unsigned h_now) __attribute__((always_inline)) -> unsigned {
#ifdef PDA_V5_NO_FREE
            return hend;                                                 // A/B build: every half-tile is tested (tools/build_variant.sh nofree -DPDA_V5_NO_FREE)
#else
            if (g.tailA == nullptr || !(tw > -1.0e30f)) return hend;
            // the first tile of [lo, hi) at which the predicate holds (hi: none).  The predicate is monotone along the order (the suffix
            // maxima fall, nw >= 0), so instead of a bisection -- a dependent pair of loads per step, twelve at config 3 -- the 64 lanes
            // probe up to 64 evenly spaced tiles per round with independent loads: the first lane that holds brackets the answer, and
            // two or three rounds end at the same tile
            int lo = (int)(h_now >> 1), hi = n_it;
            while (lo < hi) {
                const int n = hi - lo, step = (n + 63) >> 6, p = lo + lane * step;
                bool ok = false;
                if (p < hi) {
                    const size_t T = (size_t)t0 + (size_t)p * (size_t)g.n_splits;
                    ok = __builtin_fmaf(nw, g.tailB[T], g.tailA[T]) * 1.000002f < tw;
                }
                const uint64_t m = __ballot(ok);
                if (m == 0ull) {
                    lo += (n - 1) / step * step + 1;                     // behind the last probe
                } else {
                    const int f = __builtin_ctzll(m);
                    hi = lo + f * step;
                    lo = f > 0 ? hi - step + 1 : hi;
                }
                lo = __builtin_amdgcn_readfirstlane(lo);
                hi = __builtin_amdgcn_readfirstlane(hi);
            }
            return 2u * (unsigned)lo;
#endif
        };
        float* xch = reinterpret_cast<float*>(sync + 72);                // [8] the waves' lowest thresholds and largest norms
        unsigned h = 0, issued = 0, n_entries = 0;
        unsigned hlim = hend;            // the end handed to the tested body: what it issued for half-tiles >= hlim are clamped copies
        bool hend_ok = true;
        if ((ring_lds & (D == 256 ? 511u : 255u)) != 0u) { if (lane == 0) g.stats[0] = 6u; hend_ok = false; }      // (the slots must start at multiples of 256 / 512)
        for (unsigned guard = 0; hend_ok && guard < 2u * hend + 8u; ++guard) {
            float thr[NU];
#pragma unroll
            for (int u = 0; u < NU; ++u) thr[u] = thr_of(u);
            unsigned reason = 0;
            // the wave's lowest threshold: the clamp test (a popularity of the half-tile above a user's threshold) is wave-uniform
            float tmin = thr[0];
#pragma unroll
            for (int u = 1; u < NU; ++u) tmin = fminf(tmin, thr[u]);
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) tmin = fminf(tmin, __shfl_xor(tmin, o, 64));
            tmin = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(tmin)));
            // the workgroup's decided half-tile, from the thresholds as they are now (all four waves are here: every flag raised so far has
            // been acted on, nobody reads a slot)
            if (lane == 0) { xch[wave] = tmin; xch[4 + wave] = numax; }
            __syncthreads();
            const float tw = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fminf(fminf(xch[0], xch[1]), fminf(xch[2], xch[3])))));
            const float nw = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(fmaxf(fmaxf(xch[4], xch[5]), fmaxf(xch[6], xch[7])))));
            const unsigned hf = decided(tw, nw, h);
            if (h >= min(hlim, hf)) {
                // ---- the rest of the split, test-free.  The tested body runs two half-tiles past the end it was given, on clamped copies:
                // back to that end, and whatever it issued from there on is issued again (Loop6Free::run catches up at entry)
                if (h > hlim) h = hlim;
                if (issued > hlim) issued = hlim;
                if (h < hend) {
                    XP(if (xp_out != 0) { const unsigned long long t_ = wall_clock64(); xp[3] += t_ - xp_out; xp[2] += t_ - xp_re; xp_out = 0; } else xp[6] = wall_clock64() - xp_k0;
                       xp[8] = h; xp[9] = wall_clock64() - xp_k0;)
                    // the range [h, hend) is decided: it is run at the end of the kernel, behind the rows -- with sharing out of the
                    // workgroup's record, by whoever claims a chunk of it first
                    own_a = h;
                    own_b = hend;
                    if (my_rec != nullptr && tid == 0) pda_ts_publish(my_rec, h, hend);
                }
                break;
            }
            hlim = min(hlim, hf);
            ++n_entries;
            XP(if (xp_out != 0) { const unsigned long long t_ = wall_clock64(); xp[3] += t_ - xp_out; xp[2] += t_ - xp_re; } else xp[6] = wall_clock64() - xp_k0;)
            Loop6<D, NU>::run(h, issued, reason, hlim, ring_lds, flags_lds, 1024u * (unsigned)wave, t0, (unsigned)g.n_splits,
                              (unsigned)img, (unsigned)(img >> 32), (unsigned)meta, (unsigned)(meta >> 32), eu, tmin, my_ufrag, thr, lane16);
            XP(xp_out = wall_clock64(); xp_re = xp_out;)
            if (reason == 0u) {
                if (hlim == hend) break;
                continue;                                                // (the flags of every half-tile below hlim have been looked at: test-free from hlim on)
            }
            if (reason != 1u) { if (lane == 0) g.stats[0] = 5u; break; }
            // every wave of the workgroup left at half-tile h because SOME wave's lanes flagged h - 2; the flags of h - 1 were still being
            // worked out: both are scored again here (a half-tile without a candidate of this wave costs its 8 NK MFMAs)
            // (`before` has had no reader since the debug log left.  It stays for now: without this dead local hipcc allocates the kernel's
            // scalar registers differently -- a change of this kernel's code, which wants its own measurement: DESIGN 7)
            [[maybe_unused]] const unsigned before = ring_n + n_cand;
            extract2(h, hlim);
            XP(const unsigned long long xp_a = wall_clock64(); xp[0] += xp_a - xp_out; xp[4] += 1;)
            // (thresholds rise only through the lists: rescoring a ring that holds a pass's worth keeps them fresh enough)
            if (ring_n >= (unsigned)CPP) rescore_ring();
            XP(xp_re = wall_clock64(); xp[1] += xp_re - xp_a;)
        }
        if (ring_n > 0u) rescore_ring();
        if (lane == 0) atomicAdd(g.stats + 1, n_cand);
        if (lane == 0) atomicAdd(g.stats + 5, n_entries);                  // (workspace + 20: entries of the asm loop, summed over the waves)
        // (workspace + 8: the half-tiles run so far -- all of the split but its decided range, which whoever runs it adds below)
        if (lane == 0 && wave == 0) atomicAdd(reinterpret_cast<unsigned long long*>(g.stats + 2), (unsigned long long)(hend - (own_b - own_a)) * (unsigned long long)(UT / kUserTile));
    }
    // ================================== all waves: sort and emit ==================================
    // Every list comes out of the warm-up unsorted with K .. kCap4 keys, and all but a few per cent of them are untouched since: the
    // final top-K selection and sort of all 1 024 rows is a fixed cost of the launch.  With one wave per SIMD nothing hides a round
    // trip, so: the keys of eight rows are requested together, and a row is ranked out of the LDS (the row's keys written once, then
    // read back as broadcasts, two keys per ds_read_b128) -- ~150 instructions per row where compact_list's loop over the list in
    // global memory was a dependent round trip per four keys (0.87 ms of a 9.0 ms launch -> 0.2).  A wave emits its own 256 rows.
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __syncthreads();
    XP(const unsigned long long xp_e0 = wall_clock64();)
    {
        constexpr int EB = 8;
        uint64_t* scr = crings + wave * kRing5;                          // (the rings are empty now)
        auto emit_row = [&](int rb, int cnt, uint64_t kraw) __attribute__((always_inline)) {
            const int c = min(__builtin_amdgcn_readfirstlane(cnt), CAPL);                    // (failed appends may have pushed it past the capacity)
            const uint64_t key = lane < c ? kraw : (uint64_t)(63 - lane);                    // fillers: unique, below any real key
            scr[lane] = key;
            pda_wave_sync();
            int rank = 0;
            for (int jj = 0; jj < c; jj += 4) {
                const uint64_t k0 = scr[jj], k1 = scr[jj + 1], k2 = scr[jj + 2], k3 = scr[jj + 3];
                rank += ((k0 > key) ? 1 : 0) + ((k1 > key) ? 1 : 0) + ((k2 > key) ? 1 : 0) + ((k3 > key) ? 1 : 0);
            }
            pda_wave_sync();
            uint64_t* orow = g.out_keys + ((size_t)split * g.n_users_blk + rb) * K;
            if (lane < c && rank < K) orow[rank] = key;
            if (lane >= c && lane < K) orow[lane] = 0ull;
        };
        if (warm_final) {
            // out_keys holds the warm-up's sorted rows: only the rows the sweep appended to are ranked and written again
            for (int w = 0; w < UPW / 32; ++w) {
                unsigned m = touched[wave * (UPW / 32) + w];
                while (m != 0u) {
                    const int b = __builtin_ctz(m);
                    m &= m - 1u;
                    const int rr = wave * UPW + 32 * w + b;
                    emit_row(utile * UT + rr, cntl[rr], lists[(size_t)rr * CAPL + (lane < CAPL ? lane : CAPL - 1)]);
                }
            }
        } else if (starts_empty) {
            // an empty split behind a shared warm-up: every row is written here -- zeros, then the few rows the sweep appended to
            const int rb0 = utile * UT + wave * UPW, nv = max(0, min(UPW, g.n_users_blk - rb0));
            uint64_t* ob = g.out_keys + ((size_t)split * g.n_users_blk + rb0) * K;
            for (int i = lane; i < nv * K; i += 64) ob[i] = 0ull;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");       // (the same wave writes the touched rows again below)
            for (int w = 0; w < UPW / 32; ++w) {
                unsigned m = touched[wave * (UPW / 32) + w];
                while (m != 0u) {
                    const int b = __builtin_ctz(m);
                    m &= m - 1u;
                    const int rr = wave * UPW + 32 * w + b;
                    emit_row(utile * UT + rr, cntl[rr], lists[(size_t)rr * CAPL + (lane < CAPL ? lane : CAPL - 1)]);
                }
            }
        } else {
            for (int i0 = 0; i0 < UPW; i0 += EB) {
                uint64_t kraw[EB];
                int cv[EB];
#pragma unroll
                for (int q = 0; q < EB; ++q) {
                    const int rr = wave * UPW + i0 + q, rb = utile * UT + rr;
                    const bool ok = rb < g.n_users_blk;
                    kraw[q] = ok ? lists[(size_t)rr * CAPL + (lane < CAPL ? lane : CAPL - 1)] : 0ull;
                    cv[q] = ok ? cntl[rr] : 0;
                }
#pragma unroll
                for (int q = 0; q < EB; ++q) {
                    const int rb = utile * UT + wave * UPW + i0 + q;
                    if (rb >= g.n_users_blk) break;
                    emit_row(rb, cv[q], kraw[q]);
                }
            }
        }
    }
    XP(xp[7] = wall_clock64() - xp_e0; xp[11] = hend;)
    // ================================== all waves: the test-free tails ==================================
    // The rows are out, the rings and the LDS slots are free.  Chunks of the workgroup's own decided range until its record is exhausted,
    // then chunks from the record with the most left, until nothing is left anywhere: a workgroup that finds nothing leaves.  Without
    // sharing: the own range in one piece.  (PDA_SWEEP_TAIL_OTHERS_FIRST: the other records first.)  workspace + 8, + 20 and + 28 are added
    // by whoever ran the half-tiles.
    {
        unsigned n_ent2 = 0, n_ran = 0, n_chunks_other = 0, n_ran_other = 0;
        bool steal = my_rec != nullptr;
        XP(if (pda_v5_tail_pieces > 0) { steal = false; tail_fixed = (own_b - own_a + (unsigned)pda_v5_tail_pieces - 1u) / (unsigned)pda_v5_tail_pieces; })
        const bool others_first = steal && g.tail_others_first != 0;
        bool own_left = own_a < own_b;                                   // (an exhausted record stays exhausted: no second look)
        __syncthreads();
        for (;;) {
            unsigned vb = blockIdx.x, a = own_a, b = own_b;
            if (my_rec == nullptr) {
                own_a = own_b;                                           // (one piece)
            } else {
                bool got = false;
                if (others_first) {
                    got = next_chunk(false, false, vb, a, b);
                    if (!got && own_left) { got = next_chunk(true, false, vb, a, b); own_left = got; }
                } else {
                    if (own_left) { got = next_chunk(true, n_ent2 == 0u, vb, a, b); own_left = got; }
                    if (!got && steal) got = next_chunk(false, false, vb, a, b);
                }
                if (!got) a = b = 0;
            }
            if (a >= b) break;
            // the chunk's tile sequence and user image (as its workgroup's own prologue forms them)
            const int vsplit = (int)(vb % (unsigned)g.n_splits), vutile = (int)(vb / (unsigned)g.n_splits);
            const unsigned vt0 = (unsigned)(vsplit + warm_tiles_of(g, vsplit) * g.n_splits);
            const unsigned char* vfrag = g.ufrag + ((size_t)vutile * 4 + wave) * (size_t)(NU * NK * 1024);
            const size_t vimg = (size_t)g.rows5;
            ++n_ent2;
            n_ran += b - a;
            if (vb != blockIdx.x) { ++n_chunks_other; n_ran_other += b - a; }
            unsigned is = a;
            Loop6Free<D, NU>::run(a, is, b, ring_lds, 1024u * (unsigned)wave, vt0, (unsigned)g.n_splits, (unsigned)vimg, (unsigned)(vimg >> 32), vfrag, lane16);
        }
        if (lane == 0 && n_ent2 > 0u) atomicAdd(g.stats + 5, n_ent2);    // (workspace + 20)
        if (lane == 0 && wave == 0 && n_ran > 0u) {
            atomicAdd(g.stats + 7, n_ran);                               // (workspace + 28: half-tiles run test-free)
            atomicAdd(reinterpret_cast<unsigned long long*>(g.stats + 2), (unsigned long long)n_ran * (unsigned long long)(UT / kUserTile));
        }
        if (lane == 0 && wave == 0 && n_chunks_other > 0u) {
            atomicAdd(g.stats + 9, n_chunks_other);                      // (workspace + 36: chunks run for another workgroup)
            atomicAdd(g.stats + 10, n_ran_other);                        // (workspace + 40: the half-tiles in them)
        }
        XP(xp[10] = n_ran_other;)
    }
    XP(xp[5] = wall_clock64() - xp_k0;
       if (lane == 0 && blockIdx.x < (unsigned)kXpMaxWg) for (int q = 0; q < kXpWords; ++q) pda_v5_exitprof[((size_t)blockIdx.x * 4 + wave) * kXpWords + q] = xp[q];)
}

template <int D, bool BF, bool S16, int UPW>
int launch_sweep5(const Args4& g, const Call4& c, hipStream_t stream) {
    constexpr int UT = 4 * UPW;
    constexpr size_t lds = (size_t)kNSlot5 * slot_bytes5(D) + (size_t)UT * 8 + 4 * kRing5 * 8 + (80 + 4) * 4 + 64;          // (80 words of sync, 4 of a claim)
    static_assert(UPW == 256 || D == 256 || 2 * lds <= 160 * 1024, "two workgroups per CU");
    static_assert(lds <= 160 * 1024, "LDS per workgroup");
    static char attr_done[kMaxDev4] = {};
    if (const int rc = dynamic_lds_once(reinterpret_cast<const void*>(&sweep5_kernel<D, BF, S16, UPW>), lds, attr_done)) return rc;
    const int utiles = (g.n_users_blk + UT - 1) / UT, n_pad = utiles * UT;
    if (c.uprep5) {                      // (else: the warm-up of this call has written the user image and the norms -- Args4::ufrag_out)
        hipLaunchKernelGGL((uprep5_kernel<D, BF, S16, UPW>), dim3((unsigned)(((size_t)n_pad * (D / 8) + 255) / 256)), dim3(256), 0, stream, g.U, g.users, g.n_users_blk, n_pad,
                           const_cast<unsigned char*>(g.ufrag), const_cast<float*>(g.unorm));
        PDA_CHECK_LAUNCH();
    }
    hipLaunchKernelGGL((sweep5_kernel<D, BF, S16, UPW>), dim3((unsigned)(utiles * g.n_splits)), dim3(256), lds, stream, g);
    PDA_CHECK_LAUNCH();
    return PDA_OK;
}
