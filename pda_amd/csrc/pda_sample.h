// The device-side samplers (N1, MF/train_new_api.py:366-412).  The draws of a batch row -- the step, the user, the positive,
// the membership test in the train row, the rejection loop of a negative -- are defined here once, and so is what every sampler
// entry point checks on the host (sample_call_ok).  sample_one, the BPR triplet of a row, is composed of them; it is the body of
// the stand-alone and the many-batches kernels (pda_aux.hip), of the train step that draws the NEXT batch in spare workgroups of
// its own launch and of the looped trainer (pda_bpr_step.hip).  PNSM (pda_dice.hip) and the sampled-softmax sampler (pda_ssm.hip)
// are the same pieces around their own negatives, the popularity proposal (pda_negpop.hip) is sample_row and sample_block_entry
// around sample_negative_alias, the in-batch mask (pda_inbatch.hip) is the membership test: a row draws the
// same user and positive under every method for one (seed, step, row), by construction.
#pragma once
#include "pda_common.h"

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
__device__ __forceinline__ uint32_t draw(uint64_t seed, uint64_t step, uint32_t row, uint32_t k) {
    return (uint32_t)(mix64(mix64(seed ^ (step * 0xD1B54A32D192ED03ull)) ^ (((uint64_t)row << 32) | k)) >> 32);
}
__device__ __forceinline__ uint32_t bounded(uint32_t r, uint32_t n) { return (uint32_t)(((uint64_t)r * n) >> 32); }

// Keyed permutation of [0, n): a balanced Feistel network over 2 * hb bits with cycle walking.  Four rounds, and twelve more
// behind them where a half has at most kFeistelSmallHalf bits (pools <= 256).  A round function of so few bits has so few values
// that four rounds leave the permutation measurably short of uniform: with halves of <= 3 bits the users of a pool were drawn
// with frequencies up to 9 % (rms) apart, with 4 bits 0.4 % (eight rounds still show it on 2-bit halves; sixteen are flat at 200 000
// batches: tests/test_sampler_distribution.py, profiles/sampler_rounds.txt).  Wider halves keep their four rounds and their
// batch stream.
constexpr int kFeistelSmallHalf = 4, kFeistelSmallRounds = 16;

__device__ uint32_t feistel_perm(uint32_t x, uint32_t n, uint64_t key) {
    int bits = 1;
    while ((1ull << bits) < n) ++bits;
    const int hb = (bits + 1) / 2;
    const uint32_t hm = (1u << hb) - 1u;
    do {
        uint32_t l = x >> hb, r = x & hm;
#pragma unroll
        for (int round = 0; round < 4; ++round) {
            const uint32_t f = (uint32_t)mix64(key ^ ((uint64_t)round << 40) ^ r) & hm;
            const uint32_t nl = r;
            r = l ^ f;
            l = nl;
        }
        if (hb <= kFeistelSmallHalf) {
#pragma unroll 1   // (a rare path inside the step kernels: no code growth)
            for (int round = 4; round < kFeistelSmallRounds; ++round) {
                const uint32_t f = (uint32_t)mix64(key ^ ((uint64_t)round << 40) ^ r) & hm;
                const uint32_t nl = r;
                r = l ^ f;
                l = nl;
            }
        }
        x = (l << hb) | r;
    } while (x >= n);
    return x;
}

struct SampleArgs {
    int32_t* users;
    const int32_t* user_pool;
    const int64_t* indptr;
    const int32_t* indices;
    const int32_t* slots;
    const float* pop;
    int32_t* pos;
    int32_t* neg;
    float* pos_pop;
    float* neg_pop;
    uint64_t seed, step;
    int B, n_pool, gen_users, neg_lo, neg_hi, n_slots;
    const uint64_t* step_dev;   // optional device-resident step counter added to `step` (HIP-graph replay: pda_counter_add)
    uint64_t* step_next;        // optional: receives *step_dev + 1 (a DIFFERENT location: no launch in between needed)
};

// COH: the batch is handed to other workgroups of the SAME launch (pda_bpr_train_steps_f32): its five words per triplet leave
// as device-scope stores (no cache write-back needed before the grid barrier)
template <bool COH, typename T>
__device__ __forceinline__ void out_store(T* p, T v) {
    if constexpr (COH) __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else *p = v;
}

// ---- the draws: each defined once, for every sampler kernel ---------------------------------------------------------------------
// Draw numbers of a row: 0 the positive, 1 the time slot of an empty row, 2 PNSM's coin, 3 DNS's pick among the best candidates
// (kPickDraw, pda_dns.hip), 7 the user (with replacement), and from kNegDraw on the tries of the negatives, kRejectTries apiece.
constexpr uint32_t kPickDraw = 3, kNegDraw = 16, kRejectTries = 4096;

// The step a launch draws with: `step` plus the device counter where there is one; the thread for which `first` holds hands
// *step_dev + 1 on to step_next (a DIFFERENT location: other threads are still reading *step_dev).
__device__ __forceinline__ uint64_t sample_step(uint64_t step, const uint64_t* step_dev, uint64_t* step_next, bool first) {
    if (step_dev) {
        const uint64_t cur = *step_dev;
        step += cur;
        if (step_next && first) *step_next = cur + 1;
    }
    return step;
}

// The user of row r.  B <= n_pool: distinct users (rd.sample, MF/train_new_api.py:380-381); else with replacement (:383)
__device__ __forceinline__ int sample_user(uint64_t seed, uint64_t step, int r, int B, int n_pool, const int32_t* user_pool) {
    const uint64_t key = mix64(seed ^ mix64(step));
    const uint32_t x = B <= n_pool ? feistel_perm((uint32_t)r, (uint32_t)n_pool, key) : bounded(draw(seed, step, r, 7), n_pool);
    return user_pool ? user_pool[x] : (int)x;
}

// Where in its train row (len > 0 entries) row r finds its positive, :392-396
__device__ __forceinline__ int sample_pos_index(uint64_t seed, uint64_t step, int r, int len) {
    return (int)bounded(draw(seed, step, r, 0), len);
}

// Is item n in the (sorted) train row indices[b, e)?  (hi declared before lo: the order in which the compiler gives the step
// kernels of pda_bpr_step.hip the instructions they had before this was a function of its own -- profiles/sampler_pieces.txt)
__device__ __forceinline__ bool train_row_has(const int32_t* indices, int64_t b, int64_t e, int n) {
    int64_t hi = e, lo = b;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (indices[mid] < n) lo = mid + 1; else hi = mid;
    }
    return lo < e && indices[lo] == n;
}

// The negative of row r, :397-401: item_of(x), x uniform in [0, span), drawn again while the train row holds it; after
// kRejectTries tries the last draw stays.  first_draw: kNegDraw (+ kRejectTries j for the j-th negative of a row).
template <typename F>
__device__ __forceinline__ int sample_negative(uint64_t seed, uint64_t step, int r, uint32_t first_draw, uint32_t span,
                                               const int32_t* indices, int64_t b, int64_t e, F item_of) {
    int n = 0;
    for (uint32_t k = 0; k < kRejectTries; ++k) {
        n = item_of(bounded(draw(seed, step, r, first_draw + k), span));
        if (!train_row_has(indices, b, e, n)) break;
    }
    return n;
}

// The negative of row r under a popularity proposal (include/pda_hip_negpop.h): try k picks a slot of the alias table as
// sample_negative picks an item, from the same draw, and a coin from draw 0x80000000 | (first_draw + k) keeps the slot or takes
// its alias; a slot that is its own alias needs no coin, so a table of such slots draws what sample_negative draws, bit for bit.
// The two hashes of a try do not depend on each other or on the table: both are issued ahead of the 8-byte load.
constexpr uint32_t kCoinDraw = 0x80000000u;

__device__ __forceinline__ int sample_negative_alias(uint64_t seed, uint64_t step, int r, uint32_t first_draw, uint32_t span, int neg_lo,
                                                     const uint64_t* alias, const int32_t* indices, int64_t b, int64_t e) {
    int n = 0;
    for (uint32_t k = 0; k < kRejectTries; ++k) {
        const uint32_t slot = bounded(draw(seed, step, r, first_draw + k), span);
        const uint32_t coin = draw(seed, step, r, kCoinDraw | (first_draw + k));
        const uint64_t t = alias[slot];
        const uint32_t thr = (uint32_t)t, other = (uint32_t)(t >> 32);
        n = neg_lo + (int)((other == slot || coin < thr) ? slot : other);
        if (!train_row_has(indices, b, e, n)) break;
    }
    return n;
}

// one thread = one triplet r of the batch; negative_of(a, r, b, e): the negative of the row whose train items are indices[b, e)
template <bool COH, typename NEG>
__device__ __forceinline__ void sample_row(SampleArgs a, int r, NEG negative_of) {
    if (r >= a.B) return;
    a.step = sample_step(a.step, a.step_dev, a.step_next, r == 0);
    int u;
    if (a.gen_users) {
        u = sample_user(a.seed, a.step, r, a.B, a.n_pool, a.user_pool);
        out_store<COH>(&a.users[r], u);
    } else {
        u = a.users[r];
    }
    const int64_t b = a.indptr[u], e = a.indptr[u + 1];
    const int len = (int)(e - b);
    int p = 0, slot = 0;
    if (len == 0) {  // :387-390
        p = 0;
        slot = a.n_slots > 0 ? (int)bounded(draw(a.seed, a.step, r, 1), a.n_slots) : 0;
    } else {
        const int idx = sample_pos_index(a.seed, a.step, r, len);
        p = a.indices[b + idx];
        slot = a.slots ? a.slots[b + idx] : 0;
    }
    const int n = negative_of(a, r, b, e);
    out_store<COH>(&a.pos[r], p);
    out_store<COH>(&a.neg[r], n);
    if (a.pop && a.pos_pop) {  // :402-403
        out_store<COH>(&a.pos_pop[r], a.pop[(size_t)p * a.n_slots + slot]);
        out_store<COH>(&a.neg_pop[r], a.pop[(size_t)n * a.n_slots + slot]);
    }
}

// the uniform triplet of row r
template <bool COH = false>
__device__ __forceinline__ void sample_one(SampleArgs a, int r) {
    sample_row<COH>(a, r, [](const SampleArgs& a, int r, int64_t b, int64_t e) {
        return sample_negative(a.seed, a.step, r, kNegDraw, (uint32_t)(a.neg_hi - a.neg_lo), a.indices, b, e,
                               [&](uint32_t x) { return a.neg_lo + (int)x; });
    });
}

// ---- the [B, N] block of negatives (pda_ssm.hip, pda_negpop.hip): one thread per (row r, negative j) ---------------------------
struct SsmSampleArgs {
    int32_t* users;
    const int32_t* user_pool;
    const int64_t* indptr;
    const int32_t* indices;
    int32_t* pos;
    int32_t* negs;
    uint64_t seed, step;
    int B, N, n_pool, gen_users, neg_lo, neg_hi;
    const uint64_t* step_dev;   // optional device-resident step counter added to `step`
    uint64_t* step_next;        // optional: receives *step_dev + 1 (a DIFFERENT location)
};

// The pieces of sample_row without slots and popularities: every thread of a row finds the row's user, the thread of j == 0
// writes it and the positive; negative j takes the tries [kNegDraw + kRejectTries j, + kRejectTries), so column 0 is the
// triplet's negative.  negative_of(a, r, first_draw, b, e): the negative drawn from first_draw on.
template <typename NEG>
__device__ __forceinline__ void sample_block_entry(SsmSampleArgs a, size_t i, NEG negative_of) {
    if (i >= (size_t)a.B * (size_t)a.N) return;
    const int r = (int)(i / (size_t)a.N), j = (int)(i % (size_t)a.N);
    a.step = sample_step(a.step, a.step_dev, a.step_next, i == 0);
    int u;
    if (a.gen_users) {
        u = sample_user(a.seed, a.step, r, a.B, a.n_pool, a.user_pool);
        if (j == 0) a.users[r] = u;
    } else {
        u = a.users[r];
    }
    const int64_t b = a.indptr[u], e = a.indptr[u + 1];
    if (j == 0) {
        const int len = (int)(e - b);
        a.pos[r] = len == 0 ? 0 : a.indices[b + sample_pos_index(a.seed, a.step, r, len)];
    }
    a.negs[i] = negative_of(a, r, kNegDraw + kRejectTries * (uint32_t)j, b, e);
}

// (host) What every sampler entry point checks: the users, the train CSR and the two outputs every method has are there, users
// can be drawn where they are to be, and with a device counter (counter: the _dev variants) step_dev is there and step_next is
// another location -- other workgroups may still be reading *step_dev.  Sizes and ranges are each entry point's own.
inline bool sample_call_ok(const void* users, const void* indptr, const void* indices, const void* out_a, const void* out_b, int gen_users,
                           int n_pool, bool counter, const uint64_t* step_dev, const uint64_t* step_next) {
    if (!users || !indptr || !indices || !out_a || !out_b) return false;
    if (gen_users && n_pool <= 0) return false;
    return !counter || (step_dev && step_next != step_dev);
}

// (host) a triplet sampler job as a whole; B is not capped
inline bool triplet_sample_ok(const SampleArgs& a, bool counter) {
    if (!sample_call_ok(a.users, a.indptr, a.indices, a.pos, a.neg, a.gen_users, a.n_pool, counter, a.step_dev, a.step_next)) return false;
    if (a.B <= 0 || a.neg_hi <= a.neg_lo) return false;
    return !(a.pop && (!a.pos_pop || !a.neg_pop || a.n_slots <= 0));
}

// (host) a [B, N] block job as a whole: B <= 2^22 and N <= max_negs (PDA_SSM_MAX_NEGS) keep B N <= 2^30
inline bool block_sample_ok(const SsmSampleArgs& a, bool counter, int max_negs) {
    if (!sample_call_ok(a.users, a.indptr, a.indices, a.pos, a.negs, a.gen_users, a.n_pool, counter, a.step_dev, a.step_next)) return false;
    return !(a.B <= 0 || a.B > (1 << 22) || a.neg_hi <= a.neg_lo || a.N < 1 || a.N > max_negs);
}

}  // namespace
