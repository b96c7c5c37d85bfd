// Sharing the test-free tail of the huge geometry's sweep between workgroups (pda_v5_sweep.h): the claim / publish logic over ONE
// 64-bit atomic word per workgroup.  Plain functions; the same text compiles for the device (sweep5_kernel calls them) and for the host
// (tests/tail_share_host.cpp plays the workgroups with threads, under the thread and address sanitizers).
//
// A record is the range of LOCAL half-tiles [next, end) of its workgroup's split that nobody has claimed yet:  word = end << 32 | next.
//   0            the workgroup has published nothing (the call's counter memset covers the records: a record of an earlier call, or of a
//                workgroup that has not started or never reaches a decided half-tile, is 0 -- and 0 is never claimed from)
//   next < end   published (next < end at the publish, so end >= 1 and the word is not 0), half-tiles left
//   next == end  exhausted; it stays that way
// Everybody claims from the FRONT with one compare-and-swap: the owner in few large chunks, a workgroup whose own range is exhausted
// from the record with the most left.  Nobody ever waits: a failed compare-and-swap means somebody else made progress, a claim from an
// exhausted or unpublished record returns false, and the range only shrinks.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PDA_TS_FN __host__ __device__ __forceinline__
#else
#define PDA_TS_FN static inline
#endif
#if defined(__HIP_DEVICE_COMPILE__)
#define PDA_TS_LOAD(p) __hip_atomic_load((p), __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)
#define PDA_TS_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT)
#define PDA_TS_CAS(p, e, d) __hip_atomic_compare_exchange_strong((p), (e), (d), __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT)
#else
#define PDA_TS_LOAD(p) __atomic_load_n((p), __ATOMIC_ACQUIRE)
#define PDA_TS_STORE(p, v) __atomic_store_n((p), (v), __ATOMIC_RELEASE)
#define PDA_TS_CAS(p, e, d) __atomic_compare_exchange_n((p), (e), (d), false, __ATOMIC_ACQ_REL, __ATOMIC_ACQUIRE)
#endif

// half-tiles: the smallest chunk.  One more entry of the test-free loop costs at most 2.7 us and a half-tile 1.15 us at config 3
// (profiles/tail_share.txt section 2): 32 half-tiles are 37 us of work per entry.  A choice inside a wide margin, not a tuned value.
constexpr unsigned kTailMinChunk = 32;

PDA_TS_FN unsigned pda_ts_next(uint64_t w) { return (unsigned)w; }
PDA_TS_FN unsigned pda_ts_end(uint64_t w) { return (unsigned)(w >> 32); }
// half-tiles left in a record; 0 for an unpublished one (and for a word that could never have been published: next > end)
PDA_TS_FN unsigned pda_ts_left(uint64_t w) { return pda_ts_end(w) > pda_ts_next(w) ? pda_ts_end(w) - pda_ts_next(w) : 0u; }

// release: whoever claims from the record sees what the publisher wrote before
PDA_TS_FN void pda_ts_publish(uint64_t* rec, unsigned next, unsigned end) {
    if (next < end) PDA_TS_STORE(rec, ((uint64_t)end << 32) | (uint64_t)next);
}

// guided chunk sizes.  The owner: its first chunk leaves an eighth of the range to be shared, then half of what is left; a thief: half
// of what is left.  Never below min_chunk, and never leaving a rest below min_chunk behind.  (The eighth: at config 3 the workgroups of
// the unshared launch end within 6 % of each other -- 6 806 .. 7 212 us, profiles/tail_share.txt section 2 --, so an eighth of a range of
// ~5 900 half-tiles covers the spread; the fractions themselves were not tuned: one setting was measured.)  fixed > 0: chunks of that
// size (the entry-cost measurement of the profiling build).
PDA_TS_FN unsigned pda_ts_chunk(unsigned left, bool owner_first, unsigned min_chunk, unsigned fixed) {
    if (min_chunk < 1u) min_chunk = 1u;
    unsigned c = fixed > 0u ? fixed : owner_first ? left - left / 8u : left / 2u;
    if (c < min_chunk) c = min_chunk;
    if (c > left || left - c < min_chunk) c = left;
    return c;
}

// one claim from the front of *rec: true and [a, b) -- false when the record is unpublished or exhausted.  Lock-free: a failed
// compare-and-swap is retried on the fresh word, whose range is strictly shorter.
PDA_TS_FN bool pda_ts_claim(uint64_t* rec, bool owner_first, unsigned min_chunk, unsigned fixed, unsigned& a, unsigned& b) {
    uint64_t w = PDA_TS_LOAD(rec);
    for (;;) {
        const unsigned left = pda_ts_left(w);
        if (left == 0u) return false;
        const unsigned c = pda_ts_chunk(left, owner_first, min_chunk, fixed);
        const uint64_t nw = (w & 0xFFFFFFFF00000000ull) | (uint64_t)(pda_ts_next(w) + c);
        if (PDA_TS_CAS(rec, &w, nw)) {
            a = pda_ts_next(w);
            b = a + c;
            return true;
        }
    }
}

// the record with the most left among recs[lane], recs[lane + n_lanes], ... below n, other than `self`:  left << 32 | index, or 0 when
// nothing is left in any of them (a snapshot: the claim that follows decides).  The kernel calls it with the 64 lanes of a wave and takes
// the maximum of the lanes' words; one caller alone passes lane 0 of 1.
PDA_TS_FN uint64_t pda_ts_pick(uint64_t* recs, unsigned n, unsigned self, unsigned lane, unsigned n_lanes) {
    uint64_t best = 0;
    for (unsigned i = lane; i < n; i += n_lanes) {
        if (i == self) continue;
        const uint64_t key = ((uint64_t)pda_ts_left(PDA_TS_LOAD(recs + i)) << 32) | i;
        if ((key >> 32) != 0u && key > best) best = key;
    }
    return best;
}

// a chunk from the record that `key` (the largest word of pda_ts_pick) names: false when there is none, or when that record has been
// exhausted since the scan -- it stays exhausted, so a caller that scans again fails at most once per record
PDA_TS_FN bool pda_ts_steal(uint64_t* recs, uint64_t key, unsigned min_chunk, unsigned& vb, unsigned& a, unsigned& b) {
    if ((key >> 32) == 0u) return false;
    vb = (unsigned)key;
    return pda_ts_claim(recs + vb, false, min_chunk, 0u, a, b);
}
