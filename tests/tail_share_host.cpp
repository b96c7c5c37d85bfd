// Stand-alone host program around pda_amd/csrc/pda_tail_share.h (built and run by tests/test_tail_share_host.py, once with
// -fsanitize=thread and once with -fsanitize=address,undefined): N threads play the workgroups of sweep5_kernel's shared test-free tail.
//   * ranges of unequal length, late publishers, workgroups that never publish, a minimum chunk of 1 (and 2, and the product's 32),
//     the owner-first order of the product and the others-first order of the test mode
//   * records of an earlier call: the call's own records hold published-looking words until its reset (the kernel's memset) zeroes them, and
//     the records BEHIND its own keep such words -- those only show that the scan and the claims stay below n; that the RESET is what
//     protects a call from an earlier call's words is the GPU test's part (tests/test_gpu_tail_share.py, two calls on one workspace)
//   * every half-tile of every published range is claimed exactly once, nothing outside a range, nothing from an unpublished record;
//     every record ends with next == end; every thread terminates (nobody waits for anybody: a thread that finds nothing leaves)
// usage: tail_share_host [rounds = 200] [threads = 16]        exit status 0 and "ok" on success
#include <atomic>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "pda_tail_share.h"

namespace {

struct Rng {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
    uint32_t below(uint32_t n) { return next() % n; }
};

struct Plan {                       // what one workgroup does in one call
    bool publishes;
    unsigned h, hend, delay;        // its decided half-tile, the end of its split; yields before it publishes (late publishers)
};

constexpr int kStale = 4;           // records of an earlier, larger call behind the live ones
constexpr unsigned kMaxHend = 700;

int fails = 0;
#define EXPECT(c, ...) do { if (!(c)) { if (fails++ < 20) { std::fprintf(stderr, "FAIL %s:%d %s: ", __FILE__, __LINE__, #c); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); } } } while (0)

void one_call(int n, unsigned min_chunk, bool others_first, Rng& rng, std::vector<uint64_t>& recs, long& steals) {
    std::vector<Plan> plan(n);
    for (int w = 0; w < n; ++w) {
        Plan& p = plan[w];
        p.publishes = rng.below(5) != 0;                                  // one in five never reaches a decided half-tile
        p.hend = 1 + rng.below(kMaxHend);
        p.h = rng.below(p.hend);                                          // h < hend
        if (rng.below(4) == 0) p.h = p.hend - 1;                          // a range of ONE half-tile
        p.delay = rng.below(3) == 0 ? rng.below(200) : 0;
    }
    // the call's memset: its own records, whatever an earlier call left in them.  The stale ones behind them keep whatever they hold.
    for (int w = 0; w < n; ++w) recs[w] = ((uint64_t)(100 + rng.below(500)) << 32) | rng.below(100);
    for (int w = 0; w < n; ++w) recs[w] = 0;
    std::vector<uint64_t> stale(recs.begin() + n, recs.end());
    std::vector<std::atomic<unsigned char>> ran((size_t)n * kMaxHend);
    for (auto& x : ran) x.store(0, std::memory_order_relaxed);
    std::atomic<long> stolen{0};
    std::atomic<int> bad_victim{0};
    std::atomic<int> gate{0};                                             // (the harness's start line, so that the threads overlap: no part of the scheme)

    auto work = [&](int w) {
        const Plan& p = plan[w];
        gate.fetch_add(1);
        while (gate.load() < n) std::this_thread::yield();
        for (unsigned i = 0; i < p.delay; ++i) std::this_thread::yield();
        auto run = [&](int vb, unsigned a, unsigned b) {
            if (vb < 0 || vb >= n || !plan[vb].publishes || a < plan[vb].h || b > plan[vb].hend || a >= b) { bad_victim.fetch_add(1); return; }
            for (unsigned x = a; x < b; ++x) ran[(size_t)vb * kMaxHend + x].fetch_add(1, std::memory_order_relaxed);
            if (vb != w) stolen.fetch_add(1);
            std::this_thread::yield();                                    // (running a chunk takes time: the others get to claim)
        };
        unsigned a, b;
        if (p.publishes) {
            pda_ts_publish(&recs[w], p.h, p.hend);
            if (!others_first)
                for (bool first = true; pda_ts_claim(&recs[w], first, min_chunk, 0u, a, b); first = false) run(w, a, b);
        }
        // the rows are out: chunks from the record with the most left, until nothing is left anywhere
        for (;;) {
            // (the kernel's steps: the scan -- there over 64 lanes, here one --, then a claim from the record it names)
            const uint64_t key = pda_ts_pick(recs.data(), (unsigned)n, (unsigned)w, 0u, 1u);
            if ((key >> 32) != 0u) {
                unsigned vb = 0;
                if (pda_ts_steal(recs.data(), key, min_chunk, vb, a, b)) run((int)vb, a, b);
                continue;                                                 // (a failed claim: that record is exhausted for good)
            }
            if (others_first && pda_ts_claim(&recs[w], false, min_chunk, 0u, a, b)) { run(w, a, b); continue; }
            break;
        }
    };
    std::vector<std::thread> th;
    for (int w = 0; w < n; ++w) th.emplace_back(work, w);
    for (auto& t : th) t.join();                                          // every thread terminates

    EXPECT(bad_victim.load() == 0, "%d chunks outside a published range", bad_victim.load());
    for (int w = 0; w < n; ++w) {
        const Plan& p = plan[w];
        for (unsigned x = 0; x < kMaxHend; ++x) {
            const unsigned want = (p.publishes && x >= p.h && x < p.hend) ? 1u : 0u;
            const unsigned got = ran[(size_t)w * kMaxHend + x].load();
            EXPECT(got == want, "workgroup %d half-tile %u ran %u times, wanted %u (range %u .. %u, publishes %d)", w, x, got, want, p.h, p.hend, (int)p.publishes);
        }
        if (p.publishes) EXPECT(pda_ts_next(recs[w]) == p.hend && pda_ts_end(recs[w]) == p.hend, "record %d ends at %u / %u, not %u", w, pda_ts_next(recs[w]), pda_ts_end(recs[w]), p.hend);
        else EXPECT(recs[w] == 0, "unpublished record %d was written: %llx", w, (unsigned long long)recs[w]);
    }
    for (int i = 0; i < kStale; ++i) EXPECT(recs[n + i] == stale[i], "stale record %d was touched", i);
    steals += stolen.load();
}

void unit() {
    // an unpublished record and an impossible word are never claimed from; chunk sizes keep their promises
    uint64_t r = 0;
    unsigned a = 7, b = 7;
    EXPECT(!pda_ts_claim(&r, true, 1, 0, a, b) && r == 0, "claim from an unpublished record");
    r = ((uint64_t)5 << 32) | 9;                                          // next > end
    EXPECT(pda_ts_left(r) == 0 && !pda_ts_claim(&r, false, 1, 0, a, b), "claim from an impossible word");
    pda_ts_publish(&r, 3, 3);                                             // an empty range is not published
    EXPECT(r == (((uint64_t)5 << 32) | 9), "an empty range was published");
    for (unsigned left = 1; left < 3000; ++left)
        for (unsigned mc : {1u, 2u, 32u})
            for (int first = 0; first < 2; ++first) {
                const unsigned c = pda_ts_chunk(left, first != 0, mc, 0);
                EXPECT(c >= 1 && c <= left && (c == left || (c >= mc && left - c >= mc)), "chunk %u of %u at minimum %u", c, left, mc);
            }
    // one owner alone: a handful of claims for a range the size of config 3's
    r = 0;
    pda_ts_publish(&r, 375, 6250);
    int n = 0;
    unsigned at = 375;
    for (bool first = true; pda_ts_claim(&r, first, kTailMinChunk, 0, a, b); first = false, ++n) {
        EXPECT(a == at && b > a, "chunks of one owner are consecutive");
        at = b;
    }
    EXPECT(at == 6250 && n <= 8, "%d claims, ended at %u", n, at);
}

}  // namespace

int main(int argc, char** argv) {
    const int rounds = argc > 1 ? std::atoi(argv[1]) : 200, threads = argc > 2 ? std::atoi(argv[2]) : 16;
    unit();
    Rng rng{20260101};
    std::vector<uint64_t> recs(threads + kStale);
    long steals = 0;
    for (int r = 0; r < rounds; ++r) {
        const int n = 1 + (int)rng.below((uint32_t)threads);              // a smaller call behind a larger one leaves exhausted records in front
        for (int i = 0; i < kStale; ++i) recs[n + i] = ((uint64_t)(100 + rng.below(500)) << 32) | rng.below(100);   // ... and published-looking ones behind
        const unsigned mc = r % 3 == 0 ? 1u : r % 3 == 1 ? 2u : kTailMinChunk;
        one_call(n, mc, (r / 3) % 2 == 1, rng, recs, steals);
    }
    if (fails) { std::fprintf(stderr, "%d failures\n", fails); return 1; }
    std::printf("ok: %d calls of up to %d workgroups, %ld chunks run for another workgroup\n", rounds, threads, steals);
    return 0;
}
