// Check of helyim_amd/csrc/launch_split.hpp, the arithmetic that cuts a launch
// of more than `limit` workgroups into pieces: block launches of a ragged
// batch and stripe ranges of a strided one. Small limits are walked piece by
// piece; at the production limit (2^23) and at the smallgrid variant's (100)
// the pieces of long splits are counted arithmetically
// and the first, the last and sampled middle ones are checked against 64-bit
// expectations, so a 32-bit intermediate that wraps shows as a wrong field.
// For every split: the pieces are in order and cover [0, n) exactly once, each
// is non-empty with count * per_stripe <= limit, exactly the final piece is
// marked last, and map_q8 * 8 + map_r8 is the piece's workgroup count. Exits
// non-zero at the first failure.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "launch_split.hpp"

using hec::Range;

static long checked = 0;

#define CHECK(cond)                                                                                     \
    do {                                                                                                \
        if (!(cond)) {                                                                                  \
            std::printf("FAIL %s (line %d): n=%llu step=%llu per=%llu limit=%llu i=%llu\n", #cond, __LINE__, \
                        (unsigned long long)n, (unsigned long long)step, (unsigned long long)per,       \
                        (unsigned long long)limit, (unsigned long long)i);                              \
            return 1;                                                                                   \
        }                                                                                               \
    } while (0)

// Piece i of n elements in ranges of `step`, each element `per` workgroups.
static int check_piece(uint64_t n, uint64_t step, uint64_t per, uint64_t limit, uint64_t i) {
    const uint64_t nr = hec::n_ranges(n, step);
    CHECK(nr == (n + step - 1) / step);
    CHECK(i < nr);
    const Range r = hec::range_at(n, step, i);
    const uint64_t want_first = i * step, want_count = i + 1 < nr ? step : n - (nr - 1) * step;
    CHECK(uint64_t(r.first) == want_first);  // in order: piece i starts where piece i - 1 ended
    CHECK(uint64_t(r.count) == want_count);
    CHECK(r.count >= 1);
    CHECK(uint64_t(r.count) * per <= limit);
    CHECK(r.last == (i + 1 == nr));
    CHECK(want_first + want_count <= n);
    if (i + 1 == nr) CHECK(want_first + want_count == n);  // (nr - 1) full pieces + the last cover [0, n)
    if (per == 1) {
        const hec::BlockLaunch l = hec::block_launch(n, limit, i);
        CHECK(l.block_base == r.first && l.n_blocks == r.count && l.last == r.last);
        CHECK(uint64_t(l.map_q8) * 8 + l.map_r8 == uint64_t(l.n_blocks));
        CHECK(l.map_r8 < 8);
    }
    ++checked;
    return 0;
}

// Every piece, one after the other: cover [0, n) exactly once.
static int walk(uint64_t n, uint64_t step, uint64_t per, uint64_t limit) {
    uint64_t next = 0, lasts = 0, i = 0;
    const uint64_t nr = hec::n_ranges(n, step);
    for (i = 0; i < nr; ++i) {
        if (check_piece(n, step, per, limit, i)) return 1;
        const Range r = hec::range_at(n, step, i);
        CHECK(r.first == next);
        next += r.count;
        lasts += r.last ? 1 : 0;
    }
    CHECK(next == n);
    CHECK(lasts == (n ? 1u : 0u));
    return 0;
}

// First, last and sampled middle pieces of a split too long to walk.
static int sample(uint64_t n, uint64_t step, uint64_t per, uint64_t limit) {
    const uint64_t nr = hec::n_ranges(n, step);
    if (nr <= 4096) return walk(n, step, per, limit);
    const uint64_t picks[] = {0, 1, 2, nr / 3, nr / 2, (uint64_t(1) << 31) - 1, uint64_t(1) << 31, nr - 3, nr - 2, nr - 1};
    for (uint64_t i : picks)
        if (i < nr && check_piece(n, step, per, limit, i)) return 1;
    return 0;
}

int main() {
    for (uint64_t limit : {1, 7, 8, 9})
        for (uint64_t n = 0; n <= 40; ++n) {
            if (walk(n, limit, 1, limit)) return 1;  // block launches
            for (uint64_t per = 1; per <= 9 && per <= limit; ++per)  // the callers split only when per <= limit
                if (walk(n, hec::stripes_per_launch(limit, per), per, limit)) return 1;
        }
    // kMaxLaunchBlocks: the product's 2^23, and the 100 of the Makefile's
    // smallgrid variant (no multiple of 8, 3 or 5: uneven eighths and ranges)
    for (uint64_t limit : {uint64_t(1) << 23, uint64_t(100)}) {
        const uint64_t counts[] = {1, 2, limit - 1, limit, limit + 1, 3 * limit + 7, 0xFFFFFFFFull};
        for (uint64_t n : counts) {
            if (sample(n, limit, 1, limit)) return 1;  // block launches
            for (uint64_t per : {uint64_t(1), uint64_t(3), uint64_t(5), limit / 2 + 1, limit - 1, limit}) {
                const uint64_t step = hec::stripes_per_launch(limit, per);
                if (step != limit / per || step < 1) {
                    std::printf("FAIL stripes_per_launch(%llu, %llu)\n", (unsigned long long)limit,
                                (unsigned long long)per);
                    return 1;
                }
                if (sample(n, step, per, limit)) return 1;
            }
        }
    }
    std::printf("ok %ld pieces\n", checked);
    return 0;
}
