// Cutting a launch that is too large for one dispatch into pieces of at most
// `limit` workgroups (production: kMaxLaunchBlocks). Two shapes:
//   * a ragged batch is a run of n_blocks map entries: launch i takes entries
//     [i * limit, ...) and carries its own XCD eighths (map_q8 / map_r8);
//   * a strided batch whose kernel has no grid-stride loop goes in ranges of
//     whole stripes, floor(limit / per_stripe) stripes each.
// Pieces are addressed by index (n_ranges + range_at) so a caller loops and a
// test can look at any piece of 2^32 without walking them. Launches of one
// batch share a stream, so only the piece marked `last` signals completion.
// All arithmetic is 64-bit; the narrow fields hold values bounded by their
// 32-bit inputs. Plain C++ (no HIP headers) so tests/c/launch_split_check.cpp
// checks it with g++.
#pragma once
#include <cstdint>

namespace hec {

struct Range {
    uint32_t first, count;  // [first, first + count) of n
    bool last;
};

// Ranges of `step` (>= 1) consecutive elements covering [0, n), n < 2^32.
inline uint64_t n_ranges(uint64_t n, uint64_t step) { return n ? (n - 1) / step + 1 : 0; }

inline Range range_at(uint64_t n, uint64_t step, uint64_t i) {
    const uint64_t first = i * step;  // < n: no wrap for i < n_ranges
    const uint64_t count = n - first < step ? n - first : step;
    return Range{uint32_t(first), uint32_t(count), first + count == n};
}

// Stripes per launch of a kernel that runs per_stripe (1..limit) workgroups
// per stripe and one workgroup per chunk.
inline uint64_t stripes_per_launch(uint64_t limit, uint64_t per_stripe) { return limit / per_stripe; }

// Launch i of a ragged batch of n_blocks workgroups.
struct BlockLaunch {
    uint32_t block_base, n_blocks;  // first map entry and grid of this launch
    uint32_t map_q8, map_r8;        // n_blocks / 8 and % 8
    bool last;
};

inline BlockLaunch block_launch(uint64_t n_blocks, uint64_t limit, uint64_t i) {
    const Range r = range_at(n_blocks, limit, i);
    return BlockLaunch{r.first, r.count, r.count / 8, r.count % 8, r.last};
}

}  // namespace hec
