// Shared host/device declarations for the gfx950 RS kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "fastdiv.hpp"

namespace hec {

// One coding plan: nout output rows = coefficient matrix (nout x nin) applied
// to the nin input shards of a stripe. Encode is one plan (inputs = data
// shards, outputs = parity shards); decode has one plan per erasure pattern
// (inputs = first nin present shards, outputs = erased shards), matching
// upstream reconstruct's "first data_shard_count present shards" rule.
struct DevPlan {
    uint32_t nin;      // inputs (== data shard count)
    uint32_t nout;     // outputs; 0 = nothing to do (all shards present)
    uint32_t tab_off;  // word offset of this plan's tables: [nin][tab_rows][kTabWords]
    uint32_t idx_off;  // word offset of [nin] input shard ids then [nout] output ids
    uint32_t tab_rows; // table row stride (>= nout; padded rows hold coefficient 0)
    uint32_t pad[3];
};

constexpr uint32_t kNoPlan = 0xFFFFFFFFu;   // mask LUT entry: too few shards present
constexpr int kThreads = 256;               // 4 waves of 64 lanes
// Workgroups per launch: the dispatch packet's grid is 32-bit in work-items,
// so 2^23 workgroups (2^31 work-items at 256 threads) keeps every launch legal.
// HEC_MAX_LAUNCH_BLOCKS / HEC_LOCATE_MAX_BLOCKS: test builds only (the
// Makefile's smallgrid variant), so that batches of a few hundred stripes go
// in several launches, grid-stride iterations and mask rounds. The shipped
// library defines neither. Only rs_kernels.hip and rs_update_ragged.hip read
// the limits, the files that variant recompiles.
#ifdef HEC_MAX_LAUNCH_BLOCKS
constexpr uint64_t kMaxLaunchBlocks = HEC_MAX_LAUNCH_BLOCKS;
#else
constexpr uint64_t kMaxLaunchBlocks = 1ull << 23;
#endif
static_assert(kMaxLaunchBlocks >= 1 && kMaxLaunchBlocks <= (1ull << 23), "one launch: 1 to 2^23 workgroups");
constexpr int kVecBytes = 16;               // one dwordx4 per lane per access

struct ApplyArgs {
    const uint8_t* in_base;      // input shard (stripe s, id i) = in_base + s*in_stripe + i*in_shard
    uint64_t in_stripe;
    uint64_t in_shard;
    uint8_t* out_base;           // output shard (stripe s, id j) = out_base + s*out_stripe + j*out_shard
    uint64_t out_stripe;
    uint64_t out_shard;
    uint64_t len;                // shard length in bytes (same for every stripe of the batch)
    uint64_t n_items;            // n_stripes * chunks_per_stripe
    uint32_t chunks_per_stripe;  // ceil(len / chunk_bytes)
    uint32_t n_stripes;
    const DevPlan* plans;
    const uint32_t* tabs;
    const uint32_t* idx;
    const uint32_t* masks;       // optional per-stripe present mask (bit i = shard i present)
    const uint32_t* lut;         // mask -> plan id (used when masks != nullptr)
    uint32_t mask_limit;         // (1 << total shards) - 1: masks are clipped to the LUT
    uint32_t* bad_count;         // optional: stripes skipped for too few present shards
    uint32_t fast104;            // 1: RS(10,4) plan set with 4-row tables; encode = plan 0 at
                                 //    offset 0, decode = tables at lut[mask] * 200 words
    // Launcher-computed workgroup -> chunk map of the RS(10,4) fast paths, so
    // the kernels derive (stripe, chunk) in a few scalar ops with no division:
    uint32_t map_q8, map_r8;     // workgroups / 8 and % 8 (XCD eighths remap)
    uint32_t cps_mul, cps_shift; // item / chunks_per_stripe as a multiply-shift (FastDiv)
    // Optional completion signal (small host calls): the last workgroup of
    // the launch stores done_seq into done_flag (pinned host memory) after a
    // system-scope release, so the host spins on it instead of paying
    // hipStreamSynchronize. done_count: device word, 0 between launches.
    uint32_t* done_count;
    uint32_t* done_flag;
    uint32_t done_seq;
};

// Ragged RS(10,4) batch (every stripe its own length / stride / mask); all
// strides 16-byte aligned. Stripe s has shards at base + off + i*shard_stride
// and owns workgroups [first_block, first_block + ceil(len / 4 KiB)).
struct RaggedItem {
    uint64_t off;          // shard 0 (full layout) or input slot 0 (compact layout)
    uint64_t shard_stride;
    uint32_t len;
    uint32_t mask;         // present mask (decode); ignored by encode
    uint32_t first_block;
    uint32_t want;         // reconstruct some: erased shards worth rebuilding (bit i = shard i); else 0
    uint64_t out_off;      // compact decode: output slot 0 (erased shards, ascending)
};

struct RaggedArgs {
    uint8_t* base;
    const RaggedItem* items;
    const uint32_t* block_item;  // workgroup -> stripe index
    uint32_t n_blocks;
    const uint32_t* tabs;        // encode plan tables, or the dense decode set
    const uint32_t* lut;         // decode: mask -> plan id
    uint32_t* bad_count;
    uint32_t compact;            // decode: inputs = slots 0..9 at off (the first 10 present
                                 // shards), outputs = slots 0..e-1 at out_off (erased shards;
                                 // reconstruct some: the wanted ones of them only)
    uint32_t block_base;         // launcher-internal: first map entry of this launch
    uint32_t map_q8, map_r8;     // launcher-internal: that launch's workgroups / 8 and % 8
    uint32_t inline_one;         // 1: a single stripe, described by `one` (no items / map in memory)
    RaggedItem one;
    uint32_t* done_count;        // optional completion signal, as ApplyArgs
    uint32_t* done_flag;
    uint32_t done_seq;
};

hipError_t launch_rs104_ragged(const RaggedArgs& a, bool decode, hipStream_t stream);
// Ragged reconstruct some (hec.h hec_gpu_reconstruct_some_ragged): the decode
// with every item's want word; of a stripe's erased shards only the wanted
// ones are computed and stored. a.compact: the outputs at out_off are those
// shards alone, ascending, slot q at out_off + q * shard_stride. A stripe that
// wants none of its erased shards should own no map entry (its workgroups
// would leave at once).
hipError_t launch_rs104_ragged_some(const RaggedArgs& a, hipStream_t stream);
// Bit-sliced ragged encode: every stripe's length a multiple of kBsChunk bytes;
// the workgroup map has len / kBsChunk entries per stripe.
constexpr uint32_t kBsChunk = 2 * kThreads * kVecBytes;  // 8 KiB
// Column range of one workgroup of the 8-byte-per-lane table kernels.
constexpr uint32_t kNarrowChunk = kThreads * 8;  // 2 KiB
hipError_t launch_rs104_bs_ragged(const RaggedArgs& a, hipStream_t stream);

// Ragged update (hec.h hec_gpu_update_ragged): the update of UpdateArgs below
// with every stripe's own length, mask and place in three arenas. An item is
// hec_update_desc's fields plus first_block, a struct of its own: RaggedItem's
// 40 bytes are the indexing of the other ragged kernels. Parity shard j of the
// stripe is at a.base + par_off + j * par_stride; data shard c at new_base +
// new_off + c * new_stride and old_base + old_off + c * old_stride (read only
// with an old arena). a.compact (the host batch, no old arena): the new arena
// holds the shards of U alone, the q-th set bit of U at new_off + q * new_stride.
struct UpdateItem {
    uint64_t par_off, par_stride;
    uint64_t new_off, new_stride;
    uint64_t old_off, old_stride;
    uint32_t len;
    uint32_t mask;         // update mask; bits 10..31 mean nothing
    uint32_t first_block;
    uint32_t pad;
};
static_assert(sizeof(UpdateItem) == 64, "UpdateItem is indexed by the kernel and filled by the host");
// a: base = the parity arena, the workgroup map (one entry per 4 KiB column
// range of every stripe with U non-empty, none for the others), tabs = the
// RS(10,4) ENCODE plan's tables, the launcher's fields and the completion
// signal; a.items and a.one are not read (a.inline_one: `one` below).
struct RaggedUpdateArgs {
    RaggedArgs a;
    const uint8_t* new_base;
    const uint8_t* old_base;  // nullptr: old is zero
    const UpdateItem* items;
    UpdateItem one;
};
hipError_t launch_ragged_update(const RaggedUpdateArgs& v, hipStream_t stream);
// Name of the kernel launch_ragged_update runs without a.compact.
const char* ragged_update_kernel_name(bool has_old);


// Launch one coding pass. nin: number of inputs the caller guarantees (10
// selects the unrolled helyim RS(10,4) path; anything else the generic loop).
// over_pcie: an encode whose operands are host memory the kernel streams over
// PCIe (zero-copy host batches): the 8-byte-per-lane table encode where the
// shard length is a multiple of 2 KiB instead of the bit-sliced one (its
// narrower column range per workgroup ran 50.5-52.9 against 49.4-51.1 GiB/s
// in 7 alternating rounds on two boxes, profiles/r04/e2e_encode_kernels_{v,w}.jsonl).
hipError_t launch_apply(const ApplyArgs& a, int nin, bool aligned, bool over_pcie, hipStream_t stream);

// Name of the kernel an aligned RS(10,4) device encode of one stripe of this
// shard length runs under cfg (introspection for benchmarks and profiles; the
// same choice launch_apply makes, rs_kernels.hip rs104_pick).
const char* encode_kernel_name(uint64_t len, bool over_pcie);
// Same for an aligned in-place RS(10,4) device batch reconstruct.
const char* decode_kernel_name(uint64_t len);

// Reconstruct some (hec.h hec_gpu_reconstruct_some_batch) of a strided
// in-place RS(10,4) batch. a: a mask-driven decode's arguments over the dense
// decode plan set (in_* == out_*, masks, lut, bad_count); wants[s] bit i =
// shard i of stripe s is worth rebuilding. Of each stripe's erased shards only
// the wanted ones are computed and stored; a stripe that wants none is not
// read and not counted.
struct SomeArgs {
    ApplyArgs a;
    const uint32_t* wants;
};
hipError_t launch_some(const SomeArgs& v, bool aligned, hipStream_t stream);
// Name of the kernel an aligned reconstruct some of one stripe of this shard
// length runs, and of the kernel launch_some runs on a whole batch (its first
// stripe range where it goes in several).
const char* some_kernel_name(uint64_t len);
const char* some_batch_kernel_name(uint64_t len, uint64_t n_stripes, bool aligned);

// Update (hec.h hec_gpu_update_batch) of a strided RS(10,4) batch: for every
// stripe, parity ^= P[:,U] * (old[U] ^ new[U]), U = the data shards its mask
// word names (bits 0..9; the others mean nothing). a: in_* = the NEW data
// arena and out_* = the parity arena (read and written), both indexed from
// their own base (data shard c at in_base + s*in_stripe + c*in_shard, parity
// shard j at out_base + s*out_stripe + j*out_shard), masks = the update masks
// (device words), tabs = the RS(10,4) ENCODE plan's tables: column c's
// four-row table is tabs + c * 20 words. The old arena is indexed as the new
// one; old_base == nullptr: old is zero. A stripe with U empty is neither read
// nor written; no byte outside [0, len) of a parity shard is written.
struct UpdateArgs {
    ApplyArgs a;
    const uint8_t* old_base = nullptr;
    uint64_t old_stripe = 0, old_shard = 0;
};
constexpr uint32_t kUpdateBits = 0x3FFu;  // data shards 0..9; the other mask bits mean nothing
// aligned: every base and stride of the three arenas 16-byte aligned.
hipError_t launch_update(const UpdateArgs& v, bool aligned, hipStream_t stream);
// Name of the kernel an aligned update of one stripe of this shard length runs.
const char* update_kernel_name(uint64_t len);

// Parity verify (scrub) of a strided batch: the encode plan's parity is
// recomputed in registers and compared with the stored parity; nothing but
// the result words is written. a: the encode's arguments with out_* naming
// the STORED parity (read only) and bad_count the optional count of stripes
// with a non-zero word. mismatch[s] bit j = parity shard j of stripe s differs
// in at least one of its a.len bytes; the words must be zero at launch.
struct VerifyArgs {
    ApplyArgs a;
    uint32_t* mismatch;
    // launch_locate only (the verify kernels never read these):
    uint32_t* suspects = nullptr;          // one word per stripe, zero at launch
    const uint32_t* ratio_tabs = nullptr;  // [10 data shards][3][kTabWords]: P[j][c] / P[0][c], j = 1..3
    // launch_locate with pairs only: [4 syndrome rows][4][kTabWords] = T (classical
    // syndromes S = T * syn), then [2][14][kTabWords]: alpha_c^2 and alpha_c, c = 0..13
    const uint32_t* pair_tabs = nullptr;
};
// a.len is the TRUE shard length: bytes at or past it take no part (a length
// rounded up for a pitch would compare pad bytes).
hipError_t launch_verify(const VerifyArgs& v, int nin, bool aligned, hipStream_t stream);

// Locate (pass 2 of the RS(10,4) scrub, after launch_verify on the same
// stream filled v.mismatch): for every stripe with a non-zero mismatch word,
// the syndrome (stored parity XOR parity of the stored data) of each byte
// column is classified and the result ORed into v.suspects[stripe] (hec.h,
// hec_gpu_locate_corrupt_batch: bit c = shard c alone explains a column, bit
// 31 = a column no single shard explains). v.a: the RS(10,4) encode plan's
// arguments as for launch_verify; stripes whose mismatch word is 0 are not
// read. A grid-stride kernel over (stripe, 4 KiB chunk) items on at most
// kLocateMaxBlocks workgroups (a memory-bound grid-stride loop wants a few
// workgroups per CU, not one per item; speed only, unmeasured).
#ifdef HEC_LOCATE_MAX_BLOCKS
constexpr uint32_t kLocateMaxBlocks = HEC_LOCATE_MAX_BLOCKS;
#else
constexpr uint32_t kLocateMaxBlocks = 2048;
#endif
static_assert(kLocateMaxBlocks >= 1 && kLocateMaxBlocks <= (1u << 23), "locate grid: 1 to 2^23 workgroups");
constexpr uint32_t kSuspectUnexplained = 0x80000000u;  // hec.h HEC_SUSPECT_UNEXPLAINED
// pairs (hec.h hec_gpu_locate_corrupt_pairs_batch; needs v.pair_tabs): a column
// no single shard explains sets the bits of the two shards that do, bit 31
// only when no two do either. The same walk; the pair search runs behind a
// ballot of its own, only in waves that hold such a column.
hipError_t launch_locate(const VerifyArgs& v, bool aligned, bool pairs, hipStream_t stream);

// Correct (hec.h hec_gpu_correct_batch): launch_locate's pass with one
// addition -- where a column is explained, the error value is computed too and
// XORed into the wrong byte(s) of v.a.in_base / v.a.out_base, in place.
// Columns that set bit 31 are left as they are. The words are the locate's,
// of the bytes as they were.
constexpr int kFixInvU = 10 * 5;  // word offset of the second table set of fix_tabs
struct CorrectArgs : VerifyArgs {        // as for launch_locate (pair_tabs with pairs), and:
    const uint32_t* fix_tabs = nullptr;   // [10][kTabWords]: 1 / P[0][c]; then [14][kTabWords]: 1 / u_c
    uint32_t* uncorrected = nullptr;      // optional: += stripes that get bit 31
    unsigned long long* corrected_bytes = nullptr;  // optional: += bytes changed
};
hipError_t launch_correct(const CorrectArgs& c, bool aligned, bool pairs, hipStream_t stream);

// Present masks of a repair from the suspects words (hec_gpu_repair_batch):
// masks[s] = 0x3FFF & ~suspects[s] when the word names 1 to 4 shards and bit
// 31 is clear, else 0x3FFF (the reconstruct's no-op); *unrepaired (optional)
// += stripes with a non-zero word that are left alone.
hipError_t launch_repair_masks(const uint32_t* suspects, uint32_t* masks, uint32_t* unrepaired, uint32_t n_stripes,
                               hipStream_t stream);
// Name of the kernel an aligned RS(10,4) device verify of this shard length runs.
const char* verify_kernel_name(uint64_t len);

// Masked verify and locate (degraded scrub, RS(10,4); hec.h
// hec_gpu_verify_present_batch): the mask-driven decode with its stores
// replaced by a compare. Of a stripe's p >= 11 present shards the ten lowest
// (B) are the inputs, the other r = p - 10 (E) the stored rows; the "check"
// plan of a mask holds A_m (rows E of the encoding matrix times the inverse
// of rows B) as r rows of a 4-row table set, plan id = lut[mask], tables at
// plan id * 200 words. a: the in-place batch (in_* == out_*, only read), the
// check plan set, masks, lut, and bad_count = the optional count of stripes
// with a non-zero word. check[s] bit e (e in E) = syn row e is non-zero
// somewhere in the stripe; the words must be zero at launch. Stripes with
// p <= 10 are not read and add one to *unchecked (optional).
struct CheckArgs {
    ApplyArgs a;
    uint32_t* check;
    uint32_t* unchecked = nullptr;
    // launch_locate_present only (the check kernels never read these):
    uint32_t* suspects = nullptr;          // one word per stripe, zero at launch
    const uint32_t* ratio_tabs = nullptr;  // per plan [10][3][kTabWords]: A_m[j][c] / A_m[0][c], j = 1..r-1
};
hipError_t launch_check(const CheckArgs& v, bool aligned, hipStream_t stream);
// Pass 2 after launch_check on the same stream: rs104_locate_kernel's method
// with the stripe's own A_m, ratio tables and row count; stripes whose check
// word is 0 are not read. Same grid rule as launch_locate.
hipError_t launch_locate_present(const CheckArgs& v, bool aligned, hipStream_t stream);
// Masked correct (hec.h hec_gpu_correct_present_batch): launch_locate_present's
// pass with one addition -- where a column of a stripe with r >= min_spares is
// explained, the error value is computed too and XORed into the wrong byte of
// v.a.in_base, in place (the batch is one in-place layout: every shard id is
// addressed from in_base). Columns that set bit 31 and stripes with fewer
// spares are left as they are. The words are the locate's, of the bytes as
// they were.
struct CorrectPresentArgs : CheckArgs {  // as for launch_locate_present, and:
    const uint32_t* fix_tabs = nullptr;  // per plan [10][kTabWords]: 1 / A_m[0][c]
    uint32_t* uncorrected = nullptr;     // optional: += stripes left inconsistent (bit 31, or dirty with r < min_spares)
    unsigned long long* corrected_bytes = nullptr;  // optional: += bytes changed
    uint32_t min_spares = 2;             // 2..4: stripes with fewer spare shards are classified, not written
};
hipError_t launch_correct_present(const CorrectPresentArgs& v, bool aligned, hipStream_t stream);
// Use masks of a checked reconstruct (hec_gpu_reconstruct_checked_batch):
// use[s] = m = present[s] & 0x3FFF when check[s] == 0; m & ~suspects[s] when
// bit 31 is clear, a shard is named and at least 10 bits remain; else 0x3FFF
// (the reconstruct's no-op) and *unrepaired (optional) += 1.
hipError_t launch_use_masks(const uint32_t* present, const uint32_t* check, const uint32_t* suspects, uint32_t* use,
                            uint32_t* unrepaired, uint32_t n_stripes, hipStream_t stream);
// Use masks of a corrected reconstruct (hec_gpu_reconstruct_corrected_batch),
// after launch_correct_present with the same min_spares: use[s] = m when
// check[s] == 0, or when the stripe has min_spares or more spare shards and
// bit 31 of suspects[s] is clear (its survivors are consistent again: nothing
// is dropped); else 0x3FFF and *unrepaired (optional) += 1.
hipError_t launch_use_masks_corrected(const uint32_t* present, const uint32_t* check, const uint32_t* suspects,
                                      uint32_t* use, uint32_t* unrepaired, uint32_t min_spares, uint32_t n_stripes,
                                      hipStream_t stream);
// Name of the kernel an aligned masked verify of this shard length runs.
const char* check_kernel_name(uint64_t len);

// Ragged scrub (hec.h hec_gpu_verify_ragged / hec_gpu_locate_corrupt_ragged):
// the masked verify and locate over a ragged batch, every stripe with its own
// length and present mask (RaggedItem::mask). a: the batch, only read -- base,
// items, the workgroup map, tabs / lut = the check plan set (its dense LUT
// holds the full mask's plan too), bad_count = the optional count of stripes
// with a non-zero word. Stripes with 10 or fewer shards present own no map
// entry: they are never read, and the host counts them. check and suspects
// must be zero at launch.
struct RaggedScrubArgs {
    RaggedArgs a;
    uint32_t* check;                       // one word per stripe, bits by shard index
    uint32_t* suspects = nullptr;          // launch_ragged_locate only
    const uint32_t* ratio_tabs = nullptr;  // launch_ragged_locate only: CheckArgs::ratio_tabs
    uint32_t half_shift = 0;               // launch_ragged_locate sets it: 2^half_shift 4 KiB ranges per map entry
};
// Pass 1, one workgroup per map entry. bitslice: every mask full and every
// length a multiple of kBsChunk, the map in kBsChunk entries
// (rs104_bs_chunk<uint32_t, true>, its four bits moved to shards 10..13);
// otherwise 4 KiB entries and the table check over lut[mask], any length >= 1.
hipError_t launch_ragged_check(const RaggedScrubArgs& v, bool bitslice, hipStream_t stream);
// Name of the kernel launch_ragged_check runs.
const char* ragged_scrub_kernel_name(bool bitslice);
// Pass 2 after launch_ragged_check on the same stream and the same map:
// launch_locate_present's classification, a grid-stride loop over the map
// entries on at most kLocateMaxBlocks workgroups; an entry of a stripe whose
// check word is 0 costs two scalar loads. A bit-sliced map is walked as two
// 4 KiB halves per entry.
hipError_t launch_ragged_locate(const RaggedScrubArgs& v, bool bitslice, hipStream_t stream);
// Ragged correct (hec.h hec_gpu_correct_ragged): launch_ragged_locate's pass
// with launch_correct_present's addition -- where a column of a stripe with
// r >= min_spares is explained, the error value is XORed into the wrong byte
// of shard c at a.base + item.off + c * item.shard_stride, in place, bytes at
// or past the stripe's own length never written. The words are the locate's,
// of the bytes as they were.
struct RaggedCorrectArgs : RaggedScrubArgs {  // as for launch_ragged_locate, and:
    const uint32_t* fix_tabs = nullptr;  // CorrectPresentArgs::fix_tabs
    uint32_t* uncorrected = nullptr;     // optional: += stripes left inconsistent
    unsigned long long* corrected_bytes = nullptr;  // optional: += bytes changed
    uint32_t min_spares = 2;             // 2..4
};
hipError_t launch_ragged_correct(const RaggedCorrectArgs& v, bool bitslice, hipStream_t stream);
// Use masks of a corrected ragged reconstruct (hec_gpu_reconstruct_corrected_ragged),
// after launch_ragged_correct with the same min_spares: launch_use_masks_corrected's
// rule with the present masks read from the scrub's items. A stripe left alone
// also gets mask 0x3FFF in decode_items, the device copy of the items the
// ragged decode launched next on the stream reads: its workgroups do nothing.
hipError_t launch_ragged_use_masks_corrected(const RaggedItem* scrub_items, RaggedItem* decode_items,
                                             const uint32_t* check, const uint32_t* suspects, uint32_t* use,
                                             uint32_t* unrepaired, uint32_t min_spares, uint32_t n_stripes,
                                             hipStream_t stream);
// *word += n, in stream order (the ragged scrub's count of unchecked stripes).
hipError_t launch_add_word(uint32_t* word, uint32_t n, hipStream_t stream);

// splitmix64 byte stream per stripe (bench/test data generator):
// stripe s: bytes_per_stripe bytes at base + s*stripe_stride, word n (n>=1) =
// mix(seed_base + s + n*gamma), little endian.
hipError_t launch_fill_splitmix(uint8_t* base, uint64_t stripe_stride, uint64_t bytes_per_stripe,
                                uint32_t n_stripes, uint64_t seed_base, hipStream_t stream);

}  // namespace hec
