// gfx950 (CDNA4) kernels for the helyim-ec RS(10,4) hot path.
//
// Replaces the arithmetic of upstream reed-solomon-erasure's
// `ReedSolomon::encode` / `reconstruct` (called from
// /root/reference/helyim-ec/src/encoder.rs:191,288 and
// helyim-store/src/erasure_coding/mod.rs:426), whose CPU kernel is a pshufb
// nibble-table loop run 40 times per 256 KiB batch.
//
// Design (see DESIGN.md "Kernels"):
//  * One pass per stripe chunk: every input byte is read from HBM once and
//    every output byte written once (14 L bytes per encoded stripe), instead
//    of the CPU's 10 read-modify-write sweeps per output.
//  * GF(2^8) constant multiply as a byte-sliced SWAR lookup on whole dwords:
//    c*x = T0[x&7] ^ T1[(x>>3)&7] ^ T2[x>>6]; each table is <= 8 bytes, so one
//    v_perm_b32 performs four lookups. Three v_perm + 1.5 v_bitop3 (xor3) per
//    coefficient per dword; selectors are shared by all output rows.
//  * Tables and shard ids are wave-uniform -> scalar loads (SGPRs); only the
//    data is vector traffic: coalesced loads and stores (1 KiB per wave
//    instruction at 16 B per lane), non-temporal since every byte is touched
//    once.
//  * The encode of shard lengths that are a multiple of 8 KiB is bit-sliced
//    (rs104_bs_encode_kernel): the fixed parity matrix as a generated XOR
//    program over bit planes, half the table multiply's VALU work.
//  * The parity verify (scrub) kernels have no coding body of their own:
//    rs104_bs_chunk and apply_group take a compile-time VERIFY flag that
//    turns their stores into a compare with the stored rows.
//  * The locate kernel (rs104_locate_kernel) is the scrub's second pass: it
//    reads only the stripes the verify flagged and names the wrong shard of
//    each byte column from its syndrome; its PAIRS form also names two wrong
//    shards of a column (an error-locator step on the bytes left unexplained);
//    its CORRECT form (rs104_correct_kernel) also fixes, in place, every byte
//    the names explain.
//  * The masked verify and locate (rs104_check_kernel and siblings) are the
//    degraded scrub: the mask-driven decode with its stores replaced by a
//    compare against the spare present shards.
//  * The ragged scrub (rs104_bs_ragged_verify_kernel, rs104_ragged_check_kernel
//    and the masked locate's RAGGED walk) is that scrub over stripes of mixed
//    lengths and masks: the ragged workgroup map in front of the same bodies;
//    with CORRECT too (rs104_ragged_correct_kernel) the walk fixes in place.
//  * Reconstruct some (rs104_some_kernel and siblings) is the decode with a
//    want word per stripe: a compile-time SOME form of the decode bodies picks
//    the wanted rows of the mask's plan with scalar work, so only those rows
//    are computed and stored.
//  * The update (rs104_update_kernel) folds changed data shards into the
//    stored parity: the encode plan's column tables over old ^ new of the
//    shards a per-stripe mask names, XORed into the four parity shards. The
//    ragged update (rs104_ragged_update_kernel, rs_update_ragged.hip) is that
//    body behind the ragged workgroup map, every stripe with its own length
//    and place in three arenas.
//
// Every kernel here is a product path: rs104_pick / ragged_pick choose among
// them by shard length, alignment and where the bytes live. Variants measured
// and not kept (XOR-only twins, the pair kernel, chunk rotation,
// 128/512/1024-thread launches, 4 B and 8 B-load variants, occupancy caps, the
// round-6 32-byte-per-lane table decode) are in git history and
// profiles/r0*/INDEX.md; the math-free stream ceilings live in
// tools/membench.hip.
#include <algorithm>
#include <type_traits>

#include "rs_kernels.hpp"
#include "bitslice.hpp"
#include "launch_split.hpp"
#include "rs_device.hpp"

namespace hec {

// One group of R (<= 4) output rows of a plan, one 16-byte vector per lane.
// K > 0: compile-time input count (all K loads issued before any math);
// K == 0: runtime nin loop. Lanes whose vector crosses the end of the shard
// take the byte-wise tail path (only in the last chunk of a stripe).
// VERIFY: the rows at out_b are the STORED rows and are only read; bit r of
// the result is set when row r of the group differs in this lane's vector
// (the encode form returns 0). The last vector of a shard goes through
// load_tail for data and stored rows alike, which zero-fills from a.len on:
// the recomputed parity of zero bytes is zero, so bytes at or past a.len
// compare equal whatever the memory there holds.
template <int K, int R, bool ALIGNED, bool VERIFY = false>
__device__ __forceinline__ uint32_t apply_group(const ApplyArgs& a, const uint8_t* in_b, uint8_t* out_b,
                                                cu32p in_ids, cu32p out_ids, cu32p tab, uint32_t nin,
                                                uint32_t tab_row_stride, uint64_t chunk_off) {
    const uint64_t o = chunk_off + threadIdx.x * kVecBytes;
    if (o >= a.len) return 0;
    const uint64_t avail = a.len - o;
    u32x4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = u32x4{0, 0, 0, 0};
    uint32_t differs = 0;
    if (avail >= kVecBytes) {
        if constexpr (K > 0) {
            u32x4 d[K];
#pragma unroll
            for (int i = 0; i < K; ++i) d[i] = load_full(in_b + uint64_t(in_ids[i]) * a.in_shard + o, ALIGNED);
#pragma unroll
            for (int i = 0; i < K; ++i) gf_mac<R>(acc, d[i], tab + i * tab_row_stride);
        } else {
            for (uint32_t i = 0; i < nin; ++i) {
                const u32x4 d = load_full(in_b + uint64_t(in_ids[i]) * a.in_shard + o, ALIGNED);
                gf_mac<R>(acc, d, tab + i * tab_row_stride);
            }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            uint8_t* row = out_b + uint64_t(out_ids[r]) * a.out_shard + o;
            if constexpr (VERIFY) {
                const u32x4 x = acc[r] ^ load_full(row, ALIGNED);
                differs |= ((x[0] | x[1] | x[2] | x[3]) != 0 ? 1u : 0u) << r;
            } else {
                store_full(row, acc[r], ALIGNED);
            }
        }
    } else {
        for (uint32_t i = 0; i < nin; ++i) {
            const u32x4 d = load_tail(in_b + uint64_t(in_ids[i]) * a.in_shard + o, avail);
            gf_mac<R>(acc, d, tab + i * tab_row_stride);
        }
        for (int r = 0; r < R; ++r) {
            uint8_t* row = out_b + uint64_t(out_ids[r]) * a.out_shard + o;
            if constexpr (VERIFY) {
                const u32x4 x = acc[r] ^ load_tail(row, avail);
                differs |= ((x[0] | x[1] | x[2] | x[3]) != 0 ? 1u : 0u) << r;
            } else {
                store_tail(row, acc[r], avail);
            }
        }
    }
    return differs;
}

// The row groups of one plan over one (stripe, 4 KiB chunk) item: four output
// rows at a time through apply_group, the last group with what is left.
// Returns the lane's mismatch bits (bit j = output row j), 0 for the encode.
template <int K, bool ALIGNED, bool VERIFY = false>
__device__ __forceinline__ uint32_t apply_rows(const ApplyArgs& a, const uint8_t* in_b, uint8_t* out_b, cu32p in_ids,
                                               cu32p out_ids, cu32p tab, const DevPlan& p, uint32_t row_stride,
                                               uint64_t chunk_off) {
    uint32_t differs = 0;
    for (uint32_t g = 0; g < p.nout; g += 4) {
        const uint32_t R = p.nout - g < 4 ? p.nout - g : 4;
        cu32p tg = tab + g * 5;
        uint32_t f;
        switch (R) {
            case 4: f = apply_group<K, 4, ALIGNED, VERIFY>(a, in_b, out_b, in_ids, out_ids + g, tg, p.nin, row_stride, chunk_off); break;
            case 3: f = apply_group<K, 3, ALIGNED, VERIFY>(a, in_b, out_b, in_ids, out_ids + g, tg, p.nin, row_stride, chunk_off); break;
            case 2: f = apply_group<K, 2, ALIGNED, VERIFY>(a, in_b, out_b, in_ids, out_ids + g, tg, p.nin, row_stride, chunk_off); break;
            default: f = apply_group<K, 1, ALIGNED, VERIFY>(a, in_b, out_b, in_ids, out_ids + g, tg, p.nin, row_stride, chunk_off); break;
        }
        if constexpr (VERIFY) differs |= f << g;
    }
    return differs;
}

// First item of a workgroup's grid-stride loop. XCD-aware chunk mapping:
// workgroups b, b+8, b+16, ... are dealt to one XCD (MI355X_MICROARCH.md,
// dispatch), so a bijective remap hands them consecutive chunks. Speed only:
// correctness never depends on placement.
__device__ __forceinline__ uint64_t stride_first_item() {
    const uint32_t nb = gridDim.x, q = nb / 8, r = nb % 8, x = blockIdx.x % 8;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + blockIdx.x / 8;
}

// Generic plan interpreter (any k + m <= 256, unaligned bases and strides,
// ad-hoc host plans): grid-stride over (stripe, 4 KiB chunk) items.
template <int K, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void rs_apply_kernel(ApplyArgs a) {
    for (uint64_t item = stride_first_item(); item < a.n_items; item += gridDim.x) {
        const uint32_t stripe = uint32_t(item / a.chunks_per_stripe);
        const uint32_t chunk = uint32_t(item - uint64_t(stripe) * a.chunks_per_stripe);
        uint32_t pid = 0;
        if (a.masks) {
            pid = as_const(a.lut)[as_const(a.masks)[stripe] & a.mask_limit];
            if (pid == kNoPlan) {
                if (chunk == 0 && threadIdx.x == 0 && a.bad_count) atomicAdd(a.bad_count, 1u);
                continue;
            }
        }
        const __attribute__((address_space(4))) DevPlan* pp = as_const(a.plans) + pid;
        const DevPlan p{pp->nin, pp->nout, pp->tab_off, pp->idx_off, pp->tab_rows, {0, 0, 0}};
        if (p.nout == 0) continue;
        const uint8_t* in_b = a.in_base + uint64_t(stripe) * a.in_stripe;
        uint8_t* out_b = a.out_base + uint64_t(stripe) * a.out_stripe;
        cu32p in_ids = as_const(a.idx) + p.idx_off;
        cu32p out_ids = in_ids + p.nin;
        cu32p tab = as_const(a.tabs) + p.tab_off;
        const uint32_t row_stride = p.tab_rows * 5;  // words per input
        const uint64_t chunk_off = uint64_t(chunk) * (kThreads * kVecBytes);
        apply_rows<K, ALIGNED>(a, in_b, out_b, in_ids, out_ids, tab, p, row_stride, chunk_off);
    }
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

// ---------------------------------------------------------------------------
// RS(10,4) fast paths (k = 10, n = 14, 16-byte aligned strides): the shard ids
// come from kernel arguments (encode) or straight from the stripe's present
// mask with scalar bit scans (decode), so a workgroup issues its ten loads
// after at most ONE scalar load; the coefficient tables (fixed stride of 4
// rows x 5 words per input) arrive in parallel with the data.
// ---------------------------------------------------------------------------
// Workgroup -> (stripe, chunk). Workgroups b, b+8, b+16, ... are dealt to one
// XCD (observed round-robin dispatch; MI355X_MICROARCH.md), so XCD x = b % 8
// takes the contiguous x-th eighth of all chunks (+5-9% over dispatch order):
// item = x*q + min(x, r) + b/8 from the launcher's constants (map_q8 / map_r8),
// then the chunks per stripe as a multiply-shift divisor (FastDiv): a handful
// of scalar ops from blockIdx, no division, so a workgroup reaches its
// stripe's mask load (decode) or its first data load (encode) a few cycles
// after launch. A bijection: speed only, never correctness.
__device__ __forceinline__ void fast_item(const ApplyArgs& a, uint32_t per_stripe, uint32_t& stripe,
                                          uint32_t& chunk) {
    // Every kernel argument the workgroup will need, in SGPRs at entry: one
    // round trip, instead of loads the compiler sinks behind the decode's
    // mask checks (each a further trip).
    asm volatile("" ::"s"(a.in_base), "s"(a.in_stripe), "s"(a.in_shard), "s"(a.out_base), "s"(a.out_stripe),
                 "s"(a.out_shard), "s"(a.len), "s"(a.masks), "s"(a.lut), "s"(a.tabs), "s"(a.map_q8),
                 "s"(a.map_r8), "s"(a.cps_mul), "s"(a.cps_shift), "s"(a.chunks_per_stripe));
    const uint32_t b = blockIdx.x, x = b & 7u, q = a.map_q8, r = a.map_r8;
    const uint32_t item = x * q + (x < r ? x : r) + (b >> 3);
    stripe = fastdiv(item, a.cps_mul, a.cps_shift);
    chunk = item - stripe * per_stripe;
}

// One 4 KiB chunk of one RS(10,4) stripe. Encode (DEC=false): inputs 0..9 at
// in_b, outputs 0..3 at out_b. Decode (DEC=true): in place at in_b == out_b
// (or COMPACT: inputs are slots 0..9 at in_b, outputs slots 0..e-1 at out_b),
// shard ids from the present mask, tables at lut[mask] * 200 words.
// OffT: type of the lane's byte offset in the shard. uint32_t (every ragged
// stripe, and strided batches of shards below 4 GiB) lets each load address
// be a scalar shard base plus a 32-bit lane offset (global_load saddr form:
// no per-load 64-bit VALU address math).
// SOME (a decode, hec.h hec_gpu_reconstruct_some_batch): only the erased
// shards named in `want` are computed and stored (some_rows); a stripe that
// wants none of its erased shards leaves before the mask is judged, so it is
// neither read nor counted. COMPACT then holds the wanted outputs only, slot q
// = the q-th wanted erased shard.
template <bool DEC, bool COMPACT = false, typename OffT = uint64_t, bool SOME = false>
__device__ __forceinline__ void rs104_chunk(const uint8_t* in_b, uint8_t* out_b, uint64_t in_shard,
                                            uint64_t out_shard, uint64_t len, uint32_t chunk, uint32_t mask_in,
                                            cu32p tab, cu32p lut, uint32_t* bad_count, uint32_t want = 0) {
    static_assert(DEC || !SOME, "reconstruct some is a decode");
    constexpr int K = 10, N = 14, R = 4;
    uint32_t in_id[K], out_id[R];
    [[maybe_unused]] uint32_t row[R] = {0, 0, 0, 0};
    uint32_t nout = R;
    uint32_t mask = 0, plan = 0;
    if constexpr (DEC) {
        mask = mask_in & ((1u << N) - 1);
        const uint32_t present = __builtin_popcount(mask);
        if constexpr (SOME) {
            if ((want & ~mask & ((1u << N) - 1)) == 0) return;
        }
        if (present < K) {
            if (chunk == 0 && threadIdx.x == 0 && bad_count) atomicAdd(bad_count, 1u);
            return;
        }
        if (present == N) return;  // upstream: all present -> no-op
        nout = N - present;
        uint32_t m = mask;
#pragma unroll
        for (int i = 0; i < K; ++i) {  // first K present shards, ascending
            in_id[i] = COMPACT ? i : __builtin_ctz(m);
            m &= m - 1;
        }
        uint32_t e = ~mask & ((1u << N) - 1);
        if constexpr (SOME) {  // the wanted erased shards, ascending, and their plan rows
            const SomeRows sr = some_rows(e, want);
            nout = sr.nout;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                out_id[r] = COMPACT ? r : sr.out[r];
                row[r] = sr.row[r];
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {  // erased shards, ascending
                out_id[r] = COMPACT ? r : (e ? __builtin_ctz(e) : 0);
                e &= e - 1;
            }
        }
        // plan lookup issued now; its value is first needed after the data
        // loads, so the scalar round trip overlaps them
        plan = lut[mask];
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) in_id[i] = i;
#pragma unroll
        for (int r = 0; r < R; ++r) out_id[r] = r;
    }
    const OffT o = OffT(chunk) * OffT(kThreads * kVecBytes) + OffT(threadIdx.x * kVecBytes);
    if (o >= len) return;
    const uint64_t avail = len - o;
    u32x4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = u32x4{0, 0, 0, 0};
    if (avail >= kVecBytes) {
        u32x4 d[K];
#pragma unroll
        for (int i = 0; i < K; ++i) d[i] = load_at(in_b + uint64_t(in_id[i]) * in_shard, o);
        // all ten loads in flight before any math: without this fence the
        // scheduler interleaves them with the table multiply two at a time
        // (36 VGPRs, but one wave then waits on HBM five times per chunk;
        // -5% decode time with it, profiles/r02/ab_loads_first.txt)
        __builtin_amdgcn_sched_barrier(0);
        // opaque here: the table address math (and so the wait for the plan
        // lookup) cannot be hoisted above the data loads
        if constexpr (DEC) {
            asm volatile("" : "+s"(plan));
            tab += plan * (K * R * 5);
        }
#pragma unroll
        for (int i = 0; i < K; i += 2)
            gf_mac2<R, u32x4, SOME>(acc, d[i], d[i + 1], tab + i * (R * 5), tab + (i + 1) * (R * 5), nout, row);
        // Materialise every row before the uniform `r < nout` store branches:
        // otherwise the compiler sinks each row's math into its branch, keeps
        // all 200 table words live and spills SGPRs (154 VGPRs, 3 waves/SIMD).
#pragma unroll
        for (int r = 0; r < R; ++r) asm volatile("" ::"v"(acc[r]));
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < int(nout)) store_at(out_b + uint64_t(out_id[r]) * out_shard, o, acc[r]);
    } else {
        if constexpr (DEC) {
            asm volatile("" : "+s"(plan));
            tab += plan * (K * R * 5);
        }
        for (int i = 0; i < K; ++i) {
            const u32x4 d = load_tail(in_b + uint64_t(in_id[i]) * in_shard + o, avail);
            if constexpr (SOME)
                gf_mac_rows<R>(acc, d, tab + i * (R * 5), row);
            else
                gf_mac<R>(acc, d, tab + i * (R * 5));
        }
        for (int r = 0; r < R; ++r)
            if (r < int(nout)) store_tail(out_b + uint64_t(out_id[r]) * out_shard + o, acc[r], avail);
    }
}

// 16 bytes per lane, one 4 KiB column range per workgroup: the aligned
// RS(10,4) encodes the bit-sliced kernel does not take and the decodes of
// shard lengths that are not a multiple of 2 KiB. OffT = uint64_t for shards
// of 4 GiB and more.
template <bool DEC, typename OffT>
__global__ __launch_bounds__(kThreads) void rs104_kernel(ApplyArgs a) {
    uint32_t stripe, chunk;
    fast_item(a, a.chunks_per_stripe, stripe, chunk);
    const uint32_t mask = DEC ? as_const(a.masks)[stripe] : 0u;
    rs104_chunk<DEC, false, OffT>(a.in_base + uint64_t(stripe) * a.in_stripe,
                                  a.out_base + uint64_t(stripe) * a.out_stripe, a.in_shard, a.out_shard, a.len,
                                  chunk, mask, as_const(a.tabs), as_const(a.lut), a.bad_count);
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

// RS(10,4) with 8 bytes per lane (2 KiB column range per workgroup, dwordx2
// streams): less math per wave between its loads and its stores, 54 VGPRs
// (8 waves/SIMD) instead of 100. The decode of shard lengths that are a
// multiple of 2 KiB (0.9-1.7% faster than 16 B, profiles/r02/
// ab_decode_bytes_per_lane.jsonl), and the zero-copy host encode over PCIe
// (DEC=false: inputs 0..9, outputs 0..3; profiles/r04/e2e_encode_kernels_*).
// Shards below 4 GiB (32-bit lane offsets).
// SOME: rs104_chunk's, the rows of `want` only.
template <bool DEC, bool SOME = false>
__device__ __forceinline__ void rs104_narrow_chunk(const uint8_t* in_b, uint8_t* out_b, uint64_t in_shard,
                                                   uint64_t out_shard, uint32_t chunk, uint32_t mask_in, cu32p tabs,
                                                   cu32p lut, uint32_t* bad_count, uint32_t want = 0) {
    static_assert(DEC || !SOME, "reconstruct some is a decode");
    typedef u32x2 V;
    constexpr int K = 10, N = 14, R = 4, VB = int(sizeof(V));
    uint32_t in_id[K], out_id[R];
    [[maybe_unused]] uint32_t row[R] = {0, 0, 0, 0};
    uint32_t nout = R, plan = 0;
    bool work = true;
    if constexpr (DEC) {
        const uint32_t mask = mask_in & ((1u << N) - 1);
        const uint32_t present = __builtin_popcount(mask);
        uint32_t e = ~mask & ((1u << N) - 1);
        if constexpr (SOME) {
            if ((want & e) == 0) return;  // nothing wanted: not read, not counted
        }
        if (present < K && chunk == 0 && threadIdx.x == 0 && bad_count) atomicAdd(bad_count, 1u);
        work = present >= K && present < N;  // too few: skipped + counted; all present: upstream no-op
        nout = N - present;
        uint32_t m = mask;
#pragma unroll
        for (int i = 0; i < K; ++i) {  // first K present shards, ascending
            in_id[i] = m ? __builtin_ctz(m) : 0;
            m &= m - 1;
        }
        if constexpr (SOME) {  // the wanted erased shards, ascending, and their plan rows
            const SomeRows sr = some_rows(e, want);
            nout = sr.nout;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                out_id[r] = sr.out[r];
                row[r] = sr.row[r];
            }
        } else {
#pragma unroll
            for (int r = 0; r < R; ++r) {  // erased shards, ascending
                out_id[r] = e ? __builtin_ctz(e) : 0;
                e &= e - 1;
            }
        }
        if (work) plan = lut[mask];  // first used after the data loads
    } else {
#pragma unroll
        for (int i = 0; i < K; ++i) in_id[i] = i;
#pragma unroll
        for (int r = 0; r < R; ++r) out_id[r] = r;
    }
    if (work) {
        const uint32_t o = chunk * (kThreads * VB) + threadIdx.x * VB;
        V d[K];
#pragma unroll
        for (int i = 0; i < K; ++i)
            d[i] = __builtin_nontemporal_load(
                (const __attribute__((address_space(1))) V*)((gcu8p)(in_b + uint64_t(in_id[i]) * in_shard) + o));
        __builtin_amdgcn_sched_barrier(0);  // all ten loads in flight before the math
        asm volatile("" : "+s"(plan));
        cu32p tab = tabs + plan * (K * R * 5);
        V acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = V(0u);
#pragma unroll
        for (int i = 0; i < K; i += 2)
            gf_mac2<R, V, SOME>(acc, d[i], d[i + 1], tab + i * (R * 5), tab + (i + 1) * (R * 5), nout, row);
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int w = 0; w < VB / 4; ++w) asm volatile("" ::"v"(acc[r][w]));
#pragma unroll
        for (int r = 0; r < R; ++r)
            if (r < int(nout))
                __builtin_nontemporal_store(
                    acc[r], (__attribute__((address_space(1))) V*)((gu8p)(out_b + uint64_t(out_id[r]) * out_shard) + o));
    }
}

template <bool DEC>
__global__ __launch_bounds__(kThreads) void rs104_narrow_kernel(ApplyArgs a) {
    uint32_t stripe, chunk;
    fast_item(a, a.chunks_per_stripe, stripe, chunk);
    const uint32_t mask = DEC ? as_const(a.masks)[stripe] : 0u;
    rs104_narrow_chunk<DEC>(a.in_base + uint64_t(stripe) * a.in_stripe, a.out_base + uint64_t(stripe) * a.out_stripe,
                            a.in_shard, a.out_shard, chunk, mask, as_const(a.tabs), as_const(a.lut), a.bad_count);
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

// Reconstruct some (hec.h hec_gpu_reconstruct_some_batch): the two in-place
// decodes above with a want word per stripe beside its mask, the SOME form of
// their chunk bodies. The want word rides the mask's scalar round trip.
template <typename OffT>
__global__ __launch_bounds__(kThreads) void rs104_some_kernel(SomeArgs v) {
    const ApplyArgs& a = v.a;
    uint32_t stripe, chunk;
    fast_item(a, a.chunks_per_stripe, stripe, chunk);
    const uint32_t mask = as_const(a.masks)[stripe], want = as_const(v.wants)[stripe];
    uint8_t* b = a.out_base + uint64_t(stripe) * a.out_stripe;
    rs104_chunk<true, false, OffT, true>(b, b, a.in_shard, a.out_shard, a.len, chunk, mask, as_const(a.tabs),
                                         as_const(a.lut), a.bad_count, want);
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

__global__ __launch_bounds__(kThreads) void rs104_narrow_some_kernel(SomeArgs v) {
    const ApplyArgs& a = v.a;
    uint32_t stripe, chunk;
    fast_item(a, a.chunks_per_stripe, stripe, chunk);
    const uint32_t mask = as_const(a.masks)[stripe], want = as_const(v.wants)[stripe];
    uint8_t* b = a.out_base + uint64_t(stripe) * a.out_stripe;
    rs104_narrow_chunk<true, true>(b, b, a.in_shard, a.out_shard, chunk, mask, as_const(a.tabs), as_const(a.lut),
                                   a.bad_count, want);
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

// Reconstruct some on layouts the two kernels above do not take (unaligned
// bases or strides, batches rs104_pick sends to rs_apply_kernel): grid-stride
// over (stripe, 4 KiB chunk) items of the dense decode plan set, one
// apply_group of one row per wanted erased shard. The ten inputs are read once
// per wanted row, again from cache after the first: the traffic saving of the
// aligned kernels does not hold here, the footprint does.
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void rs_some_kernel(SomeArgs v) {
    const ApplyArgs& a = v.a;
    for (uint64_t item = stride_first_item(); item < a.n_items; item += gridDim.x) {
        const uint32_t stripe = uint32_t(item / a.chunks_per_stripe);
        const uint32_t chunk = uint32_t(item - uint64_t(stripe) * a.chunks_per_stripe);
        const uint32_t mask = as_const(a.masks)[stripe] & a.mask_limit;
        const uint32_t erased = ~mask & a.mask_limit;
        uint32_t w = as_const(v.wants)[stripe] & erased;
        if (w == 0) continue;  // nothing wanted: not read, not counted
        const uint32_t pid = as_const(a.lut)[mask];
        if (pid == kNoPlan) {
            if (chunk == 0 && threadIdx.x == 0 && a.bad_count) atomicAdd(a.bad_count, 1u);
            continue;
        }
        const __attribute__((address_space(4))) DevPlan* pp = as_const(a.plans) + pid;
        const uint32_t nin = pp->nin, row_stride = pp->tab_rows * 5;
        const uint8_t* in_b = a.in_base + uint64_t(stripe) * a.in_stripe;
        uint8_t* out_b = a.out_base + uint64_t(stripe) * a.out_stripe;
        cu32p in_ids = as_const(a.idx) + pp->idx_off;
        cu32p out_ids = in_ids + nin;  // the erased shards, ascending: entry `row` is the shard of that rank
        cu32p tab = as_const(a.tabs) + pp->tab_off;
        const uint64_t chunk_off = uint64_t(chunk) * (kThreads * kVecBytes);
        for (; w; w &= w - 1) {
            const uint32_t row = __builtin_popcount(erased & ((1u << __builtin_ctz(w)) - 1));
            apply_group<10, 1, ALIGNED>(a, in_b, out_b, in_ids, out_ids + row, tab + row * 5, nin, row_stride,
                                        chunk_off);
        }
    }
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

// ---------------------------------------------------------------------------
// Bit-sliced RS(10,4) encode (fixed parity matrix). A lane owns 32 bytes of
// every shard (two 16-byte vectors 4 KiB apart, so each load instruction stays
// one contiguous 1 KiB per wave). Its 8 dwords per shard are transposed into 8
// bit planes (plane k = bit k of the 32 bytes), the 80 data planes go through
// the generated XOR program (tools/gen_bitslice.py: 328 three-input XORs for
// all 32 parity planes), and the parity planes are transposed back. Per data
// dword that is ~12.5 VALU ops against ~27 for the table-lookup multiply, so
// the math hides at lower occupancy (170 VGPRs, 2 waves/SIMD).
// ---------------------------------------------------------------------------
// One 8 KiB column range (`chunk`) of one stripe: inputs 0..9 at in_b, parity
// 0..3 at out_b. VERIFY: out_b holds the STORED parity, which is read and
// compared instead of written; the result is the wave's mismatch bits (bit j =
// parity row j differs somewhere in the wave's 2 KiB), 0 for the encode. The
// parity loads are written with the data loads and left to the scheduler,
// which issues them after the XOR program: 171 VGPRs, no scratch, 2 waves/SIMD
// as the encode. Pinned up front with a sched_barrier (28 loads in flight, 196
// VGPRs) it measured no different within the run-to-run spread
// (profiles/verify/ab_parity_load_placement.jsonl).
// out_off is added to out_b here. The verify hands over its stripe offset
// this way: with the stripe's parity pointer formed in the caller's argument
// list (the same IR but for the place of that one add) the backend schedules
// the parity address math ahead of the data loads, a different instruction
// stream that ran 9.21-9.50 ms against 8.81-8.95 in three alternating
// processes each (profiles/verify/refactor_ab.jsonl, ab "by_pointer"; a second
// session's process-to-process spread was as wide as that gap, so the timing
// alone does not settle it). In this form the verify kernel's instructions are
// those of the separate kernel it replaces, up to the operand order of
// commutative ops (profiles/verify/refactor_isa.md). The encode callers pass
// their pointer and no offset, as they always have.
template <typename OffT = uint64_t, bool VERIFY = false>
__device__ __forceinline__ uint32_t rs104_bs_chunk(const uint8_t* in_b, uint8_t* out_b, uint64_t in_shard,
                                                   uint64_t out_shard, uint32_t chunk, uint64_t out_off = 0) {
    constexpr int K = 10, R = 4;
    out_b += out_off;
    const OffT base = OffT(chunk) * OffT(kBsChunk) + OffT(threadIdx.x * 16);
    uint32_t p[K * 8];
    u32x4 d[K][2];
    [[maybe_unused]] u32x4 s[R][2];
#pragma unroll
    for (int i = 0; i < K; ++i) {
        d[i][0] = load_at(in_b + uint64_t(i) * in_shard, base);
        d[i][1] = load_at(in_b + uint64_t(i) * in_shard, base + OffT(kThreads * 16));
    }
    if constexpr (VERIFY) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            s[j][0] = load_at(out_b + uint64_t(j) * out_shard, base);
            s[j][1] = load_at(out_b + uint64_t(j) * out_shard, base + OffT(kThreads * 16));
        }
    }
#pragma unroll
    for (int i = 0; i < K; ++i)
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            p[8 * i + w] = d[i][0][w];
            p[8 * i + 4 + w] = d[i][1][w];
        }
#pragma unroll
    for (int i = 0; i < K; ++i) transpose8(p + 8 * i);
    uint32_t q[R * 8];
    rs104_encode_planes(p, q);
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        transpose8(q + 8 * j);
        if constexpr (VERIFY) {
            uint32_t x = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) x |= (q[8 * j + w] ^ s[j][0][w]) | (q[8 * j + 4 + w] ^ s[j][1][w]);
            bits |= (__ballot(x != 0) != 0 ? 1u : 0u) << j;
        } else {
            store_at(out_b + uint64_t(j) * out_shard, base, u32x4{q[8 * j], q[8 * j + 1], q[8 * j + 2], q[8 * j + 3]});
            store_at(out_b + uint64_t(j) * out_shard, base + OffT(kThreads * 16),
                     u32x4{q[8 * j + 4], q[8 * j + 5], q[8 * j + 6], q[8 * j + 7]});
        }
    }
    return bits;
}

template <typename OffT>
__global__ __launch_bounds__(kThreads) void rs104_bs_encode_kernel(ApplyArgs a) {
    uint32_t stripe, chunk;
    fast_item(a, a.chunks_per_stripe, stripe, chunk);
    rs104_bs_chunk<OffT>(a.in_base + uint64_t(stripe) * a.in_stripe, a.out_base + uint64_t(stripe) * a.out_stripe,
                         a.in_shard, a.out_shard, chunk);
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

// Descriptor of the stripe workgroup blk works on: the kernel-argument copy
// for a one-stripe launch, else the workgroup map and item table (scalar loads).
// WANT: also the want word of a reconstruct-some item (RaggedItem::pad); the
// other kernels never load it.
template <bool WANT = false>
__device__ __forceinline__ RaggedItem ragged_item(const RaggedArgs& a, uint32_t blk) {
    if (a.inline_one) return a.one;
    const __attribute__((address_space(4))) RaggedItem* p = as_const(a.items) + as_const(a.block_item)[blk];
    return RaggedItem{p->off, p->shard_stride, p->len, p->mask, p->first_block, WANT ? p->want : 0, p->out_off};
}

// Ragged encode with every stripe length a multiple of 8 KiB: workgroup ->
// stripe map as rs104_ragged_kernel, one 8 KiB column range per workgroup.
__global__ __launch_bounds__(kThreads) void rs104_bs_ragged_kernel(RaggedArgs a) {
    const uint32_t blk = ragged_block(a);
    const RaggedItem it = ragged_item(a, blk);
    const uint64_t off = it.off, stride = it.shard_stride;
    const uint32_t first = it.first_block;
    const uint8_t* b = a.base + off;
    rs104_bs_chunk<uint32_t>(b, a.base + off + 10 * stride, stride, stride, blk - first);
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

hipError_t launch_rs104_bs_ragged(const RaggedArgs& a, hipStream_t stream) {
    return launch_ragged(rs104_bs_ragged_kernel, a, stream);
}

// Ragged batches: every stripe has its own length, shard stride and mask
// (degraded reads of needle intervals, mixed 64 KiB-4 MiB stripes). The host
// lays stripes out back to back and passes a workgroup -> stripe map.
template <bool DEC, bool COMPACT>
__global__ __launch_bounds__(kThreads) void rs104_ragged_kernel(RaggedArgs a) {
    const uint32_t blk = ragged_block(a);
    // one stripe (a per-call host reconstruct): its descriptor is a kernel
    // argument, so the launch needs no metadata upload and no dependent loads
    const RaggedItem it = ragged_item(a, blk);
    uint8_t* b = a.base + it.off;
    uint8_t* o = COMPACT ? a.base + it.out_off : (DEC ? b : b + 10 * it.shard_stride);
    rs104_chunk<DEC, COMPACT, uint32_t>(b, o, it.shard_stride, it.shard_stride, it.len, blk - it.first_block, it.mask,
                                        as_const(a.tabs), as_const(a.lut), a.bad_count);
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

hipError_t launch_rs104_ragged(const RaggedArgs& a, bool decode, hipStream_t stream) {
    if (!decode) return launch_ragged(rs104_ragged_kernel<false, false>, a, stream);
    return launch_ragged(a.compact ? rs104_ragged_kernel<true, true> : rs104_ragged_kernel<true, false>, a, stream);
}

// Ragged reconstruct some: the ragged decode with each item's want word
// (RaggedItem::pad) through rs104_chunk's SOME form. COMPACT: the outputs at
// out_off are the wanted erased shards only, slot q = the q-th of them.
template <bool COMPACT>
__global__ __launch_bounds__(kThreads) void rs104_ragged_some_kernel(RaggedArgs a) {
    const uint32_t blk = ragged_block(a);
    const RaggedItem it = ragged_item<true>(a, blk);
    uint8_t* b = a.base + it.off;
    uint8_t* o = COMPACT ? a.base + it.out_off : b;
    rs104_chunk<true, COMPACT, uint32_t, true>(b, o, it.shard_stride, it.shard_stride, it.len, blk - it.first_block,
                                               it.mask, as_const(a.tabs), as_const(a.lut), a.bad_count, it.want);
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

hipError_t launch_rs104_ragged_some(const RaggedArgs& a, hipStream_t stream) {
    return launch_ragged(a.compact ? rs104_ragged_some_kernel<true> : rs104_ragged_some_kernel<false>, a, stream);
}

// ---------------------------------------------------------------------------
// The launch layer of the strided batches. Two shapes of kernel:
//  * one workgroup per chunk behind fast_item (a FastKind): no loop in the
//    kernel, so a batch of more chunks than one launch takes goes in ranges
//    of whole stripes (launch_stripe_ranges);
//  * a grid-stride loop over (stripe, 4 KiB chunk) items (launch_stride): one
//    launch whatever the batch.
// The name functions ask the predicates and picks the launchers ask, so a
// reported name is the kernel that runs.
// ---------------------------------------------------------------------------
// How the workgroups of one kind of kernel cut a shard into column ranges.
struct ChunkGeom {
    uint32_t bytes;  // column range of one workgroup
    bool round_up;   // a partial last range is a workgroup too; else the kind takes whole multiples only
    constexpr uint64_t chunks(uint64_t len) const { return round_up ? (len + bytes - 1) / bytes : len / bytes; }
    constexpr bool takes(uint64_t len) const { return round_up || len % bytes == 0; }
};
constexpr ChunkGeom kBsGeom{kBsChunk, false};                // bit-sliced: 8 KiB
constexpr ChunkGeom kNarrowGeom{kNarrowChunk, false};        // 8 bytes per lane: 2 KiB
constexpr ChunkGeom kTableGeom{kThreads * kVecBytes, true};  // 16 bytes per lane: 4 KiB, any length

// Every byte offset inside a shard fits 32 bits.
static bool off32(uint64_t len) { return len <= 0xFFFFFFFFull; }

// One kind of kernel behind fast_item: its geometry and its two offset widths.
template <typename Args>
struct FastKind {
    ChunkGeom geom;
    void (*k32)(Args);  // shards below 4 GiB
    void (*k64)(Args);  // shards of 4 GiB and more; k32 again where the kind has no such form
    // The kind runs batches of this shard length: a length it takes, one
    // stripe's chunks within a launch (its stripe ranges hold whole stripes),
    // and a kernel for the offsets.
    bool serves(uint64_t len) const {
        return geom.takes(len) && geom.chunks(len) <= kMaxLaunchBlocks && (off32(len) || k64 != k32);
    }
};

// The kernel an aligned RS(10,4) batch with the fast plan layout runs, shared
// by launch_apply and the name functions.
enum class Rs104Kind { Apply, Bitslice, Narrow, Table };
static Rs104Kind rs104_pick(uint64_t len, uint64_t n_stripes, bool dec, bool over_pcie) {
    // launch_apply sizes its stripe ranges for 4 KiB chunks; a batch whose
    // chunks would pass one launch's workgroup limit takes the generic kernel
    if (kTableGeom.chunks(len) * n_stripes > kMaxLaunchBlocks) return Rs104Kind::Apply;
    if (!dec && !over_pcie && kBsGeom.takes(len)) return Rs104Kind::Bitslice;
    // the decode, and the encode over PCIe: 8 bytes per lane where the shard
    // length is a multiple of 2 KiB
    if ((dec || over_pcie) && off32(len) && kNarrowGeom.takes(len) &&
        kNarrowGeom.chunks(len) * n_stripes <= kMaxLaunchBlocks)
        return Rs104Kind::Narrow;
    return Rs104Kind::Table;
}

static const char* rs104_name(Rs104Kind k, bool dec) {
    switch (k) {
        case Rs104Kind::Apply: return "rs_apply_kernel<10> (table lookup)";
        case Rs104Kind::Bitslice: return "rs104_bs_encode_kernel (bit-sliced)";
        case Rs104Kind::Narrow:
            return dec ? "rs104_narrow_kernel<DEC=true, 8 B per lane> (table lookup)"
                       : "rs104_narrow_kernel<DEC=false, 8 B per lane> (table lookup)";
        default: return dec ? "rs104_kernel<DEC=true> (table lookup)" : "rs104_kernel<DEC=false> (table lookup)";
    }
}

constexpr const char* kNoLaunch = "none (empty shards: EmptyShard, no launch)";

const char* decode_kernel_name(uint64_t len) {
    if (len == 0) return kNoLaunch;
    return rs104_name(rs104_pick(len, 1, true, false), true);
}

const char* encode_kernel_name(uint64_t len, bool over_pcie) {
    if (len == 0) return kNoLaunch;
    return rs104_name(rs104_pick(len, 1, false, over_pcie), false);
}

// The coding arguments of either kernel argument struct (CorrectArgs and
// CorrectPresentArgs through their bases).
static ApplyArgs& apply_args(ApplyArgs& a) { return a; }
static ApplyArgs& apply_args(VerifyArgs& v) { return v.a; }
static ApplyArgs& apply_args(CheckArgs& v) { return v.a; }
static ApplyArgs& apply_args(SomeArgs& v) { return v.a; }
static ApplyArgs& apply_args(UpdateArgs& v) { return v.a; }

// One workgroup per chunk of the batch through a kind's kernel, with
// fast_item's launch constants: the XCD eighths of the grid and the chunks per
// stripe as a multiply-shift divisor.
template <typename Args>
static hipError_t launch_fast(const FastKind<Args>& k, Args v, hipStream_t stream) {
    ApplyArgs& a = apply_args(v);
    a.chunks_per_stripe = uint32_t(k.geom.chunks(a.len));
    a.n_items = uint64_t(a.chunks_per_stripe) * a.n_stripes;
    a.map_q8 = uint32_t(a.n_items / 8);
    a.map_r8 = uint32_t(a.n_items % 8);
    const FastDiv f = make_fastdiv(a.chunks_per_stripe ? a.chunks_per_stripe : 1);
    a.cps_mul = f.mul;
    a.cps_shift = f.shift;
    if (a.n_items == 0) return hipSuccess;
    hipLaunchKernelGGL(off32(a.len) ? k.k32 : k.k64, dim3(uint32_t(a.n_items)), dim3(kThreads), 0, stream, v);
    return hipGetLastError();
}

// A grid-stride kernel over n_items items on at most max_grid workgroups; an
// empty batch launches nothing.
template <typename Args>
static hipError_t launch_grid_stride(void (*kern)(Args), const Args& v, uint64_t n_items, uint64_t max_grid,
                                     hipStream_t stream) {
    if (n_items == 0) return hipSuccess;
    const uint64_t grid = std::min<uint64_t>(n_items, max_grid);  // grid-stride covers the rest
    hipLaunchKernelGGL(kern, dim3(uint32_t(grid)), dim3(kThreads), 0, stream, v);
    return hipGetLastError();
}

// A strided grid-stride kernel (rs_apply_kernel / rs_verify_kernel /
// rs104_locate_kernel, ...) over the batch's (stripe, 4 KiB chunk) items.
template <typename Args>
static hipError_t launch_stride(void (*kern)(Args), Args v, hipStream_t stream,
                                uint64_t max_grid = kMaxLaunchBlocks) {
    ApplyArgs& a = apply_args(v);
    a.chunks_per_stripe = uint32_t(kTableGeom.chunks(a.len));
    a.n_items = uint64_t(a.chunks_per_stripe) * a.n_stripes;
    return launch_grid_stride(kern, v, a.n_items, max_grid, stream);
}

// The arguments of one stripe range of a batch (launch_split.hpp): bases,
// masks and each struct's own per-stripe words advanced to its first stripe.
// The launches share a stream, so only the last range signals completion.
static ApplyArgs stripe_range(ApplyArgs a, Range r) {
    a.in_base += uint64_t(r.first) * a.in_stripe;
    a.out_base += uint64_t(r.first) * a.out_stripe;
    if (a.masks) a.masks += r.first;
    a.n_stripes = r.count;
    if (!r.last) a.done_flag = nullptr;
    return a;
}
static SomeArgs stripe_range(SomeArgs v, Range r) {
    v.a = stripe_range(v.a, r);
    v.wants += r.first;
    return v;
}
static UpdateArgs stripe_range(UpdateArgs v, Range r) {
    v.a = stripe_range(v.a, r);  // the new arena, the parity arena and the mask words
    if (v.old_base) v.old_base += uint64_t(r.first) * v.old_stripe;
    return v;
}
static VerifyArgs stripe_range(VerifyArgs v, Range r) {
    v.a = stripe_range(v.a, r);
    v.mismatch += r.first;
    return v;
}
static CheckArgs stripe_range(CheckArgs v, Range r) {
    v.a = stripe_range(v.a, r);
    v.check += r.first;
    return v;
}

// Stripes per range of a batch whose kernel runs per_stripe workgroups per
// stripe and has no grid-stride loop. The whole batch where it fits one
// launch, and where no range of whole stripes would: one stripe, or a stripe
// of more chunks than a launch takes (the callers' picks and predicates send
// those to a grid-stride kernel).
static uint64_t stripes_per_range(uint64_t n_stripes, uint64_t per_stripe) {
    if (per_stripe * n_stripes <= kMaxLaunchBlocks || n_stripes == 1 || per_stripe > kMaxLaunchBlocks) return n_stripes;
    return stripes_per_launch(kMaxLaunchBlocks, per_stripe);
}

// The batch in stripe ranges sized by per_stripe, each through launch_range
// (which takes the range's arguments).
template <typename Args, typename LaunchRange>
static hipError_t launch_stripe_ranges(Args v, uint64_t per_stripe, LaunchRange launch_range) {
    const uint64_t n_stripes = apply_args(v).n_stripes, step = stripes_per_range(n_stripes, per_stripe);
    for (uint64_t i = 0, n = n_ranges(n_stripes, step); i < n; ++i) {
        hipError_t e = launch_range(stripe_range(v, range_at(n_stripes, step, i)));
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// The batch through one kind's kernel, in stripe ranges of the kind's own chunks.
template <typename Args>
static hipError_t launch_fast_ranges(const FastKind<Args>& k, Args v, hipStream_t stream) {
    return launch_stripe_ranges(v, k.geom.chunks(apply_args(v).len),
                                [&](const Args& r) { return launch_fast(k, r, stream); });
}

template <bool DEC>
static FastKind<ApplyArgs> rs104_fast(Rs104Kind kind) {
    switch (kind) {
        case Rs104Kind::Bitslice:
            return {kBsGeom, rs104_bs_encode_kernel<uint32_t>, rs104_bs_encode_kernel<uint64_t>};
        case Rs104Kind::Narrow:  // rs104_pick: only shards below 4 GiB
            return {kNarrowGeom, rs104_narrow_kernel<DEC>, rs104_narrow_kernel<DEC>};
        default: return {kTableGeom, rs104_kernel<DEC, uint32_t>, rs104_kernel<DEC, uint64_t>};
    }
}

hipError_t launch_apply(const ApplyArgs& a, int nin, bool aligned, bool over_pcie, hipStream_t stream) {
    const auto launch_range = [&](const ApplyArgs& r) {
        const bool dec = r.masks != nullptr;
        const Rs104Kind kind = rs104_pick(r.len, r.n_stripes, dec, over_pcie && !dec);
        if (r.fast104 && aligned && kind != Rs104Kind::Apply)
            return launch_fast(dec ? rs104_fast<true>(kind) : rs104_fast<false>(kind), r, stream);
        return launch_stride(nin == 10 ? (aligned ? rs_apply_kernel<10, true> : rs_apply_kernel<10, false>)
                                       : (aligned ? rs_apply_kernel<0, true> : rs_apply_kernel<0, false>),
                             r, stream);
    };
    if (!a.fast104) return launch_range(a);  // any codec: the grid-stride kernel
    // RS(10,4) fast path: fixed 4-row table stride, one chunk of >= 2 KiB per
    // workgroup and no grid-stride loop, so one launch takes at most
    // kMaxLaunchBlocks chunks: larger batches (tens of millions of short
    // stripes) go in stripe ranges. Two rules of these ranges, pinned by
    // tests/test_launch_record.py:
    //  * they are sized in 4 KiB chunks whatever the chunk of the kernel that
    //    runs, so the 8 KiB bit-sliced encode fills half a launch per range
    //    and the 2 KiB kernels are picked only where twice the chunks fit;
    //  * the kernel is picked per range, so a short last range can run
    //    another kernel than the ranges before it (4 KiB shards: rs104_kernel
    //    on the full ranges, rs104_narrow_kernel on a last one of half a
    //    launch's stripes or fewer).
    return launch_stripe_ranges(a, kTableGeom.chunks(a.len), launch_range);
}

// Reconstruct some over a strided in-place batch: launch_apply's decode, its
// stripe ranges and rs104_pick's choice, with the SOME kernels.
static const char* some_name(Rs104Kind k) {
    switch (k) {
        case Rs104Kind::Apply: return "rs_some_kernel (table lookup, one pass per wanted row)";
        case Rs104Kind::Narrow: return "rs104_narrow_some_kernel<8 B per lane> (table lookup)";
        default: return "rs104_some_kernel (table lookup)";
    }
}

// The kernel of one stripe range of launch_some.
static Rs104Kind some_pick(uint64_t len, uint64_t n_stripes, bool aligned) {
    return aligned ? rs104_pick(len, n_stripes, true, false) : Rs104Kind::Apply;
}

const char* some_kernel_name(uint64_t len) {
    if (len == 0) return kNoLaunch;
    return some_name(some_pick(len, 1, true));
}
const char* some_batch_kernel_name(uint64_t len, uint64_t n_stripes, bool aligned) {
    if (len == 0 || n_stripes == 0) return kNoLaunch;
    return some_name(some_pick(len, stripes_per_range(n_stripes, kTableGeom.chunks(len)), aligned));
}

hipError_t launch_some(const SomeArgs& v, bool aligned, hipStream_t stream) {
    // launch_apply's two rules: ranges sized in 4 KiB chunks, the kernel picked per range
    return launch_stripe_ranges(v, kTableGeom.chunks(v.a.len), [&](const SomeArgs& r) {
        switch (some_pick(r.a.len, r.a.n_stripes, aligned)) {
            case Rs104Kind::Apply:
                return launch_stride(aligned ? rs_some_kernel<true> : rs_some_kernel<false>, r, stream);
            case Rs104Kind::Narrow:  // rs104_pick: only shards below 4 GiB
                return launch_fast({kNarrowGeom, rs104_narrow_some_kernel, rs104_narrow_some_kernel}, r, stream);
            default:
                return launch_fast({kTableGeom, rs104_some_kernel<uint32_t>, rs104_some_kernel<uint64_t>}, r, stream);
        }
    });
}

// ---------------------------------------------------------------------------
// Update (hec.h hec_gpu_update_batch): the code is linear, so when the data
// shards in U change from old to new, parity[j] ^= XOR over c in U of
// P[j][c] * (old[c] ^ new[c]). Column c of the encode plan's tables
// ([10 inputs][4 rows][5 words]) is the four-row table of shard c: one gf_mac<4>
// of the delta per changed shard, no table set of its own. A stripe moves
// 2|U| + 8 shard lengths (|U| + 8 without old) where the encode moves 14.
// ---------------------------------------------------------------------------

// old[c] ^ new[c] of this lane's vector (new[c] itself without an old arena).
template <bool HAS_OLD, typename OffT>
__device__ __forceinline__ u32x4 update_delta(const uint8_t* new_b, uint64_t new_shard, const uint8_t* old_b,
                                              uint64_t old_shard, uint32_t c, OffT o) {
    u32x4 d = load_at(new_b + uint64_t(c) * new_shard, o);
    if constexpr (HAS_OLD) d ^= load_at(old_b + uint64_t(c) * old_shard, o);
    return d;
}

// One lane's vector of one (stripe, column range) item, one changed shard at a
// time, the pointers already at the lane's offset: FULL, 16 bytes with
// alignment-free access (the generic kernel); else the `avail` (< 16) bytes
// left of the shard, byte-wise (both kernels' lane that crosses len).
template <bool HAS_OLD, bool FULL>
__device__ __forceinline__ void update_lane(const UpdateArgs& v, uint32_t u, const uint8_t* new_b, const uint8_t* old_b,
                                            uint8_t* par_b, cu32p tab, uint64_t avail) {
    constexpr int R = 4;
    const ApplyArgs& a = v.a;
    u32x4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = u32x4{0, 0, 0, 0};
    for (; u; u &= u - 1) {
        const uint32_t c = __builtin_ctz(u);
        const uint8_t* pn = new_b + uint64_t(c) * a.in_shard;
        u32x4 d = FULL ? load_full(pn, false) : load_tail(pn, avail);
        if constexpr (HAS_OLD) {
            const uint8_t* po = old_b + uint64_t(c) * v.old_shard;
            d ^= FULL ? load_full(po, false) : load_tail(po, avail);
        }
        gf_mac<R>(acc, d, tab + c * (R * 5));
    }
    for (int r = 0; r < R; ++r) {
        uint8_t* row = par_b + uint64_t(r) * a.out_shard;
        if constexpr (FULL)
            store_full(row, acc[r] ^ load_full(row, false), false);
        else
            store_tail(row, acc[r] ^ load_tail(row, avail), avail);
    }
}

// One workgroup per (stripe, 4 KiB column range), 16 bytes per lane. The mask
// is one scalar load; an empty U leaves before any vector load. Otherwise the
// four parity loads go first, then the changed shards two at a time (scalar
// bit scan): their loads, a fence, the table multiply. With one or two
// changed shards that is every load in flight before any math, as the decode.
template <bool HAS_OLD, typename OffT>
__global__ __launch_bounds__(kThreads) void rs104_update_kernel(UpdateArgs v) {
    constexpr int R = 4;
    const ApplyArgs& a = v.a;
    uint32_t stripe, chunk;
    fast_item(a, a.chunks_per_stripe, stripe, chunk);
    uint32_t u = as_const(a.masks)[stripe] & kUpdateBits;
    const OffT o = OffT(chunk) * OffT(kThreads * kVecBytes) + OffT(threadIdx.x * kVecBytes);
    if (u != 0 && o < a.len) {
        const uint64_t avail = a.len - o;
        const uint8_t* new_b = a.in_base + uint64_t(stripe) * a.in_stripe;
        const uint8_t* old_b = HAS_OLD ? v.old_base + uint64_t(stripe) * v.old_stripe : nullptr;
        uint8_t* par_b = a.out_base + uint64_t(stripe) * a.out_stripe;
        cu32p tab = as_const(a.tabs);
        u32x4 acc[R];
#pragma unroll
        for (int r = 0; r < R; ++r) acc[r] = u32x4{0, 0, 0, 0};
        if (avail >= kVecBytes) {
            u32x4 p[R];
#pragma unroll
            for (int r = 0; r < R; ++r) p[r] = load_at(par_b + uint64_t(r) * a.out_shard, o);
            while (u) {
                const uint32_t c0 = __builtin_ctz(u);
                u &= u - 1;
                const u32x4 d0 = update_delta<HAS_OLD>(new_b, a.in_shard, old_b, v.old_shard, c0, o);
                if (u) {
                    const uint32_t c1 = __builtin_ctz(u);
                    u &= u - 1;
                    const u32x4 d1 = update_delta<HAS_OLD>(new_b, a.in_shard, old_b, v.old_shard, c1, o);
                    __builtin_amdgcn_sched_barrier(0);
                    gf_mac2<R>(acc, d0, d1, tab + c0 * (R * 5), tab + c1 * (R * 5));
                } else {
                    __builtin_amdgcn_sched_barrier(0);
                    gf_mac<R>(acc, d0, tab + c0 * (R * 5));
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) store_at(par_b + uint64_t(r) * a.out_shard, o, acc[r] ^ p[r]);
        } else {  // the lane that crosses len, in the stripe's last column range
            update_lane<HAS_OLD, false>(v, u, new_b + o, HAS_OLD ? old_b + o : nullptr, par_b + o, tab, avail);
        }
    }
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

// The update on every other layout (unaligned bases or strides, a stripe whose
// column ranges pass one launch): grid-stride over (stripe, 4 KiB column
// range) items with alignment-free access, one changed shard at a time.
template <bool HAS_OLD>
__global__ __launch_bounds__(kThreads) void rs104_update_stride_kernel(UpdateArgs v) {
    const ApplyArgs& a = v.a;
    cu32p tab = as_const(a.tabs);
    for (uint64_t item = stride_first_item(); item < a.n_items; item += gridDim.x) {
        const uint32_t stripe = uint32_t(item / a.chunks_per_stripe);
        const uint32_t chunk = uint32_t(item - uint64_t(stripe) * a.chunks_per_stripe);
        const uint32_t u = as_const(a.masks)[stripe] & kUpdateBits;
        if (u == 0) continue;
        const uint64_t o = uint64_t(chunk) * (kThreads * kVecBytes) + threadIdx.x * kVecBytes;
        if (o >= a.len) continue;
        const uint64_t avail = a.len - o;
        const uint8_t* new_b = a.in_base + uint64_t(stripe) * a.in_stripe + o;
        const uint8_t* old_b = HAS_OLD ? v.old_base + uint64_t(stripe) * v.old_stripe + o : nullptr;
        uint8_t* par_b = a.out_base + uint64_t(stripe) * a.out_stripe + o;
        if (avail >= kVecBytes)
            update_lane<HAS_OLD, true>(v, u, new_b, old_b, par_b, tab, avail);
        else
            update_lane<HAS_OLD, false>(v, u, new_b, old_b, par_b, tab, avail);
    }
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

// An aligned update runs one workgroup per 4 KiB column range when one
// stripe's ranges fit a launch.
static FastKind<UpdateArgs> update_fast(bool has_old) {
    if (has_old) return {kTableGeom, rs104_update_kernel<true, uint32_t>, rs104_update_kernel<true, uint64_t>};
    return {kTableGeom, rs104_update_kernel<false, uint32_t>, rs104_update_kernel<false, uint64_t>};
}

const char* update_kernel_name(uint64_t len) {
    if (len == 0) return kNoLaunch;
    return update_fast(true).serves(len) ? "rs104_update_kernel (table lookup)"
                                         : "rs104_update_stride_kernel (table lookup)";
}

hipError_t launch_update(const UpdateArgs& v, bool aligned, hipStream_t stream) {
    const bool has_old = v.old_base != nullptr;
    const FastKind<UpdateArgs> fast = update_fast(has_old);
    if (aligned && fast.serves(v.a.len)) return launch_fast_ranges(fast, v, stream);
    return launch_stride(has_old ? rs104_update_stride_kernel<true> : rs104_update_stride_kernel<false>, v, stream);
}

// ---------------------------------------------------------------------------
// Parity verify (scrub): the encode with its stores replaced by a compare.
// A stripe's 14 shards are read once, the parity is recomputed in registers
// and XORed with the stored parity; what leaves the chip is one word per
// stripe. Each lane keeps one "differs" flag per parity row (the OR of its
// XORed dwords), a ballot per row makes the wave's bit set, and lane 0 of the
// wave ORs it into mismatch[stripe] only when it is non-zero, so clean data
// costs no write traffic and no LDS. The word is zero at launch (the host
// clears it on the same stream): the atomicOr that finds it zero is the
// stripe's first report, whatever chunk, wave or row group it comes from, and
// counts the stripe into bad_count exactly once.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void report_mismatch(uint32_t* word, uint32_t* bad_count, uint32_t bits) {
    if (bits != 0 && (threadIdx.x & 63u) == 0) {
        if (atomicOr(word, bits) == 0 && bad_count) atomicAdd(bad_count, 1u);
    }
}

// Bit-sliced RS(10,4) verify: rs104_bs_chunk<OffT, VERIFY> (the encode's loads
// and XOR program plus the four stored parity streams). One 8 KiB column range
// per workgroup, the encode's workgroup -> (stripe, chunk) map.
template <typename OffT>
__global__ __launch_bounds__(kThreads) void rs104_bs_verify_kernel(VerifyArgs v) {
    const ApplyArgs& a = v.a;
    uint32_t stripe, chunk;
    fast_item(a, a.chunks_per_stripe, stripe, chunk);
    const uint32_t bits =
        rs104_bs_chunk<OffT, true>(a.in_base + uint64_t(stripe) * a.in_stripe, a.out_base, a.in_shard, a.out_shard,
                                   chunk, uint64_t(stripe) * a.out_stripe);
    report_mismatch(v.mismatch + stripe, a.bad_count, bits);
}

// Generic verify (any codec with at most 32 parity shards, unaligned bases and
// strides, any length): rs_apply_kernel's grid-stride over (stripe, 4 KiB
// chunk) items and its row groups (apply_rows<K, ALIGNED, VERIFY>), over the
// encode plan (plan 0).
template <int K, bool ALIGNED>
__global__ __launch_bounds__(kThreads) void rs_verify_kernel(VerifyArgs v) {
    const ApplyArgs& a = v.a;
    const uint64_t first = stride_first_item();
    const __attribute__((address_space(4))) DevPlan* pp = as_const(a.plans);
    const DevPlan p{pp->nin, pp->nout, pp->tab_off, pp->idx_off, pp->tab_rows, {0, 0, 0}};
    cu32p in_ids = as_const(a.idx) + p.idx_off;
    cu32p out_ids = in_ids + p.nin;
    cu32p tab = as_const(a.tabs) + p.tab_off;
    const uint32_t row_stride = p.tab_rows * 5;  // words per input
    for (uint64_t item = first; item < a.n_items; item += gridDim.x) {
        const uint32_t stripe = uint32_t(item / a.chunks_per_stripe);
        const uint32_t chunk = uint32_t(item - uint64_t(stripe) * a.chunks_per_stripe);
        const uint8_t* in_b = a.in_base + uint64_t(stripe) * a.in_stripe;
        uint8_t* par_b = a.out_base + uint64_t(stripe) * a.out_stripe;  // only read
        const uint64_t chunk_off = uint64_t(chunk) * (kThreads * kVecBytes);
        // this lane: bit j = parity row j differs in its vector
        const uint32_t differs =
            apply_rows<K, ALIGNED, true>(a, in_b, par_b, in_ids, out_ids, tab, p, row_stride, chunk_off);
        uint32_t bits = 0;
        for (uint32_t j = 0; j < p.nout; ++j) bits |= (__ballot((differs >> j) & 1u) != 0 ? 1u : 0u) << j;
        report_mismatch(v.mismatch + stripe, a.bad_count, bits);
    }
}

constexpr const char* kBsVerifyName = "rs104_bs_verify_kernel (bit-sliced)";
constexpr const char* kGenericVerifyName = "rs_verify_kernel<10> (table lookup)";

// An aligned RS(10,4) verify runs bit-sliced when the shard length is a
// multiple of 8 KiB and one stripe's chunks fit a launch.
static const FastKind<VerifyArgs> kBsVerify{kBsGeom, rs104_bs_verify_kernel<uint32_t>,
                                            rs104_bs_verify_kernel<uint64_t>};

const char* verify_kernel_name(uint64_t len) {
    if (len == 0) return kNoLaunch;
    return kBsVerify.serves(len) ? kBsVerifyName : kGenericVerifyName;
}

hipError_t launch_verify(const VerifyArgs& v, int nin, bool aligned, hipStream_t stream) {
    if (v.a.fast104 && aligned && kBsVerify.serves(v.a.len)) return launch_fast_ranges(kBsVerify, v, stream);
    if (nin == 10) return launch_stride(aligned ? rs_verify_kernel<10, true> : rs_verify_kernel<10, false>, v, stream);
    return launch_stride(aligned ? rs_verify_kernel<0, true> : rs_verify_kernel<0, false>, v, stream);
}

// ---------------------------------------------------------------------------
// Locate (RS(10,4)): which shard of a flagged stripe is wrong. Pass 2 of the
// scrub; pass 1 (launch_verify, above) has filled mismatch[]. With H = [P | I4]
// (P the 4 x 10 parity rows), the syndrome of a byte column -- stored parity
// XOR parity of the stored data, s[0..3] -- is v * H[:,c] when shard c alone
// is wrong by v. Any four columns of H are independent (the code is MDS), so
// one wrong shard is named uniquely and two or three wrong shards in a column
// look like no single shard (DESIGN.md §4 "Locate"). Bytewise in SWAR:
//  * exactly one s[j] non-zero -> parity shard 10 + j (column 10 + j of H is
//    the unit vector e_j);
//  * all four non-zero -> data shard c when s[j] = s[0] * P[j][c] / P[0][c]
//    for j = 1..3: gf_mac<3> of s[0] over the three ratio constants of c (every
//    entry of P is non-zero; the ratios are a plan like any other);
//  * any other non-zero pattern, and an all-four byte no c matches, is
//    unexplained (bit 31).
// A clean item of a flagged stripe ends at one ballot; an item of a clean
// stripe at one scalar load, without touching a shard.
// ---------------------------------------------------------------------------
// 0x80 in every non-zero byte of x.
__device__ __forceinline__ uint32_t nz_bytes(uint32_t x) {
    return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

// ---------------------------------------------------------------------------
// Locate, two per column (hec.h hec_gpu_locate_corrupt_pairs_batch): the bytes
// the ratio method leaves unexplained are tried as two wrong shards. Shard i of
// a codeword is p(alpha_i), alpha_i = the byte i, deg p < 10, so the dual is
// generalised Reed-Solomon: H'[j][i] = u_i * alpha_i^j annihilates the code,
// H' = T * H, and S = T * syn are classical syndromes, S_j = sum e_i u_i
// alpha_i^j (DESIGN.md §4 "Locate, two per column"). Two errors make S obey
// S_{j+2} = sigma1 * S_{j+1} + sigma2 * S_j; with
//   D = S0 S2 ^ S1^2,  N1 = S0 S3 ^ S1 S2,  N2 = S1 S3 ^ S2^2
// (sigma1 = N1 / D, sigma2 = N2 / D) the wrong shards are the roots alpha_i of
// D x^2 ^ N1 x ^ N2. A pair is named only when exactly two of the 14 alpha_i
// are roots; then D != 0 (with D == 0 the polynomial is linear or zero: one
// root, none or all 14; one error always has D == 0) and S_j = A a^j ^ B b^j
// with A, B != 0, which is the contract's statement. No division is needed.
// ---------------------------------------------------------------------------
// a * b bytewise in GF(2^8) (0x11D), both operands variable: shift-and-add over
// the bits of b with a packed xtime of a. No product leaves its byte: 0x01
// bytes times 0xFF or 0x1D stay below 0x100.
__device__ __forceinline__ uint32_t gf_mul_var(uint32_t a, const uint32_t b) {
    uint32_t r = 0;
#pragma unroll 1  // rolled: six unrolled products interleave and cost the kernel a fifth of its waves
    for (int bit = 0; bit < 8; ++bit) {
        r ^= a & (((b >> bit) & 0x01010101u) * 0xFFu);
        a = ((a & 0x7F7F7F7Fu) << 1) ^ (((a >> 7) & 0x01010101u) * 0x1Du);
    }
    return r;
}

// coef * x bytewise, one dword: gf_mac's three lookups; tab -> the 5 words of coef.
__device__ __forceinline__ uint32_t gf_mul_const(const uint32_t x, cu32p tab) {
    const uint32_t a = __builtin_amdgcn_perm(tab[1], tab[0], x & 0x07070707u);
    const uint32_t b = __builtin_amdgcn_perm(tab[3], tab[2], (x >> 3) & 0x07070707u);
    const uint32_t c = __builtin_amdgcn_perm(tab[4], tab[4], (x >> 6) & 0x03030303u);
    return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}

// Set bits per byte (each count <= 8).
__device__ __forceinline__ uint32_t popcount_bytes(uint32_t x) {
    x = x - ((x >> 1) & 0x55555555u);
    x = (x & 0x33333333u) + ((x >> 2) & 0x33333333u);
    return (x + (x >> 4)) & 0x0F0F0F0Fu;
}

// Dword w (wave-uniform) of v, without indexing a register vector by a variable.
__device__ __forceinline__ uint32_t dword_of(const u32x4 v, int w) {
    return w == 0 ? v[0] : w == 1 ? v[1] : w == 2 ? v[2] : v[3];
}

// 1 / x bytewise (0 for 0): x^254 = (x^127)^2, x^127 the product of x^(2^i), i = 0..6.
__device__ __forceinline__ uint32_t gf_inv_var(const uint32_t x) {
    uint32_t p = x, acc = x;
#pragma unroll 1
    for (int i = 0; i < 6; ++i) {
        p = gf_mul_var(p, p);
        acc = gf_mul_var(acc, p);
    }
    return gf_mul_var(acc, acc);
}

// Correct (rs104_correct_kernel): the item a workgroup is fixing (uniform; the
// addresses are derived from the kernel's arguments where a fix needs them,
// not kept in registers across the walk) and how many bytes this lane has
// changed.
struct FixLane {
    const ApplyArgs* a;
    uint32_t stripe, chunk;
    uint32_t changed;
};

// The ragged correct's (rs104_ragged_correct_kernel): the batch, and the stripe
// whose RaggedItem a fix reads again (scalar loads: a fix is rare).
struct RaggedFixLane {
    const RaggedArgs* a;
    uint32_t stripe, chunk;
    uint32_t changed;
};

struct NoFix {};  // the locate kernel's

// XOR the error vector e into this lane's vector of shard c (wave-uniform).
// Only a lane with an error for c touches c; e is zero in columns at or past
// the shard's end (their syndrome is zero), and the last partial vector goes
// through load_tail / store_tail, so no byte past the end is written.
// IN_PLACE (the masked correct): the batch is one in-place layout and c is a
// shard index 0..13 of it, so every c is addressed from in_base (out_base
// equals in_base there: the c - 10 path would put shard 12's fix into shard 2).
// RAGGED (the ragged correct, always in place): shard c of the stripe is at
// base + item.off + c * item.shard_stride, and the tail rule uses item.len.
template <bool ALIGNED, bool IN_PLACE = false, bool RAGGED = false>
__device__ __forceinline__ void fix_shard(std::conditional_t<RAGGED, RaggedFixLane, FixLane>& f, int c,
                                          const u32x4 e) {
    if ((e[0] | e[1] | e[2] | e[3]) == 0) return;
    const auto& a = *f.a;
    const uint64_t o = uint64_t(f.chunk) * (kThreads * kVecBytes) + threadIdx.x * kVecBytes;  // < len: an error here
    uint8_t* p;
    uint64_t len;
    if constexpr (RAGGED) {
        static_assert(IN_PLACE, "a ragged batch is one in-place layout");
        const __attribute__((address_space(4))) RaggedItem* it = as_const(a.items) + f.stripe;
        p = a.base + it->off + uint64_t(c) * it->shard_stride + o;
        len = it->len;
    } else {
        if constexpr (IN_PLACE)
            p = const_cast<uint8_t*>(a.in_base) + uint64_t(f.stripe) * a.in_stripe + uint64_t(c) * a.in_shard + o;
        else
            p = (c < 10 ? const_cast<uint8_t*>(a.in_base) + uint64_t(f.stripe) * a.in_stripe + uint64_t(c) * a.in_shard
                        : a.out_base + uint64_t(f.stripe) * a.out_stripe + uint64_t(c - 10) * a.out_shard) +
                o;
        len = a.len;
    }
    const uint64_t avail = len - o;
    if (avail >= kVecBytes)
        store_full(p, load_full(p, ALIGNED) ^ e, ALIGNED);
    else
        store_tail(p, load_tail(p, avail) ^ e, avail);
    f.changed += uint32_t(__builtin_popcount(nz_bytes(e[0])) + __builtin_popcount(nz_bytes(e[1])) +
                          __builtin_popcount(nz_bytes(e[2])) + __builtin_popcount(nz_bytes(e[3])));
}

constexpr int kPairSynWords = 4 * 4 * 5;  // T's tables; the root tables follow

// s: the syndrome of this lane's 16 columns; unx[w]: 0x80 in the bytes of dword
// w that no single shard explains. Returns bit c for every shard c that is one
// of the two of some such byte, and clears those bytes from unx. pt: T as a
// 4-input 4-row plan, then [2][14] tables: input 0 = D with alpha_c^2, input 1
// = N1 with alpha_c, row c. One dword per round and a rolled loop over the
// shards: the registers of one round, not of four at once (the kernel keeps
// the single-shard kernel's occupancy).
template <bool ALIGNED = false, bool CORRECT = false>
__device__ __forceinline__ uint32_t rs104_pair_search(const u32x4 (&s)[4], u32x4& unx, cu32p pt,
                                                      [[maybe_unused]] FixLane* fx = nullptr,
                                                      [[maybe_unused]] cu32p inv_u = nullptr) {
    constexpr int N = 14;
    cu32p rt = pt + kPairSynWords;
    uint32_t named = 0;
#pragma unroll 1
    for (int w = 0; w < 4; ++w) {
        const uint32_t u = dword_of(unx, w);
        if (__ballot(u != 0) == 0) continue;  // wave-uniform
        uint32_t S[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t x = dword_of(s[i], w);
#pragma unroll
            for (int j = 0; j < 4; ++j) S[j] ^= gf_mul_const(x, pt + (i * 4 + j) * 5);
        }
        const uint32_t D = gf_mul_var(S[0], S[2]) ^ gf_mul_var(S[1], S[1]);
        const uint32_t N1 = gf_mul_var(S[0], S[3]) ^ gf_mul_var(S[1], S[2]);
        const uint32_t N2 = gf_mul_var(S[1], S[3]) ^ gf_mul_var(S[2], S[2]);
        uint32_t lo = 0, hi = 0;  // bit c (lo) / c - 8 (hi) of a byte: alpha_c is a root
#pragma unroll 1
        for (int c = 0; c < N; ++c) {
            const uint32_t q = gf_mul_const(D, rt + c * 5) ^ gf_mul_const(N1, rt + (N + c) * 5) ^ N2;
            const uint32_t root = (u & ~nz_bytes(q)) >> 7;  // 0x01 per byte
            if (c < 8)
                lo |= root << c;
            else
                hi |= root << (c - 8);
        }
        const uint32_t count = popcount_bytes(lo) + popcount_bytes(hi);
        const uint32_t two = u & ~nz_bytes(count ^ 0x02020202u);  // exactly two roots
        const uint32_t keep = (two >> 7) * 0xFFu;
        lo &= keep;
        hi &= keep;
        if constexpr (CORRECT) {
            // the two values of a named pair (above): e_c = (X ^ alpha_c * Y) / u_c
            // with q = D / N1, X = q * S1 ^ S0, Y = q * S0. N1 = D (a ^ b) is
            // non-zero in every named byte; the others are masked out by the
            // root flags (gf_inv_var(0) = 0 there).
            if (__ballot(two != 0) != 0) {  // wave-uniform
                const uint32_t q = gf_mul_var(D, gf_inv_var(N1));
                const uint32_t Y = gf_mul_var(q, S[0]);
                const uint32_t X = gf_mul_var(q, S[1]) ^ S[0];
#pragma unroll 1
                for (int c = 0; c < N; ++c) {
                    const uint32_t is_root = ((c < 8 ? lo >> c : hi >> (c - 8)) & 0x01010101u) * 0xFFu;
                    if (__ballot(is_root != 0) == 0) continue;  // wave-uniform: nobody fixes shard c
                    const uint32_t e =
                        gf_mul_const(X ^ gf_mul_const(Y, rt + (N + c) * 5), inv_u + c * 5) & is_root;
                    fix_shard<ALIGNED>(*fx, c, u32x4{w == 0 ? e : 0u, w == 1 ? e : 0u, w == 2 ? e : 0u,
                                                     w == 3 ? e : 0u});
                }
            }
        }
        lo |= lo >> 16;
        hi |= hi >> 16;
        named |= ((lo | (lo >> 8)) & 0xFFu) | (((hi | (hi >> 8)) & 0x3Fu) << 8);
        const uint32_t rest = u & ~two;
        unx = u32x4{w == 0 ? rest : unx[0], w == 1 ? rest : unx[1], w == 2 ? rest : unx[2],
                    w == 3 ? rest : unx[3]};
    }
    return named;
}

// The walk of the locate and the correct kernels. PAIRS: bytes the single-shard
// method leaves unexplained go on to rs104_pair_search; everything up to there
// is the same code.
//
// CORRECT (rs104_correct_kernel, hec.h hec_gpu_correct_batch): the same walk;
// where a column is explained the lane also computes the error value the
// classification implies and XORs it into the wrong byte (fix_shard): s[j] for
// parity shard 10 + j, s[0] / P[0][c] for data shard c, the pair search's two
// values. A lane's 16 columns belong to no other lane and its syndrome is
// complete before its first store, so names and values are those of the bytes
// as they were. Unexplained columns are not touched.
//
// The pairs instantiation asks for the five waves per SIMD the other one gets
// unasked (95 VGPRs): without the bound it takes 103 VGPRs and four waves, and
// a clean batch would pay for code it never reaches
// (profiles/locate_pairs/isa.md). The correct forms ask for four: unasked they
// take 130 / 135 VGPRs and three waves, and the clean walk, a chain of
// dependent scalar loads that lives on resident waves, measured outside the
// locate's spread; at four (128 VGPRs, 16 / 32 bytes of scratch in the fix
// paths) it is inside (profiles/correct/isa.md, bench_correct.json).
template <bool ALIGNED, bool PAIRS = false, bool CORRECT = false>
__global__ __launch_bounds__(kThreads, CORRECT ? 4 : PAIRS ? 5 : 1) void rs104_locate_kernel(
    std::conditional_t<CORRECT, CorrectArgs, VerifyArgs> v) {
    constexpr int K = 10, R = 4;
    const ApplyArgs& a = v.a;
    cu32p tab = as_const(a.tabs);        // encode plan: [K][R][5] words
    cu32p rat = as_const(v.ratio_tabs);  // [K][R - 1][5] words
    cu32p flagged = as_const(v.mismatch);
    for (uint64_t item = stride_first_item(); item < a.n_items; item += gridDim.x) {
        const uint32_t stripe = uint32_t(item / a.chunks_per_stripe);
        const uint32_t chunk = uint32_t(item - uint64_t(stripe) * a.chunks_per_stripe);
        if (flagged[stripe] == 0) continue;  // pass 1 found the stripe clean
        const uint8_t* in_b = a.in_base + uint64_t(stripe) * a.in_stripe;
        const uint8_t* par_b = a.out_base + uint64_t(stripe) * a.out_stripe;
        const uint64_t o = uint64_t(chunk) * (kThreads * kVecBytes) + threadIdx.x * kVecBytes;
        // the syndrome of this lane's 16 columns; lanes past the shard's end
        // keep zeros and still take part in the ballots
        u32x4 s[R];
#pragma unroll
        for (int j = 0; j < R; ++j) s[j] = u32x4{0, 0, 0, 0};
        if (o < a.len) {
            const uint64_t avail = a.len - o;
            if (avail >= kVecBytes) {
                u32x4 d[K];
#pragma unroll
                for (int i = 0; i < K; ++i) d[i] = load_full(in_b + uint64_t(i) * a.in_shard + o, ALIGNED);
#pragma unroll
                for (int i = 0; i < K; ++i) gf_mac<R>(s, d[i], tab + i * (R * 5));
#pragma unroll
                for (int j = 0; j < R; ++j) s[j] ^= load_full(par_b + uint64_t(j) * a.out_shard + o, ALIGNED);
            } else {
                // the last vector of a shard: zero-filled from a.len on, data
                // and stored parity alike, so those columns have syndrome 0
                for (int i = 0; i < K; ++i)
                    gf_mac<R>(s, load_tail(in_b + uint64_t(i) * a.in_shard + o, avail), tab + i * (R * 5));
                for (int j = 0; j < R; ++j) s[j] ^= load_tail(par_b + uint64_t(j) * a.out_shard + o, avail);
            }
        }
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < R; ++j) any |= s[j][0] | s[j][1] | s[j][2] | s[j][3];
        if (__ballot(any != 0) == 0) continue;  // wave-uniform: this wave's 1 KiB is clean
        [[maybe_unused]] std::conditional_t<CORRECT, FixLane, NoFix> fx;
        if constexpr (CORRECT)
            fx = FixLane{&a, stripe, chunk, 0};

        uint32_t one[R] = {0, 0, 0, 0};  // bytes where only s[j] is non-zero
        uint32_t all4[4];                // per dword: bytes where all four are
        uint32_t unexplained = 0, all_any = 0;
        [[maybe_unused]] u32x4 unx;  // PAIRS: `unexplained` per dword
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t n0 = nz_bytes(s[0][w]), n1 = nz_bytes(s[1][w]), n2 = nz_bytes(s[2][w]),
                           n3 = nz_bytes(s[3][w]);
            const uint32_t o0 = n0 & ~(n1 | n2 | n3), o1 = n1 & ~(n0 | n2 | n3), o2 = n2 & ~(n0 | n1 | n3),
                           o3 = n3 & ~(n0 | n1 | n2);
            one[0] |= o0;
            one[1] |= o1;
            one[2] |= o2;
            one[3] |= o3;
            all4[w] = n0 & n1 & n2 & n3;
            all_any |= all4[w];
            const uint32_t some = (n0 | n1 | n2 | n3) & ~all4[w] & ~(o0 | o1 | o2 | o3);  // two or three non-zero
            unexplained |= some;
            if constexpr (PAIRS) unx[w] = some;
        }
        uint32_t bits = 0;
        if (__ballot(all_any != 0) != 0) {  // wave-uniform: some column may name a data shard
            uint32_t matched[4] = {0, 0, 0, 0};
#pragma unroll 1
            for (int c = 0; c < K; ++c) {
                u32x4 e[R - 1];
#pragma unroll
                for (int j = 0; j < R - 1; ++j) e[j] = u32x4{0, 0, 0, 0};
                gf_mac<R - 1>(e, s[0], rat + c * ((R - 1) * 5));
                uint32_t hit = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const uint32_t diff = (e[0][w] ^ s[1][w]) | (e[1][w] ^ s[2][w]) | (e[2][w] ^ s[3][w]);
                    const uint32_t m = all4[w] & ~nz_bytes(diff);
                    matched[w] |= m;
                    hit |= m;
                    if constexpr (CORRECT) e[0][w] = (m >> 7) * 0xFFu;  // the ratios are spent: the bytes c explains
                }
                bits |= (__ballot(hit != 0) != 0 ? 1u : 0u) << c;
                if constexpr (CORRECT) {
                    if (__ballot(hit != 0) != 0) {  // wave-uniform: somebody fixes data shard c
                        u32x4 val[1] = {u32x4{0, 0, 0, 0}};
                        gf_mac<1>(val, s[0], as_const(v.fix_tabs) + c * 5);  // s[0] / P[0][c]
                        fix_shard<ALIGNED>(fx, c, val[0] & e[0]);
                    }
                }
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                unexplained |= all4[w] & ~matched[w];
                if constexpr (PAIRS) unx[w] |= all4[w] & ~matched[w];
            }
        }
        if constexpr (PAIRS) {
            if (__ballot(unexplained != 0) != 0) {  // wave-uniform: some column may name two shards
                uint32_t two;
                if constexpr (CORRECT)
                    two = rs104_pair_search<ALIGNED, true>(s, unx, as_const(v.pair_tabs), &fx,
                                                           as_const(v.fix_tabs) + kFixInvU);
                else
                    two = rs104_pair_search(s, unx, as_const(v.pair_tabs));
#pragma unroll
                for (int c = 0; c < K + R; ++c) bits |= (__ballot(((two >> c) & 1u) != 0) != 0 ? 1u : 0u) << c;
                unexplained = unx[0] | unx[1] | unx[2] | unx[3];
            }
        }
#pragma unroll
        for (int j = 0; j < R; ++j) bits |= (__ballot(one[j] != 0) != 0 ? 1u : 0u) << (K + j);
        if (__ballot(unexplained != 0) != 0) bits |= kSuspectUnexplained;
        if constexpr (!CORRECT) {
            if (bits != 0 && (threadIdx.x & 63u) == 0) atomicOr(v.suspects + stripe, bits);
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j) {
                if (__ballot(one[j] != 0) == 0) continue;  // wave-uniform: nobody fixes parity shard j
                u32x4 e;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    uint32_t others = 0;
#pragma unroll
                    for (int i = 0; i < R; ++i)
                        if (i != j) others |= nz_bytes(s[i][w]);
                    e[w] = s[j][w] & ((nz_bytes(s[j][w]) & ~others) >> 7) * 0xFFu;
                }
                fix_shard<ALIGNED>(fx, K + j, e);
            }
            // the bytes this wave changed, at most 32 a lane: six ballots
            uint32_t total = 0;
#pragma unroll
            for (int k = 0; k < 6; ++k)
                total += uint32_t(__builtin_popcountll(__ballot(((fx.changed >> k) & 1u) != 0))) << k;
            if ((threadIdx.x & 63u) == 0) {
                // the atomicOr that first sets bit 31 counts the stripe
                if (bits != 0 && (atomicOr(v.suspects + stripe, bits) & kSuspectUnexplained) == 0 &&
                    (bits & kSuspectUnexplained) != 0 && v.uncorrected)
                    atomicAdd(v.uncorrected, 1u);
                if (total != 0 && v.corrected_bytes) atomicAdd(v.corrected_bytes, (unsigned long long)total);
            }
        }
    }
}

// The locate kernel (CORRECT: its correct form, taking CorrectArgs) on the locate grid.
template <bool CORRECT, typename Args>
static hipError_t launch_locate_form(const Args& v, bool aligned, bool pairs, hipStream_t stream) {
    return launch_stride(
        pairs ? (aligned ? rs104_locate_kernel<true, true, CORRECT> : rs104_locate_kernel<false, true, CORRECT>)
              : (aligned ? rs104_locate_kernel<true, false, CORRECT> : rs104_locate_kernel<false, false, CORRECT>),
        v, stream, kLocateMaxBlocks);
}

hipError_t launch_correct(const CorrectArgs& c, bool aligned, bool pairs, hipStream_t stream) {
    return launch_locate_form<true>(c, aligned, pairs, stream);
}

hipError_t launch_locate(const VerifyArgs& v, bool aligned, bool pairs, hipStream_t stream) {
    return launch_locate_form<false>(v, aligned, pairs, stream);
}

// ---------------------------------------------------------------------------
// The mask kernels: one lane per stripe writes the stripe's present mask for
// the reconstruct that follows, by a rule of its own. rule(s) writes what
// stripe s gets and says whether the stripe is left alone; a wave counts the
// stripes it leaves alone with one atomic. Whole waves run every round, so the
// ballot sees all 64 lanes.
// ---------------------------------------------------------------------------
constexpr uint32_t kAllShards = (1u << 14) - 1;

template <typename Rule>
__device__ __forceinline__ void mask_rounds(uint32_t n_stripes, uint32_t* unrepaired, Rule rule) {
    const uint64_t per_round = uint64_t(gridDim.x) * kThreads;
    const uint32_t rounds = uint32_t((n_stripes + per_round - 1) / per_round);
    for (uint32_t r = 0; r < rounds; ++r) {
        const uint64_t s = (uint64_t(r) * gridDim.x + blockIdx.x) * kThreads + threadIdx.x;
        const bool left = s < n_stripes && rule(s);
        const unsigned long long b = __ballot(left);
        if (b != 0 && unrepaired && (threadIdx.x & 63u) == 0) atomicAdd(unrepaired, uint32_t(__builtin_popcountll(b)));
    }
}

// One lane per stripe on at most kLocateMaxBlocks workgroups; args end with n_stripes.
template <typename... Params, typename... Vals>
static hipError_t launch_mask_rounds(void (*kern)(Params...), uint32_t n_stripes, hipStream_t stream, Vals... args) {
    if (n_stripes == 0) return hipSuccess;
    const uint32_t grid = std::min<uint32_t>((n_stripes + kThreads - 1) / kThreads, kLocateMaxBlocks);
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kThreads), 0, stream, args...);
    return hipGetLastError();
}

// Present masks of a repair.
__global__ __launch_bounds__(kThreads) void repair_masks_kernel(const uint32_t* suspects, uint32_t* masks,
                                                                uint32_t* unrepaired, uint32_t n_stripes) {
    mask_rounds(n_stripes, unrepaired, [&](uint64_t s) {
        const uint32_t w = suspects[s];
        const uint32_t named = uint32_t(__builtin_popcount(w & kAllShards));
        const bool repair = (w & kSuspectUnexplained) == 0 && named >= 1 && named <= 4;
        masks[s] = repair ? (kAllShards & ~w) : kAllShards;
        return w != 0 && !repair;
    });
}

hipError_t launch_repair_masks(const uint32_t* suspects, uint32_t* masks, uint32_t* unrepaired, uint32_t n_stripes,
                               hipStream_t stream) {
    return launch_mask_rounds(repair_masks_kernel, n_stripes, stream, suspects, masks, unrepaired, n_stripes);
}

// ---------------------------------------------------------------------------
// Masked verify and locate (degraded scrub, RS(10,4)): a stripe with shards
// missing still has r = p - 10 spare shards among its p >= 11 present ones.
// The ten lowest present shards (B) are what the reconstruct would decode
// from; A_m applied to them is what the other present shards (E) must hold.
// The check kernels are the mask-driven decode with its stores replaced by a
// compare against the stored E rows; the result bits are by shard index.
// ---------------------------------------------------------------------------
// Fast form, rs104_narrow_chunk<true> with a compare: 8 bytes per lane, one
// 2 KiB column range per workgroup, the ten B loads and the r stored E loads
// in flight before the math, the plan looked up from the mask while they fly.
// Aligned bases and strides, shard_len a multiple of 2 KiB below 4 GiB.
__global__ __launch_bounds__(kThreads) void rs104_check_kernel(CheckArgs v) {
    typedef u32x2 V;
    constexpr int K = 10, N = 14, R = 4, VB = int(sizeof(V));
    const ApplyArgs& a = v.a;
    uint32_t stripe, chunk;
    fast_item(a, a.chunks_per_stripe, stripe, chunk);
    const uint32_t mask = as_const(a.masks)[stripe] & ((1u << N) - 1);
    const uint32_t present = __builtin_popcount(mask);
    if (present <= K) {  // wave-uniform: no spare shard, nothing to check and nothing read
        if (chunk == 0 && threadIdx.x == 0 && v.unchecked) atomicAdd(v.unchecked, 1u);
        return;
    }
    const uint32_t r = present - K;
    uint32_t in_id[K], out_id[R];
    uint32_t m = mask;
#pragma unroll
    for (int i = 0; i < K; ++i) {  // B: the ten lowest present shards
        in_id[i] = __builtin_ctz(m);
        m &= m - 1;
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {  // E: the other present shards, ascending
        out_id[j] = m ? __builtin_ctz(m) : 0;
        m &= m - 1;
    }
    uint32_t plan = as_const(a.lut)[mask];  // first used after the data loads
    const uint8_t* b = a.in_base + uint64_t(stripe) * a.in_stripe;
    const uint32_t o = chunk * (kThreads * VB) + threadIdx.x * VB;
    V d[K], st[R];
#pragma unroll
    for (int i = 0; i < K; ++i)
        d[i] = __builtin_nontemporal_load(
            (const __attribute__((address_space(1))) V*)((gcu8p)(b + uint64_t(in_id[i]) * a.in_shard) + o));
#pragma unroll
    for (int j = 0; j < R; ++j) {
        st[j] = V(0u);
        if (uint32_t(j) < r)
            st[j] = __builtin_nontemporal_load(
                (const __attribute__((address_space(1))) V*)((gcu8p)(b + uint64_t(out_id[j]) * a.in_shard) + o));
    }
    __builtin_amdgcn_sched_barrier(0);  // every load in flight before the math
    asm volatile("" : "+s"(plan));
    cu32p tab = as_const(a.tabs) + plan * (K * R * 5);
    V acc[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = V(0u);
#pragma unroll
    for (int i = 0; i < K; i += 2)
        gf_mac2<R, V>(acc, d[i], d[i + 1], tab + i * (R * 5), tab + (i + 1) * (R * 5), r);
    // rows at or past r: acc and st are both zero, the ballot is empty
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const uint32_t x = (acc[j][0] ^ st[j][0]) | (acc[j][1] ^ st[j][1]);
        bits |= (__ballot(x != 0) != 0 ? 1u : 0u) << out_id[j];
    }
    report_mismatch(v.check + stripe, a.bad_count, bits);
}

// Every other layout and length: rs_verify_kernel's grid-stride loop and row
// groups (apply_rows<10, ALIGNED, VERIFY>) with the stripe's check plan; the
// last vector of a shard is zero-filled from a.len on, inputs and stored rows
// alike, so bytes at or past a.len compare equal.
template <bool ALIGNED>
__global__ __launch_bounds__(kThreads) void rs104_check_stride_kernel(CheckArgs v) {
    const ApplyArgs& a = v.a;
    for (uint64_t item = stride_first_item(); item < a.n_items; item += gridDim.x) {
        const uint32_t stripe = uint32_t(item / a.chunks_per_stripe);
        const uint32_t chunk = uint32_t(item - uint64_t(stripe) * a.chunks_per_stripe);
        const uint32_t pid = as_const(a.lut)[as_const(a.masks)[stripe] & a.mask_limit];
        if (pid == kNoPlan) {  // at most ten shards present
            if (chunk == 0 && threadIdx.x == 0 && v.unchecked) atomicAdd(v.unchecked, 1u);
            continue;
        }
        const __attribute__((address_space(4))) DevPlan* pp = as_const(a.plans) + pid;
        const DevPlan p{pp->nin, pp->nout, pp->tab_off, pp->idx_off, pp->tab_rows, {0, 0, 0}};
        uint8_t* b = a.out_base + uint64_t(stripe) * a.out_stripe;  // only read
        cu32p in_ids = as_const(a.idx) + p.idx_off;
        cu32p out_ids = in_ids + p.nin;
        cu32p tab = as_const(a.tabs) + p.tab_off;
        const uint64_t chunk_off = uint64_t(chunk) * (kThreads * kVecBytes);
        const uint32_t differs =
            apply_rows<10, ALIGNED, true>(a, b, b, in_ids, out_ids, tab, p, p.tab_rows * 5, chunk_off);
        uint32_t bits = 0;
        for (uint32_t j = 0; j < p.nout; ++j) bits |= (__ballot((differs >> j) & 1u) != 0 ? 1u : 0u) << out_ids[j];
        report_mismatch(v.check + stripe, a.bad_count, bits);
    }
}

constexpr const char* kFastCheckName = "rs104_check_kernel<8 B per lane> (table lookup)";
constexpr const char* kStrideCheckName = "rs104_check_stride_kernel (table lookup)";

// The fast check takes shard lengths that are a multiple of 2 KiB below 4 GiB
// whose chunks fit one launch (launch_check's stripe ranges hold whole stripes).
static const FastKind<CheckArgs> kFastCheck{kNarrowGeom, rs104_check_kernel, rs104_check_kernel};

const char* check_kernel_name(uint64_t len) {
    if (len == 0) return kNoLaunch;
    return kFastCheck.serves(len) ? kFastCheckName : kStrideCheckName;
}

hipError_t launch_check(const CheckArgs& v, bool aligned, hipStream_t stream) {
    if (aligned && kFastCheck.serves(v.a.len)) return launch_fast_ranges(kFastCheck, v, stream);
    return launch_stride(aligned ? rs104_check_stride_kernel<true> : rs104_check_stride_kernel<false>, v, stream);
}

// rs104_locate_kernel made mask-driven: the syndrome has r = p - 10 rows (rows
// past r stay zero: zero tables, no stored row), H_m = [A_m | I_r].
//  * r = 1: every non-zero column is unexplained (one row cannot tell shards
//    apart);
//  * exactly one of r >= 2 rows non-zero -> shard E[j];
//  * all r non-zero -> shard B[c] when s[j] = s[0] * A_m[j][c] / A_m[0][c] for
//    j = 1..r-1 (no entry of A_m is zero and no two columns of H_m are
//    proportional, for every mask: tests/test_check_model.py);
//  * anything else is unexplained.
//
// CORRECT (rs104_correct_present_kernel, hec.h hec_gpu_correct_present_batch):
// the same walk over CorrectPresentArgs; in a stripe with r >= min_spares
// (wave-uniform: one scalar compare) a lane also XORs the error value into the
// wrong byte of every column it explains (fix_shard, addressed in place):
// s[j] for shard E[j], s[0] / A_m[0][c] for shard B[c], each masked to the
// bytes that name that shard. A lane's 16 columns belong to no other lane and
// its syndrome is complete before its first store, so names and values are
// those of the bytes as they were. Unexplained columns, and every column of a
// stripe with fewer spares, are not touched.
//
// RAGGED (rs104_ragged_locate_kernel, hec.h hec_gpu_locate_corrupt_ragged): the
// same classification over a ragged batch. Only the walk differs: the items
// are the 4 KiB ranges of pass 1's workgroup map (two per entry when that map
// is the bit-sliced one: no second map is built), and the stripe's base,
// stride, length and mask come from its RaggedItem. An item of a clean stripe
// costs the scalar loads of block_item[entry] and check[stripe]; neither its
// RaggedItem nor a shard is touched. The two walks are compile-time branches
// in the body, not device functions over the argument structs: with accessor
// functions that take the arguments by reference, or the body as a function
// of its own, the backend allocates the registers of the strided form
// differently (profiles/ragged_scrub/isa.md); written this way the strided
// forms keep their instruction streams.
//
// RAGGED and CORRECT (rs104_ragged_correct_kernel, hec.h hec_gpu_correct_ragged):
// the ragged walk with the fixes, over RaggedCorrectArgs. fix_shard's RAGGED
// form reads the stripe's RaggedItem again where a fix happens and addresses
// shard c from the stripe's own base, stride and length.
template <bool ALIGNED, bool CORRECT = false, bool RAGGED = false>
__global__ __launch_bounds__(kThreads) void rs104_locate_present_kernel(
    std::conditional_t<RAGGED, std::conditional_t<CORRECT, RaggedCorrectArgs, RaggedScrubArgs>,
                       std::conditional_t<CORRECT, CorrectPresentArgs, CheckArgs>> v) {
    constexpr int K = 10, N = 14, R = 4;
    const auto& a = v.a;  // ApplyArgs, or the ragged batch
    cu32p flagged = as_const(v.check);
    uint64_t n_items;
    if constexpr (RAGGED)
        n_items = uint64_t(a.n_blocks) << v.half_shift;
    else
        n_items = a.n_items;
    for (uint64_t item = stride_first_item(); item < n_items; item += gridDim.x) {
        uint32_t stripe, chunk;
        if constexpr (RAGGED) {
            stripe = as_const(a.block_item)[item >> v.half_shift];
            // the range within its entry; the entry's place in the stripe is added past the flag check
            chunk = uint32_t(item) & ((1u << v.half_shift) - 1u);
        } else {
            stripe = uint32_t(item / a.chunks_per_stripe);
            chunk = uint32_t(item - uint64_t(stripe) * a.chunks_per_stripe);
        }
        if (flagged[stripe] == 0) continue;  // pass 1 found the stripe clean, or had nothing to check
        [[maybe_unused]] const __attribute__((address_space(4))) RaggedItem* it = nullptr;
        uint32_t mask;
        if constexpr (RAGGED) {
            it = as_const(a.items) + stripe;
            chunk += (uint32_t(item >> v.half_shift) - it->first_block) << v.half_shift;
            mask = it->mask & ((1u << N) - 1);
        } else {
            mask = as_const(a.masks)[stripe] & ((1u << N) - 1);
        }
        const uint32_t pid = as_const(a.lut)[mask];
        if (pid == kNoPlan) continue;  // never flagged by pass 1
        const uint32_t r = uint32_t(__builtin_popcount(mask)) - K;
        uint32_t in_id[K], out_id[R];
        uint32_t m = mask;
#pragma unroll
        for (int i = 0; i < K; ++i) {
            in_id[i] = __builtin_ctz(m);
            m &= m - 1;
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            out_id[j] = m ? __builtin_ctz(m) : 0;
            m &= m - 1;
        }
        cu32p tab = as_const(a.tabs) + pid * (K * R * 5);              // A_m: [K][R][5] words
        cu32p rat = as_const(v.ratio_tabs) + pid * (K * (R - 1) * 5);  // [K][R - 1][5] words
        const uint8_t* b;  // the stripe's shard 0; its shard stride and length
        uint64_t shard, len;
        if constexpr (RAGGED) {
            b = a.base + it->off;
            shard = it->shard_stride;
            len = it->len;
        } else {
            b = a.in_base + uint64_t(stripe) * a.in_stripe;
            shard = a.in_shard;
            len = a.len;
        }
        const uint64_t o = uint64_t(chunk) * (kThreads * kVecBytes) + threadIdx.x * kVecBytes;
        u32x4 s[R];
#pragma unroll
        for (int j = 0; j < R; ++j) s[j] = u32x4{0, 0, 0, 0};
        if (o < len) {
            const uint64_t avail = len - o;
            if (avail >= kVecBytes) {
                u32x4 d[K];
#pragma unroll
                for (int i = 0; i < K; ++i) d[i] = load_full(b + uint64_t(in_id[i]) * shard + o, ALIGNED);
#pragma unroll
                for (int i = 0; i < K; ++i) gf_mac<R>(s, d[i], tab + i * (R * 5));
#pragma unroll
                for (int j = 0; j < R; ++j)
                    if (uint32_t(j) < r) s[j] ^= load_full(b + uint64_t(out_id[j]) * shard + o, ALIGNED);
            } else {
                for (int i = 0; i < K; ++i)
                    gf_mac<R>(s, load_tail(b + uint64_t(in_id[i]) * shard + o, avail), tab + i * (R * 5));
                for (int j = 0; j < R; ++j)
                    if (uint32_t(j) < r) s[j] ^= load_tail(b + uint64_t(out_id[j]) * shard + o, avail);
            }
        }
        uint32_t any = 0;
#pragma unroll
        for (int j = 0; j < R; ++j) any |= s[j][0] | s[j][1] | s[j][2] | s[j][3];
        if (__ballot(any != 0) == 0) continue;  // wave-uniform: this wave's 1 KiB is clean
        using Fix = std::conditional_t<RAGGED, RaggedFixLane, FixLane>;
        [[maybe_unused]] std::conditional_t<CORRECT, Fix, NoFix> fx;
        [[maybe_unused]] bool write = false;  // wave-uniform: the stripe has the spares the caller asked for
        if constexpr (CORRECT) {
            fx = Fix{&a, stripe, chunk, 0};
            write = r >= v.min_spares;
        }

        // rows at or past r count as non-zero in "all rows"; with one row
        // nothing is ever named
        const uint32_t kEach = 0x80808080u;
        const uint32_t f1 = r > 1 ? 0u : kEach, f2 = r > 2 ? 0u : kEach, f3 = r > 3 ? 0u : kEach;
        const uint32_t naming = r > 1 ? ~0u : 0u;
        uint32_t one[R] = {0, 0, 0, 0};  // bytes where only s[j] is non-zero
        uint32_t allr[4];                // per dword: bytes where all r rows are
        uint32_t unexplained = 0, all_any = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t n0 = nz_bytes(s[0][w]), n1 = nz_bytes(s[1][w]), n2 = nz_bytes(s[2][w]),
                           n3 = nz_bytes(s[3][w]);
            const uint32_t o0 = n0 & ~(n1 | n2 | n3) & naming, o1 = n1 & ~(n0 | n2 | n3) & naming,
                           o2 = n2 & ~(n0 | n1 | n3) & naming, o3 = n3 & ~(n0 | n1 | n2) & naming;
            one[0] |= o0;
            one[1] |= o1;
            one[2] |= o2;
            one[3] |= o3;
            allr[w] = n0 & (n1 | f1) & (n2 | f2) & (n3 | f3) & naming;
            all_any |= allr[w];
            unexplained |= (n0 | n1 | n2 | n3) & ~allr[w] & ~(o0 | o1 | o2 | o3);
        }
        uint32_t bits = 0;
        if (__ballot(all_any != 0) != 0) {  // wave-uniform: some column may name a shard of B
            uint32_t matched[4] = {0, 0, 0, 0};
            uint32_t bm = mask;  // its lowest set bit is B[c]
#pragma unroll 1
            for (int c = 0; c < K; ++c) {
                u32x4 e[R - 1];
#pragma unroll
                for (int j = 0; j < R - 1; ++j) e[j] = u32x4{0, 0, 0, 0};
                gf_mac<R - 1>(e, s[0], rat + c * ((R - 1) * 5));
                uint32_t hit = 0;
#pragma unroll
                for (int w = 0; w < 4; ++w) {
                    const uint32_t diff = (e[0][w] ^ s[1][w]) | (e[1][w] ^ s[2][w]) | (e[2][w] ^ s[3][w]);
                    const uint32_t mt = allr[w] & ~nz_bytes(diff);
                    matched[w] |= mt;
                    hit |= mt;
                    if constexpr (CORRECT) e[0][w] = (mt >> 7) * 0xFFu;  // the ratios are spent: the bytes B[c] explains
                }
                bits |= (__ballot(hit != 0) != 0 ? 1u : 0u) << __builtin_ctz(bm);
                if constexpr (CORRECT) {
                    if (write && __ballot(hit != 0) != 0) {  // wave-uniform: somebody fixes shard B[c]
                        u32x4 val[1] = {u32x4{0, 0, 0, 0}};
                        gf_mac<1>(val, s[0], as_const(v.fix_tabs) + pid * (K * 5) + c * 5);  // s[0] / A_m[0][c]
                        fix_shard<ALIGNED, true, RAGGED>(fx, __builtin_ctz(bm), val[0] & e[0]);
                    }
                }
                bm &= bm - 1;
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) unexplained |= allr[w] & ~matched[w];
        }
#pragma unroll
        for (int j = 0; j < R; ++j) bits |= (__ballot(one[j] != 0) != 0 ? 1u : 0u) << out_id[j];
        if (__ballot(unexplained != 0) != 0) bits |= kSuspectUnexplained;
        if constexpr (!CORRECT) {
            if (bits != 0 && (threadIdx.x & 63u) == 0) atomicOr(v.suspects + stripe, bits);
        } else {
            if (write) {
#pragma unroll
                for (int j = 0; j < R; ++j) {
                    if (__ballot(one[j] != 0) == 0) continue;  // wave-uniform: nobody fixes shard E[j]
                    u32x4 e;
#pragma unroll
                    for (int w = 0; w < 4; ++w) {
                        uint32_t others = 0;
#pragma unroll
                        for (int i = 0; i < R; ++i)
                            if (i != j) others |= nz_bytes(s[i][w]);
                        e[w] = s[j][w] & ((nz_bytes(s[j][w]) & ~others) >> 7) * 0xFFu;
                    }
                    fix_shard<ALIGNED, true, RAGGED>(fx, int(out_id[j]), e);
                }
            }
            // the bytes this wave changed, at most 16 a lane: five ballots
            uint32_t total = 0;
#pragma unroll
            for (int k = 0; k < 5; ++k)
                total += uint32_t(__builtin_popcountll(__ballot(((fx.changed >> k) & 1u) != 0))) << k;
            if ((threadIdx.x & 63u) == 0) {
                // a stripe the call leaves inconsistent is counted once: with the
                // spares, by the atomicOr that first sets bit 31; without them, by
                // the one that finds the word zero (bits != 0 in every wave here)
                if (bits != 0) {
                    const uint32_t old = atomicOr(v.suspects + stripe, bits);
                    const bool first = write ? (old & kSuspectUnexplained) == 0 && (bits & kSuspectUnexplained) != 0
                                             : old == 0;
                    if (first && v.uncorrected) atomicAdd(v.uncorrected, 1u);
                }
                if (total != 0 && v.corrected_bytes) atomicAdd(v.corrected_bytes, (unsigned long long)total);
            }
        }
    }
}

// The masked locate (CORRECT: rs104_correct_present_kernel, taking
// CorrectPresentArgs) on the locate grid; launch_ragged_walk launches the
// RAGGED forms.
template <bool CORRECT, typename Args>
static hipError_t launch_locate_present_form(const Args& v, bool aligned, hipStream_t stream) {
    return launch_stride(
        aligned ? rs104_locate_present_kernel<true, CORRECT> : rs104_locate_present_kernel<false, CORRECT>, v, stream,
        kLocateMaxBlocks);
}

hipError_t launch_locate_present(const CheckArgs& v, bool aligned, hipStream_t stream) {
    return launch_locate_present_form<false>(v, aligned, stream);
}

hipError_t launch_correct_present(const CorrectPresentArgs& v, bool aligned, hipStream_t stream) {
    return launch_locate_present_form<true>(v, aligned, stream);
}

// ---------------------------------------------------------------------------
// Ragged scrub (hec.h hec_gpu_verify_ragged / hec_gpu_locate_corrupt_ragged):
// the masked verify and locate over stripes of mixed lengths and masks. Pass 1
// is one workgroup per map entry (launch_ragged: XCD eighths, launches of at
// most kMaxLaunchBlocks), pass 2 the masked locate's RAGGED walk over the same
// map. The stripe index of a map entry is the entry itself (block_item), so
// both passes reach the stripe's result words without a search.
// ---------------------------------------------------------------------------
// Every mask full and every length a multiple of 8 KiB:
// rs104_bs_ragged_kernel's addressing over the verify form of rs104_bs_chunk
// (the stored parity handed over as base + offset, as rs104_bs_verify_kernel
// does). Its bits are by parity row; the check word's are by shard index.
__global__ __launch_bounds__(kThreads) void rs104_bs_ragged_verify_kernel(RaggedScrubArgs v) {
    const RaggedArgs& a = v.a;
    const uint32_t blk = ragged_block(a);
    const uint32_t stripe = as_const(a.block_item)[blk];
    const __attribute__((address_space(4))) RaggedItem* it = as_const(a.items) + stripe;
    const uint64_t off = it->off, stride = it->shard_stride;
    const uint32_t first = it->first_block;
    const uint32_t bits =
        rs104_bs_chunk<uint32_t, true>(a.base + off, a.base, stride, stride, blk - first, off + 10 * stride);
    report_mismatch(v.check + stripe, a.bad_count, bits << 10);
}

// Everything else: rs104_check_kernel's loads-first shape at rs104_chunk's 16
// bytes per lane, one 4 KiB range per workgroup, any length >= 1. The ten B
// loads and the r stored E loads are issued before the math and the plan
// lookup overlaps them; the last vector of a shard goes through load_tail,
// which zero-fills from the length on, inputs and stored rows alike, so bytes
// at or past it compare equal whatever memory holds there. Lanes past the end
// load nothing and keep zeros; they still take part in the ballots.
__global__ __launch_bounds__(kThreads) void rs104_ragged_check_kernel(RaggedScrubArgs v) {
    constexpr int K = 10, N = 14, R = 4;
    const RaggedArgs& a = v.a;
    const uint32_t blk = ragged_block(a);
    const uint32_t stripe = as_const(a.block_item)[blk];
    const __attribute__((address_space(4))) RaggedItem* it = as_const(a.items) + stripe;
    const uint64_t off = it->off, stride = it->shard_stride;
    const uint32_t len = it->len, first = it->first_block;
    const uint32_t mask = it->mask & ((1u << N) - 1);
    const uint32_t present = __builtin_popcount(mask);
    if (present <= K) return;  // owns no map entry (the host counts it): never taken
    const uint32_t r = present - K;
    uint32_t in_id[K], out_id[R];
    uint32_t m = mask;
#pragma unroll
    for (int i = 0; i < K; ++i) {  // B: the ten lowest present shards
        in_id[i] = __builtin_ctz(m);
        m &= m - 1;
    }
#pragma unroll
    for (int j = 0; j < R; ++j) {  // E: the other present shards, ascending
        out_id[j] = m ? __builtin_ctz(m) : 0;
        m &= m - 1;
    }
    uint32_t plan = as_const(a.lut)[mask];  // first used after the data loads
    const uint8_t* b = a.base + off;
    const uint32_t o = (blk - first) * uint32_t(kThreads * kVecBytes) + threadIdx.x * kVecBytes;
    u32x4 acc[R], st[R];
#pragma unroll
    for (int j = 0; j < R; ++j) acc[j] = st[j] = u32x4{0, 0, 0, 0};
    if (o < len) {
        const uint32_t avail = len - o;
        if (avail >= uint32_t(kVecBytes)) {
            u32x4 d[K];
#pragma unroll
            for (int i = 0; i < K; ++i) d[i] = load_at(b + uint64_t(in_id[i]) * stride, o);
#pragma unroll
            for (int j = 0; j < R; ++j)
                if (uint32_t(j) < r) st[j] = load_at(b + uint64_t(out_id[j]) * stride, o);
            __builtin_amdgcn_sched_barrier(0);  // every load in flight before the math
            asm volatile("" : "+s"(plan));
            cu32p tab = as_const(a.tabs) + plan * (K * R * 5);
#pragma unroll
            for (int i = 0; i < K; i += 2)
                gf_mac2<R>(acc, d[i], d[i + 1], tab + i * (R * 5), tab + (i + 1) * (R * 5), r);
        } else {
            asm volatile("" : "+s"(plan));
            cu32p tab = as_const(a.tabs) + plan * (K * R * 5);
            // rows at or past r: zero tables, no stored row
            for (int i = 0; i < K; ++i)
                gf_mac<R>(acc, load_tail(b + uint64_t(in_id[i]) * stride + o, avail), tab + i * (R * 5));
            for (int j = 0; j < R; ++j)
                if (uint32_t(j) < r) st[j] = load_tail(b + uint64_t(out_id[j]) * stride + o, avail);
        }
    }
    // rows at or past r: acc and st are both zero, the ballot is empty
    uint32_t bits = 0;
#pragma unroll
    for (int j = 0; j < R; ++j) {
        const u32x4 x = acc[j] ^ st[j];
        bits |= (__ballot((x[0] | x[1] | x[2] | x[3]) != 0) != 0 ? 1u : 0u) << out_id[j];
    }
    report_mismatch(v.check + stripe, a.bad_count, bits);
}

constexpr const char* kBsRaggedVerifyName = "rs104_bs_ragged_verify_kernel (bit-sliced, XCD eighths)";
constexpr const char* kRaggedCheckName = "rs104_ragged_check_kernel (table lookup, XCD eighths)";

const char* ragged_scrub_kernel_name(bool bitslice) { return bitslice ? kBsRaggedVerifyName : kRaggedCheckName; }

hipError_t launch_ragged_check(const RaggedScrubArgs& v, bool bitslice, hipStream_t stream) {
    return launch_ragged(bitslice ? rs104_bs_ragged_verify_kernel : rs104_ragged_check_kernel, v, stream);
}

// The masked locate's RAGGED form (rs104_ragged_locate_kernel, taking
// RaggedScrubArgs; CORRECT: rs104_ragged_correct_kernel, taking
// RaggedCorrectArgs) over the 4 KiB ranges of pass 1's map, on the locate grid.
template <bool CORRECT, typename Args>
static hipError_t launch_ragged_walk(Args v, bool bitslice, hipStream_t stream) {
    v.half_shift = bitslice ? 1u : 0u;  // an 8 KiB entry is two of the walk's 4 KiB ranges
    return launch_grid_stride(rs104_locate_present_kernel<true, CORRECT, true>, v,
                              uint64_t(v.a.n_blocks) << v.half_shift, kLocateMaxBlocks, stream);
}

hipError_t launch_ragged_locate(const RaggedScrubArgs& v, bool bitslice, hipStream_t stream) {
    return launch_ragged_walk<false>(v, bitslice, stream);
}

hipError_t launch_ragged_correct(const RaggedCorrectArgs& v, bool bitslice, hipStream_t stream) {
    return launch_ragged_walk<true>(v, bitslice, stream);
}

__global__ void add_word_kernel(uint32_t* word, uint32_t n) { atomicAdd(word, n); }

hipError_t launch_add_word(uint32_t* word, uint32_t n, hipStream_t stream) {
    hipLaunchKernelGGL(add_word_kernel, dim3(1), dim3(1), 0, stream, word, n);
    return hipGetLastError();
}

// repair_masks_kernel's rounds (mask_rounds) with the present mask and the
// check word taken into account.
__global__ __launch_bounds__(kThreads) void use_masks_kernel(const uint32_t* present, const uint32_t* check,
                                                             const uint32_t* suspects, uint32_t* use,
                                                             uint32_t* unrepaired, uint32_t n_stripes) {
    mask_rounds(n_stripes, unrepaired, [&](uint64_t s) {
        const uint32_t m = present[s] & kAllShards;
        if (check[s] == 0) {
            use[s] = m;  // clean, or nothing to check: the plain reconstruct
            return false;
        }
        const uint32_t w = suspects[s], kept = m & ~w;
        const bool repair =
            (w & kSuspectUnexplained) == 0 && (w & kAllShards) != 0 && __builtin_popcount(kept) >= 10;
        use[s] = repair ? kept : kAllShards;
        return !repair;
    });
}

hipError_t launch_use_masks(const uint32_t* present, const uint32_t* check, const uint32_t* suspects, uint32_t* use,
                            uint32_t* unrepaired, uint32_t n_stripes, hipStream_t stream) {
    return launch_mask_rounds(use_masks_kernel, n_stripes, stream, present, check, suspects, use, unrepaired,
                              n_stripes);
}

// The use masks after rs104_correct_present_kernel (min_spares: the call's):
// nothing is dropped; a stripe is rebuilt from its own survivors when they are
// consistent (clean, unchecked, or corrected with bit 31 clear) and left
// alone, holes included, otherwise.
__global__ __launch_bounds__(kThreads) void use_masks_corrected_kernel(const uint32_t* present, const uint32_t* check,
                                                                       const uint32_t* suspects, uint32_t* use,
                                                                       uint32_t* unrepaired, uint32_t min_spares,
                                                                       uint32_t n_stripes) {
    mask_rounds(n_stripes, unrepaired, [&](uint64_t s) {
        const uint32_t m = present[s] & kAllShards;
        const bool consistent =
            check[s] == 0 || (uint32_t(__builtin_popcount(m)) >= 10 + min_spares &&
                              (suspects[s] & kSuspectUnexplained) == 0);
        use[s] = consistent ? m : kAllShards;
        return !consistent;
    });
}

hipError_t launch_use_masks_corrected(const uint32_t* present, const uint32_t* check, const uint32_t* suspects,
                                      uint32_t* use, uint32_t* unrepaired, uint32_t min_spares, uint32_t n_stripes,
                                      hipStream_t stream) {
    return launch_mask_rounds(use_masks_corrected_kernel, n_stripes, stream, present, check, suspects, use,
                              unrepaired, min_spares, n_stripes);
}

// use_masks_corrected_kernel after rs104_ragged_correct_kernel: the present
// masks come from the scrub's items, and a stripe left alone also gets mask
// 0x3FFF in the decode's own items (a vector store into their device copy,
// read by the scalar loads of the decode kernel that follows on the stream),
// where rs104_chunk<DEC> returns at once: it keeps its holes.
__global__ __launch_bounds__(kThreads) void ragged_use_masks_corrected_kernel(
    const RaggedItem* scrub_items, RaggedItem* decode_items, const uint32_t* check, const uint32_t* suspects,
    uint32_t* use, uint32_t* unrepaired, uint32_t min_spares, uint32_t n_stripes) {
    mask_rounds(n_stripes, unrepaired, [&](uint64_t s) {
        const uint32_t m = scrub_items[s].mask & kAllShards;
        const bool consistent =
            check[s] == 0 || (uint32_t(__builtin_popcount(m)) >= 10 + min_spares &&
                              (suspects[s] & kSuspectUnexplained) == 0);
        use[s] = consistent ? m : kAllShards;
        if (!consistent) decode_items[s].mask = kAllShards;
        return !consistent;
    });
}

hipError_t launch_ragged_use_masks_corrected(const RaggedItem* scrub_items, RaggedItem* decode_items,
                                             const uint32_t* check, const uint32_t* suspects, uint32_t* use,
                                             uint32_t* unrepaired, uint32_t min_spares, uint32_t n_stripes,
                                             hipStream_t stream) {
    return launch_mask_rounds(ragged_use_masks_corrected_kernel, n_stripes, stream, scrub_items, decode_items, check,
                              suspects, use, unrepaired, min_spares, n_stripes);
}

// ---------------------------------------------------------------------------
// splitmix64 synthetic stripes (deterministic bench / test inputs)
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void fill_splitmix_kernel(uint8_t* base, uint64_t stripe_stride,
                                                                  uint64_t bytes_per_stripe,
                                                                  uint32_t n_stripes, uint64_t seed_base) {
    const uint64_t words = (bytes_per_stripe + 7) / 8;
    const uint64_t total = words * n_stripes;
    for (uint64_t t = uint64_t(blockIdx.x) * kThreads + threadIdx.x; t < total;
         t += uint64_t(gridDim.x) * kThreads) {
        const uint64_t s = t / words;
        const uint64_t w = t - s * words;
        uint64_t z = seed_base + s + (w + 1) * 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        uint8_t* p = base + s * stripe_stride + w * 8;
        const uint64_t left = bytes_per_stripe - w * 8;
        if (left >= 8 && (reinterpret_cast<uintptr_t>(p) & 7) == 0) {
            *reinterpret_cast<uint64_t*>(p) = z;
        } else {
            for (uint64_t b = 0; b < 8 && b < left; ++b) p[b] = uint8_t(z >> (8 * b));
        }
    }
}

hipError_t launch_fill_splitmix(uint8_t* base, uint64_t stripe_stride, uint64_t bytes_per_stripe,
                                uint32_t n_stripes, uint64_t seed_base, hipStream_t stream) {
    const uint64_t total = ((bytes_per_stripe + 7) / 8) * n_stripes;
    if (total == 0) return hipSuccess;
    uint64_t grid = (total + kThreads - 1) / kThreads;
    if (grid > 65536) grid = 65536;
    hipLaunchKernelGGL(fill_splitmix_kernel, dim3(uint32_t(grid)), dim3(kThreads), 0, stream, base,
                       stripe_stride, bytes_per_stripe, n_stripes, seed_base);
    return hipGetLastError();
}

}  // namespace hec

#ifdef HEC_MAX_LAUNCH_BLOCKS
// Test builds only (rs_kernels.hpp): the limits this library was compiled
// with, so a test can prove that the variant it loaded is the one it meant.
// The shipped library does not export this.
extern "C" void hec_test_launch_limits(uint64_t* max_launch_blocks, uint32_t* locate_max_blocks) {
    *max_launch_blocks = hec::kMaxLaunchBlocks;
    *locate_max_blocks = hec::kLocateMaxBlocks;
}
#endif
