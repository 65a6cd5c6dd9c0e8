// Ragged update kernels (hec.h hec_gpu_update_ragged, hec_rs_update_batch), in a
// file of their own: rs_kernels.hip and its object stay what the launch record
// (tests/test_launch_record.py) pins.
#include "rs_device.hpp"

namespace hec {

// ---------------------------------------------------------------------------
// Ragged update (hec.h hec_gpu_update_ragged): rs104_update_kernel's body
// behind the ragged workgroup map, every stripe with its own length, mask and
// place in the three arenas (UpdateItem, rs_kernels.hpp). The strided kernels
// above keep their code: the body is written out again here, not shared.
// ---------------------------------------------------------------------------

// Descriptor of the stripe workgroup blk works on, as ragged_item: scalar loads
// of the item the map names, or the kernel-argument copy of a one-stripe launch.
// The old arena's fields are loaded only where there is one.
template <bool HAS_OLD>
__device__ __forceinline__ UpdateItem update_item(const RaggedUpdateArgs& v, uint32_t blk) {
    if (v.a.inline_one) return v.one;
    const __attribute__((address_space(4))) UpdateItem* p = as_const(v.items) + as_const(v.a.block_item)[blk];
    return UpdateItem{p->par_off,       p->par_stride, p->new_off, p->new_stride,
                      HAS_OLD ? p->old_off : 0, HAS_OLD ? p->old_stride : 0, p->len, p->mask, p->first_block, 0};
}

// The lane that crosses the stripe's length: the `avail` (< 16) bytes left of
// every shard byte-wise, one changed shard at a time, the pointers already at
// the lane's offset (update_lane's tail form over an item's own strides).
template <bool HAS_OLD, bool COMPACT>
__device__ __forceinline__ void ragged_update_tail(const UpdateItem& it, uint32_t u, const uint8_t* new_b,
                                                   const uint8_t* old_b, uint8_t* par_b, cu32p tab, uint64_t avail) {
    constexpr int R = 4;
    u32x4 acc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) acc[r] = u32x4{0, 0, 0, 0};
    for (uint32_t q = 0; u; u &= u - 1, ++q) {
        const uint32_t c = __builtin_ctz(u);
        u32x4 d = load_tail(new_b + uint64_t(COMPACT ? q : c) * it.new_stride, avail);
        if constexpr (HAS_OLD) d ^= load_tail(old_b + uint64_t(c) * it.old_stride, avail);
        gf_mac<R>(acc, d, tab + c * (R * 5));
    }
    for (int r = 0; r < R; ++r) {
        uint8_t* row = par_b + uint64_t(r) * it.par_stride;
        store_tail(row, acc[r] ^ load_tail(row, avail), avail);
    }
}

// One workgroup per map entry: a stripe with U non-empty and one 4 KiB column
// range of it, 16 bytes per lane. The four parity loads go first, then the
// changed shards two at a time (scalar bit scan; COMPACT: a counter beside it
// is the shard's slot in the new arena, so no shard-id multiply there).
template <bool HAS_OLD, bool COMPACT>
__global__ __launch_bounds__(kThreads) void rs104_ragged_update_kernel(RaggedUpdateArgs v) {
    static_assert(!(HAS_OLD && COMPACT), "the compact layout holds deltas: no old arena");
    constexpr int R = 4;
    const RaggedArgs& a = v.a;
    const uint32_t blk = ragged_block(a);
    const UpdateItem it = update_item<HAS_OLD>(v, blk);
    uint32_t u = it.mask & kUpdateBits;
    // a length below 2^32: the last lane's offset fits 32 bits
    const uint32_t o = (blk - it.first_block) * uint32_t(kThreads * kVecBytes) + uint32_t(threadIdx.x * kVecBytes);
    if (u != 0 && o < it.len) {
        const uint64_t avail = it.len - o;
        const uint8_t* new_b = v.new_base + it.new_off;
        const uint8_t* old_b = HAS_OLD ? v.old_base + it.old_off : nullptr;
        uint8_t* par_b = a.base + it.par_off;
        cu32p tab = as_const(a.tabs);
        if (avail >= kVecBytes) {
            u32x4 acc[R], p[R];
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r] = u32x4{0, 0, 0, 0};
#pragma unroll
            for (int r = 0; r < R; ++r) p[r] = load_at(par_b + uint64_t(r) * it.par_stride, o);
            uint32_t q = 0;  // COMPACT: slots taken so far
            while (u) {
                const uint32_t c0 = __builtin_ctz(u);
                u &= u - 1;
                u32x4 d0 = load_at(new_b + uint64_t(COMPACT ? q : c0) * it.new_stride, o);
                if constexpr (HAS_OLD) d0 ^= load_at(old_b + uint64_t(c0) * it.old_stride, o);
                if (u) {
                    const uint32_t c1 = __builtin_ctz(u);
                    u &= u - 1;
                    u32x4 d1 = load_at(new_b + uint64_t(COMPACT ? q + 1 : c1) * it.new_stride, o);
                    if constexpr (HAS_OLD) d1 ^= load_at(old_b + uint64_t(c1) * it.old_stride, o);
                    q += 2;
                    __builtin_amdgcn_sched_barrier(0);
                    gf_mac2<R>(acc, d0, d1, tab + c0 * (R * 5), tab + c1 * (R * 5));
                } else {
                    __builtin_amdgcn_sched_barrier(0);
                    gf_mac<R>(acc, d0, tab + c0 * (R * 5));
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) store_at(par_b + uint64_t(r) * it.par_stride, o, acc[r] ^ p[r]);
        } else {  // the lane that crosses len, in the stripe's last column range
            ragged_update_tail<HAS_OLD, COMPACT>(it, u, new_b + o, HAS_OLD ? old_b + o : nullptr, par_b + o, tab, avail);
        }
    }
    if (a.done_flag) signal_done(a.done_count, a.done_flag, a.done_seq);
}

const char* ragged_update_kernel_name(bool has_old) {
    return has_old ? "rs104_ragged_update_kernel<HAS_OLD=true> (table lookup, XCD eighths)"
                   : "rs104_ragged_update_kernel<HAS_OLD=false> (table lookup, XCD eighths)";
}

hipError_t launch_ragged_update(const RaggedUpdateArgs& v, hipStream_t stream) {
    if (v.a.compact) return launch_ragged(rs104_ragged_update_kernel<false, true>, v, stream);
    return launch_ragged(v.old_base ? rs104_ragged_update_kernel<true, false> : rs104_ragged_update_kernel<false, false>,
                         v, stream);
}

}  // namespace hec
