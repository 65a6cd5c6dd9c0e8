// Host-memory stripe batches through the GPU: the path helyim actually runs
// (shard bytes start and end in host memory: .dat pages / shard files,
// helyim-ec/src/encoder.rs:169-195, 263-304). Chunks of stripes are pipelined
// over kDepth HIP streams, each with its own device slot, so the H2D copy of
// chunk i+1, the kernel of chunk i and the D2H copy of chunk i-1 overlap
// (PCIe Gen5 x16 is full duplex; the copy engines run beside the kernel).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "hec_internal.hpp"
#include "host_chunks.hpp"  // kChunkBytes: target bytes of one chunk's shards

namespace hec {
namespace {

constexpr int kDepth = 3;

// One slot of the per-device pool of pipelines (SlotPool, hec_internal.hpp):
// concurrent host batches on one device -- other threads, or two ranges of one
// multi-device call on the same GPU -- each lease their own streams and slots.
// Up to kScratchSlots (8) pipelines exist per device, but only the first
// kWarmSlots (2) keep their staging between calls (end_call), so the steady
// footprint per device is that of two pipelines (INTEGRATION.md §5 states the
// worst case).
struct Pipeline {
    std::mutex mu;
    hipStream_t streams[kDepth] = {};
    DeviceBuf<> slot[kDepth];               // exact bytes, all reallocated together
    DeviceBuf<uint32_t> mask_dev[kDepth];
    PinnedBuf<uint32_t> mask_host[kDepth];  // pinned staging for per-chunk masks
    DeviceBuf<uint32_t> want_dev[kDepth];   // reconstruct some: per-chunk want words, reserved by
    PinnedBuf<uint32_t> want_host[kDepth];  // reserve_wants on that call's first use
    // pinned staging for pageable callers: two slots the kernels code in place
    PinnedBuf<> hslot[2];
    hipEvent_t hdone[2] = {};
    int init() {
        for (auto& st : streams) HEC_HIP(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        return HEC_OK;
    }
    int reserve(size_t slot_bytes, size_t n_masks) {
        HEC_TRY(reserve_all(slot, slot_bytes));
        HEC_TRY(reserve_all(mask_dev, n_masks * 4));
        return reserve_all(mask_host, n_masks * 4);
    }
    int reserve_wants(size_t n_masks) {
        HEC_TRY(reserve_all(want_dev, n_masks * 4));
        return reserve_all(want_host, n_masks * 4);
    }
    int reserve_host(size_t bytes) {
        if (!hdone[0])
            for (auto& e : hdone) HEC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return reserve_all(hslot, bytes);
    }
    // Staging bytes held (pinned host, device).
    uint64_t pinned_bytes() const {
        uint64_t b = hslot[0].cap + hslot[1].cap;
        for (auto& m : mask_host) b += m.cap;
        for (auto& m : want_host) b += m.cap;
        return b;
    }
    uint64_t device_bytes() const {
        uint64_t b = 0;
        for (int i = 0; i < kDepth; ++i) b += slot[i].cap + mask_dev[i].cap + want_dev[i].cap;
        return b;
    }
    // Host batches code caller memory in place (zero copy) or copy into it: an
    // error return between enqueues must not leave that work in flight for the
    // caller's freed buffers (StreamDrain's rule), so every call ends by
    // draining the streams; after a successful call they are idle already. A
    // burst slot then frees its large staging (the pageable path's pinned
    // slots and the copy path's device slots); streams, events and mask words
    // stay, and the next call on this pipeline reserves again.
    void end_call(bool burst) {
        for (auto st : streams)
            if (st && hipStreamSynchronize(st) != hipSuccess) (void)hipGetLastError();
        if (!burst) return;
        for (auto& h : hslot) h.release();
        for (auto& d : slot) d.release();
    }
    ~Pipeline() {  // only a slot whose init() failed is ever destroyed
        for (auto st : streams)
            if (st) (void)hipStreamDestroy(st);
    }
};

// Copy `rows` rows of `width` bytes with pitches (2D; 1D when both are dense).
hipError_t copy2d(void* dst, uint64_t dpitch, const void* src, uint64_t spitch, uint64_t width, uint64_t rows,
                  hipMemcpyKind kind, hipStream_t s) {
    if (rows == 0 || width == 0) return hipSuccess;
    if (rows == 1 || (dpitch == width && spitch == width))
        return hipMemcpyAsync(dst, src, width * rows, kind, s);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, rows, kind, s);
}

// Zero-copy: pinned host memory that the GPU can address directly
// (hipHostMalloc / torch pin_memory) is handed to the kernel as is, so the
// kernel's loads and stores cross PCIe themselves -- no staging slots, no SDMA
// copies, both directions at once. Measured 51 GiB/s of data encoded vs 41-44
// for the copy pipeline (profiles/r02/HISTORY.md "host path"). The whole
// [p, p + span) must be one registered host range; anything else (pageable
// memory, device memory, a range running past the allocation) takes the copy
// pipeline. hec_set_host_zero_copy(0) disables it (the CUs then stay free
// while SDMA engines move the bytes).
bool host_device_view(const void* p, uint64_t span, uint8_t** dev) {
    if (!zero_copy_enabled() || span == 0) return false;
    hipPointerAttribute_t a{}, b{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    const void* last = static_cast<const uint8_t*>(p) + (span - 1);
    if (hipPointerGetAttributes(&b, last) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    if (a.type != hipMemoryTypeHost || b.type != hipMemoryTypeHost || !a.devicePointer || !b.devicePointer)
        return false;
    if (static_cast<uint8_t*>(b.devicePointer) - static_cast<uint8_t*>(a.devicePointer) != int64_t(span - 1))
        return false;
    *dev = static_cast<uint8_t*>(a.devicePointer);
    return true;
}

// bytes from the first to the last byte touched by a strided batch
uint64_t batch_span(uint64_t stripe_stride, uint64_t shard_stride, uint32_t shards, uint64_t len, uint32_t stripes) {
    return uint64_t(stripes - 1) * stripe_stride + uint64_t(shards - 1) * shard_stride + len;
}

// Test hook: HEC_TEST_HOST_FAIL_AFTER_CHUNK=i fails a copy-pipeline encode
// right after queueing chunk i's kernel, so a test can check that the work
// queued before an error return has landed when the call returns
// (tests/test_gpu_host_batch.py). Read per call; -1 = off.
int forced_failure_chunk() {
    const char* v = std::getenv("HEC_TEST_HOST_FAIL_AFTER_CHUNK");
    return v && *v ? std::atoi(v) : -1;
}

uint32_t chunk_stripes(uint64_t shard_len, int n, uint32_t n_stripes) {
    uint64_t c = std::max<uint64_t>(1, kChunkBytes / (uint64_t(n) * shard_len));
    return uint32_t(std::min<uint64_t>(c, n_stripes));
}

// A chunk's present masks, normalised (& full) into dst; returns how many of
// its stripes have fewer than k shards present. wsrc (a reconstruct some):
// wdst gets the erased shards each stripe wants, and a stripe that wants none
// is not counted.
uint32_t load_masks(uint32_t* dst, const uint32_t* src, uint32_t c, uint32_t full, int k, uint32_t* wdst = nullptr,
                    const uint32_t* wsrc = nullptr) {
    uint32_t bad = 0;
    for (uint32_t s = 0; s < c; ++s) {
        dst[s] = src[s] & full;
        if (wsrc) wdst[s] = wsrc[s] & ~dst[s] & full;
        bad += __builtin_popcount(dst[s]) < k && (!wsrc || wdst[s]) ? 1u : 0u;
    }
    return bad;
}

// fn(first, count) for each run of adjacent set bits of `bits` below n, over
// the first `cap` set bits only (the run the cap falls in is cut there).
template <typename F>
int for_bit_runs(uint32_t bits, int n, int cap, F fn) {
    int used = 0;
    for (int i = 0; i < n && used < cap;) {
        if (!((bits >> i) & 1)) {
            ++i;
            continue;
        }
        int j = i;
        while (j < n && ((bits >> j) & 1) && used + (j - i) < cap) ++j;
        HEC_TRY(fn(i, j - i));
        used += j - i;
        i = j;
    }
    return HEC_OK;
}

// Pageable batches with zero copy on: chunks of C stripes go through the two
// pinned slots, coded in place there on streams[0]. pack(s0, c, q) fills slot q
// on the host, launch(c, q) queues its kernel, unpack(s0, c, q) hands the
// results back; packing chunk i+1 and unpacking chunk i-1 overlap the kernel
// of chunk i.
template <typename Pack, typename Launch, typename Unpack>
int two_slot_loop(Pipeline* p, uint32_t n_stripes, uint32_t C, Pack pack, Launch launch, Unpack unpack) {
    uint32_t prev_s0 = 0, prev_c = 0;
    int q = 0;
    for (uint32_t s0 = 0; s0 < n_stripes; s0 += C, q ^= 1) {
        const uint32_t c = std::min(C, n_stripes - s0);
        pack(s0, c, q);
        HEC_TRY(launch(c, q));
        HEC_HIP(hipEventRecord(p->hdone[q], p->streams[0]));
        if (s0 > 0) {  // the previous chunk (other slot) is done or nearly: hand it back
            HEC_HIP(hipEventSynchronize(p->hdone[q ^ 1]));
            unpack(prev_s0, prev_c, q ^ 1);
        }
        prev_s0 = s0, prev_c = c;
    }
    HEC_HIP(hipEventSynchronize(p->hdone[q ^ 1]));
    unpack(prev_s0, prev_c, q ^ 1);
    return HEC_OK;
}

// The copy pipeline: chunk `it` of C stripes runs on stream and device slot
// q = it % kDepth. in(s0, c, q) queues its H2D copies, launch(c, q, it) its
// kernel, out(s0, c, q) its D2H copies; all streams are drained at the end.
template <typename In, typename Launch, typename Out>
int copy_loop(Pipeline* p, uint32_t n_stripes, uint32_t C, In in, Launch launch, Out out) {
    for (uint32_t s0 = 0, it = 0; s0 < n_stripes; s0 += C, ++it) {
        const uint32_t c = std::min(C, n_stripes - s0);
        const int q = int(it % kDepth);
        HEC_TRY(in(s0, c, q));
        HEC_TRY(launch(c, q, it));
        HEC_TRY(out(s0, c, q));
    }
    for (auto st : p->streams) HEC_HIP(hipStreamSynchronize(st));
    return HEC_OK;
}

// One host batch over a device set (contiguous stripe ranges
// per GPU). Range r = stripes [S*r/R, S*(r+1)/R) of R = min(n_devices, S)
// ranges runs on devices[r] from its own host thread: hipSetDevice, CPUs bound
// to that GPU's NUMA node (hec_bind_thread_to_device), and the single-device
// host path, which leases its own pipeline (streams, device slots, pinned
// staging on that node). A device listed twice runs two ranges concurrently on
// two pipelines. Every range runs to its end; the call returns the status of
// the first failing range in list order (its detail prefixed with the range).
constexpr size_t kMaxDeviceRanges = 256;
int run_device_ranges(const int* devices, size_t n_devices, uint32_t n_stripes,
                      const std::function<int(uint32_t s0, uint32_t count, size_t range)>& fn) {
    if (!devices || n_devices == 0) return fail(HEC_ERR_INVALID_ARGUMENT, "empty device list");
    if (n_devices > kMaxDeviceRanges)  // one host thread per entry
        return fail(HEC_ERR_INVALID_ARGUMENT, "more than " + std::to_string(kMaxDeviceRanges) + " device entries");
    int count = 0;
    HEC_TRY(hec_device_count(&count));
    for (size_t r = 0; r < n_devices; ++r)
        if (devices[r] < 0 || devices[r] >= count)
            return fail(HEC_ERR_INVALID_ARGUMENT,
                        "device " + std::to_string(devices[r]) + " of " + std::to_string(count) + " in the list");
    if (n_stripes == 0) return HEC_OK;
    // (Each device's host worker pools bind their workers to that GPU's node,
    // so a range's staging copies run next to its pinned memory.)
    const size_t R = std::min<size_t>(n_devices, n_stripes);
    std::vector<int> rcs(R, HEC_OK);
    std::vector<std::string> details(R);
    std::vector<ErrorValues> values(R);
    std::vector<std::thread> th;
    th.reserve(R);
    try {
        for (size_t r = 0; r < R; ++r) {
            const uint32_t s0 = uint32_t(uint64_t(n_stripes) * r / R);
            const uint32_t s1 = uint32_t(uint64_t(n_stripes) * (r + 1) / R);
            th.emplace_back([&, r, s0, s1] {
                const hipError_t e = hipSetDevice(devices[r]);
                if (e != hipSuccess) {
                    rcs[r] = hip_fail(e, "hipSetDevice");
                } else {
                    (void)hec_bind_thread_to_device(devices[r], nullptr);  // placement only: no-op when unknown
                    rcs[r] = fn(s0, s1 - s0, r);
                }
                if (rcs[r]) {
                    details[r] = hec_last_error_detail();
                    values[r] = last_error_values();
                }
            });
        }
    } catch (const std::exception& ex) {  // no thread for a range: nothing escapes the C ABI
        for (size_t r = th.size(); r < R; ++r) {
            rcs[r] = HEC_ERR_OUT_OF_MEMORY;
            details[r] = std::string("no host thread for the range: ") + ex.what();
        }
    }
    for (auto& t : th) t.join();
    for (size_t r = 0; r < R; ++r)
        if (rcs[r]) {
            const uint32_t s0 = uint32_t(uint64_t(n_stripes) * r / R);
            const uint32_t s1 = uint32_t(uint64_t(n_stripes) * (r + 1) / R);
            return fail_with(rcs[r],
                             "device " + std::to_string(devices[r]) + " stripes [" + std::to_string(s0) + ", " +
                                 std::to_string(s1) + "): " + details[r],
                             values[r]);
        }
    return HEC_OK;
}

// hec_host_reconstruct_batch (h_want_masks == nullptr: every erased shard,
// today's launches) and hec_host_reconstruct_some_batch: one body. With want
// words a stripe takes part only where it wants an erased shard, and only the
// wanted shards are computed, stored and brought back.
int host_reconstruct(const hec_rs_t* rs, uint8_t* h_shards, uint64_t stripe_stride, uint64_t shard_stride,
                     uint64_t shard_len, uint32_t n_stripes, const uint32_t* h_present_masks,
                     const uint32_t* h_want_masks, uint32_t* n_bad_stripes);

}  // namespace
}  // namespace hec

using namespace hec;

extern "C" {

int hec_host_encode_batch(const hec_rs_t* rs, const uint8_t* h_data, uint64_t data_stripe_stride,
                          uint64_t data_shard_stride, uint8_t* h_parity, uint64_t parity_stripe_stride,
                          uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes) {
    HEC_TRY(check_batch_args(rs, h_data, h_parity, shard_len));
    if (n_stripes == 0) return HEC_OK;
    HEC_TRY(check_encode_strides(rs, Batch::split(arena(h_data, data_stripe_stride, data_shard_stride),
                                                  arena(h_parity, parity_stripe_stride, parity_shard_stride),
                                                  shard_len, n_stripes)));
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    Lease<Pipeline> p;
    HEC_TRY(lease_slot(p));
    const int k = rs->k, m = rs->m;
    uint8_t *zd, *zp;
    if (host_device_view(h_data, batch_span(data_stripe_stride, data_shard_stride, k, shard_len, n_stripes), &zd) &&
        host_device_view(h_parity, batch_span(parity_stripe_stride, parity_shard_stride, m, shard_len, n_stripes),
                         &zp)) {
        HEC_TRY(p->reserve(0, 1));
        HEC_TRY(run_apply(gd->encode, uint32_t(k),
                          Batch::split(arena(zd, data_stripe_stride, data_shard_stride),
                                       arena(zp, parity_stripe_stride, parity_shard_stride), shard_len, n_stripes),
                          nullptr, nullptr, p->streams[0], nullptr, /*over_pcie=*/true));
        HEC_HIP(hipStreamSynchronize(p->streams[0]));
        return HEC_OK;
    }
    const uint64_t Lp = round_up(shard_len, 256);  // device shard pitch
    // len rounded to 16: the pad bytes of the pitch are computed but never copied back
    const uint64_t L16 = round_up(shard_len, 16);
    const uint32_t C = chunk_stripes(Lp, rs->n, n_stripes);
    const uint64_t dstripe = uint64_t(rs->n) * Lp;
    if (zero_copy_enabled()) {
        // Pageable memory: chunks are copied into two pinned slots on the host
        // pool and coded in place by the zero-copy kernel.
        HEC_TRY(p->reserve(0, 1));
        HEC_TRY(p->reserve_host(size_t(C) * dstripe));
        uint8_t* zs[2] = {pinned_device_ptr(p->hslot[0]), pinned_device_ptr(p->hslot[1])};
        if (zs[0] && zs[1])
            return two_slot_loop(
                p.sc, n_stripes, C,
                [&](uint32_t s0, uint32_t c, int q) {
                    uint8_t* h = p->hslot[q];
                    parallel_for(size_t(c) * k, uint64_t(c) * k * shard_len, [&](size_t t) {
                        const uint32_t s = uint32_t(t / k);
                        const int i = int(t % k);
                        std::memcpy(h + s * dstripe + uint64_t(i) * Lp,
                                    h_data + (s0 + s) * data_stripe_stride + i * data_shard_stride, shard_len);
                    });
                },
                [&](uint32_t c, int q) {
                    return run_apply(gd->encode, uint32_t(k), Batch::split_at(arena(zs[q], dstripe, Lp), k, L16, c),
                                     nullptr, nullptr, p->streams[0], nullptr, /*over_pcie=*/true);
                },
                [&](uint32_t s0, uint32_t c, int q) {
                    parallel_for(size_t(c) * m, uint64_t(c) * m * shard_len, [&](size_t t) {
                        const uint32_t s = uint32_t(t / m);
                        const int j = int(t % m);
                        std::memcpy(h_parity + (s0 + s) * parity_stripe_stride + j * parity_shard_stride,
                                    p->hslot[q] + s * dstripe + uint64_t(k + j) * Lp, shard_len);
                    });
                });
    }
    HEC_TRY(p->reserve(size_t(C) * rs->n * Lp, 1));
    const int fail_at = forced_failure_chunk();
    return copy_loop(
        p.sc, n_stripes, C,
        [&](uint32_t s0, uint32_t c, int q) -> int {
            for (uint32_t s = 0; s < c; ++s)  // data shards of stripe s -> [s][0..k)
                HEC_HIP(copy2d(p->slot[q] + s * dstripe, Lp, h_data + (s0 + s) * data_stripe_stride,
                               data_shard_stride, shard_len, uint64_t(k), hipMemcpyHostToDevice, p->streams[q]));
            return HEC_OK;
        },
        [&](uint32_t c, int q, uint32_t it) -> int {
            HEC_TRY(run_apply(gd->encode, uint32_t(k), Batch::split_at(arena(p->slot[q], dstripe, Lp), k, L16, c),
                              nullptr, nullptr, p->streams[q]));
            if (int(it) == fail_at) return fail(HEC_ERR_HIP, "test hook: failure after chunk " + std::to_string(it));
            return HEC_OK;
        },
        [&](uint32_t s0, uint32_t c, int q) -> int {
            for (uint32_t s = 0; s < c; ++s)
                HEC_HIP(copy2d(h_parity + (s0 + s) * parity_stripe_stride, parity_shard_stride,
                               p->slot[q] + s * dstripe + uint64_t(k) * Lp, Lp, shard_len, uint64_t(m),
                               hipMemcpyDeviceToHost, p->streams[q]));
            return HEC_OK;
        });
}

int hec_host_reconstruct_batch(const hec_rs_t* rs, uint8_t* h_shards, uint64_t stripe_stride, uint64_t shard_stride,
                               uint64_t shard_len, uint32_t n_stripes, const uint32_t* h_present_masks,
                               uint32_t* n_bad_stripes) {
    HEC_TRY(check_batch_args(rs, h_shards, h_present_masks, shard_len));
    if (n_bad_stripes) *n_bad_stripes = 0;
    if (n_stripes == 0) return HEC_OK;
    HEC_TRY(check_strided("shards", uint32_t(rs->n), arena(h_shards, stripe_stride, shard_stride), shard_len,
                          n_stripes));
    return host_reconstruct(rs, h_shards, stripe_stride, shard_stride, shard_len, n_stripes, h_present_masks, nullptr,
                            n_bad_stripes);
}

int hec_host_reconstruct_some_batch(const hec_rs_t* rs, uint8_t* h_shards, uint64_t stripe_stride,
                                    uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                    const uint32_t* h_present_masks, const uint32_t* h_want_masks,
                                    uint32_t* n_bad_stripes) {
    HEC_TRY(check_some_args(rs, Batch::in_place(arena(h_shards, stripe_stride, shard_stride), shard_len, n_stripes),
                            h_present_masks, h_want_masks));
    if (n_bad_stripes) *n_bad_stripes = 0;
    if (n_stripes == 0) return HEC_OK;
    return host_reconstruct(rs, h_shards, stripe_stride, shard_stride, shard_len, n_stripes, h_present_masks,
                            h_want_masks, n_bad_stripes);
}

}  // extern "C"

namespace hec {
namespace {

int host_reconstruct(const hec_rs_t* rs, uint8_t* h_shards, uint64_t stripe_stride, uint64_t shard_stride,
                     uint64_t shard_len, uint32_t n_stripes, const uint32_t* h_present_masks,
                     const uint32_t* h_want_masks, uint32_t* n_bad_stripes) {
    const uint32_t* const wants = h_want_masks;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    Lease<Pipeline> p;
    HEC_TRY(lease_slot(p));
    const int k = rs->k, n = rs->n;
    const uint32_t full = n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1);
    uint32_t bad = 0;
    // the erased shards stripe s of slot q's chunk rebuilds (0: it takes no part)
    auto wanted = [&](int q, uint32_t s) { return wants ? p->want_host[q][s] : ~p->mask_host[q][s] & full; };
    uint8_t* zs;
    if (host_device_view(h_shards, batch_span(stripe_stride, shard_stride, n, shard_len, n_stripes), &zs)) {
        // masks to the device (the caller's array may be pageable), then one
        // decode over the pinned host shards in place
        HEC_TRY(p->reserve(0, n_stripes));
        if (wants) HEC_TRY(p->reserve_wants(n_stripes));
        HEC_TRY(ensure_dense_decode(rs, gd, p->streams[0]));
        bad = load_masks(p->mask_host[0], h_present_masks, n_stripes, full, k, p->want_host[0], wants);
        HEC_HIP(hipMemcpyAsync(p->mask_dev[0], p->mask_host[0], size_t(n_stripes) * 4, hipMemcpyHostToDevice,
                               p->streams[0]));
        if (wants)
            HEC_HIP(hipMemcpyAsync(p->want_dev[0], p->want_host[0], size_t(n_stripes) * 4, hipMemcpyHostToDevice,
                                   p->streams[0]));
        HEC_TRY(run_some(gd->decode_dense, uint32_t(k),
                         Batch::in_place(arena(zs, stripe_stride, shard_stride), shard_len, n_stripes), p->mask_dev[0],
                         wants ? p->want_dev[0].p : nullptr, nullptr, p->streams[0]));
        HEC_HIP(hipStreamSynchronize(p->streams[0]));
        if (n_bad_stripes) *n_bad_stripes = bad;
        return HEC_OK;
    }
    const uint64_t Lp = round_up(shard_len, 256), L16 = round_up(shard_len, 16);
    const uint32_t C = chunk_stripes(Lp, n, n_stripes);
    const uint64_t dstripe = uint64_t(n) * Lp;
    auto host_shard = [&](uint32_t s, int i) { return h_shards + s * stripe_stride + uint64_t(i) * shard_stride; };
    auto finish = [&](int rc) {
        if (!rc && n_bad_stripes) *n_bad_stripes = bad;
        return rc;
    };
    if (zero_copy_enabled()) {
        // Pageable memory: the first k present shards of each stripe are copied
        // into two pinned slots on the host pool, decoded in place there by the
        // zero-copy kernel, and only the erased shards are copied back.
        HEC_TRY(p->reserve(0, C));
        if (wants) HEC_TRY(p->reserve_wants(C));
        HEC_TRY(p->reserve_host(size_t(C) * dstripe));
        HEC_TRY(ensure_dense_decode(rs, gd, p->streams[0]));
        uint8_t* hz[2] = {pinned_device_ptr(p->hslot[0]), pinned_device_ptr(p->hslot[1])};
        uint32_t* zm[2] = {reinterpret_cast<uint32_t*>(pinned_device_ptr(p->mask_host[0])),
                           reinterpret_cast<uint32_t*>(pinned_device_ptr(p->mask_host[1]))};
        uint32_t* zw[2] = {nullptr, nullptr};
        if (wants)
            for (int q = 0; q < 2; ++q) zw[q] = reinterpret_cast<uint32_t*>(pinned_device_ptr(p->want_host[q]));
        if (hz[0] && hz[1] && zm[0] && zm[1] && (!wants || (zw[0] && zw[1])))
            return finish(two_slot_loop(
                p.sc, n_stripes, C,
                [&](uint32_t s0, uint32_t c, int q) {
                    bad += load_masks(p->mask_host[q], h_present_masks + s0, c, full, k, p->want_host[q],
                                      wants ? wants + s0 : nullptr);
                    parallel_for(size_t(c) * n, uint64_t(c) * k * shard_len, [&](size_t t) {
                        const uint32_t s = uint32_t(t / n);
                        const int i = int(t % n);
                        const uint32_t mask = p->mask_host[q][s];
                        if (__builtin_popcount(mask) < k || !wanted(q, s) || !((mask >> i) & 1)) return;
                        if (__builtin_popcount(mask & ((1u << i) - 1)) >= k) return;  // only the first k present
                        std::memcpy(p->hslot[q] + s * dstripe + uint64_t(i) * Lp, host_shard(s0 + s, i), shard_len);
                    });
                },
                [&](uint32_t c, int q) {
                    return run_some(gd->decode_dense, uint32_t(k), Batch::in_place(arena(hz[q], dstripe, Lp), L16, c),
                                    zm[q], zw[q], nullptr, p->streams[0]);
                },
                [&](uint32_t s0, uint32_t c, int q) {
                    parallel_for(size_t(c) * n, uint64_t(c) * 4 * shard_len, [&](size_t t) {
                        const uint32_t s = uint32_t(t / n);
                        const int i = int(t % n);
                        const uint32_t mask = p->mask_host[q][s];
                        if (__builtin_popcount(mask) < k || !((wanted(q, s) >> i) & 1)) return;
                        std::memcpy(host_shard(s0 + s, i), p->hslot[q] + s * dstripe + uint64_t(i) * Lp, shard_len);
                    });
                }));
    }
    HEC_TRY(p->reserve(size_t(C) * n * Lp, C));
    if (wants) HEC_TRY(p->reserve_wants(C));
    HEC_TRY(ensure_dense_decode(rs, gd, p->streams[0]));
    auto dev_shard = [&](int q, uint32_t s, int i) { return p->slot[q] + s * dstripe + uint64_t(i) * Lp; };
    return finish(copy_loop(
        p.sc, n_stripes, C,
        [&](uint32_t s0, uint32_t c, int q) -> int {
            // the staging of this slot was last read by the copy issued kDepth chunks ago
            HEC_HIP(hipStreamSynchronize(p->streams[q]));
            bad += load_masks(p->mask_host[q], h_present_masks + s0, c, full, k, p->want_host[q],
                              wants ? wants + s0 : nullptr);
            for (uint32_t s = 0; s < c; ++s) {
                const uint32_t mask = p->mask_host[q][s];
                if (__builtin_popcount(mask) < k || !wanted(q, s)) continue;
                // H2D only the first k present shards (the ones the decode reads),
                // merged into runs of adjacent shard ids
                HEC_TRY(for_bit_runs(mask, n, k, [&](int i, int count) -> int {
                    HEC_HIP(copy2d(dev_shard(q, s, i), Lp, host_shard(s0 + s, i), shard_stride, shard_len,
                                   uint64_t(count), hipMemcpyHostToDevice, p->streams[q]));
                    return HEC_OK;
                }));
            }
            HEC_HIP(hipMemcpyAsync(p->mask_dev[q], p->mask_host[q], c * 4, hipMemcpyHostToDevice, p->streams[q]));
            if (wants)
                HEC_HIP(hipMemcpyAsync(p->want_dev[q], p->want_host[q], c * 4, hipMemcpyHostToDevice, p->streams[q]));
            return HEC_OK;
        },
        [&](uint32_t c, int q, uint32_t) {
            return run_some(gd->decode_dense, uint32_t(k), Batch::in_place(arena(p->slot[q], dstripe, Lp), L16, c),
                            p->mask_dev[q], wants ? p->want_dev[q].p : nullptr, nullptr, p->streams[q]);
        },
        [&](uint32_t s0, uint32_t c, int q) -> int {
            for (uint32_t s = 0; s < c; ++s) {
                const uint32_t mask = p->mask_host[q][s];
                if (__builtin_popcount(mask) < k) continue;
                // D2H the erased shards that were rebuilt, merged into runs
                HEC_TRY(for_bit_runs(wanted(q, s), n, n, [&](int i, int count) -> int {
                    HEC_HIP(copy2d(host_shard(s0 + s, i), shard_stride, dev_shard(q, s, i), Lp, shard_len,
                                   uint64_t(count), hipMemcpyDeviceToHost, p->streams[q]));
                    return HEC_OK;
                }));
            }
            return HEC_OK;
        }));
}

}  // namespace
}  // namespace hec

extern "C" {

int hec_host_verify_batch(const hec_rs_t* rs, const uint8_t* h_data, uint64_t data_stripe_stride,
                          uint64_t data_shard_stride, const uint8_t* h_parity, uint64_t parity_stripe_stride,
                          uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes, uint32_t* h_mismatch,
                          uint32_t* n_bad_stripes) {
    HEC_TRY(check_batch_args(rs, h_data, h_parity, shard_len));
    HEC_TRY(check_verify_args(rs, h_mismatch));
    if (n_bad_stripes) *n_bad_stripes = 0;
    if (n_stripes == 0) return HEC_OK;
    HEC_TRY(check_encode_strides(rs, Batch::split(arena(h_data, data_stripe_stride, data_shard_stride),
                                                  arena(h_parity, parity_stripe_stride, parity_shard_stride),
                                                  shard_len, n_stripes)));
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    Lease<Pipeline> p;
    HEC_TRY(lease_slot(p));
    const int k = rs->k, m = rs->m, n = rs->n;
    // one verify launch into slot q's words: no count
    auto verify = [&](const Batch& b, int q, hipStream_t s) {
        ScrubOut out;
        out.words = p->mask_dev[q];
        return run_scrub(*gd, b, ScrubSpec{}, out, s);
    };
    auto finish = [&](int rc) {
        if (!rc && n_bad_stripes)
            for (uint32_t s = 0; s < n_stripes; ++s) *n_bad_stripes += h_mismatch[s] ? 1u : 0u;
        return rc;
    };
    // The result words always live in device memory (the pipeline's mask
    // words): the kernels' atomics stay on the device, and only the words
    // cross PCIe back. Every launch gets the true shard_len, never a length
    // rounded up to the staging pitch: the pad bytes of a reused slot hold
    // garbage, and a verify compares what an encode merely overwrites.
    uint8_t *zd, *zp;
    if (host_device_view(h_data, batch_span(data_stripe_stride, data_shard_stride, k, shard_len, n_stripes), &zd) &&
        host_device_view(h_parity, batch_span(parity_stripe_stride, parity_shard_stride, m, shard_len, n_stripes),
                         &zp)) {
        HEC_TRY(p->reserve(0, n_stripes));
        HEC_TRY(verify(Batch::split(arena(zd, data_stripe_stride, data_shard_stride),
                                    arena(zp, parity_stripe_stride, parity_shard_stride), shard_len, n_stripes),
                       0, p->streams[0]));
        HEC_HIP(hipMemcpyAsync(p->mask_host[0], p->mask_dev[0], size_t(n_stripes) * 4, hipMemcpyDeviceToHost,
                               p->streams[0]));
        HEC_HIP(hipStreamSynchronize(p->streams[0]));
        std::memcpy(h_mismatch, p->mask_host[0], size_t(n_stripes) * 4);
        return finish(HEC_OK);
    }
    const uint64_t Lp = round_up(shard_len, 256);  // staging shard pitch
    const uint32_t C = chunk_stripes(Lp, n, n_stripes);
    const uint64_t dstripe = uint64_t(n) * Lp;
    auto host_shard = [&](uint32_t s, int i) {
        return i < k ? h_data + s * data_stripe_stride + uint64_t(i) * data_shard_stride
                     : h_parity + s * parity_stripe_stride + uint64_t(i - k) * parity_shard_stride;
    };
    if (zero_copy_enabled()) {
        // Pageable memory: all 14 shards of a chunk are packed into a pinned
        // slot the kernel reads over PCIe; nothing but the words comes back.
        HEC_TRY(p->reserve(0, C));
        HEC_TRY(p->reserve_host(size_t(C) * dstripe));
        uint8_t* zs[2] = {pinned_device_ptr(p->hslot[0]), pinned_device_ptr(p->hslot[1])};
        if (zs[0] && zs[1])
            return finish(two_slot_loop(
                p.sc, n_stripes, C,
                [&](uint32_t s0, uint32_t c, int q) {
                    uint8_t* h = p->hslot[q];
                    parallel_for(size_t(c) * n, uint64_t(c) * n * shard_len, [&](size_t t) {
                        const uint32_t s = uint32_t(t / n);
                        const int i = int(t % n);
                        std::memcpy(h + s * dstripe + uint64_t(i) * Lp, host_shard(s0 + s, i), shard_len);
                    });
                },
                [&](uint32_t c, int q) -> int {
                    HEC_TRY(verify(Batch::split_at(arena(zs[q], dstripe, Lp), k, shard_len, c), q, p->streams[0]));
                    HEC_HIP(hipMemcpyAsync(p->mask_host[q], p->mask_dev[q], size_t(c) * 4, hipMemcpyDeviceToHost,
                                           p->streams[0]));
                    return HEC_OK;
                },
                [&](uint32_t s0, uint32_t c, int q) {
                    std::memcpy(h_mismatch + s0, p->mask_host[q], size_t(c) * 4);
                }));
    }
    HEC_TRY(p->reserve(size_t(C) * dstripe, C));
    return finish(copy_loop(
        p.sc, n_stripes, C,
        [&](uint32_t s0, uint32_t c, int q) -> int {
            for (uint32_t s = 0; s < c; ++s) {  // 14-shard H2D: data then parity of stripe s -> [s][0..n)
                HEC_HIP(copy2d(p->slot[q] + s * dstripe, Lp, host_shard(s0 + s, 0), data_shard_stride, shard_len,
                               uint64_t(k), hipMemcpyHostToDevice, p->streams[q]));
                HEC_HIP(copy2d(p->slot[q] + s * dstripe + uint64_t(k) * Lp, Lp, host_shard(s0 + s, k),
                               parity_shard_stride, shard_len, uint64_t(m), hipMemcpyHostToDevice, p->streams[q]));
            }
            return HEC_OK;
        },
        [&](uint32_t c, int q, uint32_t) {
            return verify(Batch::split_at(arena(p->slot[q], dstripe, Lp), k, shard_len, c), q, p->streams[q]);
        },
        [&](uint32_t s0, uint32_t c, int q) -> int {  // D2H of the words only
            HEC_HIP(hipMemcpyAsync(h_mismatch + s0, p->mask_dev[q], size_t(c) * 4, hipMemcpyDeviceToHost,
                                   p->streams[q]));
            return HEC_OK;
        }));
}

int hec_host_encode_batch_multi(const hec_rs_t* rs, const int* devices, size_t n_devices, const uint8_t* h_data,
                                uint64_t data_stripe_stride, uint64_t data_shard_stride, uint8_t* h_parity,
                                uint64_t parity_stripe_stride, uint64_t parity_shard_stride, uint64_t shard_len,
                                uint32_t n_stripes) {
    HEC_TRY(check_batch_args(rs, h_data, h_parity, shard_len));
    HEC_TRY(check_encode_strides(rs, Batch::split(arena(h_data, data_stripe_stride, data_shard_stride),
                                                  arena(h_parity, parity_stripe_stride, parity_shard_stride),
                                                  shard_len, n_stripes)));
    return run_device_ranges(devices, n_devices, n_stripes, [&](uint32_t s0, uint32_t c, size_t) {
        return hec_host_encode_batch(rs, h_data + s0 * data_stripe_stride, data_stripe_stride, data_shard_stride,
                                     h_parity + s0 * parity_stripe_stride, parity_stripe_stride, parity_shard_stride,
                                     shard_len, c);
    });
}

int hec_host_reconstruct_batch_multi(const hec_rs_t* rs, const int* devices, size_t n_devices, uint8_t* h_shards,
                                     uint64_t stripe_stride, uint64_t shard_stride, uint64_t shard_len,
                                     uint32_t n_stripes, const uint32_t* h_present_masks, uint32_t* n_bad_stripes) {
    HEC_TRY(check_batch_args(rs, h_shards, h_present_masks, shard_len));
    if (n_bad_stripes) *n_bad_stripes = 0;
    HEC_TRY(check_strided("shards", uint32_t(rs->n), arena(h_shards, stripe_stride, shard_stride), shard_len,
                          n_stripes));
    std::vector<uint32_t> bad(std::max<size_t>(n_devices, 1), 0);
    int rc = run_device_ranges(devices, n_devices, n_stripes, [&](uint32_t s0, uint32_t c, size_t r) {
        return hec_host_reconstruct_batch(rs, h_shards + s0 * stripe_stride, stripe_stride, shard_stride, shard_len, c,
                                          h_present_masks + s0, &bad[r]);
    });
    if (rc) return rc;
    if (n_bad_stripes)
        for (uint32_t b : bad) *n_bad_stripes += b;
    return HEC_OK;
}

int hec_host_zero_copy_view(const void* p, uint64_t bytes, int* zero_copy) {
    if (!zero_copy) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    *zero_copy = 0;
    if (!p || bytes == 0) return HEC_OK;
    int dev;
    int rc = current_device(&dev);
    if (rc) return rc;
    uint8_t* d = nullptr;
    *zero_copy = host_device_view(p, bytes, &d) ? 1 : 0;
    return HEC_OK;
}

int hec_host_staging_stats(int* n_pipelines, uint64_t* pinned_bytes, uint64_t* device_bytes) {
    int dev;
    int rc = current_device(&dev);
    if (rc) return rc;
    SlotPool<Pipeline>* pool = per_device<SlotPool<Pipeline>>(dev, /*create=*/false);
    int n = 0;
    uint64_t pinned = 0, devb = 0;
    if (pool) {
        // Slots are never removed from a pool, so their addresses stay valid;
        // the pool mutex is held only to copy them, never while waiting on a
        // slot (that would stall every lease on the device behind one call).
        std::vector<Pipeline*> slots;
        {
            std::lock_guard<std::mutex> g(pool->mu);
            for (auto& sl : pool->slots) slots.push_back(sl.get());
        }
        for (Pipeline* sl : slots) {
            std::lock_guard<std::mutex> l(sl->mu);  // waits for a call in flight on it
            ++n;
            pinned += sl->pinned_bytes();
            devb += sl->device_bytes();
        }
    }
    if (n_pipelines) *n_pipelines = n;
    if (pinned_bytes) *pinned_bytes = pinned;
    if (device_bytes) *device_bytes = devb;
    return HEC_OK;
}

int hec_set_host_zero_copy(int on) {
    zero_copy_enabled() = on != 0;
    return HEC_OK;
}

#ifdef HEC_TEST_HOST_CHUNKS
// Test builds only (host_chunks.hpp): the chunk sizes this library was
// compiled with, so a test can prove that the variant it loaded is the one it
// meant. The shipped library does not export this.
void hec_test_host_chunk_limits(uint64_t* chunk_bytes, uint64_t* chunk_cols, uint64_t* read_piece) {
    *chunk_bytes = hec::kChunkBytes;
    *chunk_cols = hec::kChunkCols;
    *read_piece = hec::kReadPiece;
}
#endif

}  // extern "C"
