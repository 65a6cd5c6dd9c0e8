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

// Test hook: HEC_TEST_HOST_FAIL_AFTER_CHUNK=i fails a host batch on the copy
// pipeline (any operation: the hook sits in run_host_op's one loop) right
// after queueing chunk i's kernel, so a test can check that the work queued
// before an error return has landed when the call returns
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

// fn(first, count) for each run of adjacent i in [lo, hi) with on(i); no run
// crosses `cut`.
template <typename On, typename F>
int for_runs(int lo, int hi, int cut, On on, F fn) {
    for (int i = lo; i < hi;) {
        if (!on(i)) {
            ++i;
            continue;
        }
        int j = i + 1;
        while (j < hi && j != cut && on(j)) ++j;
        HEC_TRY(fn(i, j - i));
        i = j;
    }
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

// The shards of a stripe that move one way: those i of [lo, hi) the operation
// names for that stripe (HostOp::goes_in / comes_back). About `typical` of
// them do: the byte hint the host pool splits a pack or an unpack by.
struct ShardRange {
    int lo = 0, hi = 0, typical = 0;
};

// What a host batch operation states; run_host_op carries it down whichever
// staging path the caller's memory takes.
struct HostOp {
    const hec_rs_t* rs = nullptr;
    GeomDevice* gd = nullptr;  // rs on the current device (run_host_op sets it)
    // The caller's memory, as the Batch a launch over it would get. Shards
    // [0, split) of a stripe lie in host.in and [split, n) in host.out, each
    // arena with its own strides; split == 0: one in-place arena holds all n.
    Batch host;
    int split = 0;
    ShardRange in, out;  // staged in before the launch, brought back after it
    // Per-stripe words. masks: present masks in, with wants the want masks too;
    // goes_in, comes_back and the launch see both as load_masks normalised
    // them. words: one result word per stripe out.
    const uint32_t* masks = nullptr;
    const uint32_t* wants = nullptr;
    uint32_t* words = nullptr;
    // A launch over a staging slot gets the length rounded up to 16 (the pad
    // bytes of the pitch are computed but never copied back), or with true_len
    // the length itself.
    bool true_len = false;
    uint32_t* n_bad_stripes = nullptr;

    const Strided& arena_of(int i) const { return i < split ? host.in : host.out; }
    uint8_t* shard(uint32_t s, int i) const {  // host address of shard i of stripe s
        const Strided& a = arena_of(i);
        return a.base + s * a.stripe + uint64_t(i < split ? i : i - split) * a.shard;
    }
    // Whether shard i of a stripe with these words is staged in / brought back.
    virtual bool goes_in(uint32_t /*mask*/, uint32_t /*want*/, int /*i*/) const { return true; }
    virtual bool comes_back(uint32_t /*mask*/, uint32_t /*want*/, int /*i*/) const { return true; }
    // Once per call, before the first launch (plans the launch needs).
    virtual int prepare(hipStream_t) { return HEC_OK; }
    // Queue the kernels over b on s. words: b's per-stripe words in device
    // memory (the masks in, or the result words out); wants likewise, or null.
    virtual int launch(const Batch& b, uint32_t* words, const uint32_t* wants, hipStream_t s, bool over_pcie) = 0;
    // The last chunk is home. bad: what load_masks counted over the call.
    virtual void done(uint32_t /*bad*/) {}
    virtual ~HostOp() = default;
};

// One host batch, down one of three staging paths:
//  1. direct view: the caller's arenas are pinned, GPU-addressable ranges
//     (host_device_view): one launch runs over them in place;
//  2. pageable memory with zero copy on: chunks of C stripes are packed on the
//     host pool into the two pinned slots, coded in place there over PCIe on
//     streams[0] and unpacked; packing chunk i+1 and unpacking chunk i-1
//     overlap the kernel of chunk i;
//  3. the copy pipeline: chunk `it` runs H2D, kernel and D2H on stream and
//     device slot it % kDepth; all streams are drained at the end.
// A slot holds C stripes of n shards at pitch Lp: shard i of its stripe s is at
// slot + s * n * Lp + i * Lp.
int run_host_op(HostOp& op) {
    const hec_rs_t* rs = op.rs;
    HEC_TRY(geom_device(rs, &op.gd));
    Lease<Pipeline> p;
    HEC_TRY(lease_slot(p));
    const int k = rs->k, n = rs->n;
    const uint64_t len = op.host.len;
    const uint32_t S = op.host.n_stripes;
    const uint32_t full = n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1);
    uint32_t bad = 0;

    // slots of slot_bytes and `count` words a slot
    auto reserve = [&](size_t slot_bytes, uint32_t count) -> int {
        HEC_TRY(p->reserve(slot_bytes, op.masks || op.words ? count : 1));
        return op.wants ? p->reserve_wants(count) : HEC_OK;
    };
    // the masks of stripes [s0, s0 + c) into slot q's host words, and on to the device on streams[q]
    auto load_words = [&](int q, uint32_t s0, uint32_t c) {
        if (op.masks)
            bad += load_masks(p->mask_host[q], op.masks + s0, c, full, k, p->want_host[q],
                              op.wants ? op.wants + s0 : nullptr);
    };
    auto send_words = [&](int q, uint32_t c) -> int {
        if (!op.masks) return HEC_OK;
        HEC_HIP(hipMemcpyAsync(p->mask_dev[q], p->mask_host[q], size_t(c) * 4, hipMemcpyHostToDevice, p->streams[q]));
        if (op.wants)
            HEC_HIP(hipMemcpyAsync(p->want_dev[q], p->want_host[q], size_t(c) * 4, hipMemcpyHostToDevice,
                                   p->streams[q]));
        return HEC_OK;
    };
    // whether shard i of stripe s of slot q's chunk moves in (or back)
    auto moves = [&](bool in, int q, uint32_t s, int i) {
        uint32_t mask = full, want = 0;
        if (op.masks) {
            mask = p->mask_host[q][s];
            want = op.wants ? p->want_host[q][s] : ~mask & full;
        }
        return in ? op.goes_in(mask, want, i) : op.comes_back(mask, want, i);
    };

    // 1. direct view
    auto view = [&](const Strided& a, int shards, uint8_t** dev) {
        return host_device_view(a.base, batch_span(a.stripe, a.shard, uint32_t(shards), len, S), dev);
    };
    uint8_t *zin, *zout;
    if (view(op.host.in, op.split ? op.split : n, &zin) &&
        (op.split ? view(op.host.out, n - op.split, &zout) : (zout = zin, true))) {
        HEC_TRY(reserve(0, S));
        HEC_TRY(op.prepare(p->streams[0]));
        load_words(0, 0, S);  // to the device: the caller's array may be pageable
        HEC_TRY(send_words(0, S));
        HEC_TRY(op.launch(Batch{arena(zin, op.host.in.stripe, op.host.in.shard),
                                arena(zout, op.host.out.stripe, op.host.out.shard), len, S},
                          p->mask_dev[0], op.wants ? p->want_dev[0].p : nullptr, p->streams[0], /*over_pcie=*/true));
        if (op.words)
            HEC_HIP(hipMemcpyAsync(p->mask_host[0], p->mask_dev[0], size_t(S) * 4, hipMemcpyDeviceToHost,
                                   p->streams[0]));
        HEC_HIP(hipStreamSynchronize(p->streams[0]));
        if (op.words) std::memcpy(op.words, p->mask_host[0], size_t(S) * 4);
        op.done(bad);
        return HEC_OK;
    }

    const uint64_t Lp = round_up(len, 256);  // staging shard pitch
    const uint64_t dstripe = uint64_t(n) * Lp;
    const uint32_t C = chunk_stripes(Lp, n, S);
    auto at = [&](uint8_t* slot, uint32_t s, int i) { return slot + s * dstripe + uint64_t(i) * Lp; };
    auto slot_batch = [&](uint8_t* slot, uint32_t c) {
        const Strided a = arena(slot, dstripe, Lp);
        return Batch{a, a.from(uint64_t(op.split)), op.true_len ? len : round_up(len, 16), c};
    };

    // 2. pageable memory through the two pinned slots
    if (zero_copy_enabled()) {
        HEC_TRY(reserve(0, C));
        HEC_TRY(p->reserve_host(size_t(C) * dstripe));
        HEC_TRY(op.prepare(p->streams[0]));
        uint8_t* zs[2];
        uint32_t *zm[2] = {}, *zw[2] = {};
        for (int q = 0; q < 2; ++q) zs[q] = pinned_device_ptr(p->hslot[q]);
        if (op.masks)
            for (int q = 0; q < 2; ++q) zm[q] = reinterpret_cast<uint32_t*>(pinned_device_ptr(p->mask_host[q]));
        if (op.wants)
            for (int q = 0; q < 2; ++q) zw[q] = reinterpret_cast<uint32_t*>(pinned_device_ptr(p->want_host[q]));
        // a slot the device cannot address: the copy pipeline instead
        if (zs[0] && zs[1] && (!op.masks || (zm[0] && zm[1])) && (!op.wants || (zw[0] && zw[1]))) {
            auto host_copy = [&](bool in, uint32_t s0, uint32_t c, int q) {
                const ShardRange& r = in ? op.in : op.out;
                const size_t w = size_t(r.hi - r.lo);
                if (!w) return;
                parallel_for(size_t(c) * w, uint64_t(c) * r.typical * len, [&](size_t t) {
                    const uint32_t s = uint32_t(t / w);
                    const int i = r.lo + int(t % w);
                    if (!moves(in, q, s, i)) return;
                    uint8_t *h = op.shard(s0 + s, i), *z = at(p->hslot[q], s, i);
                    std::memcpy(in ? z : h, in ? h : z, len);
                });
            };
            auto unpack = [&](uint32_t s0, uint32_t c, int q) {
                host_copy(false, s0, c, q);
                if (op.words) std::memcpy(op.words + s0, p->mask_host[q], size_t(c) * 4);
            };
            uint32_t prev_s0 = 0, prev_c = 0;
            int q = 0;
            for (uint32_t s0 = 0; s0 < S; s0 += C, q ^= 1) {
                const uint32_t c = std::min(C, S - s0);
                load_words(q, s0, c);  // the kernel reads them where they are
                host_copy(true, s0, c, q);
                HEC_TRY(op.launch(slot_batch(zs[q], c), op.masks ? zm[q] : p->mask_dev[q].p, zw[q], p->streams[0],
                                  /*over_pcie=*/true));
                if (op.words)
                    HEC_HIP(hipMemcpyAsync(p->mask_host[q], p->mask_dev[q], size_t(c) * 4, hipMemcpyDeviceToHost,
                                           p->streams[0]));
                HEC_HIP(hipEventRecord(p->hdone[q], p->streams[0]));
                if (s0 > 0) {  // the previous chunk (other slot) is done or nearly: hand it back
                    HEC_HIP(hipEventSynchronize(p->hdone[q ^ 1]));
                    unpack(prev_s0, prev_c, q ^ 1);
                }
                prev_s0 = s0, prev_c = c;
            }
            HEC_HIP(hipEventSynchronize(p->hdone[q ^ 1]));
            unpack(prev_s0, prev_c, q ^ 1);
            op.done(bad);
            return HEC_OK;
        }
    }

    // 3. the copy pipeline
    HEC_TRY(reserve(size_t(C) * dstripe, C));
    HEC_TRY(op.prepare(p->streams[0]));
    // one copy2d per run of adjacent moving shards of a stripe that lie in one host arena
    auto dma = [&](bool in, uint32_t s0, uint32_t c, int q) -> int {
        const ShardRange& r = in ? op.in : op.out;
        for (uint32_t s = 0; s < c; ++s)
            HEC_TRY(for_runs(
                r.lo, r.hi, op.split, [&](int i) { return moves(in, q, s, i); },
                [&](int i, int count) -> int {
                    uint8_t *h = op.shard(s0 + s, i), *d = at(p->slot[q], s, i);
                    const uint64_t hpitch = op.arena_of(i).shard;
                    HEC_HIP(in ? copy2d(d, Lp, h, hpitch, len, uint64_t(count), hipMemcpyHostToDevice, p->streams[q])
                               : copy2d(h, hpitch, d, Lp, len, uint64_t(count), hipMemcpyDeviceToHost, p->streams[q]));
                    return HEC_OK;
                }));
        return HEC_OK;
    };
    const int fail_at = forced_failure_chunk();
    for (uint32_t s0 = 0, it = 0; s0 < S; s0 += C, ++it) {
        const uint32_t c = std::min(C, S - s0);
        const int q = int(it % kDepth);
        if (op.masks) {
            // the staging of this slot was last read by the copy issued kDepth chunks ago
            HEC_HIP(hipStreamSynchronize(p->streams[q]));
            load_words(q, s0, c);
        }
        HEC_TRY(dma(true, s0, c, q));
        HEC_TRY(send_words(q, c));
        HEC_TRY(op.launch(slot_batch(p->slot[q], c), p->mask_dev[q], op.wants ? p->want_dev[q].p : nullptr,
                          p->streams[q], /*over_pcie=*/false));
        if (int(it) == fail_at) return fail(HEC_ERR_HIP, "test hook: failure after chunk " + std::to_string(it));
        HEC_TRY(dma(false, s0, c, q));
        if (op.words)  // D2H of the words only
            HEC_HIP(hipMemcpyAsync(op.words + s0, p->mask_dev[q], size_t(c) * 4, hipMemcpyDeviceToHost,
                                   p->streams[q]));
    }
    for (auto st : p->streams) HEC_HIP(hipStreamSynchronize(st));
    op.done(bad);
    return HEC_OK;
}

// Encode: the k data shards of every stripe in, the m parity shards back.
struct HostEncode : HostOp {
    HostEncode(const hec_rs_t* r, const Batch& b) {
        rs = r, host = b, split = r->k;
        in = {0, r->k, r->k};
        out = {r->k, r->n, r->m};
    }
    int launch(const Batch& b, uint32_t*, const uint32_t*, hipStream_t s, bool over_pcie) override {
        return run_apply(gd->encode, uint32_t(rs->k), b, nullptr, nullptr, s, nullptr, over_pcie);
    }
};

// hec_host_reconstruct_batch (want_masks == nullptr: every erased shard,
// run_apply's launches) and hec_host_reconstruct_some_batch. A stripe takes
// part when it has k shards present and wants an erased one: its first k
// present shards go in (the ones the decode reads), and only the wanted erased
// shards are computed, stored and brought back.
struct HostReconstruct : HostOp {
    HostReconstruct(const hec_rs_t* r, const Batch& b, const uint32_t* present_masks, const uint32_t* want_masks,
                    uint32_t* n_bad) {
        rs = r, host = b, masks = present_masks, wants = want_masks, n_bad_stripes = n_bad;
        in = {0, r->n, r->k};
        out = {0, r->n, 4};
    }
    bool takes_part(uint32_t mask, uint32_t want) const { return __builtin_popcount(mask) >= rs->k && want; }
    bool goes_in(uint32_t mask, uint32_t want, int i) const override {
        return takes_part(mask, want) && ((mask >> i) & 1) && __builtin_popcount(mask & ((1u << i) - 1)) < rs->k;
    }
    bool comes_back(uint32_t mask, uint32_t want, int i) const override {
        return takes_part(mask, want) && ((want >> i) & 1);
    }
    int prepare(hipStream_t s) override { return ensure_dense_decode(rs, gd, s); }
    int launch(const Batch& b, uint32_t* words, const uint32_t* want_words, hipStream_t s, bool) override {
        return run_some(gd->decode_dense, uint32_t(rs->k), b, words, want_words, nullptr, s);
    }
    void done(uint32_t bad) override {
        if (n_bad_stripes) *n_bad_stripes = bad;
    }
};

// Verify: all n shards in, nothing but the mismatch words back. The words
// always live in device memory (the pipeline's mask words): the kernels'
// atomics stay on the device, and only the words cross PCIe back. Every launch
// gets the true shard_len, never a length rounded up to the staging pitch: the
// pad bytes of a reused slot hold garbage, and a verify compares what an encode
// merely overwrites.
struct HostVerify : HostOp {
    HostVerify(const hec_rs_t* r, const Batch& b, uint32_t* mismatch, uint32_t* n_bad) {
        rs = r, host = b, split = r->k, words = mismatch, n_bad_stripes = n_bad, true_len = true;
        in = {0, r->n, r->n};
    }
    int launch(const Batch& b, uint32_t* dev_words, const uint32_t*, hipStream_t s, bool) override {
        ScrubOut o;  // one verify launch into the chunk's words: no count
        o.words = dev_words;
        return run_scrub(*gd, b, ScrubSpec{}, o, s);
    }
    void done(uint32_t) override {
        if (n_bad_stripes)
            for (uint32_t s = 0; s < host.n_stripes; ++s) *n_bad_stripes += words[s] ? 1u : 0u;
    }
};

// Update (hec.h hec_host_update_batch): host.in holds the deltas (old ^ new,
// or the new shard where the parity has not seen it yet), host.out the parity.
// Of a stripe whose mask names a shard, the named deltas and the four parity
// shards go in, the update runs with no old arena, and the parity comes back;
// a stripe with an empty mask moves nothing. The masks are update masks, not
// present masks: what load_masks counts over them means nothing here, and the
// bits it leaves above the data shards are the kernel's to ignore.
struct HostUpdate : HostOp {
    HostUpdate(const hec_rs_t* r, const Batch& b, const uint32_t* update_masks) {
        rs = r, host = b, split = r->k, masks = update_masks;
        in = {0, r->n, r->m + 1};
        out = {r->k, r->n, r->m};
    }
    bool changed(uint32_t mask) const { return (mask & ((1u << rs->k) - 1)) != 0; }
    bool goes_in(uint32_t mask, uint32_t, int i) const override {
        return i < rs->k ? ((mask >> i) & 1) != 0 : changed(mask);
    }
    bool comes_back(uint32_t mask, uint32_t, int i) const override { return i >= rs->k && changed(mask); }
    int launch(const Batch& b, uint32_t* words, const uint32_t*, hipStream_t s, bool) override {
        return run_update(gd->encode, Strided{}, b, words, s);
    }
};

}  // namespace
}  // namespace hec

using namespace hec;

extern "C" {

int hec_host_encode_batch(const hec_rs_t* rs, const uint8_t* h_data, uint64_t data_stripe_stride,
                          uint64_t data_shard_stride, uint8_t* h_parity, uint64_t parity_stripe_stride,
                          uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes) {
    HEC_TRY(check_batch_args(rs, h_data, h_parity, shard_len));
    if (n_stripes == 0) return HEC_OK;
    const Batch b = Batch::split(arena(h_data, data_stripe_stride, data_shard_stride),
                                 arena(h_parity, parity_stripe_stride, parity_shard_stride), shard_len, n_stripes);
    HEC_TRY(check_encode_strides(rs, b));
    HostEncode op(rs, b);
    return run_host_op(op);
}

int hec_host_reconstruct_batch(const hec_rs_t* rs, uint8_t* h_shards, uint64_t stripe_stride, uint64_t shard_stride,
                               uint64_t shard_len, uint32_t n_stripes, const uint32_t* h_present_masks,
                               uint32_t* n_bad_stripes) {
    HEC_TRY(check_batch_args(rs, h_shards, h_present_masks, shard_len));
    if (n_bad_stripes) *n_bad_stripes = 0;
    if (n_stripes == 0) return HEC_OK;
    const Batch b = Batch::in_place(arena(h_shards, stripe_stride, shard_stride), shard_len, n_stripes);
    HEC_TRY(check_strided("shards", uint32_t(rs->n), b.in, shard_len, n_stripes));
    HostReconstruct op(rs, b, h_present_masks, nullptr, n_bad_stripes);
    return run_host_op(op);
}

int hec_host_reconstruct_some_batch(const hec_rs_t* rs, uint8_t* h_shards, uint64_t stripe_stride,
                                    uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                    const uint32_t* h_present_masks, const uint32_t* h_want_masks,
                                    uint32_t* n_bad_stripes) {
    const Batch b = Batch::in_place(arena(h_shards, stripe_stride, shard_stride), shard_len, n_stripes);
    HEC_TRY(check_some_args(rs, b, h_present_masks, h_want_masks));
    if (n_bad_stripes) *n_bad_stripes = 0;
    if (n_stripes == 0) return HEC_OK;
    HostReconstruct op(rs, b, h_present_masks, h_want_masks, n_bad_stripes);
    return run_host_op(op);
}

int hec_host_verify_batch(const hec_rs_t* rs, const uint8_t* h_data, uint64_t data_stripe_stride,
                          uint64_t data_shard_stride, const uint8_t* h_parity, uint64_t parity_stripe_stride,
                          uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes, uint32_t* h_mismatch,
                          uint32_t* n_bad_stripes) {
    HEC_TRY(check_batch_args(rs, h_data, h_parity, shard_len));
    HEC_TRY(check_verify_args(rs, h_mismatch));
    if (n_bad_stripes) *n_bad_stripes = 0;
    if (n_stripes == 0) return HEC_OK;
    const Batch b = Batch::split(arena(h_data, data_stripe_stride, data_shard_stride),
                                 arena(h_parity, parity_stripe_stride, parity_shard_stride), shard_len, n_stripes);
    HEC_TRY(check_encode_strides(rs, b));
    HostVerify op(rs, b, h_mismatch, n_bad_stripes);
    return run_host_op(op);
}

int hec_host_update_batch(const hec_rs_t* rs, const uint8_t* h_delta, uint64_t delta_stripe_stride,
                          uint64_t delta_shard_stride, uint8_t* h_parity, uint64_t parity_stripe_stride,
                          uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes,
                          const uint32_t* h_update_masks) {
    const Batch b = Batch::split(arena(h_delta, delta_stripe_stride, delta_shard_stride),
                                 arena(h_parity, parity_stripe_stride, parity_shard_stride), shard_len, n_stripes);
    HEC_TRY(check_update_args(rs, Strided{}, b, h_update_masks));
    if (n_stripes == 0) return HEC_OK;
    HostUpdate op(rs, b, h_update_masks);
    return run_host_op(op);
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
