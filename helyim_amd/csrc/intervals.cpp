// Batched reconstruct of many small, independent stripes in one launch: the
// degraded-read path (helyim-store/src/erasure_coding/mod.rs:403-491 calls
// ReedSolomon::reconstruct once per needle interval, bytes to KiB each).
// Stripes are packed back to back into one pinned staging area, copied to the
// GPU once, decoded by rs104_ragged_kernel (one workgroup per 4 KiB chunk of
// each stripe, per-stripe length and erasure pattern), and copied back once.
#include <algorithm>
#include <atomic>
#include <cstring>
#include <memory>
#include <thread>

#include "hec_internal.hpp"

namespace hec {
namespace {

// Metadata (RaggedItems + workgroup map) of one device-resident ragged call:
// pinned staging and its device copy. The calls take slots round-robin, so a
// call waits only for the kernel that used its slot kMetaSlots calls ago, not
// for the previous call's kernel (a back-to-back encode / reconstruct stream
// keeps the GPU fed while the host builds the next map).
struct MetaSlot {
    PinnedBuf<> h;
    DeviceBuf<> d;
    hipEvent_t free = nullptr;  // recorded after the kernel that read this slot
    int reserve(size_t bytes) {
        if (free) HEC_HIP(hipEventSynchronize(free));
        else HEC_HIP(hipEventCreateWithFlags(&free, hipEventDisableTiming));
        HEC_TRY(h.reserve(bytes, kMetaFloor));
        return d.reserve(bytes, kMetaFloor);
    }
};
constexpr int kMetaSlots = 4;

// One slot of the per-device pool of ragged scratch (SlotPool, hec_internal.hpp).
struct RaggedScratch {
    std::mutex mu;
    hipStream_t stream = nullptr;
    MetaSlot slots[kMetaSlots];  // device-API ragged calls
    unsigned next_slot = 0;
    Completion done;             // small host calls (compact_reconstruct_104)
    PinnedBuf<> host, hmeta;     // compact payload and its metadata,
    DeviceBuf<> dev, dmeta;      // and their device copies
    int init() {
        HEC_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        return HEC_OK;
    }
    int reserve(size_t bytes, size_t meta) {
        HEC_TRY(host.reserve(bytes, kStagingFloor));
        HEC_TRY(dev.reserve(bytes, kStagingFloor));
        HEC_TRY(hmeta.reserve(meta, kMetaFloor));
        return dmeta.reserve(meta, kMetaFloor);
    }
    // A burst slot frees its compact payload above kStagingKeep when its call
    // ends (Scratch's rule); the metadata stays.
    void end_call(bool burst) {
        if (!burst || host.cap <= kStagingKeep) return;
        (void)hipStreamSynchronize(stream);  // an error return may leave copies in flight
        host.release();
        dev.release();
    }
};

}  // namespace

int compact_reconstruct_104(const hec_rs* rs, const std::vector<CompactJob>& jobs, const CompactFill& fill,
                            const CompactTake& take, bool io_bound_fill) {
    const int k = rs->k, n = rs->n;
    struct Lay {
        uint64_t Lp, off, out_off;
        uint32_t w;  // the erased shards the job wants; 0: the job is left out of everything below
    };
    std::vector<Lay> lay(jobs.size());
    uint64_t total = 0;
    bool some = false, any = false;  // some: a job wants fewer shards than it lost
    for (size_t j = 0; j < jobs.size(); ++j) {
        if (__builtin_popcount(jobs[j].mask) < k || jobs[j].len == 0 || jobs[j].len > 0xFFFFFFFFull)
            return fail(HEC_ERR_INVALID_ARGUMENT, "compact job without k survivors");
        const uint32_t erased = ~jobs[j].mask & ((1u << n) - 1);
        lay[j].w = jobs[j].want & erased;
        some |= lay[j].w != erased;
        any |= lay[j].w != 0;
        lay[j].Lp = round_up(jobs[j].len, 16);
        lay[j].off = total;
        if (lay[j].w) total += round_up(uint64_t(k) * lay[j].Lp, 256);  // compact inputs: the first k present shards
    }
    if (!any) return HEC_OK;
    const uint64_t in_total = total;
    for (size_t j = 0; j < jobs.size(); ++j) {  // compact outputs: the wanted erased shards, ascending
        lay[j].out_off = total;
        total += round_up(uint64_t(__builtin_popcount(lay[j].w)) * lay[j].Lp, 256);
    }
    GeomDevice* gd;
    int rc = geom_device(rs, &gd);
    if (rc) return rc;
    Lease<RaggedScratch> lease;
    if ((rc = lease_slot(lease))) return rc;
    RaggedScratch* sc = lease.sc;
    std::vector<RaggedItem> items(jobs.size());
    std::vector<uint32_t> block_item;
    for (size_t j = 0; j < jobs.size(); ++j) {
        const uint32_t chunks = lay[j].w ? uint32_t((jobs[j].len + 4095) / 4096) : 0;
        items[j] = RaggedItem{lay[j].off, lay[j].Lp, uint32_t(jobs[j].len), jobs[j].mask,
                              uint32_t(block_item.size()), lay[j].w, lay[j].out_off};
        block_item.insert(block_item.end(), chunks, uint32_t(j));
    }
    const size_t items_bytes = items.size() * sizeof(RaggedItem);
    const size_t map_off = round_up(items_bytes, 256);
    const size_t meta = map_off + block_item.size() * 4;
    if ((rc = sc->reserve(total, meta))) return rc;
    if ((rc = ensure_dense_decode(rs, gd, sc->stream))) return rc;
    // survivors the decode reads (the first k present shards) -> slots 0..k-1
    // The fills may run on host-pool workers, whose failure detail and values
    // are thread-local to them: the first failure's (code, detail, values) is
    // captured on its thread and re-raised on the caller's.
    ErrorSlot err;
    // one task per (job, slot): a single large interval's 10 survivor reads run
    // in parallel too
    auto fill_one = [&](size_t t) {
        const size_t j = t / size_t(k);
        const int want = int(t % size_t(k));
        if (!lay[j].w) return;
        int used = 0;
        for (int i = 0; i < n; ++i)
            if ((jobs[j].mask >> i) & 1) {
                if (used == want) {
                    const int r = fill(j, used, i, sc->host + lay[j].off + used * lay[j].Lp);
                    if (r) err.capture(r);
                    return;
                }
                ++used;
            }
    };
    if (io_bound_fill)
        parallel_io_for(jobs.size() * size_t(k), in_total, fill_one);
    else
        parallel_for(jobs.size() * size_t(k), in_total, fill_one);
    if ((rc = err.raise())) return rc;
    // zero-copy: the kernel reads the packed survivors and writes the rebuilt
    // shards in the pinned staging itself (no H2D / D2H of the payload)
    uint8_t* zh = zero_copy_enabled() ? pinned_device_ptr(sc->host) : nullptr;
    if (!zh) HEC_HIP(hipMemcpyAsync(sc->dev, sc->host, in_total, hipMemcpyHostToDevice, sc->stream));
    RaggedArgs ra{};
    ra.base = zh ? zh : sc->dev;
    ra.n_blocks = uint32_t(block_item.size());
    ra.tabs = gd->decode_dense.tabs;
    ra.lut = gd->decode_dense.lut;
    ra.compact = 1;
    if (items.size() == 1) {  // one stripe (a per-call reconstruct): descriptor as a kernel argument
        ra.inline_one = 1;
        ra.one = items[0];
    } else {
        std::memcpy(sc->hmeta, items.data(), items_bytes);
        std::memcpy(sc->hmeta + map_off, block_item.data(), block_item.size() * 4);
        HEC_HIP(hipMemcpyAsync(sc->dmeta, sc->hmeta, meta, hipMemcpyHostToDevice, sc->stream));
        ra.items = reinterpret_cast<const RaggedItem*>(sc->dmeta.p);
        ra.block_item = reinterpret_cast<const uint32_t*>(sc->dmeta + map_off);
    }
    // small zero-copy calls: completion from the kernel's own signal
    const bool signal = zh && in_total <= completion_flag_max();
    if (signal && (rc = sc->done.arm(sc->stream, &ra.done_count, &ra.done_flag, &ra.done_seq))) return rc;
    if (some)
        HEC_HIP(launch_rs104_ragged_some(ra, sc->stream));
    else
        HEC_HIP(launch_rs104_ragged(ra, true, sc->stream));
    if (!zh)
        HEC_HIP(hipMemcpyAsync(sc->host + in_total, sc->dev + in_total, total - in_total, hipMemcpyDeviceToHost,
                               sc->stream));
    if (signal) {
        if ((rc = sc->done.wait(sc->stream))) return rc;
    } else {
        HEC_HIP(hipStreamSynchronize(sc->stream));
    }
    // hand back the wanted erased shards
    parallel_for(jobs.size(), total - in_total, [&](size_t j) {
        int r = 0;
        for (int i = 0; i < n; ++i)
            if ((lay[j].w >> i) & 1) take(j, i, sc->host + lay[j].out_off + uint64_t(r++) * lay[j].Lp);
    });
    return HEC_OK;
}

}  // namespace hec

using namespace hec;

// hec_rs_reconstruct_batch (required == nullptr: every missing shard, or with
// data_only the data shards) and hec_rs_reconstruct_some_batch (required: n
// flags per stripe, the missing shards to rebuild): one body.
static int reconstruct_batch(const hec_rs_t* rs, uint8_t* const* shards, const size_t* lens, const uint8_t* present,
                             const uint8_t* required, size_t n_stripes, int data_only, size_t* bad_index) {
    const int k = rs->k, n = rs->n;
    if (bad_index) *bad_index = n_stripes;
    auto need = [&](size_t s, int i) { return required ? required[s * n + i] != 0 : !(data_only && i >= k); };
    // 1. validate every stripe first (upstream reconstruct checks, per stripe)
    struct Active {
        size_t s;
        uint64_t L;
        uint32_t mask, want;
    };
    std::vector<Active> act;
    for (size_t s = 0; s < n_stripes; ++s) {
        const uint8_t* pr = present + s * n;
        uint64_t L = 0;
        int np = 0, err = HEC_OK;
        uint32_t mask = 0, want = 0;
        for (int i = 0; i < n && !err; ++i) {
            if (i < 32 && need(s, i)) want |= 1u << i;
            if (!pr[i]) continue;
            const size_t li = lens[s * n + i];
            if (li == 0) err = HEC_ERR_EMPTY_SHARD;
            else if (np && li != L) err = HEC_ERR_INCORRECT_SHARD_SIZE;
            L = li;
            ++np;
            if (i < 32) mask |= 1u << i;  // used by the RS(10,4) path only; n may be up to 256
        }
        if (!err && np < n && np < k) err = HEC_ERR_TOO_FEW_SHARDS_PRESENT;
        if (!err && np < n)
            for (int i = 0; i < n; ++i)
                if (!pr[i] && need(s, i) && !shards[s * n + i])
                    err = fail(HEC_ERR_INVALID_ARGUMENT, "missing shard without a buffer");
        if (err) {
            if (bad_index) *bad_index = s;
            return err == HEC_ERR_INVALID_ARGUMENT ? err : fail(err, "stripe " + std::to_string(s));
        }
        if (np == n) continue;  // upstream no-op
        act.push_back({s, L, mask, want});
    }
    if (act.empty()) return HEC_OK;

    // Other geometries: one host-API reconstruct per stripe (same kernels, generic path).
    if (!(k == 10 && rs->m == 4)) {
        for (const Active& a : act) {
            int rc = required ? hec_rs_reconstruct_some(rs, shards + a.s * n, lens + a.s * n, present + a.s * n,
                                                        required + a.s * n, n)
                     : data_only
                         ? hec_rs_reconstruct_data(rs, shards + a.s * n, lens + a.s * n, present + a.s * n, n)
                         : hec_rs_reconstruct(rs, shards + a.s * n, lens + a.s * n, present + a.s * n, n);
            if (rc) {
                if (bad_index) *bad_index = a.s;
                return rc;
            }
        }
        return HEC_OK;
    }

    std::vector<CompactJob> jobs(act.size());
    for (size_t j = 0; j < act.size(); ++j) jobs[j] = CompactJob{act[j].L, act[j].mask, act[j].want};
    return compact_reconstruct_104(
        rs, jobs,
        [&](size_t j, int, int shard, uint8_t* dst) {
            std::memcpy(dst, shards[act[j].s * n + shard], act[j].L);
            return HEC_OK;
        },
        [&](size_t j, int shard, const uint8_t* src) {
            std::memcpy(shards[act[j].s * n + shard], src, act[j].L);
        });
}

extern "C" {

int hec_rs_reconstruct_batch(const hec_rs_t* rs, uint8_t* const* shards, const size_t* lens, const uint8_t* present,
                             size_t n_stripes, int data_only, size_t* bad_index) {
    if (!rs || (n_stripes && (!shards || !lens || !present))) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    return reconstruct_batch(rs, shards, lens, present, nullptr, n_stripes, data_only, bad_index);
}

int hec_rs_reconstruct_some_batch(const hec_rs_t* rs, uint8_t* const* shards, const size_t* lens,
                                  const uint8_t* present, const uint8_t* required, size_t n_stripes,
                                  size_t* bad_index) {
    if (!rs || (n_stripes && (!shards || !lens || !present || !required)))
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    return reconstruct_batch(rs, shards, lens, present, required, n_stripes, 0, bad_index);
}

}  // extern "C"

namespace hec {
namespace {

// What a device-resident ragged call does with its stripes.
enum class RaggedOp { Encode, Decode, Scrub };

// Workgroups of one ragged stripe: none for a decode of a stripe whose 14
// shards are all present (upstream's no-op), none for a scrub of a stripe
// with no spare shard (nothing to compare: it is not read), so those launch
// nothing. want: a reconstruct some's word for the stripe (a decode of a
// stripe that wants none of its erased shards is a no-op too).
uint64_t ragged_chunks(const hec_stripe_desc& d, RaggedOp op, uint32_t chunk_bytes, uint32_t want = 0xFFFFFFFFu) {
    const uint32_t m = d.present_mask & 0x3FFFu;
    if (op == RaggedOp::Decode && (want & ~m & 0x3FFFu) == 0) return 0;
    if (op == RaggedOp::Scrub && __builtin_popcount(m) <= 10) return 0;
    return (uint64_t(d.shard_len) + chunk_bytes - 1) / chunk_bytes;
}

// The kernel of one ragged launch, shared by gpu_ragged and
// hec_ragged_kernel_name so a reported name is the kernel that runs. Both
// ragged kernels deal each XCD a contiguous eighth of the launch's column
// ranges (ragged_block, rs_device.hpp).
struct RaggedPick {
    bool bitslice;  // encode with every length a multiple of 8 KiB: rs104_bs_ragged_kernel
};
RaggedPick ragged_pick(const hec_stripe_desc* descs, uint32_t n, bool decode) {
    RaggedPick p;
    p.bitslice = !decode;
    for (uint32_t j = 0; j < n && p.bitslice; ++j) p.bitslice = descs[j].shard_len % kBsChunk == 0;
    return p;
}

const char* ragged_name(const RaggedPick& p, bool decode) {
    if (decode) return "rs104_ragged_kernel<DEC=true> (table lookup, XCD eighths)";
    if (p.bitslice) return "rs104_bs_ragged_kernel (bit-sliced, XCD eighths)";
    return "rs104_ragged_kernel<DEC=false> (table lookup, XCD eighths)";
}

// Pass 1 of a ragged scrub, shared by gpu_ragged_scrub and
// hec_ragged_scrub_kernel_name: bit-sliced when every stripe has all 14 shards
// and a length that is a multiple of 8 KiB (the table check on full masks runs
// 1.13x the bit-sliced verify on strided batches), else the
// table check over each stripe's own mask.
RaggedPick ragged_scrub_pick(const hec_stripe_desc* descs, uint32_t n) {
    RaggedPick p;
    p.bitslice = true;
    for (uint32_t j = 0; j < n && p.bitslice; ++j)
        p.bitslice = descs[j].shard_len % kBsChunk == 0 && (descs[j].present_mask & 0x3FFFu) == 0x3FFFu;
    return p;
}

// The argument and descriptor checks of every device-resident ragged call,
// all before device work; *n_blocks = the workgroup map's entries.
int ragged_check_args(const hec_rs_t* rs, const uint8_t* d_base, const hec_stripe_desc* descs, uint32_t n, RaggedOp op,
                      uint32_t chunk_bytes, uint64_t* n_blocks, const uint32_t* wants = nullptr) {
    if (!rs || !d_base || (n && !descs)) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (!(rs->k == 10 && rs->m == 4))
        return fail(HEC_ERR_INVALID_ARGUMENT, "ragged device batches are RS(10,4) only");
    *n_blocks = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const hec_stripe_desc& d = descs[j];
        if (d.shard_len == 0) return fail(HEC_ERR_EMPTY_SHARD, "stripe " + std::to_string(j));
        if ((d.offset | d.shard_stride | uint64_t(reinterpret_cast<uintptr_t>(d_base))) % 16 != 0 ||
            d.shard_stride < d.shard_len)
            return fail(HEC_ERR_INVALID_ARGUMENT, "stripe " + std::to_string(j) +
                                                      ": offset/stride must be 16-byte aligned, stride >= len");
        // 64-bit: a shard_len near 2^32 must not wrap to 0 or 1 chunks
        *n_blocks += ragged_chunks(d, op, chunk_bytes, wants ? wants[j] : 0xFFFFFFFFu);
        if (*n_blocks > UINT32_MAX) return fail(HEC_ERR_INVALID_ARGUMENT, "ragged batch above 2^32 workgroups");
    }
    return HEC_OK;
}

// Descriptors -> RaggedItems + workgroup map in a pinned metadata slot,
// uploaded on the caller's stream ahead of the kernels that read it. The
// caller records slot->free after the last of them.
// The corrected reconstruct keeps a second pair in the same slot, the decode's
// (its map has entries for every stripe with a shard missing, the scrub's for
// every stripe with a spare one, so first_block differs between the two).
struct RaggedMeta {
    Lease<RaggedScratch> lease;
    MetaSlot* slot = nullptr;
    size_t map_off = 0, bytes = 0;
    size_t items2_off = 0, map2_off = 0;  // the second pair, when there is one
    // waits for this slot's previous kernels only
    int reserve(uint32_t n, uint64_t n_blocks, bool second = false, uint64_t n_blocks2 = 0) {
        HEC_TRY(lease_slot(lease));
        map_off = round_up(size_t(n) * sizeof(RaggedItem), 256);
        bytes = map_off + n_blocks * 4;
        if (second) {
            items2_off = round_up(bytes, 256);
            map2_off = items2_off + map_off;
            bytes = map2_off + n_blocks2 * 4;
        }
        slot = &lease.sc->slots[lease.sc->next_slot++ % kMetaSlots];
        return slot->reserve(bytes);
    }
    // items and workgroup map of one pair written straight into the pinned slot
    // wants (a reconstruct some): each item's want word, and no map entry for a stripe that wants nothing
    void fill(const hec_stripe_desc* descs, uint32_t n, RaggedOp op, uint32_t chunk_bytes, size_t items_at,
              size_t map_at, uint8_t* d_base, uint64_t n_blocks, RaggedArgs& ra, const uint32_t* wants = nullptr) {
        RaggedItem* items = reinterpret_cast<RaggedItem*>(slot->h + items_at);
        uint32_t* block_item = reinterpret_cast<uint32_t*>(slot->h + map_at);
        uint32_t first = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const hec_stripe_desc& d = descs[j];
            const uint32_t chunks = uint32_t(ragged_chunks(d, op, chunk_bytes, wants ? wants[j] : 0xFFFFFFFFu));
            items[j] = RaggedItem{d.offset, d.shard_stride, d.shard_len, d.present_mask, first, wants ? wants[j] : 0, 0};
            std::fill(block_item + first, block_item + first + chunks, j);
            first += chunks;
        }
        ra.base = d_base;
        ra.items = reinterpret_cast<const RaggedItem*>(slot->d + items_at);
        ra.block_item = reinterpret_cast<const uint32_t*>(slot->d + map_at);
        ra.n_blocks = uint32_t(n_blocks);
    }
    // decode2: the arguments of the second pair, a 4 KiB decode map of n_blocks2 entries
    int upload(const hec_stripe_desc* descs, uint32_t n, RaggedOp op, uint32_t chunk_bytes, uint8_t* d_base,
               uint64_t n_blocks, hipStream_t stream, RaggedArgs& ra, RaggedArgs* decode2 = nullptr,
               uint64_t n_blocks2 = 0, const uint32_t* wants = nullptr) {
        fill(descs, n, op, chunk_bytes, 0, map_off, d_base, n_blocks, ra, wants);
        if (decode2) fill(descs, n, RaggedOp::Decode, 4096, items2_off, map2_off, d_base, n_blocks2, *decode2);
        HEC_HIP(hipMemcpyAsync(slot->d, slot->h, bytes, hipMemcpyHostToDevice, stream));
        return HEC_OK;
    }
};

// What every device-resident ragged call does before its first launch and
// after its last: stripe descriptors come from the host, data stays in HBM.
struct RaggedCall {
    bool bitslice = false;
    uint64_t n_blocks = 0, n_decode = 0;  // map entries of the call's own pair, and of a decode's second pair
    GeomDevice* gd = nullptr;             // stays null for an empty batch: nothing to launch or record
    RaggedMeta meta;
    // The pick, the argument checks (all before device work; a null descriptor
    // list fails inside ragged_check_args, after the caller's own null checks),
    // the geometry's plan sets (every one before any launch: their first call
    // uploads and waits) and the metadata upload; ra: the arguments of the
    // call's own pair. wants: a reconstruct some's want words. decode2: the
    // arguments of a second, decode pair (the corrected reconstruct).
    int begin(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs, uint32_t n, RaggedOp op,
              hipStream_t stream, RaggedArgs& ra, const uint32_t* wants = nullptr, RaggedArgs* decode2 = nullptr,
              uint32_t min_spares = 2) {
        const bool scrub = op == RaggedOp::Scrub;
        bitslice = (n == 0 || descs) &&  // a null list fails below
                   (scrub ? ragged_scrub_pick(descs, n) : ragged_pick(descs, n, op == RaggedOp::Decode)).bitslice;
        const uint32_t chunk_bytes = bitslice ? kBsChunk : 4096;
        HEC_TRY(ragged_check_args(rs, d_base, descs, n, op, chunk_bytes, &n_blocks, wants));
        if (decode2) HEC_TRY(ragged_check_args(rs, d_base, descs, n, RaggedOp::Decode, 4096, &n_decode));
        HEC_TRY(check_min_spares(min_spares));
        if (n == 0) return HEC_OK;
        GeomDevice* g;
        HEC_TRY(geom_device(rs, &g));
        // a scrub's plan sets upload on the caller's stream, before a metadata slot is taken
        if (scrub) HEC_TRY(ensure_check_plans(rs, g, stream));
        if (decode2) HEC_TRY(ensure_dense_decode(rs, g, stream));
        HEC_TRY(meta.reserve(n, n_blocks, decode2 != nullptr, n_decode));
        // a plain decode's on the slot's own stream
        if (op == RaggedOp::Decode) HEC_TRY(ensure_dense_decode(rs, g, meta.lease.sc->stream));
        HEC_TRY(meta.upload(descs, n, op, chunk_bytes, d_base, n_blocks, stream, ra, decode2, n_decode, wants));
        gd = g;
        return HEC_OK;
    }
    // After the last kernel that reads the slot, launched or not.
    int end(hipStream_t stream) {
        HEC_HIP(hipEventRecord(meta.slot->free, stream));
        return HEC_OK;
    }
};

// The ragged encode, reconstruct and (wants) reconstruct some: one launch.
int gpu_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs, uint32_t n, bool decode,
               uint32_t* d_bad, hipStream_t stream, const uint32_t* wants = nullptr) {
    RaggedCall c;
    RaggedArgs ra{};
    HEC_TRY(c.begin(rs, d_base, descs, n, decode ? RaggedOp::Decode : RaggedOp::Encode, stream, ra, wants));
    if (!c.gd) return HEC_OK;
    ra.tabs = decode ? c.gd->decode_dense.tabs : c.gd->encode.tabs;
    ra.lut = decode ? c.gd->decode_dense.lut : nullptr;
    ra.bad_count = d_bad;
    if (c.n_blocks == 0) return c.end(stream);  // every stripe already complete (upstream no-op)
    if (c.bitslice)
        HEC_HIP(launch_rs104_bs_ragged(ra, stream));
    else if (wants)
        HEC_HIP(launch_rs104_ragged_some(ra, stream));
    else
        HEC_HIP(launch_rs104_ragged(ra, decode, stream));
    return c.end(stream);
}

// The decode after a corrected ragged scrub: use[] = the masks it decodes
// from, bad += the decode's count (stripes with fewer than ten shards),
// unrepaired += the dirty stripes that keep their holes.
struct RaggedDecodeTail {
    uint32_t* use = nullptr;
    uint32_t* bad = nullptr;
    uint32_t* unrepaired = nullptr;
};

// The ragged scrubs (hec.h has each call's contract): the masked check of every
// stripe over its own length and mask, out as run_scrub's; pass 2 walks pass
// 1's map over the flagged stripes, naming (Locate) or also fixing in place
// (Correct) what it explains. tail (hec_gpu_reconstruct_corrected_ragged): the
// use masks are then set and the stripes whose survivors are consistent
// decoded, from a map of its own in the same metadata slot.
int gpu_ragged_scrub(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs, uint32_t n, Pass2 pass2,
                     uint32_t min_spares, const ScrubOut& out, const RaggedDecodeTail* tail, hipStream_t stream) {
    if (!out.words || (pass2 != Pass2::None && !out.suspects) || (tail && !tail->use))
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    RaggedCall c;
    RaggedCorrectArgs v{};
    RaggedArgs dec{};
    HEC_TRY(c.begin(rs, d_base, descs, n, RaggedOp::Scrub, stream, v.a, nullptr, tail ? &dec : nullptr, min_spares));
    if (!c.gd) return HEC_OK;
    uint32_t unchecked = 0;  // stripes without a spare shard: no scrub map entry, never read
    for (uint32_t j = 0; j < n; ++j) unchecked += __builtin_popcount(descs[j].present_mask & 0x3FFFu) <= 10;
    v.a.tabs = c.gd->check.tabs;
    v.a.lut = c.gd->check.lut;
    v.a.bad_count = out.bad;
    v.check = out.words;
    v.suspects = out.suspects;
    v.ratio_tabs = c.gd->check_ratio.tabs;
    if (pass2 == Pass2::Correct) {
        v.fix_tabs = c.gd->check_fix.tabs;
        v.min_spares = min_spares;
        v.uncorrected = out.left;
        v.corrected_bytes = out.corrected_bytes;
    }
    // the kernels only ever OR bits in: stale words must not leak through
    HEC_HIP(hipMemsetAsync(out.words, 0, size_t(n) * 4, stream));
    if (pass2 != Pass2::None) HEC_HIP(hipMemsetAsync(out.suspects, 0, size_t(n) * 4, stream));
    if (unchecked && out.unchecked) HEC_HIP(launch_add_word(out.unchecked, unchecked, stream));
    if (c.n_blocks) {
        HEC_HIP(launch_ragged_check(v, c.bitslice, stream));
        // pass 2: only the stripes pass 1 flagged are read again (the counts are pass 1's)
        if (pass2 == Pass2::Locate) HEC_HIP(launch_ragged_locate(v, c.bitslice, stream));
        if (pass2 == Pass2::Correct) HEC_HIP(launch_ragged_correct(v, c.bitslice, stream));
    }
    if (tail) {
        HEC_HIP(launch_ragged_use_masks_corrected(v.a.items, const_cast<RaggedItem*>(dec.items), out.words,
                                                  out.suspects, tail->use, tail->unrepaired, min_spares, n, stream));
        dec.tabs = c.gd->decode_dense.tabs;
        dec.lut = c.gd->decode_dense.lut;
        dec.bad_count = tail->bad;
        if (c.n_decode) HEC_HIP(launch_rs104_ragged(dec, true, stream));
    }
    return c.end(stream);
}

// One arena of a ragged update descriptor: 16-byte aligned, shards apart, the
// extent offset + shards * stride inside 64 bits.
bool update_arena_ok(const void* base, uint64_t off, uint64_t stride, uint32_t len, uint64_t shards) {
    uint64_t ext;
    if ((off | stride | uint64_t(reinterpret_cast<uintptr_t>(base))) % 16 != 0 || stride < len) return false;
    return !__builtin_mul_overflow(stride, shards, &ext) && !__builtin_add_overflow(ext, off, &ext);
}

// The argument and descriptor checks of hec_gpu_update_ragged in
// ragged_check_args' order, all before device work; *n_blocks = the workgroup
// map's entries (4 KiB column ranges of the stripes with U non-empty).
int update_ragged_check_args(const hec_rs_t* rs, const uint8_t* d_old, const uint8_t* d_new, const uint8_t* d_parity,
                             const hec_update_desc* descs, uint32_t n, uint64_t* n_blocks) {
    if (!rs || !d_new || !d_parity || (n && !descs)) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (!(rs->k == 10 && rs->m == 4)) return fail(HEC_ERR_INVALID_ARGUMENT, "ragged update is RS(10,4) only");
    *n_blocks = 0;
    for (uint32_t j = 0; j < n; ++j) {
        const hec_update_desc& d = descs[j];
        if (d.shard_len == 0) return fail(HEC_ERR_EMPTY_SHARD, "stripe " + std::to_string(j));
        if (!update_arena_ok(d_parity, d.parity_offset, d.parity_stride, d.shard_len, 4) ||
            !update_arena_ok(d_new, d.new_offset, d.new_stride, d.shard_len, 10) ||
            (d_old && !update_arena_ok(d_old, d.old_offset, d.old_stride, d.shard_len, 10)))
            return fail(HEC_ERR_INVALID_ARGUMENT, "stripe " + std::to_string(j) +
                                                      ": offsets/strides must be 16-byte aligned, stride >= len");
        if (d.update_mask & 0x3FFu) *n_blocks += (uint64_t(d.shard_len) + 4095) / 4096;
        if (*n_blocks > UINT32_MAX) return fail(HEC_ERR_INVALID_ARGUMENT, "ragged batch above 2^32 workgroups");
    }
    return HEC_OK;
}

// hec_gpu_update_ragged: a sibling of RaggedCall (its descriptor, its item and
// its three arenas are the update's own), over the same metadata slots.
int gpu_update_ragged(const hec_rs_t* rs, const uint8_t* d_old, const uint8_t* d_new, uint8_t* d_parity,
                      const hec_update_desc* descs, uint32_t n, hipStream_t stream) {
    uint64_t n_blocks = 0;
    HEC_TRY(update_ragged_check_args(rs, d_old, d_new, d_parity, descs, n, &n_blocks));
    if (n == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    Lease<RaggedScratch> lease;
    HEC_TRY(lease_slot(lease));
    const size_t map_off = round_up(size_t(n) * sizeof(UpdateItem), 256);
    const size_t bytes = map_off + n_blocks * 4;
    MetaSlot* slot = &lease.sc->slots[lease.sc->next_slot++ % kMetaSlots];
    HEC_TRY(slot->reserve(bytes));  // waits for this slot's previous kernels only
    if (n_blocks) {
        UpdateItem* items = reinterpret_cast<UpdateItem*>(slot->h.p);
        uint32_t* block_item = reinterpret_cast<uint32_t*>(slot->h + map_off);
        uint32_t first = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const hec_update_desc& d = descs[j];
            const uint32_t chunks = (d.update_mask & 0x3FFu) ? uint32_t((uint64_t(d.shard_len) + 4095) / 4096) : 0;
            items[j] = UpdateItem{d.parity_offset, d.parity_stride, d.new_offset,  d.new_stride, d.old_offset,
                                  d.old_stride,    d.shard_len,     d.update_mask, first,        0};
            std::fill(block_item + first, block_item + first + chunks, j);
            first += chunks;
        }
        HEC_HIP(hipMemcpyAsync(slot->d, slot->h, bytes, hipMemcpyHostToDevice, stream));
        RaggedUpdateArgs v{};
        v.a.base = d_parity;
        v.a.block_item = reinterpret_cast<const uint32_t*>(slot->d + map_off);
        v.a.n_blocks = uint32_t(n_blocks);
        v.a.tabs = gd->encode.tabs;
        v.new_base = d_new;
        v.old_base = d_old;
        v.items = reinterpret_cast<const UpdateItem*>(slot->d.p);
        HEC_HIP(launch_ragged_update(v, stream));
    }
    // every mask empty: nothing launched, the slot free again in stream order
    HEC_HIP(hipEventRecord(slot->free, stream));
    return HEC_OK;
}

}  // namespace

// hec_rs_update_batch's RS(10,4) path, compact_reconstruct_104's shape: per job
// the deltas old ^ new of its changed shards packed compactly (XORed while
// packing) and its four parity shards behind them in the pinned staging, one
// rs104_ragged_update_kernel<false, true> launch over them in place (zero copy)
// or through the device copy, and the parity handed back.
int compact_update_104(const hec_rs* rs, const std::vector<UpdateJob>& jobs) {
    const int k = rs->k, m = rs->m;
    struct Lay {
        uint64_t Lp, off, par_off;
    };
    std::vector<Lay> lay(jobs.size());
    uint64_t total = 0, n_blocks = 0;
    for (size_t j = 0; j < jobs.size(); ++j) {  // the deltas of every job first: one upload
        if (jobs[j].len == 0 || jobs[j].len > 0xFFFFFFFFull || (jobs[j].mask & 0x3FFu) == 0)
            return fail(HEC_ERR_INVALID_ARGUMENT, "compact update job without a length or a changed shard");
        lay[j].Lp = round_up(jobs[j].len, 16);
        lay[j].off = total;
        total += round_up(uint64_t(__builtin_popcount(jobs[j].mask & 0x3FFu)) * lay[j].Lp, 256);
        n_blocks += (jobs[j].len + 4095) / 4096;
    }
    if (jobs.empty()) return HEC_OK;
    if (n_blocks > UINT32_MAX) return fail(HEC_ERR_INVALID_ARGUMENT, "update batch above 2^32 workgroups");
    const uint64_t delta_total = total;
    for (size_t j = 0; j < jobs.size(); ++j) {  // then the parity, read and written
        lay[j].par_off = total;
        total += round_up(uint64_t(m) * lay[j].Lp, 256);
    }
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    Lease<RaggedScratch> lease;
    HEC_TRY(lease_slot(lease));
    RaggedScratch* sc = lease.sc;
    std::vector<UpdateItem> items(jobs.size());
    std::vector<uint32_t> block_item;
    block_item.reserve(n_blocks);
    for (size_t j = 0; j < jobs.size(); ++j) {
        items[j] = UpdateItem{lay[j].par_off, lay[j].Lp, lay[j].off, lay[j].Lp, 0, 0, uint32_t(jobs[j].len),
                              jobs[j].mask & 0x3FFu, uint32_t(block_item.size()), 0};
        block_item.insert(block_item.end(), size_t((jobs[j].len + 4095) / 4096), uint32_t(j));
    }
    const size_t items_bytes = items.size() * sizeof(UpdateItem);
    const size_t map_off = round_up(items_bytes, 256);
    const size_t meta = map_off + block_item.size() * 4;
    HEC_TRY(sc->reserve(total, meta));
    // one task per (job, slot): slots 0..k-1 the data shards (a changed one packs
    // its delta at its rank in U), slots k..k+m-1 the parity shards
    parallel_for(jobs.size() * size_t(k + m), total, [&](size_t t) {
        const size_t j = t / size_t(k + m);
        const int i = int(t % size_t(k + m));
        const UpdateJob& job = jobs[j];
        const size_t L = job.len;
        if (i >= k) {
            std::memcpy(sc->host + lay[j].par_off + uint64_t(i - k) * lay[j].Lp, job.shards[i], L);
        } else if ((job.mask >> i) & 1) {
            const uint32_t q = uint32_t(__builtin_popcount(job.mask & ((1u << i) - 1)));
            uint8_t* dst = sc->host + lay[j].off + uint64_t(q) * lay[j].Lp;
            const uint8_t *o = job.shards[i], *w = job.new_data[i];
            for (size_t b = 0; b < L; ++b) dst[b] = o[b] ^ w[b];
        }
    });
    // zero-copy: the kernel reads the deltas and updates the parity in the pinned staging itself
    uint8_t* zh = zero_copy_enabled() ? pinned_device_ptr(sc->host) : nullptr;
    StreamDrain drain{sc->stream};
    if (!zh) HEC_HIP(hipMemcpyAsync(sc->dev, sc->host, total, hipMemcpyHostToDevice, sc->stream));
    RaggedUpdateArgs v{};
    v.a.base = zh ? zh : sc->dev.p;
    v.new_base = v.a.base;
    v.a.n_blocks = uint32_t(block_item.size());
    v.a.tabs = gd->encode.tabs;
    v.a.compact = 1;
    if (items.size() == 1) {  // one stripe: descriptor as a kernel argument
        v.a.inline_one = 1;
        v.one = items[0];
    } else {
        std::memcpy(sc->hmeta, items.data(), items_bytes);
        std::memcpy(sc->hmeta + map_off, block_item.data(), block_item.size() * 4);
        HEC_HIP(hipMemcpyAsync(sc->dmeta, sc->hmeta, meta, hipMemcpyHostToDevice, sc->stream));
        v.items = reinterpret_cast<const UpdateItem*>(sc->dmeta.p);
        v.a.block_item = reinterpret_cast<const uint32_t*>(sc->dmeta + map_off);
    }
    const bool signal = zh && total <= completion_flag_max();
    if (signal) HEC_TRY(sc->done.arm(sc->stream, &v.a.done_count, &v.a.done_flag, &v.a.done_seq));
    HEC_HIP(launch_ragged_update(v, sc->stream));
    if (!zh)
        HEC_HIP(hipMemcpyAsync(sc->host + delta_total, sc->dev + delta_total, total - delta_total,
                               hipMemcpyDeviceToHost, sc->stream));
    if (signal) HEC_TRY(sc->done.wait(sc->stream));
    else HEC_HIP(hipStreamSynchronize(sc->stream));
    parallel_for(jobs.size() * size_t(m), total - delta_total, [&](size_t t) {
        const size_t j = t / size_t(m), r = t % size_t(m);
        std::memcpy(jobs[j].shards[size_t(k) + r], sc->host + lay[j].par_off + r * lay[j].Lp, jobs[j].len);
    });
    return HEC_OK;
}

}  // namespace hec

extern "C" {

int hec_gpu_update_ragged(const hec_rs_t* rs, const uint8_t* d_old, const uint8_t* d_new, uint8_t* d_parity,
                          const hec_update_desc* descs, uint32_t n_stripes, void* stream) {
    return hec::gpu_update_ragged(rs, d_old, d_new, d_parity, descs, n_stripes, static_cast<hipStream_t>(stream));
}

const char* hec_update_ragged_kernel_name(int with_old) { return hec::ragged_update_kernel_name(with_old != 0); }

// Every stripe through hec_rs_update's checks, in its order, before any work.
int hec_rs_update_batch(const hec_rs_t* rs, uint8_t* const* shards, const size_t* lens,
                        const uint8_t* const* new_data, size_t n_stripes, size_t* bad_index) {
    if (!rs || (n_stripes && (!shards || !lens || !new_data))) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    const int k = rs->k, n = rs->n;
    if (bad_index) *bad_index = n_stripes;
    std::vector<hec::UpdateJob> jobs;
    std::vector<size_t> act;
    for (size_t s = 0; s < n_stripes; ++s) {
        uint8_t* const* sh = shards + s * n;
        const size_t* ln = lens + s * n;
        const uint8_t* const* nd = new_data + s * k;
        int err = HEC_OK;
        const char* what = nullptr;
        uint32_t mask = 0;
        bool any = false;
        for (int i = 0; i < n && !err; ++i) {
            const bool used = i >= k || nd[i];
            if (i < k && used) {
                any = true;
                if (i < 32) mask |= 1u << i;  // the RS(10,4) path's; k may be up to 255
            }
            if (used && !sh[i]) {
                err = HEC_ERR_INVALID_ARGUMENT;
                what = i < k ? "changed shard without its old buffer" : "null parity shard";
            }
        }
        size_t L = 0;
        for (int i = 0; i < n && !err; ++i) {
            if (i < k && !nd[i]) continue;
            if (ln[i] == 0) err = HEC_ERR_EMPTY_SHARD;
            else if (L && ln[i] != L) err = HEC_ERR_INCORRECT_SHARD_SIZE;
            L = ln[i];
        }
        if (!err && L > 0xFFFFFFFFull) {
            err = HEC_ERR_INVALID_ARGUMENT;
            what = "shard length above 2^32 - 1";
        }
        if (err) {
            if (bad_index) *bad_index = s;
            return fail(err, "stripe " + std::to_string(s) + (what ? std::string(": ") + what : std::string()));
        }
        if (!any) continue;  // nothing changed: the stripe is skipped untouched
        act.push_back(s);
        jobs.push_back(hec::UpdateJob{L, mask, sh, nd});
    }
    if (act.empty()) return HEC_OK;
    // Other geometries: one host-API update per active stripe (generic path).
    if (!(k == 10 && rs->m == 4)) {
        for (size_t s : act) {
            const int rc = hec_rs_update(rs, shards + s * n, lens + s * n, new_data + s * k, size_t(n));
            if (rc) {
                if (bad_index) *bad_index = s;
                return rc;
            }
        }
        return HEC_OK;
    }
    return hec::compact_update_104(rs, jobs);
}

int hec_gpu_correct_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs, uint32_t n_stripes,
                           uint32_t min_spares, uint32_t* d_check, uint32_t* d_suspects, uint32_t* d_bad_stripes,
                           uint32_t* d_unchecked, uint32_t* d_uncorrected, unsigned long long* d_corrected_bytes,
                           void* stream) {
    hec::ScrubOut out;
    out.words = d_check;
    out.suspects = d_suspects;
    out.bad = d_bad_stripes;
    out.unchecked = d_unchecked;
    out.left = d_uncorrected;
    out.corrected_bytes = d_corrected_bytes;
    return hec::gpu_ragged_scrub(rs, d_base, descs, n_stripes, hec::Pass2::Correct, min_spares, out, nullptr,
                                 static_cast<hipStream_t>(stream));
}

int hec_gpu_reconstruct_corrected_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs,
                                         uint32_t n_stripes, uint32_t min_spares, uint32_t* d_check,
                                         uint32_t* d_suspects, uint32_t* d_use_masks, uint32_t* d_bad_stripes,
                                         uint32_t* d_unrepaired, unsigned long long* d_corrected_bytes, void* stream) {
    hec::ScrubOut out;  // the counts are the decode's
    out.words = d_check;
    out.suspects = d_suspects;
    out.corrected_bytes = d_corrected_bytes;
    hec::RaggedDecodeTail tail;
    tail.use = d_use_masks;
    tail.bad = d_bad_stripes;
    tail.unrepaired = d_unrepaired;
    return hec::gpu_ragged_scrub(rs, d_base, descs, n_stripes, hec::Pass2::Correct, min_spares, out, &tail,
                                 static_cast<hipStream_t>(stream));
}

int hec_gpu_encode_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs, uint32_t n_stripes,
                          void* stream) {
    return hec::gpu_ragged(rs, d_base, descs, n_stripes, false, nullptr, static_cast<hipStream_t>(stream));
}

int hec_gpu_reconstruct_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs,
                               uint32_t n_stripes, uint32_t* d_bad_stripes, void* stream) {
    return hec::gpu_ragged(rs, d_base, descs, n_stripes, true, d_bad_stripes, static_cast<hipStream_t>(stream));
}

int hec_gpu_reconstruct_some_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs,
                                    const uint32_t* h_want_masks, uint32_t n_stripes, uint32_t* d_bad_stripes,
                                    void* stream) {
    // the ragged reconstruct's checks, in its order: a null want list fails with its null descriptor list
    if (rs && d_base && n_stripes && !h_want_masks) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    return hec::gpu_ragged(rs, d_base, descs, n_stripes, true, d_bad_stripes, static_cast<hipStream_t>(stream),
                           n_stripes ? h_want_masks : nullptr);
}

int hec_gpu_verify_ragged(const hec_rs_t* rs, const uint8_t* d_base, const hec_stripe_desc* descs,
                          uint32_t n_stripes, uint32_t* d_check, uint32_t* d_bad_stripes, uint32_t* d_unchecked,
                          void* stream) {
    hec::ScrubOut out;
    out.words = d_check;
    out.bad = d_bad_stripes;
    out.unchecked = d_unchecked;
    return hec::gpu_ragged_scrub(rs, const_cast<uint8_t*>(d_base) /* only read */, descs, n_stripes, hec::Pass2::None,
                                 2, out, nullptr, static_cast<hipStream_t>(stream));
}

int hec_gpu_locate_corrupt_ragged(const hec_rs_t* rs, const uint8_t* d_base, const hec_stripe_desc* descs,
                                  uint32_t n_stripes, uint32_t* d_check, uint32_t* d_suspects,
                                  uint32_t* d_bad_stripes, uint32_t* d_unchecked, void* stream) {
    hec::ScrubOut out;
    out.words = d_check;
    out.suspects = d_suspects;
    out.bad = d_bad_stripes;
    out.unchecked = d_unchecked;
    return hec::gpu_ragged_scrub(rs, const_cast<uint8_t*>(d_base) /* only read */, descs, n_stripes,
                                 hec::Pass2::Locate, 2, out, nullptr, static_cast<hipStream_t>(stream));
}

const char* hec_ragged_scrub_kernel_name(const hec_stripe_desc* descs, uint32_t n_stripes) {
    if (n_stripes && !descs) return "invalid argument";
    return hec::ragged_scrub_kernel_name(hec::ragged_scrub_pick(descs, n_stripes).bitslice);
}

const char* hec_ragged_kernel_name(const hec_stripe_desc* descs, uint32_t n_stripes, int decode) {
    if (n_stripes && !descs) return "invalid argument";
    return hec::ragged_name(hec::ragged_pick(descs, n_stripes, decode != 0), decode != 0);
}

}  // extern "C"
