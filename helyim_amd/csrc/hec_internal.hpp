// Internal declarations of libhec, shared by every csrc/*.cpp: the error
// record (errors.cpp), the strided batch view (Strided, Batch), staging
// buffers, the per-device registry and slot leases, the host worker pool
// (host_pool.cpp), plans, per-geometry device state and the launches of a
// plan set or a scrub over a batch (plans.cpp: run_apply, run_some, run_update, run_scrub)
// and the per-call host paths' scratch (host_calls.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hec.h"
#include "gf256.hpp"
#include "rs_kernels.hpp"

struct hec_rs {
    int k = 0, m = 0, n = 0;
    hec::Mat matrix;  // n x k
};

namespace hec {

// Thread-local failure detail (hec_last_error_detail) and the payload of the
// failure (hec_last_error_values): helyim's EcShardError variants carry
// (usize, usize) or an io::Error (helyim-ec/src/errors.rs:55-66), which the C
// ABI's status code alone cannot rebuild.
struct ErrorValues {
    uint64_t a = 0, b = 0;  // UnexpectedEcShardSize(expected, actual), UnexpectedBlockSize(block, buf), Underflow
    int os_errno = 0;       // errno behind an HEC_ERR_IO (0: no OS error, e.g. a short read)
};
void set_detail(const std::string& s);
int fail(int code, const std::string& detail);  // clears the values
int fail_values(int code, const std::string& detail, uint64_t a, uint64_t b);
// detail = what + ": " + strerror(err), os_errno = err
int fail_errno(int code, const std::string& what, int err);
// Re-raise a failure captured on another thread with its values.
int fail_with(int code, const std::string& detail, const ErrorValues& v);
ErrorValues last_error_values();

// First failure among several threads (host-pool workers, the file pipeline's
// reader and writer): failure detail and values are thread-local, so a worker
// captures its own and the caller's thread re-raises them.
struct ErrorSlot {
    std::mutex mu;
    std::atomic<int> code{HEC_OK};
    std::string detail;
    ErrorValues values;
    void set(int c, const std::string& d, const ErrorValues& v = ErrorValues{}) {
        std::lock_guard<std::mutex> lk(mu);
        if (code.load() == HEC_OK) {
            detail = d;
            values = v;
            code.store(c);
        }
    }
    // Record status c of a call that just failed on the calling thread.
    void capture(int c) { set(c, hec_last_error_detail(), last_error_values()); }
    bool failed() const { return code.load() != HEC_OK; }
    // Re-raise the first failure on the calling thread and clear the record
    // (HEC_OK, the thread's record untouched, when there was none).
    int raise() {
        std::lock_guard<std::mutex> lk(mu);
        const int c = code.exchange(HEC_OK);
        if (!c) return HEC_OK;
        fail_with(c, detail, values);
        detail.clear();
        values = ErrorValues{};
        return c;
    }
};

constexpr uint64_t round_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// One [stripe][shard] arena of a strided batch: shard i of stripe st starts at
// base + st * stripe + i * shard.
struct Strided {
    uint8_t* base = nullptr;
    uint64_t stripe = 0, shard = 0;
    Strided from(uint64_t i) const { return Strided{base + i * shard, stripe, shard}; }  // the arena from shard i on
    uint64_t low_bits() const { return uint64_t(reinterpret_cast<uintptr_t>(base)) | stripe | shard; }
};
// An arena the call only reads is viewed through the same struct.
inline Strided arena(const void* base, uint64_t stripe, uint64_t shard) {
    return Strided{static_cast<uint8_t*>(const_cast<void*>(base)), stripe, shard};
}
// A strided batch as the launches see it: n_stripes stripes of len-byte shards,
// read from `in`, written to (a verify: compared with) `out`.
struct Batch {
    Strided in, out;
    uint64_t len = 0;
    uint32_t n_stripes = 0;
    static Batch in_place(const Strided& a, uint64_t len, uint32_t n) { return Batch{a, a, len, n}; }
    static Batch split(const Strided& data, const Strided& parity, uint64_t len, uint32_t n) {
        return Batch{data, parity, len, n};
    }
    // an in-place arena as data shards [0, k) and the parity shards behind them
    static Batch split_at(const Strided& a, int k, uint64_t len, uint32_t n) {
        return Batch{a, a.from(uint64_t(k)), len, n};
    }
    // every base and stride 16-byte aligned: the launches' vector-access kernels
    bool aligned() const { return ((in.low_bits() | out.low_bits()) % 16) == 0; }
};

// Strided-batch geometry sanity (the C ABI sees only pointers, so sizes cannot
// be checked): shards of a stripe and stripes of a shard must not overlap,
// and the batch's byte extent must not wrap the address space.
inline int check_strided(const char* what, uint32_t shards, const Strided& a, uint64_t len, uint32_t n_stripes) {
    if (shards > 1 && a.shard < len)
        return fail(HEC_ERR_INVALID_ARGUMENT, std::string(what) + ": shard stride below shard length");
    if (n_stripes > 1 && a.stripe < len)
        return fail(HEC_ERR_INVALID_ARGUMENT, std::string(what) + ": stripe stride below shard length");
    uint64_t x, y, e;
    if (__builtin_mul_overflow(uint64_t(n_stripes ? n_stripes - 1 : 0), a.stripe, &x) ||
        __builtin_mul_overflow(uint64_t(shards ? shards - 1 : 0), a.shard, &y) ||
        __builtin_add_overflow(x, y, &e) || __builtin_add_overflow(e, len, &e))
        return fail(HEC_ERR_INVALID_ARGUMENT, std::string(what) + ": batch extent overflows");
    return HEC_OK;
}
// Prologue of the strided batch entry points (hec_gpu_*_batch, hec_host_*_batch,
// hec_host_*_batch_multi): the null / empty-shard checks, and an encode's two
// stride checks. What an entry point does between and after them is its own.
inline int check_batch_args(const hec_rs* rs, const void* a, const void* b, uint64_t len) {
    if (!rs || !a || !b) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (len == 0) return fail(HEC_ERR_EMPTY_SHARD, "");
    return HEC_OK;
}
inline int check_batch_args(const hec_rs* rs, const Batch& b) {
    return check_batch_args(rs, b.in.base, b.out.base, b.len);
}
inline int check_encode_strides(const hec_rs* rs, const Batch& b) {
    if (int rc = check_strided("data", uint32_t(rs->k), b.in, b.len, b.n_stripes)) return rc;
    return check_strided("parity", uint32_t(rs->m), b.out, b.len, b.n_stripes);
}
int hip_fail(hipError_t e, const char* what);

// One pwrite of exactly n bytes (the .ecx tombstone, the .ecj append); a
// short write is an error with errno EIO (errno would otherwise be stale).
inline bool pwrite_exact(int fd, const void* p, size_t n, off_t off) {
    const ssize_t w = ::pwrite(fd, p, n, off);
    if (w == ssize_t(n)) return true;
    if (w >= 0) errno = EIO;
    return false;
}

// Propagate a non-zero hec status.
#define HEC_TRY(call)            \
    do {                         \
        int rc_ = (call);        \
        if (rc_) return rc_;     \
    } while (0)

// NUMA placement (numa.cpp): node of a GPU's PCI function (-1 unknown), and
// pinned host memory on the current device's node.
int device_numa_node(int device, int* node);
int pinned_alloc(void** p, size_t bytes);

#define HEC_HIP(call)                                          \
    do {                                                       \
        hipError_t e_ = (call);                                \
        if (e_ != hipSuccess) return ::hec::hip_fail(e_, #call); \
    } while (0)

// Staging buffer of T, in device memory (hipMalloc) or pinned host memory
// (pinned_alloc), grown on demand. No destructor: its owners live for the
// process (a static destructor could run after the HIP runtime is gone);
// owners that do end call release().
template <typename T, bool Pinned>
struct StagingBuf {
    T* p = nullptr;
    size_t cap = 0;  // bytes
    StagingBuf() = default;
    StagingBuf(const StagingBuf&) = delete;
    StagingBuf& operator=(const StagingBuf&) = delete;
    operator T*() const { return p; }
    // At least `bytes`: nothing when it fits; otherwise the old allocation is
    // freed first (the peak is never old + new), then max(bytes, floor) is
    // allocated. Empty (null, cap 0) after a failure.
    int reserve(size_t bytes, size_t floor = 0) {
        if (bytes <= cap) return HEC_OK;
        release();
        const size_t want = std::max(bytes, floor);
        void* q = nullptr;
        if (Pinned) HEC_TRY(pinned_alloc(&q, want));
        else HEC_HIP(hipMalloc(&q, want));
        p = static_cast<T*>(q);
        cap = want;
        return HEC_OK;
    }
    void release() {
        if (p && (Pinned ? hipHostFree(p) : hipFree(p)) != hipSuccess) (void)hipGetLastError();
        p = nullptr;
        cap = 0;
    }
};
template <typename T = uint8_t>
using DeviceBuf = StagingBuf<T, false>;
template <typename T = uint8_t>
using PinnedBuf = StagingBuf<T, true>;
// Buffers sized together (a pipeline's slots): when the last one, allocated
// last, does not fit, all are freed before any is allocated.
template <typename B, size_t N>
int reserve_all(B (&bufs)[N], size_t bytes) {
    if (bytes <= bufs[N - 1].cap) return HEC_OK;
    for (B& b : bufs) b.release();
    for (B& b : bufs) HEC_TRY(b.reserve(bytes));
    return HEC_OK;
}

// Host-side plan list, uploaded as one DevicePlanSet.
struct HostPlans {
    std::vector<DevPlan> plans;
    std::vector<uint32_t> tabs;
    std::vector<uint32_t> idx;
    // > 0: every plan (no-ops included) gets exactly nin * fixed_rows table
    // rows, so plan p's tables start at p * nin * fixed_rows * kTabWords.
    uint32_t fixed_rows = 0;
    // Append a plan: out rows = coefs (nout x nin) over inputs in_ids.
    uint32_t add(const Mat& coefs, const std::vector<uint32_t>& in_ids,
                 const std::vector<uint32_t>& out_ids);
    uint32_t add_noop(uint32_t nin);
};

// Device copy of a HostPlans (+ optional mask LUT).
struct DevicePlanSet {
    DeviceBuf<DevPlan> plans;
    DeviceBuf<uint32_t> tabs, idx, lut;
    bool fast104 = false;  // RS(10,4) set with fixed 4-row tables (rs104_kernel eligible)
    uint32_t lut_bits = 0; // total shards the LUT covers (2^lut_bits entries)
    int upload(const HostPlans& hp, const std::vector<uint32_t>* lut_host, hipStream_t s);
    void release();
};

// Decode plan of one erasure pattern (upstream reconstruct semantics).
// present: n flags. required: n flags, the missing shards worth a row
// (nullptr = all of them; reconstruct_data passes the data shards). Returns
// HEC_OK or TOO_FEW_SHARDS_PRESENT; *noop = true when no row is left.
int decode_plan(const hec_rs* rs, const uint8_t* present, const uint8_t* required, Mat& coefs,
                std::vector<uint32_t>& in_ids, std::vector<uint32_t>& out_ids, bool* noop);

// Per-device state shared by all contexts of one geometry.
struct GeomDevice {
    uint32_t k = 0;              // data shards, fixed per cached geometry (the cache key has k): run_scrub's verify nin
    DevicePlanSet encode;        // plan 0 = encode
    DevicePlanSet decode_dense;  // LUT over all 2^n present masks (n <= 16)
    bool decode_ready = false;
    // RS(10,4) only: the locate kernel's ratio constants as one 3 x 10 plan,
    // row j - 1, input c = P[j][c] / P[0][c] (P = the parity rows; run_scrub)
    DevicePlanSet locate;
    // RS(10,4) only: the pair search's constants (rs_kernels.hpp
    // VerifyArgs::pair_tabs): plan 0 = T, 4 x 4, classical syndromes S = T *
    // syn; plan 1 = 14 rows (alpha_c^2, alpha_c) over the inputs (D, N1)
    DevicePlanSet locate_pairs;
    // RS(10,4) only: the correct kernel's constants (rs_kernels.hpp
    // CorrectArgs::fix_tabs): plan 0 = 1 / P[0][c], 1 x 10; plan 1 = 1 / u_c, 1 x 14
    DevicePlanSet correct;
    // RS(10,4) only, built on first use (ensure_check_plans): the degraded
    // scrub's plans. check: a dense LUT over the 2^14 present masks to one
    // plan per mask with 11 or more shards present (inputs B, outputs E,
    // coefficients A_m, 4-row tables); check_ratio: the same plan ids with the
    // masked locate's ratios A_m[j][c] / A_m[0][c] as 3-row tables; check_fix:
    // the same plan ids with the masked correct's 1 / A_m[0][c] as 1-row tables.
    DevicePlanSet check, check_ratio, check_fix;
    bool check_ready = false;
};
int geom_device(const hec_rs* rs, GeomDevice** out);
int ensure_dense_decode(const hec_rs* rs, GeomDevice* gd, hipStream_t s);
// Check plan of one present mask: in_ids = the first k present shards (B, the
// reconstruct's inputs), out_ids = the other present shards (E), coefs = A_m.
int check_plan(const hec_rs* rs, const uint8_t* present, Mat& coefs, std::vector<uint32_t>& in_ids,
               std::vector<uint32_t>& out_ids);
int ensure_check_plans(const hec_rs* rs, GeomDevice* gd, hipStream_t s);

int current_device(int* dev);

// Completion of one small host call without hipStreamSynchronize: the
// launch's last workgroup stores a sequence number into a pinned host flag
// (signal_done in rs_device.hpp) and the caller spins on it. Measured on
// MI355X (profiles/r02/latency_completion_signal.jsonl): a one-workgroup zero-copy stripe
// completes in 9.2 us this way against 13.3 us through hipStreamSynchronize.
// Owned by a scratch object, so calls on it are serialised by its mutex.
struct Completion {
    uint32_t* host = nullptr;   // pinned, coherent
    uint32_t* dflag = nullptr;  // device address of host
    uint32_t* count = nullptr;  // device word, 0 between launches
    uint32_t seq = 0;
    // Next sequence number, filling the launch arguments' done fields; the
    // signalling launch must go on stream s (or one ordered after it).
    int arm(hipStream_t s, uint32_t** count_out, uint32_t** flag_out, uint32_t* seq_out);
    // Spin on the flag for up to kSpinUs, then fall back to
    // hipStreamSynchronize (a long call, or a GPU busy with other streams);
    // a stream that completes without the flag set is an error.
    int wait(hipStream_t s);
    static constexpr int kSpinUs = 200;
};
// Small host calls signal completion (input bytes at most this); 0 disables.
std::atomic<uint64_t>& completion_flag_max();

// Per-device scratch for host-memory entry points (serialised by mu).
struct Scratch {
    std::mutex mu;
    hipStream_t stream = nullptr;
    DeviceBuf<> dbuf;  // reserved with floor kStagingFloor
    PinnedBuf<> hbuf;  // pinned staging for small calls (one H2D + one D2H), same floor
    DevicePlanSet adhoc;
    Completion done;
    int init();
    void end_call(bool burst);  // a burst slot frees staging above kStagingKeep
};
constexpr size_t kStagingFloor = size_t(16) << 20;
constexpr size_t kMetaFloor = size_t(1) << 20;
// Slots created beyond the first kWarmSlots of a pool (bursts of concurrent
// calls) free their large staging when their call ends (S::end_call), so the
// steady footprint per device is that of kWarmSlots slots, not kScratchSlots:
// a burst of large per-call encodes (say 1 GiB shards: 14 GiB of HBM each)
// must not stay resident in every slot for the life of the process.
constexpr size_t kWarmSlots = 2;
constexpr size_t kStagingKeep = size_t(64) << 20;
// Drains a stream when its scope ends, whatever the return path. For calls
// that queue copies or kernels onto CALLER memory: an error return between
// two enqueues must not leave that work in flight once the caller, told the
// call failed, frees or reuses its buffers. Success paths have synchronised
// already, so the drain finds the stream idle.
struct StreamDrain {
    hipStream_t s;
    ~StreamDrain() {
        if (s && hipStreamSynchronize(s) != hipSuccess) (void)hipGetLastError();
    }
};
// Scratch slots per device: a host call leases one (its own stream, staging
// buffers and completion flag), so concurrent calls from several threads
// overlap on the GPU instead of queueing behind one mutex (SURVEY.md §8b:
// reentrant, a stream per call). Free slots are taken first; a new slot is
// created while fewer than kScratchSlots exist; past that a call waits for
// one. The lease holds the slot's mutex until it is destroyed, and ends the
// call itself: S::end_call(burst slot?) runs with the mutex still held.
constexpr int kScratchSlots = 8;
template <typename S>
struct Lease {
    S* sc = nullptr;
    std::unique_lock<std::mutex> lk;
    size_t index = 0;  // the slot's creation order in its pool
    Lease() = default;
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    S* operator->() const { return sc; }
    ~Lease() {
        if (sc) sc->end_call(index >= kWarmSlots);
    }
};
// Per-device pool of S. S has `std::mutex mu`, `int init()` (called once when
// a slot is created: its streams) and `void end_call(bool burst)`.
template <typename S>
struct SlotPool {
    std::mutex mu;
    std::vector<std::unique_ptr<S>> slots;
    unsigned rr = 0;
    int lease(Lease<S>& out) {
        {
            std::lock_guard<std::mutex> g(mu);
            for (size_t i = 0; i < slots.size(); ++i) {
                std::unique_lock<std::mutex> l(slots[i]->mu, std::try_to_lock);
                if (l.owns_lock()) {
                    out.sc = slots[i].get();
                    out.lk = std::move(l);
                    out.index = i;
                    return 0;
                }
            }
            if (slots.size() < size_t(kScratchSlots)) {
                std::unique_ptr<S> s(new S());
                if (int rc = s->init()) return rc;
                out.lk = std::unique_lock<std::mutex>(s->mu);
                out.sc = s.get();
                out.index = slots.size();
                slots.push_back(std::move(s));
                return 0;
            }
            out.index = rr++ % slots.size();
            out.sc = slots[out.index].get();
        }
        out.lk = std::unique_lock<std::mutex>(out.sc->mu);  // every slot busy: wait for one
        return 0;
    }
};
// One T per device, created on first use and never destroyed (threads and
// HIP resources live for the process). create = false only looks it up.
template <typename T>
T* per_device(int dev, bool create = true) {
    static std::mutex mu;
    static auto* reg = new std::map<int, T*>();
    std::lock_guard<std::mutex> lk(mu);
    auto it = reg->find(dev);
    if (it != reg->end()) return it->second;
    return create ? (*reg)[dev] = new T() : nullptr;
}
// Lease a slot of the calling thread's current device.
template <typename S>
int lease_slot(Lease<S>& out) {
    int dev;
    HEC_TRY(current_device(&dev));
    return per_device<SlotPool<S>>(dev)->lease(out);
}

// Zero-copy switch (hec_set_host_zero_copy): pinned host memory the GPU can
// address is coded by the kernels in place over PCIe instead of being copied.
std::atomic<bool>& zero_copy_enabled();
// Device address of a hipHostMalloc'd pinned buffer (nullptr if unavailable).
uint8_t* pinned_device_ptr(void* host);

// Host calls whose k * shard_len input is at most this many bytes go through
// pinned staging (one H2D, one D2H) instead of one pageable copy per shard.
std::atomic<uint64_t>& host_staging_max();

// Batched RS(10,4) reconstruct of independent stripes through pinned compact
// staging and one rs104_ragged_kernel launch (intervals.cpp). Job j has shard
// length len and present mask; the decode reads its first 10 present shards,
// which fill(j, slot, shard, dst) writes (len bytes) straight into staging
// (non-zero return = that status aborts the call); take(j, shard, src) then
// receives every erased shard named in want (bits of present shards mean
// nothing; a job that wants none of its erased shards takes part in nothing).
// Only those are laid out, computed and stored: when some job wants fewer than
// it lost, the launch is the ragged reconstruct-some kernel, else today's
// decode. fill / take run on up to 16 threads (io_bound_fill: fill does
// preads, worth threads at smaller sizes).
struct CompactJob {
    uint64_t len;
    uint32_t mask;
    uint32_t want = 0xFFFFFFFFu;
};
using CompactFill = std::function<int(size_t job, int slot, int shard, uint8_t* dst)>;
using CompactTake = std::function<void(size_t job, int shard, const uint8_t* src)>;
int compact_reconstruct_104(const hec_rs* rs, const std::vector<CompactJob>& jobs, const CompactFill& fill,
                            const CompactTake& take, bool io_bound_fill = false);

// Batched RS(10,4) update of independent stripes through the same compact
// staging and one rs104_ragged_update_kernel<false, true> launch
// (intervals.cpp; hec.h hec_rs_update_batch is the contract). Job j has shard
// length len (1 .. 2^32 - 1) and a non-empty update mask; shards / new_data are
// hec_rs_update's arrays of that stripe, already checked. The deltas old ^ new
// of the changed shards are packed at their rank in the mask, the four parity
// shards behind them; the updated parity is copied back into shards[10..13].
// Synchronous, error returns included.
struct UpdateJob {
    uint64_t len;
    uint32_t mask;
    uint8_t* const* shards;
    const uint8_t* const* new_data;
};
int compact_update_104(const hec_rs* rs, const std::vector<UpdateJob>& jobs);

// Run fn(i) for i in [0, n) on a persistent host worker pool of the calling
// thread's current device (host memcpy of staging): up to 16 threads, at
// least 1 MiB of `bytes` per thread and 4 MiB in all (below that, waking
// workers costs more than the copy saves: measured at 256 KiB shards,
// tools/bench_latency.py). Each device has up to 2 pools; concurrent callers
// do not wait for each other: a call that finds every pool of its device
// busy runs serially on its own thread.
void pool_run(size_t n, unsigned max_threads, const std::function<void(size_t)>& fn);

// Same pool for I/O-bound tasks (pread / fill callbacks): syscalls gain from
// threads at smaller sizes than memcpy, so >= 128 KiB per thread.
template <typename F>
void parallel_io_for(size_t n, uint64_t bytes, F fn) {
    const unsigned nt = unsigned(std::min<uint64_t>(16, bytes >> 17));
    if (nt <= 1 || n < 2) {
        for (size_t i = 0; i < n; ++i) fn(i);
        return;
    }
    pool_run(n, nt, std::function<void(size_t)>(fn));
}

template <typename F>
void parallel_for(size_t n, uint64_t bytes, F fn) {
    const unsigned nt = unsigned(std::min<uint64_t>(16, std::max<uint64_t>(1, bytes >> 20)));  // >= 1 MiB/thread
    if (nt <= 1 || n < 2 || bytes < (uint64_t(4) << 20)) {
        for (size_t i = 0; i < n; ++i) fn(i);
        return;
    }
    pool_run(n, nt, std::function<void(size_t)>(fn));
}

// Run one plan set over a strided batch (plan 0 for every stripe unless masks).
// done (optional): the launch signals it (Completion::arm) when it finishes.
// over_pcie: an encode whose buffers are host memory (zero copy).
int run_apply(const DevicePlanSet& ps, uint32_t nin, const Batch& b, const uint32_t* masks, uint32_t* bad,
              hipStream_t s, Completion* done = nullptr, bool over_pcie = false);

// Reconstruct some over a strided in-place RS(10,4) batch (hec.h
// hec_gpu_reconstruct_some_batch is the contract), asynchronously on s. ps:
// the dense decode set (ensure_dense_decode first). wants == nullptr means
// "all": run_apply's decode of any codec (nin inputs), launch for launch.
int run_some(const DevicePlanSet& ps, uint32_t nin, const Batch& b, const uint32_t* masks, const uint32_t* wants,
             uint32_t* bad, hipStream_t s);
// Prologue of the reconstruct-some batch entry points: nulls, the empty shard,
// the codec, the layout. All before device work.
inline int check_some_args(const hec_rs* rs, const Batch& b, const void* masks, const void* wants) {
    if (!rs || !b.in.base || !masks || !wants) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (b.len == 0) return fail(HEC_ERR_EMPTY_SHARD, "");
    if (rs->k != 10 || rs->m != 4)
        return fail(HEC_ERR_INVALID_ARGUMENT, "batched reconstruct some is RS(10,4) only");
    return check_strided("shards", uint32_t(rs->n), b.in, b.len, b.n_stripes);
}

// Update over a strided RS(10,4) batch (hec.h hec_gpu_update_batch is the
// contract), asynchronously on s: parity ^= P[:,U] * (old[U] ^ new[U]) with U
// from masks (device words). enc: the RS(10,4) encode set. old.base == nullptr:
// old is zero. b.in = the new data arena, b.out = the parity arena.
int run_update(const DevicePlanSet& enc, const Strided& old, const Batch& b, const uint32_t* masks, hipStream_t s,
               Completion* done = nullptr);
// Prologue of the update batch entry points: nulls, the empty shard, the
// codec, the layouts (the old arena only when given). All before device work.
inline int check_update_args(const hec_rs* rs, const Strided& old, const Batch& b, const void* masks) {
    if (!rs || !b.in.base || !b.out.base || !masks) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (b.len == 0) return fail(HEC_ERR_EMPTY_SHARD, "");
    if (rs->k != 10 || rs->m != 4) return fail(HEC_ERR_INVALID_ARGUMENT, "batched update is RS(10,4) only");
    if (old.base) HEC_TRY(check_strided("old data", uint32_t(rs->k), old, b.len, b.n_stripes));
    HEC_TRY(check_strided("new data", uint32_t(rs->k), b.in, b.len, b.n_stripes));
    return check_strided("parity", uint32_t(rs->m), b.out, b.len, b.n_stripes);
}

// The scrub of a strided batch, asynchronously on s with no host
// synchronisation and no allocation: pass 1 finds the bad stripes, pass 2
// (optional) reads only those again.
// Pass 1, masks == nullptr: the stored parity (b.out) is verified against gd's
// encode plan over b.in, any codec with at most 32 parity shards (the caller
// checks): bit j of words[st] is set when parity shard j of stripe st differs
// within its len bytes. len is the true shard length, never a rounded-up one:
// pad bytes would be compared. Pass 1 with masks: the masked check of an
// in-place RS(10,4) batch over gd's check plans (ensure_check_plans first;
// hec.h hec_gpu_verify_present_batch is the contract of words).
// Pass 2 is RS(10,4) only (the caller checks the codec). Locate names the wrong
// shards of each flagged stripe in suspects (hec.h hec_gpu_locate_corrupt_batch,
// with masks hec_gpu_locate_corrupt_present_batch); pairs: two shards per
// column (full masks only). Correct also fixes the columns it explains in
// place (hec_gpu_correct_batch; with masks, in stripes with min_spares or more
// spare shards: hec_gpu_correct_present_batch).
enum class Pass2 { None, Locate, Correct };
struct ScrubSpec {
    const uint32_t* masks = nullptr;  // device words, one present mask per stripe
    Pass2 pass2 = Pass2::None;
    bool pairs = false;
    uint32_t min_spares = 2;
};
// What a scrub writes, device memory all. words and (with a pass 2) suspects:
// one word per stripe, cleared on s before the kernels OR bits in. The rest
// are optional counters, accumulated: bad += stripes with a non-zero word,
// unchecked += stripes without a spare shard (masked pass 1), left += stripes
// pass 2 could not correct, corrected_bytes += bytes changed.
struct ScrubOut {
    uint32_t* words = nullptr;
    uint32_t* suspects = nullptr;
    uint32_t* bad = nullptr;
    uint32_t* unchecked = nullptr;
    uint32_t* left = nullptr;
    unsigned long long* corrected_bytes = nullptr;
};
int run_scrub(const GeomDevice& gd, const Batch& b, const ScrubSpec& spec, const ScrubOut& out, hipStream_t s);
// The verify entry points' extra argument checks, after check_batch_args.
inline int check_verify_args(const hec_rs* rs, const void* mismatch) {
    if (!mismatch) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (rs->m > 32)
        return fail(HEC_ERR_INVALID_ARGUMENT, "verify needs at most 32 parity shards (one result bit each)");
    return HEC_OK;
}
// The locate entry points' extra argument checks, after check_verify_args.
inline int check_locate_args(const hec_rs* rs, const void* suspects) {
    if (!suspects) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (rs->k != 10 || rs->m != 4)
        return fail(HEC_ERR_INVALID_ARGUMENT, "locate and repair are RS(10,4) only");
    return HEC_OK;
}
inline int check_min_spares(uint32_t min_spares) {
    if (min_spares < 2 || min_spares > 4) return fail(HEC_ERR_INVALID_ARGUMENT, "min_spares must be 2, 3 or 4");
    return HEC_OK;
}
// Prologue of the masked entry points: nulls, the empty shard, the codec, the
// layout. All before device work.
inline int check_present_args(const hec_rs* rs, const Batch& b, const void* masks, const void* check) {
    if (!rs || !b.in.base || !masks || !check) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (b.len == 0) return fail(HEC_ERR_EMPTY_SHARD, "");
    if (rs->k != 10 || rs->m != 4)
        return fail(HEC_ERR_INVALID_ARGUMENT, "masked verify, locate and checked reconstruct are RS(10,4) only");
    return check_strided("shards", uint32_t(rs->n), b.in, b.len, b.n_stripes);
}

}  // namespace hec
