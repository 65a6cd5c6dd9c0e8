// Scrub of a volume's shard files base.ec00 .. base.ec13 (hec_verify_ec_files,
// and hec_locate_corrupt_ec_files: the same walk with the locate pass, which
// also names the wrong shard file of each bad block;
// hec_locate_corrupt_pairs_ec_files: that walk naming two files per column; and
// hec_locate_corrupt_ec_files_present: that walk over a degraded volume, its
// missing files treated as erased shards; hec_correct_ec_files and its pairs
// form: the locate walk with the correct pass, whose fixes are written back;
// hec_correct_ec_files_present: the degraded walk with the masked correct pass).
//
// RS parity is bytewise: byte o of every parity file is a function of byte o
// of the ten data files, whatever large / small block geometry laid the .dat
// out over them. The scrub therefore treats the 14 files as 14 equal-length
// byte streams cut into column blocks of block_size bytes, and needs no
// geometry. Chunks of whole blocks are pread into two pinned slots (shard
// major: [14][chunk columns]); the verify kernels read a slot in place over
// PCIe while the preads of the next chunk fill the other slot, and only one
// word per block comes back. The files are opened read-only, except by the
// correct calls: their kernel fixes the slot in place (its stores cross PCIe
// like the zero-copy encode's) and the changed rows of each bad block are
// written back to their files.
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cstdio>
#include <cstring>

#include "file_util.hpp"
#include "host_chunks.hpp"  // kChunkCols per shard of one chunk, kReadPiece per pread task

namespace hec {
namespace {

constexpr int K = 10, M = 4, N = 14;

// One slot of the per-device pool of scrubs (SlotPool): its stream, the two
// pinned chunk slots and the result words of each.
struct Scrub {
    std::mutex mu;
    hipStream_t stream = nullptr;
    PinnedBuf<> slot[2];
    DeviceBuf<uint32_t> words_dev[2];
    DeviceBuf<uint32_t> masks_dev;  // degraded scrub: the volume's present mask, one word per block of a chunk
    PinnedBuf<uint32_t> words_host[2];
    hipEvent_t done[2] = {};
    int init() {
        HEC_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
        for (auto& e : done) HEC_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        return HEC_OK;
    }
    int reserve(size_t slot_bytes, size_t n_words) {
        HEC_TRY(reserve_all(slot, slot_bytes));
        HEC_TRY(reserve_all(words_dev, n_words * 4));
        return reserve_all(words_host, n_words * 4);
    }
    void end_call(bool burst) {
        if (stream && hipStreamSynchronize(stream) != hipSuccess) (void)hipGetLastError();
        if (!burst) return;
        for (auto& s : slot) s.release();
    }
    ~Scrub() {  // only a slot whose init() failed is ever destroyed
        if (stream) (void)hipStreamDestroy(stream);
        for (auto e : done)
            if (e) (void)hipEventDestroy(e);
    }
};

// n bytes of fd at off into dst; a file that ends early is a short read
// (HEC_ERR_IO without an OS error).
void read_exact(ErrorSlot& err, int fd, const std::string& name, uint8_t* dst, uint64_t n, uint64_t off) {
    const ssize_t got = pread_full(fd, dst, n, off);
    if (got < 0)
        io_error(err, "read " + name);
    else if (uint64_t(got) < n)  // the offset where the file ended
        err.set(HEC_ERR_IO, "short read of " + name + " at offset " + std::to_string(off + uint64_t(got)));
}

enum class ScrubMode { Verify, Locate, LocatePairs, Correct, CorrectPairs };

// Every launch is one run_scrub whose ScrubSpec is fixed before the chunk loop.
// mode Locate / LocatePairs: pass 2 is the locate (LocatePairs: with the pair
// search), a chunk's suspects words follow its mismatch words at +per_chunk in
// the same result buffers, and the bad blocks go to sus[] with their suspects
// word instead of to bad[].
// mode Correct / CorrectPairs: the files are opened for writing, pass 2 is the
// correct, and once a chunk's event has fired each bad block's rows of the
// shards its suspects word names are written back at the block's offset: the
// only bytes of any file that are written. Every file written is fdatasync'ed
// once before the return.
// degraded (with locate): a missing file is an erased shard, not an error; its
// row of a slot is neither read into nor read by the kernels, pass 1 is the
// masked check with the volume's present mask, and the words are the masked
// calls' (shard-index bits). *present_out (optional) = the files found.
// degraded with mode Correct (hec_correct_ec_files_present): the present files
// are opened for writing and pass 2 is the masked correct with min_spares, a
// named row is written back as above (the kernel names present shards only);
// a volume with fewer spare files is only located.
int verify_ec_files_impl(const std::string& base, uint64_t block, ScrubMode mode, hec_scrub_bad* bad,
                         hec_scrub_suspect* sus, size_t cap, size_t* n_bad, uint64_t* n_blocks,
                         bool degraded = false, uint32_t* present_out = nullptr, uint32_t min_spares = 2) {
    const bool locate = mode != ScrubMode::Verify;
    bool correct = mode == ScrubMode::Correct || mode == ScrubMode::CorrectPairs;
    const bool pairs = mode == ScrubMode::LocatePairs || mode == ScrubMode::CorrectPairs;
    // files and sizes first: these failures need no device
    Fd fd[N];
    std::string names[N];
    uint64_t size = 0;
    uint32_t present = 0;
    for (int i = 0; i < N; ++i) {
        names[i] = shard_name(base, i);
        fd[i].fd = ::open(names[i].c_str(), correct ? O_RDWR : O_RDONLY);
        if (fd[i].fd < 0) {
            if (errno == ENOENT && degraded) continue;
            if (errno == ENOENT) return fail(HEC_ERR_SHARD_NOT_FOUND, "no shard file " + names[i]);
            return fail_errno(HEC_ERR_IO, "open " + names[i], errno);
        }
        present |= 1u << i;
    }
    if (present_out) *present_out = present;
    const int n_present = __builtin_popcount(present);
    if (n_present == 0) return fail(HEC_ERR_SHARD_NOT_FOUND, "no shard file " + names[0] + " .. " + names[N - 1]);
    if (n_present <= K)
        return fail(HEC_ERR_TOO_FEW_SHARDS_PRESENT, std::to_string(n_present) + " of " + std::to_string(N) +
                                                        " shard files present, the check needs at least " +
                                                        std::to_string(K + 1));
    if (degraded && correct && uint32_t(n_present - K) < min_spares) correct = false;  // too few spares: the locate
    const int first_present = __builtin_ctz(present);
    for (int i = 0; i < N; ++i) {
        if (fd[i].fd < 0) continue;
        struct stat st;
        if (::fstat(fd[i].fd, &st) != 0) return fail_errno(HEC_ERR_IO, "stat " + names[i], errno);
        if (i == first_present) size = uint64_t(st.st_size);
        if (uint64_t(st.st_size) != size)
            return fail_values(HEC_ERR_UNEXPECTED_EC_SHARD_SIZE,
                               "ec shard size expected " + std::to_string(size) + " but actually is " +
                                   std::to_string(st.st_size) + " (" + names[i] + ")",
                               size, uint64_t(st.st_size));
    }
    if (size == 0) return HEC_OK;

    RsGuard codec;
    HEC_TRY(hec_rs_new(K, M, &codec.rs));
    GeomDevice* gd;
    HEC_TRY(geom_device(codec.rs, &gd));
    Lease<Scrub> sc;
    HEC_TRY(lease_slot(sc));
    StreamDrain drain{sc->stream};  // the kernels read the slots: idle before the lease ends, error returns too

    const uint64_t per_chunk = std::max<uint64_t>(1, kChunkCols / block);  // blocks per chunk
    const uint64_t cols = per_chunk * block;                               // columns per chunk
    const uint64_t pitch = round_up(std::min(cols, round_up(size, block)), 256);
    HEC_TRY(sc->reserve(size_t(N) * pitch, size_t(per_chunk) * (locate ? 2 : 1)));
    if (degraded) {
        HEC_TRY(ensure_check_plans(codec.rs, gd, sc->stream));
        // one mask word per block, uploaded once per call
        HEC_TRY(sc->masks_dev.reserve(size_t(per_chunk) * 4));
        HEC_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(sc->masks_dev.p), int(present), size_t(per_chunk),
                                  sc->stream));
    }
    uint8_t* zs[2] = {pinned_device_ptr(sc->slot[0]), pinned_device_ptr(sc->slot[1])};
    if (!zs[0] || !zs[1]) return fail(HEC_ERR_HIP, "pinned scrub slots are not addressable by the device");

    ScrubSpec spec;  // of every launch
    if (degraded) spec.masks = sc->masks_dev;
    spec.pass2 = correct ? Pass2::Correct : locate ? Pass2::Locate : Pass2::None;
    spec.pairs = pairs;
    spec.min_spares = min_spares;

    const uint64_t total_blocks = (size + block - 1) / block;
    const uint64_t n_chunks = (size + cols - 1) / cols;
    size_t found = 0;
    bool written[N] = {};
    auto chunk_len = [&](uint64_t c) { return std::min(cols, size - c * cols); };
    // results of chunk c (its words are in words_host[c & 1] once done[c & 1] fired)
    auto collect = [&](uint64_t c) -> int {
        const int q = int(c & 1);
        HEC_HIP(hipEventSynchronize(sc->done[q]));
        const uint64_t len = chunk_len(c), nb = (len + block - 1) / block;
        for (uint64_t b = 0; b < nb; ++b) {
            const uint32_t w = sc->words_host[q][b];
            if (!w) continue;
            const uint64_t offset = c * cols + b * block;
            const uint32_t length = uint32_t(std::min(block, len - b * block));
            if (found < cap && locate)
                sus[found] = hec_scrub_suspect{offset, length, w, sc->words_host[q][per_chunk + b], 0};
            else if (found < cap)
                bad[found] = hec_scrub_bad{offset, length, w};
            ++found;
            if (!correct) continue;
            // the rows the kernel changed: the shards the block's word names
            const uint32_t named = sc->words_host[q][per_chunk + b] & ((1u << N) - 1);
            for (int i = 0; i < N; ++i) {
                if (!((named >> i) & 1u)) continue;
                const uint8_t* slot = sc->slot[q];
                const uint8_t* row = slot + uint64_t(i) * pitch + b * block;
                if (!pwrite_full(fd[i].fd, row, length, offset)) return io("write " + names[i]);
                written[i] = true;
            }
        }
        return HEC_OK;
    };
    ErrorSlot err;
    for (uint64_t c = 0; c < n_chunks; ++c) {
        const int q = int(c & 1);
        if (c >= 2) HEC_TRY(collect(c - 2));  // the kernel of chunk c - 2 has left this slot
        const uint64_t off = c * cols, len = chunk_len(c);
        const uint64_t pieces = (len + kReadPiece - 1) / kReadPiece;
        uint8_t* h = sc->slot[q];
        parallel_io_for(size_t(N * pieces), uint64_t(N) * len, [&](size_t t) {
            const int i = int(t / pieces);
            if (fd[i].fd < 0) return;  // an erased shard: its row stays unread
            const uint64_t p0 = (t % pieces) * kReadPiece;
            read_exact(err, fd[i].fd, names[i], h + uint64_t(i) * pitch + p0, std::min(kReadPiece, len - p0),
                       off + p0);
        });
        if (err.failed()) return err.raise();
        // whole blocks in one launch, a shorter last block in its own: every
        // launch compares exactly the bytes read, never the slot's stale rest
        const uint64_t full = len / block, tail = len - full * block;
        uint32_t* wd = sc->words_dev[q];
        // n blocks of blen bytes from column `first` of the slot on
        auto launch = [&](uint64_t first, uint64_t blen, uint64_t n) -> int {
            const Strided rows = arena(zs[q] + first * block, block, pitch);
            ScrubOut out;
            out.words = wd + first;
            if (locate) out.suspects = wd + per_chunk + first;
            const Batch b = degraded ? Batch::in_place(rows, blen, uint32_t(n))
                                     : Batch::split_at(rows, K, blen, uint32_t(n));
            return run_scrub(*gd, b, spec, out, sc->stream);
        };
        if (full) HEC_TRY(launch(0, block, full));
        if (tail) HEC_TRY(launch(full, tail, 1));
        const size_t n_words = size_t(full + (tail ? 1 : 0));
        HEC_HIP(hipMemcpyAsync(sc->words_host[q], wd, n_words * 4, hipMemcpyDeviceToHost, sc->stream));
        if (locate)
            HEC_HIP(hipMemcpyAsync(sc->words_host[q] + per_chunk, wd + per_chunk, n_words * 4, hipMemcpyDeviceToHost,
                                   sc->stream));
        HEC_HIP(hipEventRecord(sc->done[q], sc->stream));
    }
    if (n_chunks >= 2) HEC_TRY(collect(n_chunks - 2));
    HEC_TRY(collect(n_chunks - 1));
    for (int i = 0; i < N; ++i)
        if (written[i] && ::fdatasync(fd[i].fd) != 0) return io("sync " + names[i]);
    if (n_bad) *n_bad = found;
    if (n_blocks) *n_blocks = total_blocks;
    return HEC_OK;
}

}  // namespace
}  // namespace hec

extern "C" {

// The entry points' shared prologue, then the walk. Exactly one of bad and sus
// may be there: the result array.
static int scrub_files(const char* base_filename, uint64_t block_size, hec::ScrubMode mode, hec_scrub_bad* bad,
                       hec_scrub_suspect* sus, size_t cap, size_t* n_bad, uint64_t* n_blocks, bool degraded = false,
                       uint32_t* present_mask = nullptr, uint32_t min_spares = 2) {
    if (present_mask) *present_mask = 0;
    if (n_bad) *n_bad = 0;
    if (n_blocks) *n_blocks = 0;
    if (!base_filename || (cap && !bad && !sus)) return hec::fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    const uint64_t block = block_size ? block_size : HEC_SMALL_BLOCK_SIZE;
    if (block % 4096 != 0 || block > 0xFFFFF000ull)
        return hec::fail(HEC_ERR_INVALID_ARGUMENT, "block_size must be a multiple of 4096 below 4 GiB");
    HEC_TRY(hec::check_min_spares(min_spares));
    return hec::verify_ec_files_impl(base_filename, block, mode, bad, sus, cap, n_bad, n_blocks, degraded, present_mask,
                                     min_spares);
}

int hec_verify_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_bad* bad, size_t cap, size_t* n_bad,
                        uint64_t* n_blocks) {
    return scrub_files(base_filename, block_size, hec::ScrubMode::Verify, bad, nullptr, cap, n_bad, n_blocks);
}

int hec_locate_corrupt_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad, size_t cap,
                                size_t* n_bad, uint64_t* n_blocks) {
    return scrub_files(base_filename, block_size, hec::ScrubMode::Locate, nullptr, bad, cap, n_bad, n_blocks);
}

int hec_locate_corrupt_pairs_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad,
                                      size_t cap, size_t* n_bad, uint64_t* n_blocks) {
    return scrub_files(base_filename, block_size, hec::ScrubMode::LocatePairs, nullptr, bad, cap, n_bad, n_blocks);
}

int hec_correct_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad, size_t cap,
                         size_t* n_bad, uint64_t* n_blocks) {
    return scrub_files(base_filename, block_size, hec::ScrubMode::Correct, nullptr, bad, cap, n_bad, n_blocks);
}

int hec_correct_pairs_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad, size_t cap,
                               size_t* n_bad, uint64_t* n_blocks) {
    return scrub_files(base_filename, block_size, hec::ScrubMode::CorrectPairs, nullptr, bad, cap, n_bad, n_blocks);
}

int hec_locate_corrupt_ec_files_present(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad,
                                        size_t cap, size_t* n_bad, uint64_t* n_blocks, uint32_t* present_mask) {
    return scrub_files(base_filename, block_size, hec::ScrubMode::Locate, nullptr, bad, cap, n_bad, n_blocks, true,
                       present_mask);
}

int hec_correct_ec_files_present(const char* base_filename, uint64_t block_size, uint32_t min_spares,
                                 hec_scrub_suspect* bad, size_t cap, size_t* n_bad, uint64_t* n_blocks,
                                 uint32_t* present_mask) {
    return scrub_files(base_filename, block_size, hec::ScrubMode::Correct, nullptr, bad, cap, n_bad, n_blocks, true,
                       present_mask, min_spares);
}

}  // extern "C"
