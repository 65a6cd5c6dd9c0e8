// Chunk sizes of the host layer's staging loops: how much of a host batch
// (host_pipeline.cpp) or of a volume's shard files (verify_files.cpp) goes
// through one reusable staging slot at a time.
// HEC_HOST_CHUNK_BYTES / HEC_SCRUB_CHUNK_COLS / HEC_SCRUB_READ_PIECE: test
// builds only (the Makefile's smallchunk variant), so that host batches and
// volumes of a few hundred KiB go in many chunks, reuse every slot and stream
// and end in a short chunk. The shipped library defines none of them. Only
// host_pipeline.cpp and verify_files.cpp read these constants, the two files
// that variant recompiles.
#pragma once
#include <cstdint>

namespace hec {

#ifdef HEC_HOST_CHUNK_BYTES
constexpr uint64_t kChunkBytes = HEC_HOST_CHUNK_BYTES;
#else
constexpr uint64_t kChunkBytes = 96ull << 20;  // target bytes of one chunk's shards (all n of every stripe)
#endif
#ifdef HEC_SCRUB_CHUNK_COLS
constexpr uint64_t kChunkCols = HEC_SCRUB_CHUNK_COLS;
#else
constexpr uint64_t kChunkCols = 4ull << 20;  // target bytes per shard of one chunk (14 x that per slot)
#endif
#ifdef HEC_SCRUB_READ_PIECE
constexpr uint64_t kReadPiece = HEC_SCRUB_READ_PIECE;
#else
constexpr uint64_t kReadPiece = 1ull << 20;  // bytes of one pread task
#endif
static_assert(kChunkBytes >= 1 && kChunkCols >= 1 && kReadPiece >= 1, "a chunk and a read hold at least one byte");

#if defined(HEC_HOST_CHUNK_BYTES) || defined(HEC_SCRUB_CHUNK_COLS) || defined(HEC_SCRUB_READ_PIECE)
#define HEC_TEST_HOST_CHUNKS 1  // host_pipeline.cpp exports hec_test_host_chunk_limits
#endif

}  // namespace hec
