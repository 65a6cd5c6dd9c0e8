/*
 * hec.h -- C ABI of the MI355X-native RS(10,4) erasure-coding engine that
 * replaces helyim-ec's CPU path (libhec.so, built for gfx950).
 *
 * Every entry point takes plain pointers and sizes. Each one names the
 * reference interface it replaces (paths relative to /root/reference):
 *
 *  - the arithmetic boundary: reed_solomon_erasure::ReedSolomon<galois_8::Field>
 *    {new, encode, reconstruct} as called at helyim-ec/src/encoder.rs:191,
 *    208-209, 249-250, 288 and helyim-store/src/erasure_coding/mod.rs:411-412,
 *    426 (crate 6.0.0, git helyim/reed-solomon-erasure, Cargo.toml:72);
 *  - the crate API boundary: helyim_ec::write_ec_files / rebuild_ec_files
 *    (helyim-ec/src/encoder.rs:39-50, exported at helyim-ec/src/lib.rs:17),
 *    called by helyim-store/src/server.rs:468 and :497.
 *
 * All compute runs on the GPU through HIP kernels. There is no CPU fallback:
 * without a usable GPU every compute entry point returns HEC_ERR_NO_DEVICE or
 * HEC_ERR_HIP.
 *
 * Threading: a hec_rs_t is immutable after hec_rs_new and may be shared by
 * threads (upstream ReedSolomon is Send + Sync). Device state (tables,
 * decode-pattern cache, staging buffers) is per device and mutex guarded.
 * Host-memory entry points synchronise before returning, on error returns
 * too (no copy or kernel touching caller memory is left in flight); the
 * hec_gpu_* batch entry points are asynchronous on the caller's stream.
 */
#ifndef HEC_H
#define HEC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes -------------------------------------------------------
 * 1..13 are 1:1 with reed_solomon_erasure::Error (declaration order);
 * 32..35 with helyim_ec::EcShardError (helyim-ec/src/errors.rs:55-66);
 * 64.. are device / argument errors of this library. */
enum hec_status {
    HEC_OK = 0,
    HEC_ERR_TOO_FEW_SHARDS = 1,
    HEC_ERR_TOO_MANY_SHARDS = 2,
    HEC_ERR_TOO_FEW_DATA_SHARDS = 3,
    HEC_ERR_TOO_MANY_DATA_SHARDS = 4,
    HEC_ERR_TOO_FEW_PARITY_SHARDS = 5,
    HEC_ERR_TOO_MANY_PARITY_SHARDS = 6,
    HEC_ERR_TOO_FEW_BUFFER_SHARDS = 7,
    HEC_ERR_TOO_MANY_BUFFER_SHARDS = 8,
    HEC_ERR_INCORRECT_SHARD_SIZE = 9,
    HEC_ERR_TOO_FEW_SHARDS_PRESENT = 10,
    HEC_ERR_EMPTY_SHARD = 11,
    HEC_ERR_INVALID_SHARD_FLAGS = 12,
    HEC_ERR_INVALID_INDEX = 13,
    HEC_ERR_IO = 32,                      /* EcShardError::Io */
    HEC_ERR_UNDERFLOW = 33,               /* EcShardError::Underflow */
    HEC_ERR_UNEXPECTED_EC_SHARD_SIZE = 34,/* EcShardError::UnexpectedEcShardSize */
    HEC_ERR_UNEXPECTED_BLOCK_SIZE = 35,   /* EcShardError::UnexpectedBlockSize */
    HEC_ERR_NEEDLE_NOT_FOUND = 48,        /* EcVolumeError::NeedleNotFound */
    HEC_ERR_SHARD_NOT_FOUND = 49,         /* EcVolumeError::ShardNotFound */
    HEC_ERR_HIP = 64,                     /* a HIP runtime call failed */
    HEC_ERR_NO_DEVICE = 65,               /* no usable GPU */
    HEC_ERR_INVALID_ARGUMENT = 66,        /* null pointer, bad stride, ... */
    HEC_ERR_OUT_OF_MEMORY = 67
};

/* Static text for a status code (the upstream Display string where one exists). */
const char* hec_strerror(int status);
/* Thread-local detail of the last failure on this thread (e.g. the errno text,
 * the two sizes of UnexpectedEcShardSize). Empty string when none. */
const char* hec_last_error_detail(void);
/* Payload of the last failure on this thread, so a binding can rebuild the
 * reference's error values (helyim-ec/src/errors.rs:55-66), not only its
 * variant: *a / *b = the two usizes of UnexpectedEcShardSize(expected, actual)
 * (encoder.rs:276-279) and UnexpectedBlockSize(block_size, buf_size)
 * (encoder.rs:140-143); *os_errno = the errno behind an HEC_ERR_IO (the
 * io::Error of EcShardError::Io, encoder.rs:175 -- 0 when the failure had no OS
 * error, e.g. a short read). Meaningful right after a call returned one of
 * codes 32..35 (every such return sets all three; 0 where the variant has no
 * such value); other statuses may leave stale values. Null pointers are
 * skipped. Returns HEC_OK. */
int hec_last_error_values(uint64_t* a, uint64_t* b, int* os_errno);

/* ---- device selection (no reference counterpart: helyim has no GPU) -------
 * Every entry point works on the calling thread's current HIP device. A
 * multi-GPU volume server that does not link HIP itself picks the device per
 * call with these, e.g. volume_id % count before hec_write_ec_files (whole
 * volumes per GPU); per-device state is independent, so calls
 * on different devices run concurrently. */
int hec_device_count(int* count);  /* HEC_ERR_NO_DEVICE (and 0) without a GPU */
int hec_set_device(int device);    /* this thread only; HEC_ERR_INVALID_ARGUMENT if out of range */
int hec_get_device(int* device);

/* ---- NUMA placement of the host side of a GPU (no reference
 * counterpart: helyim is CPU-only) -------------------------------------------
 * Every pinned buffer libhec allocates (host-batch and file-layer staging,
 * small-call staging, degraded-read staging) lives on the NUMA node of the
 * device it serves. */
/* sysfs NUMA node of the device's PCI function; -1 when the platform does not
 * say. */
int hec_device_numa_node(int device, int* node);
/* Restrict the calling thread (and threads it creates later) to the CPUs of
 * the device's NUMA node that it is allowed to run on; *n_cpus (optional) =
 * how many. No-op (HEC_OK, 0 CPUs) when the node is unknown or none of its
 * CPUs is in the thread's allowed set. */
int hec_bind_thread_to_device(int device, int* n_cpus);
/* Pinned host memory on the current device's NUMA node, addressable by the
 * GPU (host-batch entry points code it zero-copy). Free with hec_host_free. */
int hec_host_alloc(size_t bytes, void** out);
/* One pinned host batch of n_stripes * stripe_stride bytes for the _multi
 * calls over the same device list: range r = stripes [S*r/R, S*(r+1)/R)
 * (R = min(n_devices, n_stripes), the split hec_host_*_batch_multi uses) has
 * its pages preferred on devices[r]'s NUMA node (mbind before the first
 * touch; a page straddling two ranges goes with the earlier one), so on a
 * two-socket node every GPU's range is read and written on its own socket.
 * Zero-filled, pinned and mapped for every device (zero-copy for any range).
 * Placement is speed only: a node short of memory spills to the others.
 * Free with hec_host_free. Errors: HEC_ERR_INVALID_ARGUMENT (empty list, > 256
 * entries, a device out of range, empty or overflowing batch). */
int hec_host_alloc_multi(const int* devices, size_t n_devices, uint64_t stripe_stride, uint32_t n_stripes,
                         void** out);
int hec_host_free(void* p);
/* NUMA node holding the page at p (diagnostic; HEC_ERR_IO if not resident). */
int hec_host_numa_node(const void* p, int* node);

/* ---- geometry constants (helyim-ec/src/lib.rs:46-50) ---------------------- */
#define HEC_DATA_SHARDS_COUNT 10u
#define HEC_PARITY_SHARDS_COUNT 4u
#define HEC_TOTAL_SHARDS_COUNT 14u
#define HEC_LARGE_BLOCK_SIZE (1024ull * 1024ull * 1024ull)
#define HEC_SMALL_BLOCK_SIZE (1024ull * 1024ull)

/* ---- codec context: replaces ReedSolomon<galois_8::Field> ----------------- */
typedef struct hec_rs hec_rs_t;

/* ReedSolomon::new(data_shards, parity_shards) (encoder.rs:208-209).
 * Errors: TOO_FEW_DATA_SHARDS (0 data), TOO_FEW_PARITY_SHARDS (0 parity),
 * TOO_MANY_SHARDS (data + parity > 256). */
int hec_rs_new(size_t data_shards, size_t parity_shards, hec_rs_t** out);
void hec_rs_free(hec_rs_t* rs);
size_t hec_rs_data_shard_count(const hec_rs_t* rs);
size_t hec_rs_parity_shard_count(const hec_rs_t* rs);
size_t hec_rs_total_shard_count(const hec_rs_t* rs);
/* Copies the (total x data) row-major encoding matrix into out. */
int hec_rs_matrix(const hec_rs_t* rs, uint8_t* out, size_t out_len);

/* ReedSolomon::encode(&mut shards) (encoder.rs:191), host memory.
 * shards[0..data) are read, shards[data..total) receive parity in place.
 * shard_lens[i] is the length of shards[i]. Errors: TOO_FEW_SHARDS /
 * TOO_MANY_SHARDS (n_shards != total), EMPTY_SHARD, INCORRECT_SHARD_SIZE. */
int hec_rs_encode(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                  size_t n_shards);

/* ReedSolomon::verify(&shards): *ok = 1 when the parity matches the data. */
int hec_rs_verify(const hec_rs_t* rs, const uint8_t* const* shards, const size_t* shard_lens,
                  size_t n_shards, int* ok);

/* ReedSolomon::reconstruct(&mut [Option<Vec<u8>>]) (encoder.rs:288,
 * erasure_coding/mod.rs:426). present[i] != 0 marks Some(shard); shard_lens
 * of absent slots are ignored. Absent slots must point at a caller buffer of
 * the common shard length (upstream allocates vec![0; len]); they are filled.
 * All present -> no-op. Errors: TOO_FEW_SHARDS / TOO_MANY_SHARDS,
 * EMPTY_SHARD, INCORRECT_SHARD_SIZE, TOO_FEW_SHARDS_PRESENT. Decode uses the
 * first data_shards present shards in index order, as upstream does. */
int hec_rs_reconstruct(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                       const uint8_t* present, size_t n_shards);
/* ReedSolomon::reconstruct_data: as above but absent parity slots are left
 * untouched. */
int hec_rs_reconstruct_data(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                            const uint8_t* present, size_t n_shards);

/* Batched ReedSolomon::reconstruct over n_stripes independent stripes of any
 * lengths in ONE GPU round trip -- the degraded-read path
 * (helyim-store/src/erasure_coding/mod.rs:403-491 reconstructs one needle
 * interval per call). shards / lens / present are n_stripes * total entries,
 * stripe-major; per stripe the semantics and errors are hec_rs_reconstruct's
 * (reconstruct_data when data_only != 0). Every stripe is validated before
 * any work; on error nothing is written and *bad_index (optional) names the
 * first failing stripe. */
int hec_rs_reconstruct_batch(const hec_rs_t* rs, uint8_t* const* shards, const size_t* lens,
                             const uint8_t* present, size_t n_stripes, int data_only, size_t* bad_index);

/* Reconstruct some (klauspost's ReconstructSome; upstream's reconstruct_data
 * is the case "the data shards"): hec_rs_reconstruct with required[i] != 0
 * marking the absent shards worth rebuilding (n_shards flags; flags of
 * present shards mean nothing). Validation and errors are hec_rs_reconstruct's,
 * in its order. An absent slot that is not required may be NULL and is left
 * alone; an absent required slot that is NULL returns
 * HEC_ERR_INVALID_ARGUMENT. Only the required absent shards are computed,
 * stored and copied back. All flags set is hec_rs_reconstruct; the data flags
 * only is hec_rs_reconstruct_data. Any codec. */
int hec_rs_reconstruct_some(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                            const uint8_t* present, const uint8_t* required, size_t n_shards);
/* hec_rs_reconstruct_batch with required flags (n_stripes * total entries,
 * stripe-major) in the place of data_only; per stripe the semantics are
 * hec_rs_reconstruct_some's. */
int hec_rs_reconstruct_some_batch(const hec_rs_t* rs, uint8_t* const* shards, const size_t* lens,
                                  const uint8_t* present, const uint8_t* required, size_t n_stripes,
                                  size_t* bad_index);

/* Update (klauspost's Update): fold changed data shards into the parity
 * without re-encoding. shards: total pointers; shards[i] for i < data is the
 * OLD data shard i, needed only where new_data[i] is non-NULL (the other data
 * slots and their lengths are ignored and may be NULL); shards[data..total)
 * are the parity shards, all required, updated in place: parity[j] ^= sum over
 * the changed c of P[j][c] * (old[c] ^ new[c]). new_data: data pointers, the
 * new bytes of each changed shard (shard_lens[c] bytes), NULL = unchanged; no
 * non-NULL entry: HEC_OK, nothing touched. Neither old nor new shards are
 * written, and the call does not copy new over old. Errors, in this order:
 * null rs / arrays (HEC_ERR_INVALID_ARGUMENT), TOO_FEW_SHARDS /
 * TOO_MANY_SHARDS (n_shards != total), a changed shard without an old buffer
 * or a NULL parity pointer (HEC_ERR_INVALID_ARGUMENT), then EMPTY_SHARD and
 * INCORRECT_SHARD_SIZE over the lengths in use. Any codec. */
int hec_rs_update(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                  const uint8_t* const* new_data, size_t n_shards);

/* Batched hec_rs_update over n_stripes independent stripes of any lengths in
 * ONE GPU round trip, as hec_rs_reconstruct_batch is for degraded reads: the
 * small-write path, byte ranges of a few hundred bytes to a few MiB that each
 * touch one or two data shards. shards / lens are n_stripes * total entries,
 * stripe-major; new_data is n_stripes * data entries. Per stripe the semantics
 * and errors are hec_rs_update's, in its order. Every stripe is validated
 * before any work; on error nothing is written and *bad_index (optional) names
 * the first failing stripe; it is n_stripes on success. A stripe with no
 * non-NULL new_data entry is skipped untouched (and a batch of such stripes
 * needs no device). Null rs, or n_stripes > 0 with a null array:
 * HEC_ERR_INVALID_ARGUMENT; a shard length in use above 2^32 - 1 likewise.
 * RS(10,4): the deltas old ^ new of the changed shards are packed compactly
 * into pinned staging with the four parity shards behind them, one
 * rs104_ragged_update_kernel launch runs over them (in place over PCIe with
 * zero copy, else through one upload and one download), and the parity is
 * copied back. Any other codec: hec_rs_update per active stripe after the
 * validation pass. Synchronous: nothing queued is in flight on return, error
 * returns included.
 * Measured on one MI355X, 1024 updates of 4 KiB shards with one changed shard,
 * wall clock, medians (min..max) of 9 alternating rounds
 * (tools/bench_update_ragged.py,
 * profiles/update_ragged/bench_update_ragged.json): 1024 hec_rs_update calls
 * 14.35 ms (14.12..14.47); one hec_rs_update_batch 1.78 ms (1.69..1.86). */
int hec_rs_update_batch(const hec_rs_t* rs, uint8_t* const* shards, const size_t* lens,
                        const uint8_t* const* new_data, size_t n_stripes, size_t* bad_index);

/* ---- device-resident batches (no reference counterpart: the GPU form of the
 * encode_data_one_batch loop, encoder.rs:158-198, over many stripes) -------
 * Shard (stripe s, shard i) lives at base + s*stripe_stride + i*shard_stride.
 * Pointers are device pointers on the current HIP device; stream is a
 * hipStream_t (NULL = default stream). Calls are asynchronous.
 * Any strides that keep shards apart are supported, on device and host
 * batches alike: stripe-major [S][shards][L] with or without padding and gaps
 * between stripes, shard-major [shards][S][L] (stripe stride below shard
 * stride), different layouts for data and parity (and separate buffers), odd
 * bases and strides (those take the generic kernel). A call writes the parity
 * or erased shard ranges and no other byte: not the gaps, not the survivors,
 * not a skipped stripe (tests/test_gpu_footprint.py compares whole buffers).
 * Layout (speed only): with 1 MiB shards, a 64 KiB gap after each shard
 * (shard_stride = shard_len + 65536) runs encode and decode ~1.6% faster than
 * packed shards (the bench's batch is laid out so). */

/* Encode n_stripes stripes: read data shards 0..data from d_data, write parity
 * shards 0..parity to d_parity (shard index relative to each base).
 * All strided batches (device and host) return HEC_ERR_INVALID_ARGUMENT,
 * before any device work, when shards of a stripe overlap (shard stride <
 * shard_len), stripes overlap (stripe stride < shard_len) or the batch's byte
 * extent wraps 64 bits. Buffer sizes themselves cannot be checked here. */
int hec_gpu_encode_batch(const hec_rs_t* rs,
                         const uint8_t* d_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                         uint8_t* d_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                         uint64_t shard_len, uint32_t n_stripes, void* stream);

/* Reconstruct n_stripes stripes of all total shards in place. d_present_masks
 * (device, n_stripes words): bit i set = shard i present. Stripes with every
 * shard present are left untouched (upstream no-op); stripes with fewer than
 * data_shards present are skipped and counted into *d_bad_stripes (device
 * word, optional, accumulated). Requires total shards <= 16. */
int hec_gpu_reconstruct_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                              uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                              const uint32_t* d_present_masks, uint32_t* d_bad_stripes,
                              void* stream);

/* Reconstruct only the wanted shards. A want mask has bit i set when shard i
 * is worth rebuilding. Per stripe, let E be the erased shards (clear bits of
 * the present mask below 14) and W = want & E:
 *  - want bits of present shards, and bits 14 to 31, mean nothing;
 *  - W empty: the stripe is a no-op: not read, not written, not counted,
 *    however few of its shards are present;
 *  - fewer than 10 shards present and W non-empty: the stripe is skipped and
 *    counted into *d_bad_stripes (device word, optional, accumulated);
 *  - otherwise exactly the shards of W get the bytes
 *    hec_gpu_reconstruct_batch would give them, decoded from the first 10
 *    present shards in index order;
 *  - nothing else is written: not an erased shard outside W, not a survivor,
 *    not a gap;
 *  - with every want bit set the call gives hec_gpu_reconstruct_batch's bytes
 *    and counter.
 * d_want_masks: device, n_stripes words. Layouts, strides and lengths as
 * hec_gpu_reconstruct_batch; its argument errors in its order, plus a null
 * d_want_masks (HEC_ERR_INVALID_ARGUMENT, with the other nulls) and, after
 * HEC_ERR_EMPTY_SHARD, any codec but RS(10,4) (HEC_ERR_INVALID_ARGUMENT, as
 * the scrub calls), all before any device work.
 * Cost: on 16-byte aligned layouts a stripe moves (10 + |W|) shard lengths
 * and does |W| rows of GF math, where the full decode moves (10 + |E|) and
 * does |E| rows. Unaligned bases or strides take a generic kernel that makes
 * one pass over the ten inputs per wanted shard (again from cache after the
 * first): the footprint holds there, the traffic claim does not. */
int hec_gpu_reconstruct_some_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                   uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                   const uint32_t* d_present_masks, const uint32_t* d_want_masks,
                                   uint32_t* d_bad_stripes, void* stream);

/* Update: fold changed data shards into the stored parity without re-encoding
 * the stripe (klauspost's Update, ISA-L's ec_encode_data_update). RS(10,4).
 * d_update_masks (device, n_stripes words): bit c set = data shard c of that
 * stripe changed, c in 0..9; bits 10..31 mean nothing. Per stripe, with U the
 * set bits:
 *     parity[j] ^= XOR over c in U of P[j][c] * (old[c] ^ new[c]),  j = 0..3
 * (P = the parity rows of hec_rs_matrix). Data shard c of stripe s is at
 * d_old + s*old_stripe_stride + c*old_shard_stride, and likewise for d_new:
 * both are indexed by shard id 0..9, so an in-place [S][14][pitch] batch
 * passes its own base as d_old and base + 10*shard_stride as d_parity.
 *  - only the shards in U are read, of d_old and d_new alike;
 *  - d_old == NULL means old is zero: the parity accumulates P[:,U] * new[U]
 *    (klauspost's EncodeIdx). Over zeroed parity, any partition of 0..9 into
 *    calls gives hec_gpu_encode_batch's bytes, so a caller that receives a
 *    stripe's shards one after another never needs to hold all ten;
 *  - U empty: the stripe is not read and not written;
 *  - the call writes bytes [0, shard_len) of the four parity shards of the
 *    stripes with U non-empty and no other byte; d_old and d_new are never
 *    written. It does NOT copy new over old ("commit"): the caller swaps
 *    buffers or copies;
 *  - d_parity must overlap neither d_old nor d_new (not checked).
 * Layouts, strides and lengths as hec_gpu_encode_batch (any shard_len >= 1;
 * bases or strides that are not 16-byte aligned take a generic kernel).
 * Asynchronous on `stream`, no host synchronisation beyond the first plan
 * upload on a device, nothing allocated. Errors, all before device work and in
 * this order: a null rs, d_new, d_parity or d_update_masks, also with
 * n_stripes == 0 (HEC_ERR_INVALID_ARGUMENT); shard_len == 0
 * (HEC_ERR_EMPTY_SHARD); any codec but RS(10,4) (HEC_ERR_INVALID_ARGUMENT,
 * detail "RS(10,4) only"); overlapping shards or stripes, or an extent that
 * wraps 64 bits, in any of the three arenas, the old one only when given
 * (HEC_ERR_INVALID_ARGUMENT). With valid pointers n_stripes == 0 returns
 * HEC_OK and writes nothing.
 * Cost: a stripe moves 2|U| + 8 shard lengths (old and new of U read, four
 * parity shards read and four written), |U| + 8 without d_old, where
 * hec_gpu_encode_batch moves 14: one changed shard is 10 against 14. With
 * d_old, from |U| = 3 on a re-encode moves no more bytes.
 * Measured on one MI355X, 4096 x 1 MiB stripes with the 64 KiB shard pad,
 * medians (min..max) of 9 alternating rounds (tools/bench_update.py,
 * profiles/update/bench_update.json): hec_gpu_encode_batch 9.61 ms
 * (9.60..9.75); with d_old, |U| = 1: 6.82 ms (6.82..6.89), 0.710 of the
 * encode where the bytes say 10/14 = 0.714; |U| = 2: 8.26 ms (8.26..8.28);
 * |U| = 3: 9.74 ms (9.71..9.76), 1.013 of the encode at the same 14 shard
 * lengths. Without d_old, |U| = 1: 6.11 ms (6.10..6.13); |U| = 5: 8.91 ms
 * (8.89..8.91); |U| = 10: 12.33 ms (12.30..12.34) for 18 shard lengths. Every
 * leg moves 6.18 to 6.33 TB/s: the time follows the bytes. */
int hec_gpu_update_batch(const hec_rs_t* rs,
                         const uint8_t* d_old, uint64_t old_stripe_stride, uint64_t old_shard_stride,
                         const uint8_t* d_new, uint64_t new_stripe_stride, uint64_t new_shard_stride,
                         uint8_t* d_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                         uint64_t shard_len, uint32_t n_stripes, const uint32_t* d_update_masks, void* stream);

/* Verify (scrub) n_stripes stripes: the batched, on-device form of
 * ReedSolomon::verify. Reads the data shards from d_data and the STORED parity
 * shards from d_parity (layouts as hec_gpu_encode_batch), recomputes the parity
 * in registers and compares. Result contract: d_mismatch[s] (device, 32-bit
 * words) gets bit j set when parity shard j of stripe s differs, in at least
 * one of its shard_len bytes, from the parity of that stripe's data shards; a
 * clean stripe gives 0. The call overwrites words [0, n_stripes): it clears
 * them on `stream` before the launch, so stale contents never leak through.
 * It writes no other byte anywhere: not a shard, not a gap, not word
 * n_stripes. *d_bad_stripes (device word, optional, accumulated): plus one per
 * stripe with a non-zero word, counted exactly once however many chunks or
 * parity shards of it mismatch. Bytes at or past shard_len (pads of a pitch,
 * gaps) take no part in the comparison. Any codec with at most 32 parity
 * shards (more: HEC_ERR_INVALID_ARGUMENT), any strides and lengths; RS(10,4)
 * with 16-byte-aligned bases and strides and shard_len a multiple of 8 KiB
 * runs bit-sliced (hec_verify_kernel_name). Argument errors as
 * hec_gpu_encode_batch plus a null d_mismatch, all before any device work;
 * n_stripes == 0 returns HEC_OK and writes nothing. */
int hec_gpu_verify_batch(const hec_rs_t* rs,
                         const uint8_t* d_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                         const uint8_t* d_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                         uint64_t shard_len, uint32_t n_stripes,
                         uint32_t* d_mismatch, uint32_t* d_bad_stripes, void* stream);

/* Locate: hec_gpu_verify_batch that also names the corrupt shard. RS(10,4)
 * only (any other codec: HEC_ERR_INVALID_ARGUMENT before any device work, the
 * detail says so). d_mismatch and d_bad_stripes are exactly
 * hec_gpu_verify_batch's. Result contract of d_suspects[s] (device, 32-bit
 * words), over the byte columns o < shard_len of stripe s: let syn(o) = stored
 * parity XOR parity of the stored data at column o (4 bytes), and H = [P | I4]
 * the 4 x 14 check matrix (P = the 4 x 10 parity rows of hec_rs_matrix).
 *   - syn(o) == 0: the column contributes nothing;
 *   - there is a shard c in 0..13 and a byte v != 0 with syn(o) == v * H[:,c]
 *     (such a c is unique): bit c is set. Data shards are bits 0..9, parity
 *     shard j is bit 10 + j;
 *   - otherwise HEC_SUSPECT_UNEXPLAINED (bit 31) is set.
 * A clean stripe gives 0. Different columns of one stripe may name different
 * shards; then all their bits are set. Guarantee (RS(10,4) is MDS: any four
 * columns of H are independent): a column with at most 3 wrong shards never
 * sets the bit of an intact shard; one wrong shard sets its own bit; two or
 * three wrong shards set bit 31. 4 or more wrong shards in ONE byte column
 * are outside any guarantee (no decoder can do better). Bytes at or past
 * shard_len take no part, as in verify.
 * Two passes on `stream`, no host synchronisation: hec_gpu_verify_batch's
 * kernels, then a second kernel that reads only the stripes the first flagged.
 * Measured on one MI355X, 4096 x 1 MiB stripes, medians of 9 alternating
 * rounds (tools/bench_locate.py, profiles/locate/bench_locate.json): verify
 * alone 8.70 ms, locate on the clean batch 8.91 ms (1.025 x, 1.018..1.026 over
 * the rounds), with 1 stripe holding a flipped byte 8.94 ms, with 64 such
 * stripes 9.11 ms.
 * The call overwrites words [0, n_stripes) of d_mismatch and d_suspects and
 * writes no other byte anywhere. d_mismatch and d_suspects must be two
 * distinct arrays that overlap neither each other nor any shard (not checked:
 * the second pass clears d_suspects while it still reads d_mismatch). Argument errors are hec_gpu_verify_batch's
 * plus a null d_suspects and the codec, all before any device work; n_stripes
 * == 0 returns HEC_OK and writes nothing. Any strides, bases and lengths (odd
 * ones take the unaligned kernel). */
#define HEC_SUSPECT_UNEXPLAINED 0x80000000u
int hec_gpu_locate_corrupt_batch(const hec_rs_t* rs,
                                 const uint8_t* d_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                                 const uint8_t* d_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                                 uint64_t shard_len, uint32_t n_stripes,
                                 uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_bad_stripes, void* stream);

/* Repair in place what locate can name: hec_gpu_reconstruct_batch's layout
 * (RS(10,4); parity at d_shards + 10 * shard_stride). In stream order: (1)
 * locate into d_mismatch / d_suspects as above; (2) d_present_masks[s] =
 * 0x3FFF & ~d_suspects[s] when the word names 1 to 4 shards and bit 31 is
 * clear, else 0x3FFF, and *d_unrepaired (device word, optional, accumulated)
 * gets plus one per stripe with a non-zero word that is left alone; (3)
 * hec_gpu_reconstruct_batch with those masks. Only the suspect shards of
 * repaired stripes are written; everything else, the unrepaired stripes
 * included, stays byte for byte. All three arrays hold n_stripes words, are
 * overwritten, and must be distinct arrays that overlap neither one another
 * nor any shard (not checked). The repair trusts the guarantee above: a caller who wants proof
 * runs hec_gpu_verify_batch afterwards. Argument errors as locate's (all
 * three arrays required), before any device work. */
int hec_gpu_repair_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                         uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                         uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_present_masks,
                         uint32_t* d_unrepaired, void* stream);

/* Locate out to the code's radius: hec_gpu_locate_corrupt_batch that also names
 * TWO wrong shards of a byte column. RS(10,4) has distance 5, so with all 14
 * shards present two wrong shards at unknown positions are still decodable
 * (2t + e <= 4 with e = 0 erased); the call above names one and answers bit 31
 * for two. Opt-in: arguments, clearing rules, footprint promise (words
 * [0, n_stripes) of d_mismatch and d_suspects, no other byte anywhere),
 * stream order and argument errors are exactly hec_gpu_locate_corrupt_batch's;
 * RS(10,4) only. d_mismatch and d_bad_stripes are exactly
 * hec_gpu_verify_batch's. Result contract of d_suspects[s], with H and syn(o)
 * as above, per byte column o < shard_len:
 *   - syn(o) == 0: nothing;
 *   - a shard c and a byte v != 0 with syn(o) == v * H[:,c]: bit c (the rule
 *     above, unchanged: on such columns both calls give the same bits);
 *   - otherwise, shards a < b and bytes v, w != 0 with syn(o) == v * H[:,a] ^
 *     w * H[:,b]: bits a and b. The pair is unique (two explanations would
 *     make at most four columns of H dependent);
 *   - otherwise HEC_SUSPECT_UNEXPLAINED (bit 31).
 * The stripe's word is the OR over its columns. Guarantees:
 *   - a column with at most 2 wrong shards names exactly those shards;
 *   - a column with 3 wrong shards never names a SINGLE intact shard, but it
 *     may name an intact PAIR: 91 * 255^2 of the 2^32 syndromes (0.138 %) are
 *     pair-explainable, and about that share of random triple errors (182 of
 *     200,000 in a CPU count) comes back as a pair, each time with an intact
 *     shard in it. This is the price of decoding to the radius;
 *   - 4 or more wrong shards in one column: no guarantee;
 *   - a caller who wants the stricter "at most 3 wrong shards never blame an
 *     intact shard" keeps calling hec_gpu_locate_corrupt_batch.
 * The degraded calls below have no pair form: with a shard missing one wrong
 * shard is already the bound (2t + e <= 4).
 * Pass 2 is the same kernel walk; only waves that hold a column no single
 * shard explains run the pair search (classical syndromes of the dual
 * generalised Reed-Solomon code, a quadratic error locator evaluated at the
 * 14 shard points; DESIGN.md §4 "Locate, two per column"). Measured on one
 * MI355X, 4096 x 1 MiB stripes, medians of 9 alternating rounds
 * (tools/bench_locate_pairs.py, profiles/locate_pairs/bench_locate_pairs.json):
 * on the clean batch hec_gpu_locate_corrupt_batch 9.45 ms (9.38..9.78 over the
 * rounds) and this call 9.46 ms, inside that spread; with 64 stripes holding
 * one flipped byte 9.59 ms and 9.66 ms; with 64 stripes where two shards carry
 * a corrupted 4 KiB run at the same offset this call 9.68 ms. */
int hec_gpu_locate_corrupt_pairs_batch(const hec_rs_t* rs,
                                       const uint8_t* d_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                                       const uint8_t* d_parity, uint64_t parity_stripe_stride,
                                       uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                       uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_bad_stripes,
                                       void* stream);

/* hec_gpu_repair_batch over hec_gpu_locate_corrupt_pairs_batch's words: the
 * same three steps, arguments, footprint and errors, with step (1) the pair
 * locate. Whole shards per stripe, as there: a stripe whose columns name 1 to
 * 4 shards in total with bit 31 clear has those shards rebuilt from the other
 * ten or more; any other stripe (five or more shards named over its columns,
 * or bit 31) is left byte for byte and counted into *d_unrepaired. So a stripe
 * with two shards wrong in one column and a third wrong elsewhere is repaired
 * here and left alone by hec_gpu_repair_batch. The repair trusts the
 * guarantees above. hec_gpu_verify_batch afterwards shows that every repaired
 * stripe is a codeword again; in the three-wrong-shards case named as a pair
 * it is a codeword 5 shards away from the one written, which no parity check
 * can tell apart: a caller who cannot accept that keeps hec_gpu_repair_batch. */
int hec_gpu_repair_pairs_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                               uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                               uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_present_masks,
                               uint32_t* d_unrepaired, void* stream);

/* Correct in place, per byte column: hec_gpu_locate_corrupt_batch's two passes
 * with one addition -- where a column is explained, the error value the
 * syndrome implies is computed too and XORed into the wrong byte. RS(10,4)
 * only; d_data and d_parity are read and written. With H, syn(o) and the names
 * exactly as above, per byte column o < shard_len:
 *   - syn(o) == 0: nothing;
 *   - one shard c explains it, syn(o) == v * H[:,c]: byte o of shard c becomes
 *     stored ^ v (parity shard 10 + j: v = syn[j]; data shard c: v = syn[0] /
 *     P[0][c]);
 *   - (pairs call only) otherwise shards a < b explain it with v, w != 0: both
 *     bytes are fixed;
 *   - otherwise (bit 31): the column is left exactly as it is.
 * d_mismatch[s] and d_suspects[s] carry exactly hec_gpu_locate_corrupt_batch's
 * contracts (the pairs call: hec_gpu_locate_corrupt_pairs_batch's), evaluated
 * on the bytes as they were BEFORE the call; d_bad_stripes is verify's.
 * *d_uncorrected (device word, optional, accumulated) gets plus one per stripe
 * whose word has bit 31; *d_corrected_bytes (device 64-bit word, optional,
 * accumulated) the number of bytes changed. After the call:
 *   - every column with at most one wrong shard (two with the pairs call)
 *     holds the bytes that were written;
 *   - a stripe whose word has bit 31 clear is a codeword again;
 *   - a stripe with bit 31 set still has its other explainable columns fixed
 *     (unlike the repair calls, which leave such a stripe alone);
 *   - the set of bytes that differ from before is exactly the set of wrong
 *     bytes of explained columns: no other byte of any shard, no byte at or
 *     past shard_len and no byte between shards is written.
 * Limits. Single call: a column with 2 or 3 wrong shards is never touched; 4
 * or more carry no guarantee. Pairs call: 3 wrong shards in a column are
 * "corrected" to a codeword five shards away in 0.138 % of cases, the pair
 * locate's price (above); a caller who cannot accept that uses the single
 * call. When to use which: for a shard that is wrong throughout (a stale
 * file) the reconstruct of hec_gpu_repair_batch does less math per byte;
 * correct is for scattered damage, writes only the wrong bytes' vectors, and
 * repairs stripes that repair must leave alone (five or more shards named
 * over the columns, or bit 31 somewhere). Measured on one MI355X, 4096 x 1 MiB
 * stripes, medians of 9 alternating rounds (tools/bench_correct.py,
 * profiles/correct/bench_correct.json): on the clean batch
 * hec_gpu_locate_corrupt_batch 9.00 ms (8.99..9.05 over the rounds) and this
 * call 9.03 ms, inside that spread; 64 stripes with one flipped byte, repair
 * 9.81 ms and correct 9.24 ms; 64 stripes with a 4 KiB run wrong in two shards,
 * the pairs call 9.47 ms; 64 stripes with five shards hit at five offsets
 * (repair leaves all 64) 9.37 ms; 64 stripes whose shard 3 is wrong throughout,
 * repair 10.11 ms and correct 9.96 ms: on this batch the reconstruct's
 * smaller math did not show, its two extra passes (masks, decode walk) cost as
 * much, so the choice between the two is one of contract, not of speed.
 * Asynchronous on `stream`, no host synchronisation, nothing allocated.
 * Argument errors are locate's, before any device work; n_stripes == 0
 * returns HEC_OK and writes nothing. Any strides, bases and lengths (odd ones
 * take the unaligned kernel). The arrays must not overlap one another or any
 * shard (not checked). */
int hec_gpu_correct_batch(const hec_rs_t* rs,
                          uint8_t* d_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                          uint8_t* d_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                          uint64_t shard_len, uint32_t n_stripes,
                          uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_bad_stripes,
                          uint32_t* d_uncorrected, unsigned long long* d_corrected_bytes, void* stream);
int hec_gpu_correct_pairs_batch(const hec_rs_t* rs,
                                uint8_t* d_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                                uint8_t* d_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                                uint64_t shard_len, uint32_t n_stripes,
                                uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_bad_stripes,
                                uint32_t* d_uncorrected, unsigned long long* d_corrected_bytes, void* stream);

/* ---- degraded scrub: check and locate with shards missing (RS(10,4)) -------
 * The calls above need all 14 shards. These take hec_gpu_reconstruct_batch's
 * in-place layout and d_present_masks (bit i set = shard i present) and use
 * the redundancy a degraded stripe still has. Definitions, for stripe s:
 *   m = d_present_masks[s] & 0x3FFF, p = popcount(m), r = p - 10; for p >= 11
 *   B    = the ten lowest set bits of m (upstream's "first data_shards present"
 *          rule: the shards hec_gpu_reconstruct_batch decodes from);
 *   E    = the remaining r set bits, ascending (the spare shards);
 *   A_m  = (r x 10) rows E of the encoding matrix (hec_rs_matrix) times the
 *          inverse of its rows B: what the reconstruct would apply to B had E
 *          been erased;
 *   H_m  = [A_m | I_r], columns labelled by shard ids B then E;
 *   syn(o) = for byte column o < shard_len, the stored bytes of E XOR A_m
 *          times the stored bytes of B (r bytes).
 * The present shards form an MDS [p,10] code of distance r + 1. For each of
 * the 469 masks with 11..13 shards present no entry of A_m is zero and, for
 * r >= 2, no two columns of H_m are proportional (tests/test_check_model.py),
 * so one wrong shard is named uniquely:
 *   shards lost  r   one corrupt survivor is
 *   0            4   detected and named (hec_gpu_locate_corrupt_batch's case)
 *   1            3   detected and named
 *   2            2   detected and named
 *   3            1   detected
 * Any other codec: HEC_ERR_INVALID_ARGUMENT before any device work, the
 * detail says "RS(10,4) only". All are asynchronous on `stream` with no host
 * synchronisation (the first call on a device uploads the plan tables and
 * waits for that copy once).
 *
 * Masked verify. d_check[s] gets bit e set, for e in E, when row e of syn is
 * non-zero in at least one column: bits are by SHARD INDEX 0..13, so with the
 * full mask 0x3FFF the word is hec_gpu_verify_batch's shifted left by 10. A
 * stripe with p <= 10 has no spare shard and nothing to check: its word is 0,
 * it is not read, and it adds one to *d_unchecked (device word, optional,
 * accumulated). *d_bad_stripes (optional, accumulated): plus one per stripe
 * with a non-zero word, exactly once. Words [0, n_stripes) are cleared on
 * `stream` first; no other byte anywhere is written, absent shards are never
 * read, and bytes at or past shard_len take no part. Argument errors are
 * hec_gpu_reconstruct_batch's plus a null d_present_masks / d_check, all
 * before device work; n_stripes == 0 returns HEC_OK and writes nothing.
 * 16-byte-aligned bases and strides with shard_len a multiple of 2 KiB below
 * 4 GiB run the 8-byte-per-lane kernel, everything else a grid-stride kernel
 * (hec_check_kernel_name).
 * Measured on one MI355X, 4096 x 1 MiB stripes, medians of 9 alternating
 * rounds (tools/bench_check.py, profiles/degraded/bench_check.json), bytes
 * read per second: with 1 shard of every stripe erased 7.79 ms (13 shards
 * read, 7.17 TB/s, 0.90 of 8 TB/s), with 2 erased 6.92 ms (7.45 TB/s, 0.93),
 * with 3 erased 6.39 ms (7.39 TB/s, 0.92), with full masks 9.23 ms (6.52 TB/s,
 * 0.81) against hec_gpu_verify_batch's bit-sliced 8.18 ms (7.35 TB/s, 0.92):
 * with every shard present call that one. The route a degraded batch had
 * before, hec_gpu_reconstruct_batch then hec_gpu_verify_batch, takes 15.91 /
 * 16.69 / 17.45 ms with 1 / 2 / 3 erased; the masked verify was faster in
 * every round (0.48..0.50 of it with 1 erased). */
int hec_gpu_verify_present_batch(const hec_rs_t* rs, const uint8_t* d_shards, uint64_t stripe_stride,
                                 uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                 const uint32_t* d_present_masks, uint32_t* d_check, uint32_t* d_bad_stripes,
                                 uint32_t* d_unchecked, void* stream);

/* Masked locate: the masked verify (d_check, d_bad_stripes, d_unchecked are
 * exactly its), then a second kernel that reads only the flagged stripes.
 * Contract of d_suspects[s], per byte column o < shard_len:
 *   - syn(o) == 0: the column contributes nothing;
 *   - r >= 2 and there is a present shard c and a byte v != 0 with
 *     syn(o) == v * H_m[:,c] (such a c is unique): bit c is set;
 *   - any other non-zero column, and every non-zero column when r == 1:
 *     HEC_SUSPECT_UNEXPLAINED (bit 31).
 * With the full mask both words equal hec_gpu_locate_corrupt_batch's (d_check
 * = its d_mismatch shifted left by 10). Guarantees, per byte column:
 *   r = 4: as hec_gpu_locate_corrupt_batch;
 *   r = 3: one wrong shard is named; two wrong shards give bit 31; an intact
 *          shard is never named while at most two are wrong;
 *   r = 2: one wrong shard is named; two or more wrong shards in ONE column
 *          are outside any guarantee and may name an intact shard;
 *   r = 1: detection only (bit 31 on every dirty stripe).
 * d_check and d_suspects must be distinct arrays that overlap neither each
 * other nor the masks nor any shard (not checked). Both are overwritten in
 * [0, n_stripes); no other byte is written. Argument errors as the masked
 * verify plus a null d_suspects. */
int hec_gpu_locate_corrupt_present_batch(const hec_rs_t* rs, const uint8_t* d_shards, uint64_t stripe_stride,
                                         uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                         const uint32_t* d_present_masks, uint32_t* d_check, uint32_t* d_suspects,
                                         uint32_t* d_bad_stripes, uint32_t* d_unchecked, void* stream);

/* Checked reconstruct: the rebuild that does not launder corruption.
 * hec_gpu_reconstruct_batch decodes from the ten lowest present shards on
 * faith; one silently corrupt survivor among them is multiplied into every
 * rebuilt shard, and a later scrub that finds the stripe inconsistent has
 * more wrong shards to explain than it can name. This call looks at the spare
 * shards first. In stream order:
 *  (1) masked locate into d_check / d_suspects, as above;
 *  (2) d_use_masks[s] = m when d_check[s] == 0 (clean stripes, and unchecked
 *      stripes with p <= 10: exactly hec_gpu_reconstruct_batch's behaviour);
 *      = m & ~d_suspects[s] when bit 31 is clear, at least one shard is named
 *      and at least 10 bits remain (the named shards are treated as erased);
 *      otherwise 0x3FFF: the stripe is left byte for byte as it was, its
 *      holes included, and *d_unrepaired (device word, optional, accumulated)
 *      gets plus one;
 *  (3) hec_gpu_reconstruct_batch with d_use_masks; *d_bad_stripes is its count
 *      (stripes whose use mask has fewer than 10 bits).
 * Only shards in ~d_use_masks[s] & 0x3FFF of a stripe are written; the caller
 * reads d_use_masks to learn what was rebuilt. d_present_masks is only read.
 * The call trusts the guarantees above, r = 2's limit included (two wrong
 * shards in one column of a stripe with two spares may name, and so rebuild,
 * an intact shard from corrupt ones); hec_gpu_verify_batch afterwards is the
 * proof. d_check, d_suspects and d_use_masks hold n_stripes words each, are
 * overwritten, and must be distinct arrays that overlap nothing else.
 * Argument errors as the masked locate plus a null d_use_masks. */
int hec_gpu_reconstruct_checked_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                      uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                      const uint32_t* d_present_masks, uint32_t* d_check, uint32_t* d_suspects,
                                      uint32_t* d_use_masks, uint32_t* d_bad_stripes, uint32_t* d_unrepaired,
                                      void* stream);

/* Masked correct: the masked locate that also fixes, in place, every byte
 * column one present shard explains -- hec_gpu_correct_batch for a degraded
 * stripe. d_check, d_suspects, d_bad_stripes and d_unchecked carry exactly
 * hec_gpu_locate_corrupt_present_batch's contracts, evaluated on the bytes as
 * they were BEFORE the call. min_spares must be 2, 3 or 4
 * (HEC_ERR_INVALID_ARGUMENT otherwise, before device work): a stripe with
 * r < min_spares is classified but never written. Per byte column o <
 * shard_len of a stripe with r >= min_spares:
 *   - syn(o) == 0: nothing;
 *   - one present shard c explains it, syn(o) == v * H_m[:,c]: byte o of shard
 *     c becomes stored ^ v (shard E[j]: v = syn[j]; shard B[c]: v = syn[0] /
 *     A_m[0][c]);
 *   - otherwise (bit 31): the column is left exactly as it is.
 * *d_uncorrected (device word, optional, accumulated) gets plus one per stripe,
 * exactly once, that the call leaves inconsistent as far as it can tell: bit 31
 * in its suspects word, or a non-zero check word with r < min_spares.
 * *d_corrected_bytes (device 64-bit word, optional, accumulated): the bytes
 * changed. After the call:
 *   - a stripe with r >= min_spares and bit 31 clear has consistent present
 *     shards: a masked verify gives 0, and a reconstruct from it is the
 *     original whenever the guarantees below held;
 *   - a stripe with bit 31 set still has its other explainable columns fixed;
 *   - the set of bytes that differ from before is exactly the set of wrong
 *     bytes of explained columns; absent shards are never read or written, and
 *     no byte at or past shard_len and no byte between shards is written.
 * Guarantees, per byte column:
 *   r   one wrong survivor   two wrong in one column      three wrong in one column
 *   4   corrected (as        bit 31, untouched            bit 31, untouched
 *       hec_gpu_correct_batch)
 *   3   corrected            bit 31, untouched            may be taken for one intact
 *                                                         shard, which is "corrected"
 *   2   corrected            NO GUARANTEE: may be taken   --
 *                            for an intact shard, which
 *                            is then written
 *   1   bit 31, nothing written
 * Why min_spares exists: with r = 2 the present shards have distance 3, and two
 * wrong survivors in one column look like one wrong intact shard in 10 * 255 /
 * 65535 = 3.9 % of cases (the CPU model of tests/correct_present_model.py:
 * 786 of 20,000 random cases with shards 0 and 12 lost named an intact shard,
 * none named one of the wrong two); with r = 3, three wrong survivors do so in
 * about 0.015 %. A caller who cannot accept r = 2's limit passes 3: then no
 * intact byte is ever changed while at most two shards of a column are wrong.
 * The counters are accumulated and optional. Asynchronous on `stream`, no host
 * synchronisation (only the first plan upload on a device waits), nothing
 * allocated. Argument errors are the masked locate's plus min_spares, all
 * before device work; n_stripes == 0 returns HEC_OK and writes nothing. Any
 * strides, bases and lengths (odd ones take the unaligned kernel). */
int hec_gpu_correct_present_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                  uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                  const uint32_t* d_present_masks, uint32_t min_spares,
                                  uint32_t* d_check, uint32_t* d_suspects, uint32_t* d_bad_stripes,
                                  uint32_t* d_unchecked, uint32_t* d_uncorrected,
                                  unsigned long long* d_corrected_bytes, void* stream);

/* Corrected reconstruct: correct the survivors, then rebuild the lost shards
 * from them. In stream order:
 *  (1) hec_gpu_correct_present_batch into d_check / d_suspects (the count of
 *      uncorrected stripes is not reported; *d_corrected_bytes is its);
 *  (2) d_use_masks[s] = m when d_check[s] == 0 (clean stripes, and unchecked
 *      stripes with p <= 10, decoded on faith exactly as
 *      hec_gpu_reconstruct_batch does); = m also when r >= min_spares and bit
 *      31 of d_suspects[s] is clear (every dirty column was corrected);
 *      otherwise 0x3FFF: the stripe's holes stay, and *d_unrepaired (device
 *      word, optional, accumulated) gets plus one;
 *  (3) hec_gpu_reconstruct_batch with d_use_masks; *d_bad_stripes is its count.
 * Unlike hec_gpu_reconstruct_checked_batch no survivor is dropped, so a stripe
 * whose columns name many different shards (one lost and five survivors each
 * wrong at another offset: 13 - 5 = 8 trusted shards, which the checked call
 * must leave alone) is rebuilt in full. When to prefer which: a survivor that
 * is wrong throughout (a stale file) is cheaper as an erasure, the checked
 * call's way; scattered damage needs this call. Measured on one MI355X, 4096 x
 * 1 MiB stripes with one shard of each erased, medians of 9 alternating rounds
 * (tools/bench_correct_present.py,
 * profiles/correct_present/bench_correct_present.json): on the clean batch
 * hec_gpu_locate_corrupt_present_batch 8.65 ms (8.58..8.78 over the rounds) and
 * hec_gpu_correct_present_batch 8.71 ms, inside that spread; 64 stripes with
 * one flipped byte, the checked reconstruct 16.59 ms and this call 16.64 ms;
 * 64 stripes with five survivors hit at five offsets (the checked reconstruct
 * leaves all 64) 16.96 ms; 64 stripes with one survivor wrong throughout, the
 * checked reconstruct 17.02 ms and this call 17.26 ms. The guarantees are the masked
 * correct's, r = 2's limit and min_spares included; hec_gpu_verify_batch
 * afterwards is the proof. d_check, d_suspects and d_use_masks hold n_stripes
 * words each, are overwritten, and must be distinct arrays that overlap nothing
 * else. Argument errors as the masked correct plus a null d_use_masks. */
int hec_gpu_reconstruct_corrected_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                        uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                        const uint32_t* d_present_masks, uint32_t min_spares,
                                        uint32_t* d_check, uint32_t* d_suspects, uint32_t* d_use_masks,
                                        uint32_t* d_bad_stripes, uint32_t* d_unrepaired,
                                        unsigned long long* d_corrected_bytes, void* stream);

/* ---- host-memory batches (the path helyim runs: bytes start and end in host
 * memory, encoder.rs:169-195 / 263-304) -------------------------------------
 * Same strided layout as above but on HOST pointers; synchronous on return.
 * Pinned buffers the GPU can address (hipHostMalloc, torch pin_memory) are
 * coded zero-copy: the kernel reads and writes them over PCIe directly.
 * Pageable memory is copied chunk by chunk (host worker pool) into pinned
 * slots that the kernel codes in place, the copies of one chunk overlapping
 * the kernel of the next. With hec_set_host_zero_copy(0) both go through
 * H2D -> kernel -> D2H over 3 HIP streams. */
int hec_host_encode_batch(const hec_rs_t* rs,
                          const uint8_t* h_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                          uint8_t* h_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                          uint64_t shard_len, uint32_t n_stripes);
/* Reconstruct in place with per-stripe host masks (bit i = shard i present):
 * only the first data_shards present shards of a stripe cross PCIe H2D and
 * only its erased shards cross D2H. Stripes with fewer than data_shards
 * present are skipped and counted into *n_bad_stripes (optional). Requires
 * total shards <= 16. */
int hec_host_reconstruct_batch(const hec_rs_t* rs, uint8_t* h_shards, uint64_t stripe_stride,
                               uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                               const uint32_t* h_present_masks, uint32_t* n_bad_stripes);
/* hec_gpu_verify_batch on host memory, with its result contract: h_mismatch
 * (host, n_stripes words) is overwritten, *n_bad_stripes (optional) is SET to
 * the number of stripes with a non-zero word. Only the result words come back
 * over PCIe: pinned GPU-addressable data and parity are read in place
 * (zero copy), pageable memory is packed, all shards of a chunk, into the
 * pinned slots, and with hec_set_host_zero_copy(0) the shards are copied H2D.
 * The three paths give identical words. Neither buffer is written. */
int hec_host_verify_batch(const hec_rs_t* rs,
                          const uint8_t* h_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                          const uint8_t* h_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                          uint64_t shard_len, uint32_t n_stripes,
                          uint32_t* h_mismatch, uint32_t* n_bad_stripes);

/* One host batch spread over several GPUs of this process (SURVEY.md §8e:
 * contiguous stripe ranges per GPU; helyim's volume server is one process,
 * helyim-store/src/server.rs:451-506, so without this one call is capped by
 * one GPU's PCIe link). devices[0..n_devices) may repeat a device (two
 * concurrent ranges on it). Range r = stripes [S*r/R, S*(r+1)/R), R =
 * min(n_devices, n_stripes), runs on devices[r] from its own host thread
 * (CPUs bound to that GPU's NUMA node) through hec_host_encode_batch /
 * hec_host_reconstruct_batch, with its own streams and staging. Synchronous:
 * returns when every range is done; on failure the status of the first
 * failing range in list order (hec_last_error_detail names the range).
 * Arguments and results otherwise as the single-device calls;
 * *n_bad_stripes is the sum over ranges. An empty list or a device out of
 * range, or more than 256 entries -> HEC_ERR_INVALID_ARGUMENT before any work. */
int hec_host_encode_batch_multi(const hec_rs_t* rs, const int* devices, size_t n_devices,
                                const uint8_t* h_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                                uint8_t* h_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                                uint64_t shard_len, uint32_t n_stripes);
int hec_host_reconstruct_batch_multi(const hec_rs_t* rs, const int* devices, size_t n_devices,
                                     uint8_t* h_shards, uint64_t stripe_stride, uint64_t shard_stride,
                                     uint64_t shard_len, uint32_t n_stripes, const uint32_t* h_present_masks,
                                     uint32_t* n_bad_stripes);

/* hec_gpu_reconstruct_some_batch's contract on host memory (h_want_masks:
 * host, n_stripes words), over the three paths of hec_host_reconstruct_batch:
 * pinned memory in place, pageable memory through the pinned slots, and H2D /
 * D2H copies with zero copy off. Only the shards of W come back over PCIe; a
 * stripe with W empty sends nothing either way. RS(10,4) only. Argument
 * errors as the device call's. *n_bad_stripes (optional) = stripes with fewer
 * than 10 shards present and W non-empty. Synchronous. */
int hec_host_reconstruct_some_batch(const hec_rs_t* rs, uint8_t* h_shards, uint64_t stripe_stride,
                                    uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                    const uint32_t* h_present_masks, const uint32_t* h_want_masks,
                                    uint32_t* n_bad_stripes);

/* hec_gpu_update_batch on host memory, in delta form: h_delta shard c (indexed
 * by shard id 0..9 as d_new) holds old ^ new of data shard c, or the new shard
 * itself when the parity has not seen that shard yet; h_update_masks: host,
 * n_stripes words. parity[j] ^= XOR over c in U of P[j][c] * delta[c]. The
 * host call takes a delta and not old plus new because this path is bound by
 * PCIe: one shard crossing the link per changed shard instead of two is worth
 * a CPU XOR, and |U| + 8 shard lengths cross where a host encode moves 14 (9
 * against 14 for one changed shard; the untouched shards need not be in
 * memory). Over the three paths of hec_host_encode_batch: pinned memory in
 * place, pageable memory through the pinned slots, H2D / D2H copies with zero
 * copy off; they give identical parity. Of a stripe only the deltas of U and
 * the parity are read, only bytes [0, shard_len) of its parity shards are
 * written, and a stripe with U empty moves nothing either way. h_delta is
 * never written. RS(10,4) only. Argument errors as the device call's, in its
 * order. Synchronous: nothing queued is in flight on return, error returns
 * included. */
int hec_host_update_batch(const hec_rs_t* rs,
                          const uint8_t* h_delta, uint64_t delta_stripe_stride, uint64_t delta_shard_stride,
                          uint8_t* h_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                          uint64_t shard_len, uint32_t n_stripes, const uint32_t* h_update_masks);

/* Ragged device batches (RS(10,4)): every stripe has its own length, shard
 * stride and erasure pattern -- BASELINE config 5's mixed 64 KiB-4 MiB
 * stripes in ONE launch. Stripe j's shard i is at d_base + offset + i *
 * shard_stride (offset, stride and d_base 16-byte aligned, stride >=
 * shard_len). Encode reads shards 0..9 and writes 10..13; reconstruct uses
 * present_mask like hec_gpu_reconstruct_batch. descs are HOST memory; the
 * launch is asynchronous on `stream`. */
typedef struct hec_stripe_desc {
    uint64_t offset;
    uint64_t shard_stride;
    uint32_t shard_len;
    uint32_t present_mask;
} hec_stripe_desc;
int hec_gpu_encode_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs,
                          uint32_t n_stripes, void* stream);
int hec_gpu_reconstruct_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs,
                               uint32_t n_stripes, uint32_t* d_bad_stripes, void* stream);
/* hec_gpu_reconstruct_ragged with hec_gpu_reconstruct_some_batch's contract
 * per stripe. h_want_masks: HOST memory beside descs, n_stripes words (NULL
 * with n_stripes > 0: HEC_ERR_INVALID_ARGUMENT). A stripe with W empty gets no
 * workgroups at all. */
int hec_gpu_reconstruct_some_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs,
                                    const uint32_t* h_want_masks, uint32_t n_stripes,
                                    uint32_t* d_bad_stripes, void* stream);

/* Ragged scrub (RS(10,4)): the masked verify and the masked locate over a
 * ragged batch, stripes of mixed lengths and mixed present masks in one pass
 * over HBM (plus, for the locate, a second pass over the flagged stripes
 * only). The result contracts are exactly hec_gpu_verify_present_batch's and
 * hec_gpu_locate_corrupt_present_batch's, evaluated per stripe with m =
 * descs[s].present_mask & 0x3FFF and that stripe's own shard_len:
 *   - d_check[s]: bit e, by shard index, for every spare shard e in E whose
 *     syndrome row is non-zero somewhere in the stripe;
 *   - d_suspects[s]: bit c when present shard c alone explains a byte column,
 *     HEC_SUSPECT_UNEXPLAINED (bit 31) for every other non-zero column and for
 *     every non-zero column when r == 1;
 *   - a stripe with p <= 10 present shards is not read: its words are 0 and it
 *     adds one to *d_unchecked (device word, optional, accumulated);
 *   - *d_bad_stripes (device word, optional, accumulated): plus one per stripe
 *     with a non-zero check word, exactly once however many column ranges,
 *     waves or launches report the stripe;
 *   - a full mask gives hec_gpu_locate_corrupt_batch's words, d_check = its
 *     d_mismatch shifted left by 10.
 * Words [0, n_stripes) of each result array are cleared on `stream` and then
 * written; no other byte anywhere is written (no shard, no gap, not word
 * n_stripes), absent shards are never read, and bytes at or past a stripe's
 * shard_len take no part. d_check and d_suspects are distinct device arrays
 * that overlap nothing else (not checked). descs are HOST memory; layout and
 * alignment rules are hec_gpu_encode_ragged's (d_base, offset and stride
 * 16-byte aligned, stride >= shard_len >= 1). Errors, all before any device
 * work: a null rs, d_base, d_check (for the locate also d_suspects), or descs
 * with n_stripes > 0, and a misaligned or overlapping stripe:
 * HEC_ERR_INVALID_ARGUMENT; any other codec: HEC_ERR_INVALID_ARGUMENT, the
 * detail says "RS(10,4) only"; shard_len == 0: HEC_ERR_EMPTY_SHARD, the detail
 * names the stripe; a batch above 2^32 column ranges: HEC_ERR_INVALID_ARGUMENT.
 * With valid pointers n_stripes == 0 returns HEC_OK and writes nothing.
 * Asynchronous on `stream`; the host waits only as the other ragged calls do
 * (for the call four ragged calls ago that used the same metadata slot, and
 * once per device for the plan upload).
 * Pass 1 runs bit-sliced when every stripe has all 14 shards and a length that
 * is a multiple of 8 KiB, otherwise as a table check that takes any length
 * (hec_ragged_scrub_kernel_name reports which).
 * Repair on the device, with no host round trip: hec_gpu_correct_ragged and
 * hec_gpu_reconstruct_corrected_ragged, below. The checked recipe (drop the
 * named survivors) stays the caller's: read d_suspects, clear the named bits
 * in the stripe's present_mask on the host (where bit 31 is clear and at least
 * 10 bits remain), and call hec_gpu_reconstruct_ragged; hec_gpu_verify_ragged
 * with the original masks is the proof.
 * Measured on one MI355X against the strided calls on the same bytes in the
 * same process, 4096 x 1 MiB stripes with a 64 KiB shard pad, medians of 9
 * alternating rounds, the map's upload included (tools/bench_ragged_scrub.py,
 * profiles/ragged_scrub/bench_ragged_scrub.json): full masks, bit-sliced,
 * 8.86 ms against hec_gpu_verify_batch's 8.75 (8.73..8.78 over the rounds),
 * 1.012x, outside that spread (1.005x in two other runs of the tool, inside
 * the spread in one of them); one shard of every stripe erased 8.48 ms against
 * hec_gpu_verify_present_batch's 8.13 (8.10..8.26), 1.044x, outside; the locate
 * with 64 stripes holding a flipped byte 9.50 ms against
 * hec_gpu_locate_corrupt_batch's 9.12 (9.10..9.14), 1.041x, outside. A uniform
 * batch is cheaper through the strided calls; what this call is for is the
 * mixed batch: 2048 stripes of 64 KiB..4 MiB with 0..3 shards lost each, 25.2
 * GB read in 4.09 ms, 6.17 TB/s, 0.77 of 8 TB/s, in one call (6.26 and 6.53
 * TB/s in the other two runs). */
int hec_gpu_verify_ragged(const hec_rs_t* rs, const uint8_t* d_base, const hec_stripe_desc* descs,
                          uint32_t n_stripes, uint32_t* d_check, uint32_t* d_bad_stripes,
                          uint32_t* d_unchecked, void* stream);
int hec_gpu_locate_corrupt_ragged(const hec_rs_t* rs, const uint8_t* d_base, const hec_stripe_desc* descs,
                                  uint32_t n_stripes, uint32_t* d_check, uint32_t* d_suspects,
                                  uint32_t* d_bad_stripes, uint32_t* d_unchecked, void* stream);

/* Ragged correct and corrected reconstruct (RS(10,4)): the masked correct calls
 * over a ragged batch, in one call with no host round trip.
 * hec_gpu_correct_ragged has exactly hec_gpu_correct_present_batch's contract,
 * evaluated per stripe with m = descs[s].present_mask & 0x3FFF and that
 * stripe's own shard_len: d_check, d_suspects, *d_bad_stripes and *d_unchecked
 * are hec_gpu_locate_corrupt_ragged's, of the bytes as they were before the
 * call; in a stripe with r >= min_spares (2, 3 or 4) every byte column that
 * one present shard explains gets its error value XORed into the wrong byte,
 * in place; a bit-31 column keeps its bytes; a stripe with r < min_spares is
 * classified and never written; *d_uncorrected (optional, accumulated) gets
 * plus one, once, per stripe left inconsistent; *d_corrected_bytes (optional,
 * accumulated) counts the bytes changed. The guarantee table and the reason
 * for min_spares are hec_gpu_correct_present_batch's, above. Nothing else is
 * written: no absent shard, no byte at or past shard_len, no slack up to the
 * stride, no gap between stripes, not word n_stripes of a result array. A
 * stripe with p <= 10 is not read.
 * hec_gpu_reconstruct_corrected_ragged is hec_gpu_reconstruct_corrected_batch's
 * three steps in stream order: (1) the ragged correct (the uncorrected count
 * is not reported); (2) d_use_masks[s] = m when d_check[s] == 0, or when r >=
 * min_spares and bit 31 of d_suspects[s] is clear, otherwise 0x3FFF and
 * *d_unrepaired (optional, accumulated) gets plus one; (3)
 * hec_gpu_reconstruct_ragged with those masks: *d_bad_stripes is that
 * reconstruct's count of stripes with fewer than ten shards, no survivor is
 * dropped, and a stripe left alone keeps its holes.
 * Errors, all before any device work: everything hec_gpu_locate_corrupt_ragged
 * refuses; min_spares outside 2..4; a null d_use_masks:
 * HEC_ERR_INVALID_ARGUMENT. With valid pointers n_stripes == 0 returns HEC_OK
 * and writes nothing. Host waits are those of the other ragged calls. Pass 1
 * is the ragged scrub's (hec_ragged_scrub_kernel_name reports it); pass 2 is
 * rs104_ragged_correct_kernel; the reconstruct decodes from a workgroup map of
 * its own kept in the same metadata slot.
 * Measured on one MI355X, 4096 x 1 MiB stripes with a 64 KiB shard pad, one
 * shard of every stripe erased, medians of 9 alternating rounds in one process,
 * the maps' upload included (tools/bench_ragged_correct.py,
 * profiles/ragged_correct/bench_ragged_correct.json): on a clean batch the
 * correct 9.01 ms against hec_gpu_locate_corrupt_ragged's 8.96 (8.86..9.03 over
 * the rounds), 1.005x, inside that spread; with 64 stripes holding a flipped
 * byte 9.24 ms against the locate's 9.11 (8.98..9.15), 1.014x, outside, and
 * against hec_gpu_correct_present_batch's 8.78 on the same bytes, 1.052x,
 * outside; the corrected reconstruct 17.04 ms against
 * hec_gpu_reconstruct_corrected_batch's 16.51 (16.39..16.55), 1.032x, outside.
 * A config-5 batch (2048 clean stripes of 64 KiB..4 MiB, 0..3 shards lost)
 * is corrected and rebuilt in 7.25 ms, 43.6 GB moved, 6.02 TB/s, 0.75 of 8
 * TB/s. */
int hec_gpu_correct_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs, uint32_t n_stripes,
                           uint32_t min_spares, uint32_t* d_check, uint32_t* d_suspects, uint32_t* d_bad_stripes,
                           uint32_t* d_unchecked, uint32_t* d_uncorrected, unsigned long long* d_corrected_bytes,
                           void* stream);
int hec_gpu_reconstruct_corrected_ragged(const hec_rs_t* rs, uint8_t* d_base, const hec_stripe_desc* descs,
                                         uint32_t n_stripes, uint32_t min_spares, uint32_t* d_check,
                                         uint32_t* d_suspects, uint32_t* d_use_masks, uint32_t* d_bad_stripes,
                                         uint32_t* d_unrepaired, unsigned long long* d_corrected_bytes, void* stream);

/* Ragged update (RS(10,4)): hec_gpu_update_batch over stripes of mixed
 * lengths in one launch -- small writes arrive as byte ranges of their own
 * lengths, not as n_stripes equal stripes. Per stripe the contract is exactly
 * hec_gpu_update_batch's (what is read, what is written, d_old == NULL as the
 * accumulate form, no commit, no overlap of d_parity with a data arena),
 * evaluated with that stripe's own shard_len, its place in the three arenas
 * and U = update_mask & 0x3FF; over zeroed parity, any partition of 0..9 into
 * calls without d_old gives hec_gpu_encode_ragged's bytes. A stripe with U
 * empty is not read, not written and owns no workgroup. No byte outside
 * [0, shard_len) of the four parity shards of the stripes with U non-empty is
 * written: not the slack up to the stride, not a gap, not d_old or d_new.
 * Three arenas, so the in-place ragged layout and separate buffers both fit:
 * a stripe of an arena hec_gpu_encode_ragged made with descriptor d passes
 * d_old = d_parity = d_base, old_offset = d.offset, parity_offset = d.offset +
 * 10 * d.shard_stride and both strides d.shard_stride.
 * Alignment as the ragged family: the three bases and every offset and stride
 * 16-byte aligned, each stride >= shard_len >= 1. descs are HOST memory; the
 * call is asynchronous on `stream`; the host waits only as the other ragged
 * calls do (the metadata slot used four ragged calls ago, the first plan
 * upload on a device) and nothing else is allocated.
 * Errors, all before any device work, in the ragged calls' order: a null rs,
 * d_new or d_parity, also with n_stripes == 0, or null descs with n_stripes >
 * 0 (HEC_ERR_INVALID_ARGUMENT); any codec but RS(10,4)
 * (HEC_ERR_INVALID_ARGUMENT, detail "RS(10,4) only"); then per descriptor in
 * index order, whatever its mask: shard_len == 0 (HEC_ERR_EMPTY_SHARD, detail
 * names the stripe); a misaligned base, offset or stride, a stride below
 * shard_len, or an extent (offset + 10 * stride; + 4 * for the parity) that
 * wraps 64 bits, in the parity and new arenas and, only when d_old is given,
 * the old one (HEC_ERR_INVALID_ARGUMENT, detail names the stripe); more than
 * 2^32 column ranges of 4 KiB in total (HEC_ERR_INVALID_ARGUMENT). With valid
 * pointers n_stripes == 0 returns HEC_OK and writes nothing.
 * The kernel is rs104_ragged_update_kernel (hec_update_ragged_kernel_name):
 * one workgroup per 4 KiB column range of a stripe with U non-empty, dealt to
 * the XCDs in eighths, launches of at most 2^23 workgroups.
 * Measured on one MI355X, medians (min..max) of 9 alternating rounds, HIP
 * events, the map's upload included (tools/bench_update_ragged.py,
 * profiles/update_ragged/bench_update_ragged.json). 4096 x 1 MiB stripes with
 * the 64 KiB pad, d_old given, |U| = 1: hec_gpu_update_batch 6.95 ms
 * (6.94..6.98), this call on the same bytes 7.14 (7.12..7.55), 1.027x, outside
 * the strided call's spread: a batch of one length is cheaper there. 2048
 * stripes of 64 KiB..4 MiB: hec_gpu_encode_ragged 4.83 ms (4.81..4.89); with
 * d_old, |U| = 1: 3.37 (3.36..3.38), 0.697 of the encode where the bytes say
 * 10/14; |U| = 2: 4.04; |U| = 3: 4.73; without d_old, |U| = 1: 3.02. Every
 * update leg moves 6.10 to 6.15 TB/s. */
typedef struct hec_update_desc {
    uint64_t parity_offset, parity_stride; /* parity shard j (0..3) at d_parity + parity_offset + j*parity_stride */
    uint64_t new_offset,    new_stride;    /* new data shard c (shard id 0..9) at d_new + new_offset + c*new_stride */
    uint64_t old_offset,    old_stride;    /* old data shard c likewise in d_old; ignored when d_old == NULL */
    uint32_t shard_len;
    uint32_t update_mask;                  /* bit c = data shard c changed; bits 10..31 mean nothing */
} hec_update_desc;                         /* 56 bytes */
int hec_gpu_update_ragged(const hec_rs_t* rs, const uint8_t* d_old, const uint8_t* d_new, uint8_t* d_parity,
                          const hec_update_desc* descs, uint32_t n_stripes, void* stream);

/* Deterministic splitmix64 stripe data (bench / test inputs): stripe s gets
 * bytes_per_stripe bytes at d_base + s*stripe_stride, 64-bit word n (n >= 1)
 * = splitmix64_mix(seed_base + s + n * 0x9E3779B97F4A7C15), little endian. */
int hec_gpu_fill_splitmix(uint8_t* d_base, uint64_t stripe_stride, uint64_t bytes_per_stripe,
                          uint32_t n_stripes, uint64_t seed_base, void* stream);

/* ---- file level: helyim_ec::write_ec_files / rebuild_ec_files ------------ */

/* write_ec_files(base_filename) (encoder.rs:39-46): base.dat -> base.ec00..ec13. */
int hec_write_ec_files(const char* base_filename);
/* generate_ec_files(base, buf_size, large_block_size, small_block_size)
 * (encoder.rs:52-71): same, with explicit geometry (tests use small blocks to
 * exercise the large-row path). */
int hec_write_ec_files_ex(const char* base_filename, uint64_t buf_size, uint64_t large_block_size,
                          uint64_t small_block_size);
/* rebuild_ec_files(base_filename) -> Vec<u32> (encoder.rs:48-50, 73-109,
 * 244-307): recreates every missing .ecNN. rebuilt_ids (capacity 14) receives
 * the rebuilt shard ids in ascending order, *n_rebuilt their count. */
int hec_rebuild_ec_files(const char* base_filename, uint32_t* rebuilt_ids, size_t* n_rebuilt);

/* Scrub of base.ec00 .. base.ec13 (no reference counterpart: helyim never
 * checks its shards). RS parity is bytewise -- byte o of every parity file is
 * a function of byte o of the ten data files, whatever block geometry wrote
 * them -- so the 14 files are checked as 14 equal-length streams cut into
 * column blocks of block_size bytes (0 = 1 MiB; otherwise a non-zero multiple
 * of 4096 below 4 GiB, else HEC_ERR_INVALID_ARGUMENT; two pinned slots of
 * about 14 x max(block_size, 4 MiB) bytes are staged). The last block may be
 * shorter. *n_blocks = blocks checked; *n_bad = blocks whose stored parity
 * differs from their data's (the total, even past cap); the first
 * min(cap, *n_bad) of them go to bad[] in ascending offset: offset in the
 * shard files, length of the block, parity_mask (bit j = .ec(10+j) differs, as
 * hec_gpu_verify_batch's word). bad may be NULL when cap is 0. Files are
 * opened read-only and none is written. Errors, the first three before any
 * device work: any of the 14 files missing -> HEC_ERR_SHARD_NOT_FOUND (detail
 * names it); sizes not all equal -> HEC_ERR_UNEXPECTED_EC_SHARD_SIZE with
 * hec_last_error_values = (size of .ec00, size of the first file that
 * differs); a short read or OS error -> HEC_ERR_IO with its errno. Empty
 * files: HEC_OK, zero blocks. */
typedef struct hec_scrub_bad {
    uint64_t offset;
    uint32_t length;
    uint32_t parity_mask;
} hec_scrub_bad;
int hec_verify_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_bad* bad, size_t cap,
                        size_t* n_bad, uint64_t* n_blocks);
/* hec_verify_ec_files that also names the corrupt file of each bad block:
 * arguments, block rules, errors and the read-only promise are identical;
 * each entry carries the block's suspects word (hec_gpu_locate_corrupt_batch's
 * contract: bit c = .ec(c) alone explains a byte column of the block, bit 31 =
 * a column no single file explains). How the result is used: scattered damage
 * is fixed in place by hec_correct_ec_files (below). For whole-file damage,
 * when a volume's blocks name one file (up to four) and bit 31 is clear
 * everywhere, delete the named .ecNN and call hec_rebuild_ec_files, which
 * recreates them from the other files; then scrub again. No file is written
 * here. */
typedef struct hec_scrub_suspect {
    uint64_t offset;
    uint32_t length;
    uint32_t parity_mask;
    uint32_t suspects;
    uint32_t reserved;  /* 0 */
} hec_scrub_suspect;
int hec_locate_corrupt_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad, size_t cap,
                                size_t* n_bad, uint64_t* n_blocks);
/* hec_locate_corrupt_ec_files with hec_gpu_locate_corrupt_pairs_batch's
 * suspects words: arguments, struct, block rules, errors and the read-only
 * promise are identical; a byte column that two files explain sets both
 * their bits instead of bit 31 (the same torn sector in two files, a stale
 * file plus one bit-rot). Scattered damage is fixed in place by
 * hec_correct_pairs_ec_files (below). Recipe for whole-file damage: take the
 * union of the named files over all bad blocks; when it holds at most four files and bit 31 is clear everywhere,
 * delete the named .ecNN and call hec_rebuild_ec_files, then scrub again. With
 * five or more files named in total or bit 31 set somewhere, rebuild nothing
 * from the volume as a whole. The guarantees and their limit (three wrong
 * files in one column may name an intact pair) are those of
 * hec_gpu_locate_corrupt_pairs_batch. */
int hec_locate_corrupt_pairs_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad,
                                      size_t cap, size_t* n_bad, uint64_t* n_blocks);
/* hec_locate_corrupt_ec_files that also fixes what it explains, in the files:
 * arguments, block rules and entries are identical, and the entries carry the
 * words from BEFORE the correction (hec_gpu_correct_batch's contract; the
 * pairs form: hec_gpu_correct_pairs_batch's, with its limit). The 14 files are
 * opened for reading and writing: one that cannot be (a read-only file) gives
 * HEC_ERR_IO with its errno before any device work; the other errors are
 * hec_verify_ec_files's. For each bad block, and each file .ec(c) whose bit c
 * is set in the block's suspects word, that file's `length` bytes at the
 * block's offset are rewritten with the corrected bytes. No other byte of any
 * file is written, no file is written for a clean block, and a column that
 * stays unexplained (bit 31) keeps its bytes. Each file that was written is
 * fdatasync'ed once before the return. A second scrub reports only the blocks
 * that hold unexplained columns. Every file must be present; a degraded
 * volume goes to hec_correct_ec_files_present. */
int hec_correct_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad, size_t cap,
                         size_t* n_bad, uint64_t* n_blocks);
int hec_correct_pairs_ec_files(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad, size_t cap,
                               size_t* n_bad, uint64_t* n_blocks);
/* hec_locate_corrupt_ec_files for a degraded volume: a missing .ecNN (ENOENT)
 * is an erased shard, not an error. *present_mask (optional) reports which
 * files were found (bit i = base.ec(i)). Each entry's parity_mask field
 * carries the block's check word and its suspects field the masked-locate
 * word (hec_gpu_locate_corrupt_present_batch's contracts, bits by file index
 * 0..13); with all 14 files present the entries equal
 * hec_locate_corrupt_ec_files's with parity_mask << 10. Only present files are
 * opened and read, and none is written. Errors, all before device work: no
 * file present -> HEC_ERR_SHARD_NOT_FOUND; 1 to 10 present ->
 * HEC_ERR_TOO_FEW_SHARDS_PRESENT (the detail gives the count); present sizes
 * not all equal -> HEC_ERR_UNEXPECTED_EC_SHARD_SIZE with hec_last_error_values
 * = (size of the first present file, size of the first that differs). Block,
 * cap and bad rules are unchanged.
 * Recipe for a degraded volume: scrub it with hec_correct_ec_files_present
 * (below), which heals the surviving files in place; if bit 31 is clear in
 * every entry, hec_rebuild_ec_files; then scrub again. (Read-only
 * alternative, for files that are wrong throughout: scrub with this call,
 * delete the named files too -- at most four missing in total -- and rebuild.)
 * With bit 31 set somewhere (always so with three files missing) the volume
 * has damage this library cannot attribute: rebuild nothing from it. */
int hec_locate_corrupt_ec_files_present(const char* base_filename, uint64_t block_size, hec_scrub_suspect* bad,
                                        size_t cap, size_t* n_bad, uint64_t* n_blocks, uint32_t* present_mask);
/* hec_locate_corrupt_ec_files_present that also fixes what it explains, in the
 * present files (every launch is hec_gpu_correct_present_batch's kernel with
 * min_spares: 2, 3 or 4, HEC_ERR_INVALID_ARGUMENT otherwise). The entries
 * equal hec_locate_corrupt_ec_files_present's and hold the words from BEFORE
 * the correction. The present files are opened for reading and writing: one
 * that cannot be (a read-only file) gives HEC_ERR_IO with its errno before
 * any device work; ENOENT is an erased shard; the other errors are
 * hec_locate_corrupt_ec_files_present's. For each bad block, and each present
 * file .ec(c) whose bit c is set in the block's suspects word, that file's
 * `length` bytes at the block's offset are rewritten from the corrected
 * block; nothing else is written, no missing file is created, and each file
 * written is fdatasync'ed once before the return. A volume with fewer than
 * min_spares spare files (r < min_spares) is only located: nothing is
 * written. */
int hec_correct_ec_files_present(const char* base_filename, uint64_t block_size, uint32_t min_spares,
                                 hec_scrub_suspect* bad, size_t cap, size_t* n_bad, uint64_t* n_blocks,
                                 uint32_t* present_mask);

/* ---- EC volume files around the shards (host-side byte formats) ----------- */
/* write_sorted_file_from_index(base, ext) (encoder.rs:21-37): replay base.idx
 * (16-byte BE entries; offset 0 or negative size deletes) and write the live
 * entries sorted by needle id to base+ext (".ecx"). */
int hec_write_sorted_file_from_index(const char* base_filename, const char* ext);
/* rebuild_ecx_file(base) (lib.rs:95-133): apply base.ecj tombstones to base.ecx,
 * then delete base.ecj; no .ecj -> HEC_OK. */
int hec_rebuild_ecx_file(const char* base_filename);
/* save_volume_info(filename, VolumeInfo{version}) as the generate RPC writes it
 * (volume_info.rs:121-132, server.rs:470-475). */
int hec_save_volume_info(const char* filename, uint32_t version);
/* find_data_filesize(base) (decoder.rs:46-66). */
int hec_find_data_filesize(const char* base_filename, uint64_t* data_filesize);
/* write_data_file(base, size) (decoder.rs:142-180): .ec00-.ec09 -> base.dat. */
int hec_write_data_file(const char* base_filename, int64_t data_filesize);
/* write_index_file_from_ec_index(base) (decoder.rs:22-44): .ecx + .ecj -> .idx. */
int hec_write_index_file_from_ec_index(const char* base_filename);

/* ---- needle reads from EC shards (locate + degraded read) ----------------- */
/* Interval (helyim-ec/src/locate.rs:3-9). */
typedef struct hec_interval {
    uint64_t block_index;
    uint64_t inner_block_offset;
    uint64_t size;
    uint64_t large_block_rows;
    uint32_t is_large_block;
    uint32_t reserved;
} hec_interval;
/* locate_data(large_block_len, small_block_len, data_size, offset, size)
 * (locate.rs:29-72, with locate_offset :74-100 and its own large-row count).
 * Writes up to cap intervals; *n_out = the number locate_data yields (an
 * HEC_ERR_INVALID_ARGUMENT when it exceeds cap). */
int hec_locate_data(uint64_t large_block_len, uint64_t small_block_len, uint64_t data_size, uint64_t offset,
                    uint64_t size, hec_interval* out, size_t cap, size_t* n_out);
/* Interval::shard_id (locate.rs:12-15) and Interval::offset (:17-27). */
uint32_t hec_interval_shard_id(const hec_interval* interval);
uint64_t hec_interval_offset(const hec_interval* interval, uint64_t large_block_size, uint64_t small_block_size);
/* EcVolume::find_needle_from_ecx (volume/mod.rs:153-155 ->
 * search_needle_from_sorted_index, lib.rs:54-82): binary search of base.ecx.
 * *offset is the stored Offset (units of 8 bytes), *size the stored Size (< 0
 * = deleted). Absent id -> HEC_ERR_IO ("Needle {id} is not found",
 * io::ErrorKind::NotFound). */
int hec_find_needle_from_ecx(const char* base_filename, uint64_t needle_id, uint32_t* offset, int32_t* size);
/* read_ec_shard_intervals (erasure_coding/mod.rs:303-401) over n_ranges
 * (offset, size) ranges of the volume's data, against the local shard files
 * base.ec00..ec13 (data_size = first shard file's size x 10, volume/mod.rs:146).
 * An interval on a present shard is read from it (short read -> HEC_ERR_IO);
 * an interval on a missing shard is rebuilt from the other shards' same range
 * (recover_one_remote_ec_shard_interval, :403-491: full-length reads count as
 * present; fewer than 10 -> HEC_ERR_TOO_FEW_SHARDS_PRESENT). All rebuilt
 * intervals of the call go to the GPU as one batch. out receives the ranges
 * back to back (sum of sizes bytes). No shard file -> HEC_ERR_SHARD_NOT_FOUND. */
int hec_read_ec_data(const char* base_filename, uint64_t large_block_size, uint64_t small_block_size,
                     const uint64_t* offsets, const uint64_t* sizes, size_t n_ranges, uint8_t* out);
/* read_ec_shard_needle's data path (erasure_coding/mod.rs:129-171): look the
 * needle up in base.ecx, HEC_ERR_NEEDLE_NOT_FOUND if deleted, then read its
 * actual_size bytes at actual_offset (Offset * 8 as u32, Size::actual_size)
 * through hec_read_ec_data with the 1 GiB / 1 MiB blocks. *n_out = the
 * needle's byte count; cap smaller than that -> HEC_ERR_INVALID_ARGUMENT.
 * Parsing the needle record is the caller's (Needle::read_bytes). */
int hec_read_ec_needle(const char* base_filename, uint64_t needle_id, uint8_t* out, size_t cap, size_t* n_out);
/* hec_read_ec_needle with explicit block sizes (tests exercise large rows). */
int hec_read_ec_needle_ex(const char* base_filename, uint64_t large_block_size, uint64_t small_block_size,
                          uint64_t needle_id, uint8_t* out, size_t cap, size_t* n_out);
/* Many needle reads of one volume in one call (a server's concurrent reads):
 * every lost interval of every needle is rebuilt in one GPU batch.
 * statuses[i] = HEC_OK, HEC_ERR_IO (id not in .ecx) or HEC_ERR_NEEDLE_NOT_FOUND
 * (deleted); found needles' bytes go back to back into out, needle i at
 * [out_offsets[i], out_offsets[i+1]) (empty when not found); out_offsets has
 * n + 1 entries and is filled even when cap is too small (then
 * HEC_ERR_INVALID_ARGUMENT). A shard read or reconstruct failure fails the
 * whole call with that status. */
int hec_read_ec_needles(const char* base_filename, uint64_t large_block_size, uint64_t small_block_size,
                        const uint64_t* needle_ids, size_t n, uint8_t* out, size_t cap, uint64_t* out_offsets,
                        int* statuses);

/* ---- mounted EC volume (EcVolume, helyim-ec/src/volume/mod.rs:30-171) -------
 * A handle that keeps the volume's files open for a stream of reads, so a
 * needle read costs the lookup and the preads only. */
typedef struct hec_ec_volume hec_ec_volume_t;
/* EcVolume::new (mod.rs:45-92) + add_ec_shard (mod.rs:94-108) for every local
 * base.ecNN: opens base.ecx read-write (missing -> HEC_ERR_IO), opens or
 * creates base.ecj, loads the version from base.vif -- a missing .vif or one
 * whose `files` list is empty (maybe_load_volume_info, volume_info.rs:107-119)
 * is (re)written as the default VolumeInfo with version 2 -- and mounts every
 * shard file present. 1 GiB / 1 MiB blocks (ERASURE_CODING_*_BLOCK_SIZE). */
int hec_ec_volume_open(const char* base_filename, hec_ec_volume_t** out);
/* hec_ec_volume_open with explicit block sizes (tests exercise large rows). */
int hec_ec_volume_open_ex(const char* base_filename, uint64_t large_block_size, uint64_t small_block_size,
                          hec_ec_volume_t** out);
void hec_ec_volume_close(hec_ec_volume_t* vol);
/* EcVolume::version; 0 for a null handle. */
uint32_t hec_ec_volume_version(const hec_ec_volume_t* vol);
/* Bit i set = shard i mounted. */
uint32_t hec_ec_volume_shard_bits(const hec_ec_volume_t* vol);
/* find_needle_from_ecx (mod.rs:153-155), as hec_find_needle_from_ecx. */
int hec_ec_volume_find_needle(const hec_ec_volume_t* vol, uint64_t needle_id, uint32_t* offset, int32_t* size);
/* delete_needle_from_ecx (mod.rs:157-171): the entry's size becomes the
 * tombstone (-1) in .ecx (mark_needle_deleted, lib.rs:88-93) and the id is
 * appended to .ecj (8 bytes, big-endian). Absent id -> HEC_ERR_IO ("Needle {id}
 * is not found"), nothing written. Deletes are serialised per handle. */
int hec_ec_volume_delete_needle(hec_ec_volume_t* vol, uint64_t needle_id);
/* hec_read_ec_needle / hec_read_ec_needles against the mounted files (same
 * arguments, statuses and errors). Reads may run concurrently on one handle. */
int hec_ec_volume_read_needle(hec_ec_volume_t* vol, uint64_t needle_id, uint8_t* out, size_t cap, size_t* n_out);
int hec_ec_volume_read_needles(hec_ec_volume_t* vol, const uint64_t* needle_ids, size_t n, uint8_t* out, size_t cap,
                               uint64_t* out_offsets, int* statuses);

/* ---- tuning / introspection ----------------------------------------------- */
/* Kernel choice has no knob: it follows the shard length, the alignment and
 * where the bytes live (hec_*_kernel_name below report it). The knobs left
 * (process-wide, results identical) are the host paths' thresholds and mode. */
/* Host-memory encode / reconstruct calls whose input (data shards x shard
 * length) is at most max_bytes are packed into pinned staging and moved with
 * one H2D and one D2H copy; larger calls copy each shard directly. 0 disables
 * staging. Default 16 MiB (the measured crossover). Speed only. Returns HEC_OK. */
int hec_set_host_staging(uint64_t max_bytes);
/* Host batches (and the per-call and degraded-read staging): 1 = zero-copy
 * kernels that stream host memory over PCIe themselves (default), 0 = the
 * copy pipeline: DMA copies H2D -> kernel at HBM speed -> D2H over 3 HIP
 * streams, so the CUs are not held for the transfer (a GPU shared with other
 * work) at a lower link rate (41-44 against 51-53 GiB/s of data, DESIGN.md
 * section 5). Identical results. Returns HEC_OK. */
int hec_set_host_zero_copy(int on);
/* Name of the kernel a zero-copy host-batch encode of this shard length runs
 * (static string): over PCIe the 8-byte-per-lane table encode where the shard
 * length is a multiple of 2 KiB (~3.5% faster there than the bit-sliced kernel,
 * profiles/r04/e2e_encode_kernels_{v,w}.jsonl). */
const char* hec_host_encode_kernel_name(uint64_t shard_len);
/* Diagnostic: *zero_copy = 1 when [p, p + bytes) is one pinned range the
 * current device can address, i.e. host batches on it are coded zero-copy
 * (hec_host_alloc, hec_host_alloc_multi, hipHostMalloc, torch pin_memory),
 * 0 when they go through staging copies (pageable memory), or with
 * hec_set_host_zero_copy(0). */
int hec_host_zero_copy_view(const void* p, uint64_t bytes, int* zero_copy);
/* Diagnostic: host-batch pipelines of the current device (at most 8; only
 * the first 2 keep their staging between calls, the others free it when
 * their call ends) and the pinned host / device staging bytes they hold now.
 * Waits for calls in flight on those pipelines. */
int hec_host_staging_stats(int* n_pipelines, uint64_t* pinned_bytes, uint64_t* device_bytes);
/* Host-memory calls coded zero-copy whose input is at most max_bytes learn
 * that the kernel finished from a flag the kernel's last workgroup stores in
 * pinned memory (the caller spins on it, up to 200 us, then falls back to a
 * stream synchronise) instead of hipStreamSynchronize: ~4 us less per small
 * call. 0 disables. Default 1 MiB. Speed only. Returns HEC_OK. */
int hec_set_completion_signal(uint64_t max_bytes);
/* Version string of the library build. */
const char* hec_version(void);
/* Name of the kernel a 16-byte-aligned RS(10,4) device batch encode of this
 * shard length runs (static string;
 * shard_len 0, which fails with HEC_ERR_EMPTY_SHARD before any launch, names
 * no kernel: "none (...)"). */
const char* hec_encode_kernel_name(uint64_t shard_len);
/* Same for a 16-byte-aligned in-place RS(10,4) device batch reconstruct. */
const char* hec_decode_kernel_name(uint64_t shard_len);
/* Kernel an aligned hec_gpu_reconstruct_some_batch of one stripe of this shard
 * length runs, and the kernel the call runs on a whole batch with this base,
 * strides and stripe count (odd bases or strides: the generic one). */
const char* hec_reconstruct_some_kernel_name(uint64_t shard_len);
const char* hec_reconstruct_some_batch_kernel_name(const uint8_t* d_shards, uint64_t stripe_stride,
                                                   uint64_t shard_stride, uint64_t shard_len,
                                                   uint32_t n_stripes);
/* Same for a 16-byte-aligned hec_gpu_update_batch of one stripe. */
const char* hec_update_kernel_name(uint64_t shard_len);
/* Kernel hec_gpu_update_ragged runs with d_old given (with_old != 0) or NULL. */
const char* hec_update_ragged_kernel_name(int with_old);
/* Same for a 16-byte-aligned RS(10,4) device batch verify. */
const char* hec_verify_kernel_name(uint64_t shard_len);
/* Same for a 16-byte-aligned hec_gpu_verify_present_batch (masked verify). */
const char* hec_check_kernel_name(uint64_t shard_len);
/* Kernel hec_gpu_encode_ragged (decode = 0) or hec_gpu_reconstruct_ragged
 * (decode != 0) runs on these descriptors: the same choice the launch makes
 * (static string). */
const char* hec_ragged_kernel_name(const hec_stripe_desc* descs, uint32_t n_stripes, int decode);
/* Pass-1 kernel hec_gpu_verify_ragged / hec_gpu_locate_corrupt_ragged run on
 * these descriptors: the same choice the launch makes (static string). */
const char* hec_ragged_scrub_kernel_name(const hec_stripe_desc* descs, uint32_t n_stripes);

#ifdef __cplusplus
}
#endif
#endif /* HEC_H */
