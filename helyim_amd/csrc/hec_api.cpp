// C ABI of libhec (include/hec.h): device selection, version, knobs and the
// device batch entry points. All compute goes through the gfx950 kernels in
// rs_kernels.hip; there is no CPU fallback.
#include "hec_internal.hpp"

namespace hec {

int current_device(int* dev) {
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        (void)hipGetLastError();
        return fail(HEC_ERR_NO_DEVICE, "no HIP device visible (libhec has no CPU fallback)");
    }
    HEC_HIP(hipGetDevice(dev));
    return HEC_OK;
}

}  // namespace hec

using namespace hec;

extern "C" {

const char* hec_version(void) { return "libhec 0.2.0 (gfx950)"; }

int hec_device_count(int* count) {
    if (!count) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    *count = 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        (void)hipGetLastError();
        return fail(HEC_ERR_NO_DEVICE, "no HIP device visible (libhec has no CPU fallback)");
    }
    *count = n;
    return HEC_OK;
}

int hec_set_device(int device) {
    int n;
    int rc = hec_device_count(&n);
    if (rc) return rc;
    if (device < 0 || device >= n)
        return fail(HEC_ERR_INVALID_ARGUMENT, "device " + std::to_string(device) + " of " + std::to_string(n));
    HEC_HIP(hipSetDevice(device));
    return HEC_OK;
}

int hec_get_device(int* device) {
    if (!device) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    return current_device(device);
}

const char* hec_encode_kernel_name(uint64_t shard_len) { return encode_kernel_name(shard_len, false); }
const char* hec_decode_kernel_name(uint64_t shard_len) { return decode_kernel_name(shard_len); }
const char* hec_verify_kernel_name(uint64_t shard_len) { return verify_kernel_name(shard_len); }
const char* hec_host_encode_kernel_name(uint64_t shard_len) {
    return encode_kernel_name(shard_len, true);
}

int hec_set_host_staging(uint64_t max_bytes) {
    host_staging_max() = max_bytes;
    return HEC_OK;
}

int hec_set_completion_signal(uint64_t max_bytes) {
    completion_flag_max() = max_bytes;
    return HEC_OK;
}

int hec_gpu_encode_batch(const hec_rs_t* rs, const uint8_t* d_data, uint64_t data_stripe_stride,
                         uint64_t data_shard_stride, uint8_t* d_parity, uint64_t parity_stripe_stride,
                         uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes, void* stream) {
    const Batch b = Batch::split(arena(d_data, data_stripe_stride, data_shard_stride),
                                 arena(d_parity, parity_stripe_stride, parity_shard_stride), shard_len, n_stripes);
    HEC_TRY(check_batch_args(rs, b));
    HEC_TRY(check_encode_strides(rs, b));
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    return run_apply(gd->encode, uint32_t(rs->k), b, nullptr, nullptr, static_cast<hipStream_t>(stream));
}

int hec_gpu_reconstruct_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride, uint64_t shard_stride,
                              uint64_t shard_len, uint32_t n_stripes, const uint32_t* d_present_masks,
                              uint32_t* d_bad_stripes, void* stream) {
    const Batch b = Batch::in_place(arena(d_shards, stripe_stride, shard_stride), shard_len, n_stripes);
    HEC_TRY(check_batch_args(rs, d_shards, d_present_masks, shard_len));
    HEC_TRY(check_strided("shards", uint32_t(rs->n), b.in, shard_len, n_stripes));
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HEC_TRY(ensure_dense_decode(rs, gd, s));
    return run_apply(gd->decode_dense, uint32_t(rs->k), b, d_present_masks, d_bad_stripes, s);
}

int hec_gpu_reconstruct_some_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                   uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                   const uint32_t* d_present_masks, const uint32_t* d_want_masks,
                                   uint32_t* d_bad_stripes, void* stream) {
    const Batch b = Batch::in_place(arena(d_shards, stripe_stride, shard_stride), shard_len, n_stripes);
    HEC_TRY(check_some_args(rs, b, d_present_masks, d_want_masks));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HEC_TRY(ensure_dense_decode(rs, gd, s));
    return run_some(gd->decode_dense, 10, b, d_present_masks, d_want_masks, d_bad_stripes, s);
}

const char* hec_reconstruct_some_kernel_name(uint64_t shard_len) { return some_kernel_name(shard_len); }
const char* hec_reconstruct_some_batch_kernel_name(const uint8_t* d_shards, uint64_t stripe_stride,
                                                   uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes) {
    const Batch b = Batch::in_place(arena(d_shards, stripe_stride, shard_stride), shard_len, n_stripes);
    return some_batch_kernel_name(shard_len, n_stripes, b.aligned());
}

int hec_gpu_update_batch(const hec_rs_t* rs, const uint8_t* d_old, uint64_t old_stripe_stride,
                         uint64_t old_shard_stride, const uint8_t* d_new, uint64_t new_stripe_stride,
                         uint64_t new_shard_stride, uint8_t* d_parity, uint64_t parity_stripe_stride,
                         uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes,
                         const uint32_t* d_update_masks, void* stream) {
    const Strided old = arena(d_old, old_stripe_stride, old_shard_stride);
    const Batch b = Batch::split(arena(d_new, new_stripe_stride, new_shard_stride),
                                 arena(d_parity, parity_stripe_stride, parity_shard_stride), shard_len, n_stripes);
    HEC_TRY(check_update_args(rs, old, b, d_update_masks));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    return run_update(gd->encode, old, b, d_update_masks, static_cast<hipStream_t>(stream));
}

const char* hec_update_kernel_name(uint64_t shard_len) { return update_kernel_name(shard_len); }

// The scrubs of separate data and parity arenas (hec_gpu_verify_batch, the
// locates and the corrects): one body. spec: the pass 2 and its pairs form.
static int scrub_batch(const hec_rs_t* rs, const uint8_t* d_data, uint64_t data_stripe_stride,
                       uint64_t data_shard_stride, const uint8_t* d_parity, uint64_t parity_stripe_stride,
                       uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes, Pass2 pass2, bool pairs,
                       const ScrubOut& out, void* stream) {
    const Batch b = Batch::split(arena(d_data, data_stripe_stride, data_shard_stride),
                                 arena(d_parity, parity_stripe_stride, parity_shard_stride), shard_len, n_stripes);
    HEC_TRY(check_batch_args(rs, b));
    HEC_TRY(check_verify_args(rs, out.words));
    if (pass2 != Pass2::None) HEC_TRY(check_locate_args(rs, out.suspects));
    HEC_TRY(check_encode_strides(rs, b));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    ScrubSpec spec;
    spec.pass2 = pass2;
    spec.pairs = pairs;
    return run_scrub(*gd, b, spec, out, static_cast<hipStream_t>(stream));
}
// The two word arrays of a scrub's results; the counters are set by name.
static ScrubOut scrub_words(uint32_t* words, uint32_t* suspects = nullptr) {
    ScrubOut out;
    out.words = words;
    out.suspects = suspects;
    return out;
}

int hec_gpu_verify_batch(const hec_rs_t* rs, const uint8_t* d_data, uint64_t data_stripe_stride,
                         uint64_t data_shard_stride, const uint8_t* d_parity, uint64_t parity_stripe_stride,
                         uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch,
                         uint32_t* d_bad_stripes, void* stream) {
    ScrubOut out = scrub_words(d_mismatch);
    out.bad = d_bad_stripes;
    return scrub_batch(rs, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                       parity_shard_stride, shard_len, n_stripes, Pass2::None, false, out, stream);
}

int hec_gpu_locate_corrupt_batch(const hec_rs_t* rs, const uint8_t* d_data, uint64_t data_stripe_stride,
                                 uint64_t data_shard_stride, const uint8_t* d_parity, uint64_t parity_stripe_stride,
                                 uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                 uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_bad_stripes, void* stream) {
    ScrubOut out = scrub_words(d_mismatch, d_suspects);
    out.bad = d_bad_stripes;
    return scrub_batch(rs, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                       parity_shard_stride, shard_len, n_stripes, Pass2::Locate, false, out, stream);
}

int hec_gpu_locate_corrupt_pairs_batch(const hec_rs_t* rs, const uint8_t* d_data, uint64_t data_stripe_stride,
                                       uint64_t data_shard_stride, const uint8_t* d_parity,
                                       uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                                       uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch,
                                       uint32_t* d_suspects, uint32_t* d_bad_stripes, void* stream) {
    ScrubOut out = scrub_words(d_mismatch, d_suspects);
    out.bad = d_bad_stripes;
    return scrub_batch(rs, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                       parity_shard_stride, shard_len, n_stripes, Pass2::Locate, true, out, stream);
}

int hec_gpu_correct_batch(const hec_rs_t* rs, uint8_t* d_data, uint64_t data_stripe_stride,
                          uint64_t data_shard_stride, uint8_t* d_parity, uint64_t parity_stripe_stride,
                          uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch,
                          uint32_t* d_suspects, uint32_t* d_bad_stripes, uint32_t* d_uncorrected,
                          unsigned long long* d_corrected_bytes, void* stream) {
    ScrubOut out = scrub_words(d_mismatch, d_suspects);
    out.bad = d_bad_stripes;
    out.left = d_uncorrected;
    out.corrected_bytes = d_corrected_bytes;
    return scrub_batch(rs, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                       parity_shard_stride, shard_len, n_stripes, Pass2::Correct, false, out, stream);
}

int hec_gpu_correct_pairs_batch(const hec_rs_t* rs, uint8_t* d_data, uint64_t data_stripe_stride,
                                uint64_t data_shard_stride, uint8_t* d_parity, uint64_t parity_stripe_stride,
                                uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_bad_stripes,
                                uint32_t* d_uncorrected, unsigned long long* d_corrected_bytes, void* stream) {
    ScrubOut out = scrub_words(d_mismatch, d_suspects);
    out.bad = d_bad_stripes;
    out.left = d_uncorrected;
    out.corrected_bytes = d_corrected_bytes;
    return scrub_batch(rs, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                       parity_shard_stride, shard_len, n_stripes, Pass2::Correct, true, out, stream);
}

// hec_gpu_repair_batch and its pairs form: one body.
static int repair_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride, uint64_t shard_stride,
                        uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch, uint32_t* d_suspects,
                        uint32_t* d_present_masks, uint32_t* d_unrepaired, void* stream, bool pairs) {
    if (!rs || !d_shards || !d_mismatch || !d_suspects || !d_present_masks)
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (shard_len == 0) return fail(HEC_ERR_EMPTY_SHARD, "");
    HEC_TRY(check_locate_args(rs, d_suspects));  // the codec
    const Strided shards = arena(d_shards, stripe_stride, shard_stride);
    HEC_TRY(check_strided("shards", uint32_t(rs->n), shards, shard_len, n_stripes));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HEC_TRY(ensure_dense_decode(rs, gd, s));  // before any launch: its first call uploads and waits
    ScrubSpec spec;
    spec.pass2 = Pass2::Locate;
    spec.pairs = pairs;
    HEC_TRY(run_scrub(*gd, Batch::split_at(shards, rs->k, shard_len, n_stripes), spec,
                      scrub_words(d_mismatch, d_suspects), s));
    HEC_HIP(launch_repair_masks(d_suspects, d_present_masks, d_unrepaired, n_stripes, s));
    // a stripe left alone has every shard present: the reconstruct's no-op
    return run_apply(gd->decode_dense, uint32_t(rs->k), Batch::in_place(shards, shard_len, n_stripes),
                     d_present_masks, nullptr, s);
}

int hec_gpu_repair_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride, uint64_t shard_stride,
                         uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch, uint32_t* d_suspects,
                         uint32_t* d_present_masks, uint32_t* d_unrepaired, void* stream) {
    return repair_batch(rs, d_shards, stripe_stride, shard_stride, shard_len, n_stripes, d_mismatch, d_suspects,
                        d_present_masks, d_unrepaired, stream, false);
}

int hec_gpu_repair_pairs_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride, uint64_t shard_stride,
                               uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch, uint32_t* d_suspects,
                               uint32_t* d_present_masks, uint32_t* d_unrepaired, void* stream) {
    return repair_batch(rs, d_shards, stripe_stride, shard_stride, shard_len, n_stripes, d_mismatch, d_suspects,
                        d_present_masks, d_unrepaired, stream, true);
}

// The masked entry points, after each one's own null check: the shared
// argument checks, the plan sets (every one before any launch: their first
// call uploads and waits; decode: the reconstructs' too), then the scrub.
// *gd_out (the reconstructs' tail needs it) is set unless the batch is empty.
static int scrub_present(const hec_rs_t* rs, const Batch& b, const ScrubSpec& spec, const ScrubOut& out, bool decode,
                         hipStream_t s, GeomDevice** gd_out = nullptr) {
    HEC_TRY(check_present_args(rs, b, spec.masks, out.words));
    HEC_TRY(check_min_spares(spec.min_spares));
    if (b.n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    HEC_TRY(ensure_check_plans(rs, gd, s));
    if (decode) HEC_TRY(ensure_dense_decode(rs, gd, s));
    if (gd_out) *gd_out = gd;
    return run_scrub(*gd, b, spec, out, s);
}
static ScrubSpec present_spec(const uint32_t* masks, Pass2 pass2, uint32_t min_spares = 2) {
    ScrubSpec spec;
    spec.masks = masks;
    spec.pass2 = pass2;
    spec.min_spares = min_spares;
    return spec;
}

int hec_gpu_verify_present_batch(const hec_rs_t* rs, const uint8_t* d_shards, uint64_t stripe_stride,
                                 uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                 const uint32_t* d_present_masks, uint32_t* d_check, uint32_t* d_bad_stripes,
                                 uint32_t* d_unchecked, void* stream) {
    ScrubOut out = scrub_words(d_check);
    out.bad = d_bad_stripes;
    out.unchecked = d_unchecked;
    return scrub_present(rs, Batch::in_place(arena(d_shards, stripe_stride, shard_stride), shard_len, n_stripes),
                         present_spec(d_present_masks, Pass2::None), out, false, static_cast<hipStream_t>(stream));
}

int hec_gpu_locate_corrupt_present_batch(const hec_rs_t* rs, const uint8_t* d_shards, uint64_t stripe_stride,
                                         uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                         const uint32_t* d_present_masks, uint32_t* d_check, uint32_t* d_suspects,
                                         uint32_t* d_bad_stripes, uint32_t* d_unchecked, void* stream) {
    if (rs && d_shards && d_present_masks && d_check && !d_suspects)
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    ScrubOut out = scrub_words(d_check, d_suspects);
    out.bad = d_bad_stripes;
    out.unchecked = d_unchecked;
    return scrub_present(rs, Batch::in_place(arena(d_shards, stripe_stride, shard_stride), shard_len, n_stripes),
                         present_spec(d_present_masks, Pass2::Locate), out, false, static_cast<hipStream_t>(stream));
}

int hec_gpu_reconstruct_checked_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                      uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                      const uint32_t* d_present_masks, uint32_t* d_check, uint32_t* d_suspects,
                                      uint32_t* d_use_masks, uint32_t* d_bad_stripes, uint32_t* d_unrepaired,
                                      void* stream) {
    if (rs && d_shards && d_present_masks && d_check && (!d_suspects || !d_use_masks))
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    const Batch b = Batch::in_place(arena(d_shards, stripe_stride, shard_stride), shard_len, n_stripes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    GeomDevice* gd = nullptr;
    HEC_TRY(scrub_present(rs, b, present_spec(d_present_masks, Pass2::Locate), scrub_words(d_check, d_suspects), true,
                          s, &gd));
    if (n_stripes == 0) return HEC_OK;
    HEC_HIP(launch_use_masks(d_present_masks, d_check, d_suspects, d_use_masks, d_unrepaired, n_stripes, s));
    // a stripe left alone has every shard "present": the reconstruct's no-op
    return run_apply(gd->decode_dense, uint32_t(rs->k), b, d_use_masks, d_bad_stripes, s);
}

int hec_gpu_correct_present_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                  uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                  const uint32_t* d_present_masks, uint32_t min_spares, uint32_t* d_check,
                                  uint32_t* d_suspects, uint32_t* d_bad_stripes, uint32_t* d_unchecked,
                                  uint32_t* d_uncorrected, unsigned long long* d_corrected_bytes, void* stream) {
    if (rs && d_shards && d_present_masks && d_check && !d_suspects)
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    ScrubOut out = scrub_words(d_check, d_suspects);
    out.bad = d_bad_stripes;
    out.unchecked = d_unchecked;
    out.left = d_uncorrected;
    out.corrected_bytes = d_corrected_bytes;
    return scrub_present(rs, Batch::in_place(arena(d_shards, stripe_stride, shard_stride), shard_len, n_stripes),
                         present_spec(d_present_masks, Pass2::Correct, min_spares), out, false,
                         static_cast<hipStream_t>(stream));
}

int hec_gpu_reconstruct_corrected_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                        uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                        const uint32_t* d_present_masks, uint32_t min_spares, uint32_t* d_check,
                                        uint32_t* d_suspects, uint32_t* d_use_masks, uint32_t* d_bad_stripes,
                                        uint32_t* d_unrepaired, unsigned long long* d_corrected_bytes, void* stream) {
    if (rs && d_shards && d_present_masks && d_check && (!d_suspects || !d_use_masks))
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    const Batch b = Batch::in_place(arena(d_shards, stripe_stride, shard_stride), shard_len, n_stripes);
    hipStream_t s = static_cast<hipStream_t>(stream);
    GeomDevice* gd = nullptr;
    ScrubOut out = scrub_words(d_check, d_suspects);  // the counts are the masks kernel's and the decode's
    out.corrected_bytes = d_corrected_bytes;
    HEC_TRY(scrub_present(rs, b, present_spec(d_present_masks, Pass2::Correct, min_spares), out, true, s, &gd));
    if (n_stripes == 0) return HEC_OK;
    HEC_HIP(launch_use_masks_corrected(d_present_masks, d_check, d_suspects, d_use_masks, d_unrepaired, min_spares,
                                       n_stripes, s));
    // a stripe left alone has every shard "present": the reconstruct's no-op
    return run_apply(gd->decode_dense, uint32_t(rs->k), b, d_use_masks, d_bad_stripes, s);
}

const char* hec_check_kernel_name(uint64_t shard_len) { return check_kernel_name(shard_len); }

int hec_gpu_fill_splitmix(uint8_t* d_base, uint64_t stripe_stride, uint64_t bytes_per_stripe, uint32_t n_stripes,
                          uint64_t seed_base, void* stream) {
    if (!d_base) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    int dev;
    int rc = current_device(&dev);
    if (rc) return rc;
    HEC_HIP(launch_fill_splitmix(d_base, stripe_stride, bytes_per_stripe, n_stripes, seed_base,
                                 static_cast<hipStream_t>(stream)));
    return HEC_OK;
}

}  // extern "C"
