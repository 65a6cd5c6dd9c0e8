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
    HEC_TRY(check_batch_args(rs, d_data, d_parity, shard_len));
    HEC_TRY(check_encode_strides(rs, data_stripe_stride, data_shard_stride, parity_stripe_stride,
                                 parity_shard_stride, shard_len, n_stripes));
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    return run_apply(gd->encode, uint32_t(rs->k), d_data, data_stripe_stride, data_shard_stride, d_parity,
                     parity_stripe_stride, parity_shard_stride, shard_len, n_stripes, nullptr, nullptr,
                     static_cast<hipStream_t>(stream));
}

int hec_gpu_reconstruct_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride, uint64_t shard_stride,
                              uint64_t shard_len, uint32_t n_stripes, const uint32_t* d_present_masks,
                              uint32_t* d_bad_stripes, void* stream) {
    HEC_TRY(check_batch_args(rs, d_shards, d_present_masks, shard_len));
    HEC_TRY(check_strided("shards", uint32_t(rs->n), stripe_stride, shard_stride, shard_len, n_stripes));
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HEC_TRY(ensure_dense_decode(rs, gd, s));
    return run_apply(gd->decode_dense, uint32_t(rs->k), d_shards, stripe_stride, shard_stride, d_shards,
                     stripe_stride, shard_stride, shard_len, n_stripes, d_present_masks, d_bad_stripes, s);
}

int hec_gpu_reconstruct_some_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                   uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                   const uint32_t* d_present_masks, const uint32_t* d_want_masks,
                                   uint32_t* d_bad_stripes, void* stream) {
    HEC_TRY(check_some_args(rs, d_shards, d_present_masks, d_want_masks, stripe_stride, shard_stride, shard_len,
                            n_stripes));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HEC_TRY(ensure_dense_decode(rs, gd, s));
    return run_some(gd->decode_dense, 10, d_shards, stripe_stride, shard_stride, shard_len, n_stripes, d_present_masks,
                    d_want_masks, d_bad_stripes, s);
}

const char* hec_reconstruct_some_kernel_name(uint64_t shard_len) { return some_kernel_name(shard_len); }
const char* hec_reconstruct_some_batch_kernel_name(const uint8_t* d_shards, uint64_t stripe_stride,
                                                   uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes) {
    const uint64_t align = uint64_t(reinterpret_cast<uintptr_t>(d_shards)) | stripe_stride | shard_stride;
    return some_batch_kernel_name(shard_len, n_stripes, align % 16 == 0);
}

int hec_gpu_verify_batch(const hec_rs_t* rs, const uint8_t* d_data, uint64_t data_stripe_stride,
                         uint64_t data_shard_stride, const uint8_t* d_parity, uint64_t parity_stripe_stride,
                         uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch,
                         uint32_t* d_bad_stripes, void* stream) {
    HEC_TRY(check_batch_args(rs, d_data, d_parity, shard_len));
    HEC_TRY(check_verify_args(rs, d_mismatch));
    HEC_TRY(check_encode_strides(rs, data_stripe_stride, data_shard_stride, parity_stripe_stride,
                                 parity_shard_stride, shard_len, n_stripes));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    return run_verify(gd->encode, uint32_t(rs->k), d_data, data_stripe_stride, data_shard_stride, d_parity,
                      parity_stripe_stride, parity_shard_stride, shard_len, n_stripes, d_mismatch, d_bad_stripes,
                      static_cast<hipStream_t>(stream));
}

// hec_gpu_locate_corrupt_batch and its pairs form: one body.
static int locate_batch(const hec_rs_t* rs, const uint8_t* d_data, uint64_t data_stripe_stride,
                        uint64_t data_shard_stride, const uint8_t* d_parity, uint64_t parity_stripe_stride,
                        uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch,
                        uint32_t* d_suspects, uint32_t* d_bad_stripes, void* stream, bool pairs) {
    HEC_TRY(check_batch_args(rs, d_data, d_parity, shard_len));
    HEC_TRY(check_verify_args(rs, d_mismatch));
    HEC_TRY(check_locate_args(rs, d_suspects));
    HEC_TRY(check_encode_strides(rs, data_stripe_stride, data_shard_stride, parity_stripe_stride,
                                 parity_shard_stride, shard_len, n_stripes));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    return run_locate(*gd, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                      parity_shard_stride, shard_len, n_stripes, d_mismatch, d_suspects, d_bad_stripes,
                      static_cast<hipStream_t>(stream), pairs);
}

int hec_gpu_locate_corrupt_batch(const hec_rs_t* rs, const uint8_t* d_data, uint64_t data_stripe_stride,
                                 uint64_t data_shard_stride, const uint8_t* d_parity, uint64_t parity_stripe_stride,
                                 uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                 uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_bad_stripes, void* stream) {
    return locate_batch(rs, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                        parity_shard_stride, shard_len, n_stripes, d_mismatch, d_suspects, d_bad_stripes, stream,
                        false);
}

int hec_gpu_locate_corrupt_pairs_batch(const hec_rs_t* rs, const uint8_t* d_data, uint64_t data_stripe_stride,
                                       uint64_t data_shard_stride, const uint8_t* d_parity,
                                       uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                                       uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch,
                                       uint32_t* d_suspects, uint32_t* d_bad_stripes, void* stream) {
    return locate_batch(rs, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                        parity_shard_stride, shard_len, n_stripes, d_mismatch, d_suspects, d_bad_stripes, stream,
                        true);
}

// hec_gpu_correct_batch and its pairs form: one body.
static int correct_batch(const hec_rs_t* rs, uint8_t* d_data, uint64_t data_stripe_stride, uint64_t data_shard_stride,
                         uint8_t* d_parity, uint64_t parity_stripe_stride, uint64_t parity_shard_stride,
                         uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch, uint32_t* d_suspects,
                         uint32_t* d_bad_stripes, uint32_t* d_uncorrected, unsigned long long* d_corrected_bytes,
                         void* stream, bool pairs) {
    HEC_TRY(check_batch_args(rs, d_data, d_parity, shard_len));
    HEC_TRY(check_verify_args(rs, d_mismatch));
    HEC_TRY(check_locate_args(rs, d_suspects));
    HEC_TRY(check_encode_strides(rs, data_stripe_stride, data_shard_stride, parity_stripe_stride,
                                 parity_shard_stride, shard_len, n_stripes));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    return run_correct(*gd, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                       parity_shard_stride, shard_len, n_stripes, d_mismatch, d_suspects, d_bad_stripes,
                       d_uncorrected, d_corrected_bytes, static_cast<hipStream_t>(stream), pairs);
}

int hec_gpu_correct_batch(const hec_rs_t* rs, uint8_t* d_data, uint64_t data_stripe_stride,
                          uint64_t data_shard_stride, uint8_t* d_parity, uint64_t parity_stripe_stride,
                          uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch,
                          uint32_t* d_suspects, uint32_t* d_bad_stripes, uint32_t* d_uncorrected,
                          unsigned long long* d_corrected_bytes, void* stream) {
    return correct_batch(rs, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                         parity_shard_stride, shard_len, n_stripes, d_mismatch, d_suspects, d_bad_stripes,
                         d_uncorrected, d_corrected_bytes, stream, false);
}

int hec_gpu_correct_pairs_batch(const hec_rs_t* rs, uint8_t* d_data, uint64_t data_stripe_stride,
                                uint64_t data_shard_stride, uint8_t* d_parity, uint64_t parity_stripe_stride,
                                uint64_t parity_shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                uint32_t* d_mismatch, uint32_t* d_suspects, uint32_t* d_bad_stripes,
                                uint32_t* d_uncorrected, unsigned long long* d_corrected_bytes, void* stream) {
    return correct_batch(rs, d_data, data_stripe_stride, data_shard_stride, d_parity, parity_stripe_stride,
                         parity_shard_stride, shard_len, n_stripes, d_mismatch, d_suspects, d_bad_stripes,
                         d_uncorrected, d_corrected_bytes, stream, true);
}

// hec_gpu_repair_batch and its pairs form: one body.
static int repair_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride, uint64_t shard_stride,
                        uint64_t shard_len, uint32_t n_stripes, uint32_t* d_mismatch, uint32_t* d_suspects,
                        uint32_t* d_present_masks, uint32_t* d_unrepaired, void* stream, bool pairs) {
    if (!rs || !d_shards || !d_mismatch || !d_suspects || !d_present_masks)
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (shard_len == 0) return fail(HEC_ERR_EMPTY_SHARD, "");
    HEC_TRY(check_locate_args(rs, d_suspects));  // the codec
    HEC_TRY(check_strided("shards", uint32_t(rs->n), stripe_stride, shard_stride, shard_len, n_stripes));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HEC_TRY(ensure_dense_decode(rs, gd, s));  // before any launch: its first call uploads and waits
    const uint8_t* parity = d_shards + uint64_t(rs->k) * shard_stride;
    HEC_TRY(run_locate(*gd, d_shards, stripe_stride, shard_stride, parity, stripe_stride, shard_stride, shard_len,
                       n_stripes, d_mismatch, d_suspects, nullptr, s, pairs));
    HEC_HIP(launch_repair_masks(d_suspects, d_present_masks, d_unrepaired, n_stripes, s));
    // a stripe left alone has every shard present: the reconstruct's no-op
    return run_apply(gd->decode_dense, uint32_t(rs->k), d_shards, stripe_stride, shard_stride, d_shards, stripe_stride,
                     shard_stride, shard_len, n_stripes, d_present_masks, nullptr, s);
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

int hec_gpu_verify_present_batch(const hec_rs_t* rs, const uint8_t* d_shards, uint64_t stripe_stride,
                                 uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                 const uint32_t* d_present_masks, uint32_t* d_check, uint32_t* d_bad_stripes,
                                 uint32_t* d_unchecked, void* stream) {
    HEC_TRY(check_present_args(rs, d_shards, d_present_masks, d_check, stripe_stride, shard_stride, shard_len,
                               n_stripes));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HEC_TRY(ensure_check_plans(rs, gd, s));
    return run_check(*gd, d_shards, stripe_stride, shard_stride, shard_len, n_stripes, d_present_masks, d_check,
                     d_bad_stripes, d_unchecked, s);
}

int hec_gpu_locate_corrupt_present_batch(const hec_rs_t* rs, const uint8_t* d_shards, uint64_t stripe_stride,
                                         uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                         const uint32_t* d_present_masks, uint32_t* d_check, uint32_t* d_suspects,
                                         uint32_t* d_bad_stripes, uint32_t* d_unchecked, void* stream) {
    if (rs && d_shards && d_present_masks && d_check && !d_suspects)
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    HEC_TRY(check_present_args(rs, d_shards, d_present_masks, d_check, stripe_stride, shard_stride, shard_len,
                               n_stripes));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HEC_TRY(ensure_check_plans(rs, gd, s));
    return run_locate_present(*gd, d_shards, stripe_stride, shard_stride, shard_len, n_stripes, d_present_masks,
                              d_check, d_suspects, d_bad_stripes, d_unchecked, s);
}

int hec_gpu_reconstruct_checked_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                      uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                      const uint32_t* d_present_masks, uint32_t* d_check, uint32_t* d_suspects,
                                      uint32_t* d_use_masks, uint32_t* d_bad_stripes, uint32_t* d_unrepaired,
                                      void* stream) {
    if (rs && d_shards && d_present_masks && d_check && (!d_suspects || !d_use_masks))
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    HEC_TRY(check_present_args(rs, d_shards, d_present_masks, d_check, stripe_stride, shard_stride, shard_len,
                               n_stripes));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // both plan sets before any launch: their first call uploads and waits
    HEC_TRY(ensure_check_plans(rs, gd, s));
    HEC_TRY(ensure_dense_decode(rs, gd, s));
    HEC_TRY(run_locate_present(*gd, d_shards, stripe_stride, shard_stride, shard_len, n_stripes, d_present_masks,
                               d_check, d_suspects, nullptr, nullptr, s));
    HEC_HIP(launch_use_masks(d_present_masks, d_check, d_suspects, d_use_masks, d_unrepaired, n_stripes, s));
    // a stripe left alone has every shard "present": the reconstruct's no-op
    return run_apply(gd->decode_dense, uint32_t(rs->k), d_shards, stripe_stride, shard_stride, d_shards, stripe_stride,
                     shard_stride, shard_len, n_stripes, d_use_masks, d_bad_stripes, s);
}

int hec_gpu_correct_present_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                  uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                  const uint32_t* d_present_masks, uint32_t min_spares, uint32_t* d_check,
                                  uint32_t* d_suspects, uint32_t* d_bad_stripes, uint32_t* d_unchecked,
                                  uint32_t* d_uncorrected, unsigned long long* d_corrected_bytes, void* stream) {
    if (rs && d_shards && d_present_masks && d_check && !d_suspects)
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    HEC_TRY(check_present_args(rs, d_shards, d_present_masks, d_check, stripe_stride, shard_stride, shard_len,
                               n_stripes));
    HEC_TRY(check_min_spares(min_spares));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    HEC_TRY(ensure_check_plans(rs, gd, s));
    return run_correct_present(*gd, d_shards, stripe_stride, shard_stride, shard_len, n_stripes, d_present_masks,
                               min_spares, d_check, d_suspects, d_bad_stripes, d_unchecked, d_uncorrected,
                               d_corrected_bytes, s);
}

int hec_gpu_reconstruct_corrected_batch(const hec_rs_t* rs, uint8_t* d_shards, uint64_t stripe_stride,
                                        uint64_t shard_stride, uint64_t shard_len, uint32_t n_stripes,
                                        const uint32_t* d_present_masks, uint32_t min_spares, uint32_t* d_check,
                                        uint32_t* d_suspects, uint32_t* d_use_masks, uint32_t* d_bad_stripes,
                                        uint32_t* d_unrepaired, unsigned long long* d_corrected_bytes, void* stream) {
    if (rs && d_shards && d_present_masks && d_check && (!d_suspects || !d_use_masks))
        return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    HEC_TRY(check_present_args(rs, d_shards, d_present_masks, d_check, stripe_stride, shard_stride, shard_len,
                               n_stripes));
    HEC_TRY(check_min_spares(min_spares));
    if (n_stripes == 0) return HEC_OK;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    hipStream_t s = static_cast<hipStream_t>(stream);
    // both plan sets before any launch: their first call uploads and waits
    HEC_TRY(ensure_check_plans(rs, gd, s));
    HEC_TRY(ensure_dense_decode(rs, gd, s));
    HEC_TRY(run_correct_present(*gd, d_shards, stripe_stride, shard_stride, shard_len, n_stripes, d_present_masks,
                                min_spares, d_check, d_suspects, nullptr, nullptr, nullptr, d_corrected_bytes, s));
    HEC_HIP(launch_use_masks_corrected(d_present_masks, d_check, d_suspects, d_use_masks, d_unrepaired, min_spares,
                                       n_stripes, s));
    // a stripe left alone has every shard "present": the reconstruct's no-op
    return run_apply(gd->decode_dense, uint32_t(rs->k), d_shards, stripe_stride, shard_stride, d_shards, stripe_stride,
                     shard_stride, shard_len, n_stripes, d_use_masks, d_bad_stripes, s);
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
