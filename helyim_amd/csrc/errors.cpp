// The thread-local error record behind every hec status: detail text and
// values (hec_last_error_detail / hec_last_error_values), and hec_strerror.
#include <cstring>

#include "hec_internal.hpp"

namespace hec {

static thread_local std::string g_detail;
static thread_local ErrorValues g_values;

void set_detail(const std::string& s) {
    g_detail = s;
    g_values = ErrorValues{};
}

int fail(int code, const std::string& detail) {
    set_detail(detail);
    return code;
}

int fail_values(int code, const std::string& detail, uint64_t a, uint64_t b) {
    set_detail(detail);
    g_values.a = a;
    g_values.b = b;
    return code;
}

int fail_errno(int code, const std::string& what, int err) {
    set_detail(what + ": " + std::strerror(err));
    g_values.os_errno = err;
    return code;
}

int fail_with(int code, const std::string& detail, const ErrorValues& v) {
    g_detail = detail;
    g_values = v;
    return code;
}

ErrorValues last_error_values() { return g_values; }

int hip_fail(hipError_t e, const char* what) {
    set_detail(std::string(what) + ": " + hipGetErrorString(e));
    if (e == hipErrorOutOfMemory) return HEC_ERR_OUT_OF_MEMORY;
    if (e == hipErrorNoDevice || e == hipErrorInvalidDevice) return HEC_ERR_NO_DEVICE;
    return HEC_ERR_HIP;
}

}  // namespace hec

using namespace hec;

extern "C" {

const char* hec_strerror(int status) {
    switch (status) {
        case HEC_OK: return "ok";
        // reed_solomon_erasure::Error Display texts (upstream 6.0.0)
        case HEC_ERR_TOO_FEW_SHARDS: return "The number of provided shards is smaller than the one in codec";
        case HEC_ERR_TOO_MANY_SHARDS: return "The number of provided shards is greater than the one in codec";
        case HEC_ERR_TOO_FEW_DATA_SHARDS: return "The number of provided data shards is smaller than the one in codec";
        case HEC_ERR_TOO_MANY_DATA_SHARDS: return "The number of provided data shards is greater than the one in codec";
        case HEC_ERR_TOO_FEW_PARITY_SHARDS: return "The number of provided parity shards is smaller than the one in codec";
        case HEC_ERR_TOO_MANY_PARITY_SHARDS: return "The number of provided parity shards is greater than the one in codec";
        case HEC_ERR_TOO_FEW_BUFFER_SHARDS: return "The number of provided buffer shards is smaller than the number of parity shards in codec";
        case HEC_ERR_TOO_MANY_BUFFER_SHARDS: return "The number of provided buffer shards is greater than the number of parity shards in codec";
        case HEC_ERR_INCORRECT_SHARD_SIZE: return "At least one of the provided shards is not of the correct size";
        case HEC_ERR_TOO_FEW_SHARDS_PRESENT: return "The number of shards present is smaller than number of parity shards, cannot reconstruct missing shards";
        case HEC_ERR_EMPTY_SHARD: return "The first shard provided is of zero length";
        case HEC_ERR_INVALID_SHARD_FLAGS: return "The number of flags does not match the total number of shards";
        case HEC_ERR_INVALID_INDEX: return "The data shard index provided is greater or equal to the number of data shards in codec";
        // helyim_ec::EcShardError (helyim-ec/src/errors.rs:55-66)
        case HEC_ERR_IO: return "Io error";
        case HEC_ERR_UNDERFLOW: return "Only {0} shards found but {0} required";
        case HEC_ERR_UNEXPECTED_EC_SHARD_SIZE: return "ec shard size expected {0} but actually is {1}";
        case HEC_ERR_UNEXPECTED_BLOCK_SIZE: return "unexpected block size {0}, buffer size {1}";
        case HEC_ERR_NEEDLE_NOT_FOUND: return "Needle not found in volume";
        case HEC_ERR_SHARD_NOT_FOUND: return "Shard not found in volume";
        case HEC_ERR_HIP: return "HIP runtime error";
        case HEC_ERR_NO_DEVICE: return "no usable GPU device";
        case HEC_ERR_INVALID_ARGUMENT: return "invalid argument";
        case HEC_ERR_OUT_OF_MEMORY: return "out of device memory";
        default: return "unknown status";
    }
}

const char* hec_last_error_detail(void) { return g_detail.c_str(); }

int hec_last_error_values(uint64_t* a, uint64_t* b, int* os_errno) {
    if (a) *a = g_values.a;
    if (b) *b = g_values.b;
    if (os_errno) *os_errno = g_values.os_errno;
    return HEC_OK;
}

}  // extern "C"
