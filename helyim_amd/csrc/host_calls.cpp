// The per-call host paths: the ReedSolomon<galois_8::Field> surface helyim-ec
// calls (encoder.rs:191,208-209,249-250,288;
// helyim-store/src/erasure_coding/mod.rs:411-412,426) on shards in host
// memory, through a leased per-device scratch (stream, staging, completion
// flag).
#include <chrono>
#include <cstring>

#include "hec_internal.hpp"

namespace hec {

std::atomic<bool>& zero_copy_enabled() {
    static std::atomic<bool> on{true};
    return on;
}

uint8_t* pinned_device_ptr(void* host) {
    void* d = nullptr;
    if (!host || hipHostGetDevicePointer(&d, host, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return static_cast<uint8_t*>(d);
}

std::atomic<uint64_t>& host_staging_max() {
    static std::atomic<uint64_t> v{uint64_t(16) << 20};  // measured crossover
    return v;
}

std::atomic<uint64_t>& completion_flag_max() {
    static std::atomic<uint64_t> v{uint64_t(1) << 20};
    return v;
}

int Completion::arm(hipStream_t s, uint32_t** count_out, uint32_t** flag_out, uint32_t* seq_out) {
    if (!host) {
        HEC_HIP(hipHostMalloc(reinterpret_cast<void**>(&host), 64, hipHostMallocCoherent));
        *host = 0;
        HEC_HIP(hipHostGetDevicePointer(reinterpret_cast<void**>(&dflag), host, 0));
        HEC_HIP(hipMalloc(reinterpret_cast<void**>(&count), 64));
        HEC_HIP(hipMemsetAsync(count, 0, 64, s));  // ordered before the first signalling launch
    }
    if (++seq == 0) seq = 1;  // 0 is the flag's initial value
    *count_out = count;
    *flag_out = dflag;
    *seq_out = seq;
    return HEC_OK;
}

int Completion::wait(hipStream_t s) {
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    while (__atomic_load_n(host, __ATOMIC_ACQUIRE) != seq) {
        if ((++spins & 255) == 0 &&
            std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(kSpinUs)) {
            const hipError_t e = hipStreamSynchronize(s);
            if (e == hipSuccess && __atomic_load_n(host, __ATOMIC_ACQUIRE) == seq) return HEC_OK;
            // a launch that did not finish every workgroup leaves the arrival
            // count non-zero: clear it so the next signalled call counts right
            (void)hipMemset(count, 0, 64);
            if (e != hipSuccess) return hip_fail(e, "hipStreamSynchronize (completion fallback)");
            return fail(HEC_ERR_HIP, "kernel finished without its completion signal");
        }
    }
    return HEC_OK;
}

int Scratch::init() {
    HEC_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
    return HEC_OK;
}

// A burst slot frees each staging buffer above kStagingKeep when its call
// ends; the warm slots keep theirs.
void Scratch::end_call(bool burst) {
    if (!burst || (dbuf.cap <= kStagingKeep && hbuf.cap <= kStagingKeep)) return;
    (void)hipStreamSynchronize(stream);  // an error return may leave copies in flight
    if (dbuf.cap > kStagingKeep) dbuf.release();
    if (hbuf.cap > kStagingKeep) hbuf.release();
}

// upstream check_piece_count!(all) + check_slices!(multi)
static int check_shards(const hec_rs* rs, const void* shards, const size_t* lens, size_t n_shards) {
    if (!shards || !lens) return fail(HEC_ERR_INVALID_ARGUMENT, "null shards");
    if (n_shards < size_t(rs->n)) return fail(HEC_ERR_TOO_FEW_SHARDS, "");
    if (n_shards > size_t(rs->n)) return fail(HEC_ERR_TOO_MANY_SHARDS, "");
    if (lens[0] == 0) return fail(HEC_ERR_EMPTY_SHARD, "");
    for (size_t i = 1; i < n_shards; ++i)
        if (lens[i] != lens[0]) return fail(HEC_ERR_INCORRECT_SHARD_SIZE, "");
    return HEC_OK;
}

static int encode_host(const hec_rs* rs, const uint8_t* const* data, uint8_t* const* parity_out,
                       std::vector<uint8_t>* parity_vec, size_t L) {
    GeomDevice* gd;
    int rc = geom_device(rs, &gd);
    if (rc) return rc;
    Lease<Scratch> lease;
    if ((rc = lease_slot(lease))) return rc;
    Scratch* sc = lease.sc;
    const uint64_t Lp = round_up(L, 256);
    if ((rc = sc->dbuf.reserve(size_t(Lp) * rs->n, kStagingFloor))) return rc;
    uint8_t* par = sc->dbuf + size_t(rs->k) * Lp;
    // the stripe in device staging
    const Batch dev = Batch::split_at(arena(sc->dbuf, 0, Lp), rs->k, round_up(L, 16), 1);
    auto dst_of = [&](int j) { return parity_out ? parity_out[j] : parity_vec->data() + size_t(j) * L; };
    if (uint64_t(rs->k) * L <= host_staging_max()) {
        // pinned staging: k shards packed -> one H2D, one D2H of the m parity
        // rows. (Splitting the call into column chunks on one or two streams
        // to overlap packing with the copies measured slower at 256 KiB and
        // 1 MiB shards: the extra HIP calls cost more than the overlap saves.)
        if ((rc = sc->hbuf.reserve(size_t(Lp) * rs->n, kStagingFloor))) return rc;
        parallel_for(size_t(rs->k), uint64_t(rs->k) * L,
                     [&](size_t i) { std::memcpy(sc->hbuf + i * Lp, data[i], L); });
        uint8_t* hpar = sc->hbuf + size_t(rs->k) * Lp;
        uint8_t* zh = zero_copy_enabled() ? pinned_device_ptr(sc->hbuf) : nullptr;
        if (zh) {  // the kernel reads the packed shards and writes parity over PCIe
            Completion* done = uint64_t(rs->k) * L <= completion_flag_max() ? &sc->done : nullptr;
            const Batch host = Batch::split_at(arena(zh, 0, Lp), rs->k, round_up(L, 16), 1);
            if ((rc = run_apply(gd->encode, uint32_t(rs->k), host, nullptr, nullptr, sc->stream, done)))
                return rc;
            if (done) {
                if ((rc = done->wait(sc->stream))) return rc;
                parallel_for(size_t(rs->m), uint64_t(rs->m) * L,
                             [&](size_t j) { std::memcpy(dst_of(int(j)), hpar + j * Lp, L); });
                return HEC_OK;
            }
        } else {
            HEC_HIP(hipMemcpyAsync(sc->dbuf, sc->hbuf, size_t(rs->k) * Lp, hipMemcpyHostToDevice, sc->stream));
            if ((rc = run_apply(gd->encode, uint32_t(rs->k), dev, nullptr, nullptr, sc->stream)))
                return rc;
            HEC_HIP(hipMemcpyAsync(hpar, par, size_t(rs->m - 1) * Lp + L, hipMemcpyDeviceToHost, sc->stream));
        }
        HEC_HIP(hipStreamSynchronize(sc->stream));
        parallel_for(size_t(rs->m), uint64_t(rs->m) * L,
                     [&](size_t j) { std::memcpy(dst_of(int(j)), hpar + j * Lp, L); });
        return HEC_OK;
    }
    const StreamDrain drain{sc->stream};  // the D2H copies below write caller memory
    for (int i = 0; i < rs->k; ++i)
        HEC_HIP(hipMemcpyAsync(sc->dbuf + i * Lp, data[i], L, hipMemcpyHostToDevice, sc->stream));
    if ((rc = run_apply(gd->encode, uint32_t(rs->k), dev, nullptr, nullptr, sc->stream)))
        return rc;
    for (int j = 0; j < rs->m; ++j)
        HEC_HIP(hipMemcpyAsync(dst_of(j), par + j * Lp, L, hipMemcpyDeviceToHost, sc->stream));
    HEC_HIP(hipStreamSynchronize(sc->stream));
    return HEC_OK;
}

// required: n flags, the missing shards to rebuild (nullptr = all of them).
static int reconstruct_host(const hec_rs* rs, uint8_t* const* shards, const size_t* lens,
                            const uint8_t* present, size_t n_shards, const uint8_t* required) {
    if (!shards || !lens || !present) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_shards < size_t(rs->n)) return fail(HEC_ERR_TOO_FEW_SHARDS, "");
    if (n_shards > size_t(rs->n)) return fail(HEC_ERR_TOO_MANY_SHARDS, "");
    size_t L = 0;
    int npresent = 0;
    for (size_t i = 0; i < n_shards; ++i) {
        if (!present[i]) continue;
        if (lens[i] == 0) return fail(HEC_ERR_EMPTY_SHARD, "");
        if (npresent && lens[i] != L) return fail(HEC_ERR_INCORRECT_SHARD_SIZE, "");
        L = lens[i];
        ++npresent;
    }
    if (npresent == rs->n) return HEC_OK;
    if (npresent < rs->k) return fail(HEC_ERR_TOO_FEW_SHARDS_PRESENT, "");
    if (rs->k == 10 && rs->m == 4 && uint64_t(rs->k) * L <= host_staging_max())
        // one-stripe degraded read: pinned compact staging + the dense-LUT kernel
        return required ? hec_rs_reconstruct_some_batch(rs, shards, lens, present, required, 1, nullptr)
                        : hec_rs_reconstruct_batch(rs, shards, lens, present, 1, 0, nullptr);
    Mat coefs;
    std::vector<uint32_t> in_ids, out_ids;
    bool noop = false;
    int rc = decode_plan(rs, present, required, coefs, in_ids, out_ids, &noop);
    if (rc) return rc;
    for (uint32_t id : out_ids)
        if (!shards[id]) return fail(HEC_ERR_INVALID_ARGUMENT, "missing shard without a buffer");
    if (noop) return HEC_OK;
    Lease<Scratch> lease;
    if ((rc = lease_slot(lease))) return rc;
    Scratch* sc = lease.sc;
    const uint64_t Lp = round_up(L, 256);
    if ((rc = sc->dbuf.reserve(size_t(Lp) * rs->n, kStagingFloor))) return rc;
    HostPlans hp;
    hp.add(coefs, in_ids, out_ids);
    if ((rc = sc->adhoc.upload(hp, nullptr, sc->stream))) return rc;
    const StreamDrain drain{sc->stream};  // the D2H copies below write caller memory
    for (uint32_t id : in_ids)
        HEC_HIP(hipMemcpyAsync(sc->dbuf + id * Lp, shards[id], L, hipMemcpyHostToDevice, sc->stream));
    const Batch dev = Batch::in_place(arena(sc->dbuf, 0, Lp), round_up(L, 16), 1);
    if ((rc = run_apply(sc->adhoc, uint32_t(rs->k), dev, nullptr, nullptr, sc->stream)))
        return rc;
    for (uint32_t id : out_ids)
        HEC_HIP(hipMemcpyAsync(shards[id], sc->dbuf + id * Lp, L, hipMemcpyDeviceToHost, sc->stream));
    HEC_HIP(hipStreamSynchronize(sc->stream));
    return HEC_OK;
}

// hec_rs_update after its checks: the deltas old ^ new of the changed shards
// (XORed while packing) and the m parity shards in pinned staging, shard i at
// i * Lp, coded in place there over PCIe or through device staging, and the
// parity copied back. RS(10,4): the update kernel with no old arena, its mask
// word behind the shards. Any other codec: the generic plan interpreter over an
// ad-hoc plan whose inputs are the deltas and the parity shards and whose
// outputs are the parity shards in place, coefficients [P[:,U] | I]. A lane
// loads its vector of every input before it stores its rows (apply_group), and
// a later row group re-reads the rows an earlier one stored with coefficient 0
// only, so in place is safe.
static int update_host(const hec_rs* rs, uint8_t* const* shards, const uint8_t* const* new_data, size_t L) {
    const int k = rs->k, m = rs->m, n = rs->n;
    const bool is104 = k == 10 && m == 4;
    GeomDevice* gd;
    HEC_TRY(geom_device(rs, &gd));
    Lease<Scratch> lease;
    HEC_TRY(lease_slot(lease));
    Scratch* sc = lease.sc;
    const uint64_t Lp = round_up(L, 256);
    const size_t words_off = size_t(n) * Lp, bytes = words_off + 256;
    HEC_TRY(sc->hbuf.reserve(bytes, kStagingFloor));
    std::vector<uint32_t> in_ids, out_ids;
    uint32_t mask = 0;
    for (int c = 0; c < k; ++c)
        if (new_data[c]) {
            in_ids.push_back(uint32_t(c));
            if (is104) mask |= 1u << c;
        }
    const size_t n_changed = in_ids.size();
    if (!is104) {
        for (int j = 0; j < m; ++j) {
            in_ids.push_back(uint32_t(k + j));
            out_ids.push_back(uint32_t(k + j));
        }
        Mat coefs(m, int(in_ids.size()));
        for (int j = 0; j < m; ++j) {
            for (size_t t = 0; t < n_changed; ++t) coefs.at(j, int(t)) = rs->matrix.at(k + j, int(in_ids[t]));
            coefs.at(j, int(n_changed) + j) = 1;
        }
        HostPlans hp;
        hp.add(coefs, in_ids, out_ids);
        HEC_TRY(sc->adhoc.upload(hp, nullptr, sc->stream));
    }
    const uint64_t moved = uint64_t(n_changed + size_t(m)) * L;
    parallel_for(size_t(n), moved, [&](size_t i) {
        uint8_t* dst = sc->hbuf + i * Lp;
        if (i >= size_t(k)) {
            std::memcpy(dst, shards[i], L);
        } else if (new_data[i]) {
            const uint8_t *o = shards[i], *w = new_data[i];
            for (size_t b = 0; b < L; ++b) dst[b] = o[b] ^ w[b];
        }
    });
    std::memcpy(sc->hbuf + words_off, &mask, sizeof mask);
    uint8_t* zh = zero_copy_enabled() ? pinned_device_ptr(sc->hbuf) : nullptr;
    uint8_t* dev = zh;
    const size_t par_off = size_t(k) * Lp;
    if (!zh) {
        HEC_TRY(sc->dbuf.reserve(bytes, kStagingFloor));
        dev = sc->dbuf;
        for (size_t t = 0; t < n_changed; ++t)
            HEC_HIP(hipMemcpyAsync(dev + in_ids[t] * Lp, sc->hbuf + in_ids[t] * Lp, L, hipMemcpyHostToDevice,
                                   sc->stream));
        // the parity shards and the mask word behind them
        HEC_HIP(hipMemcpyAsync(dev + par_off, sc->hbuf + par_off, bytes - par_off, hipMemcpyHostToDevice, sc->stream));
    }
    const Strided st = arena(dev, 0, Lp);
    Completion* done = zh && moved <= completion_flag_max() ? &sc->done : nullptr;
    if (is104)
        HEC_TRY(run_update(gd->encode, Strided{}, Batch::split_at(st, k, round_up(L, 16), 1),
                           reinterpret_cast<const uint32_t*>(dev + words_off), sc->stream, done));
    else
        HEC_TRY(run_apply(sc->adhoc, uint32_t(in_ids.size()), Batch::in_place(st, round_up(L, 16), 1), nullptr, nullptr,
                          sc->stream, done));
    if (!zh)
        HEC_HIP(hipMemcpyAsync(sc->hbuf + par_off, dev + par_off, size_t(m - 1) * Lp + L, hipMemcpyDeviceToHost,
                               sc->stream));
    if (done) HEC_TRY(done->wait(sc->stream));
    else HEC_HIP(hipStreamSynchronize(sc->stream));
    parallel_for(size_t(m), uint64_t(m) * L,
                 [&](size_t j) { std::memcpy(shards[size_t(k) + j], sc->hbuf + par_off + j * Lp, L); });
    return HEC_OK;
}

}  // namespace hec

using namespace hec;

extern "C" {

int hec_rs_new(size_t data_shards, size_t parity_shards, hec_rs_t** out) {
    if (!out) return fail(HEC_ERR_INVALID_ARGUMENT, "null out");
    *out = nullptr;
    if (data_shards == 0) return fail(HEC_ERR_TOO_FEW_DATA_SHARDS, "");
    if (parity_shards == 0) return fail(HEC_ERR_TOO_FEW_PARITY_SHARDS, "");
    if (data_shards + parity_shards > 256) return fail(HEC_ERR_TOO_MANY_SHARDS, "");
    hec_rs_t* rs = new hec_rs_t();
    rs->k = int(data_shards);
    rs->m = int(parity_shards);
    rs->n = rs->k + rs->m;
    rs->matrix = build_encoding_matrix(rs->k, rs->n);
    *out = rs;
    return HEC_OK;
}

void hec_rs_free(hec_rs_t* rs) { delete rs; }

size_t hec_rs_data_shard_count(const hec_rs_t* rs) { return rs ? size_t(rs->k) : 0; }
size_t hec_rs_parity_shard_count(const hec_rs_t* rs) { return rs ? size_t(rs->m) : 0; }
size_t hec_rs_total_shard_count(const hec_rs_t* rs) { return rs ? size_t(rs->n) : 0; }

int hec_rs_matrix(const hec_rs_t* rs, uint8_t* out, size_t out_len) {
    if (!rs || !out || out_len < rs->matrix.v.size()) return fail(HEC_ERR_INVALID_ARGUMENT, "bad matrix buffer");
    std::memcpy(out, rs->matrix.v.data(), rs->matrix.v.size());
    return HEC_OK;
}

int hec_rs_encode(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens, size_t n_shards) {
    if (!rs) return fail(HEC_ERR_INVALID_ARGUMENT, "null codec");
    int rc = check_shards(rs, shards, shard_lens, n_shards);
    if (rc) return rc;
    return encode_host(rs, const_cast<const uint8_t* const*>(shards), shards + rs->k, nullptr, shard_lens[0]);
}

int hec_rs_verify(const hec_rs_t* rs, const uint8_t* const* shards, const size_t* shard_lens, size_t n_shards,
                  int* ok) {
    if (!rs || !ok) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    int rc = check_shards(rs, shards, shard_lens, n_shards);
    if (rc) return rc;
    const size_t L = shard_lens[0];
    std::vector<uint8_t> par(size_t(rs->m) * L);
    if ((rc = encode_host(rs, shards, nullptr, &par, L))) return rc;
    *ok = 1;
    for (int j = 0; j < rs->m; ++j)
        if (std::memcmp(par.data() + size_t(j) * L, shards[rs->k + j], L) != 0) *ok = 0;
    return HEC_OK;
}

int hec_rs_reconstruct(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                       const uint8_t* present, size_t n_shards) {
    if (!rs) return fail(HEC_ERR_INVALID_ARGUMENT, "null codec");
    return reconstruct_host(rs, shards, shard_lens, present, n_shards, nullptr);
}

int hec_rs_reconstruct_data(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                            const uint8_t* present, size_t n_shards) {
    if (!rs) return fail(HEC_ERR_INVALID_ARGUMENT, "null codec");
    std::vector<uint8_t> data_flags(size_t(rs->n), 0);  // reconstruct some of the data shards
    std::fill(data_flags.begin(), data_flags.begin() + rs->k, uint8_t(1));
    return reconstruct_host(rs, shards, shard_lens, present, n_shards, data_flags.data());
}

int hec_rs_reconstruct_some(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                            const uint8_t* present, const uint8_t* required, size_t n_shards) {
    if (!rs) return fail(HEC_ERR_INVALID_ARGUMENT, "null codec");
    if (!required) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    return reconstruct_host(rs, shards, shard_lens, present, n_shards, required);
}

int hec_rs_update(const hec_rs_t* rs, uint8_t* const* shards, const size_t* shard_lens,
                  const uint8_t* const* new_data, size_t n_shards) {
    if (!rs || !shards || !shard_lens || !new_data) return fail(HEC_ERR_INVALID_ARGUMENT, "null argument");
    if (n_shards < size_t(rs->n)) return fail(HEC_ERR_TOO_FEW_SHARDS, "");
    if (n_shards > size_t(rs->n)) return fail(HEC_ERR_TOO_MANY_SHARDS, "");
    bool any = false;
    for (int i = 0; i < rs->n; ++i) {
        const bool used = i >= rs->k || new_data[i];
        if (i < rs->k) any = any || used;
        if (used && !shards[i])
            return fail(HEC_ERR_INVALID_ARGUMENT,
                        i < rs->k ? "changed shard without its old buffer" : "null parity shard");
    }
    // the lengths in use: the old slots of the changed shards and the parity
    size_t L = 0;
    for (int i = 0; i < rs->n; ++i) {
        if (i < rs->k && !new_data[i]) continue;
        if (shard_lens[i] == 0) return fail(HEC_ERR_EMPTY_SHARD, "");
        if (L && shard_lens[i] != L) return fail(HEC_ERR_INCORRECT_SHARD_SIZE, "");
        L = shard_lens[i];
    }
    if (!any) return HEC_OK;
    return update_host(rs, shards, new_data, L);
}

}  // extern "C"
