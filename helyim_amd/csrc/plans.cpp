// Coding plans and the per-device state of one geometry: the host-side plan
// list and its device copy, the decode plan of an erasure pattern, the encode
// plan and dense decode LUT shared by all contexts of a geometry, and the
// launch of one plan set over a strided batch.
#include <tuple>

#include "hec_internal.hpp"

namespace hec {

// ---------------------------------------------------------------------------
// Plans
// ---------------------------------------------------------------------------
uint32_t HostPlans::add(const Mat& coefs, const std::vector<uint32_t>& in_ids,
                        const std::vector<uint32_t>& out_ids) {
    DevPlan p{};
    p.nin = uint32_t(in_ids.size());
    p.nout = uint32_t(out_ids.size());
    p.tab_off = uint32_t(tabs.size());
    p.idx_off = uint32_t(idx.size());
    p.tab_rows = fixed_rows ? fixed_rows : p.nout;
    for (uint32_t i = 0; i < p.nin; ++i)
        for (uint32_t r = 0; r < p.tab_rows; ++r) {
            uint32_t t[kTabWords];
            perm_tables(r < p.nout ? coefs.at(int(r), int(i)) : uint8_t(0), t);
            tabs.insert(tabs.end(), t, t + kTabWords);
        }
    idx.insert(idx.end(), in_ids.begin(), in_ids.end());
    idx.insert(idx.end(), out_ids.begin(), out_ids.end());
    plans.push_back(p);
    return uint32_t(plans.size() - 1);
}

uint32_t HostPlans::add_noop(uint32_t nin) {
    DevPlan p{nin, 0, uint32_t(tabs.size()), uint32_t(idx.size()), fixed_rows, {0, 0, 0}};
    tabs.insert(tabs.end(), size_t(nin) * fixed_rows * kTabWords, 0u);
    plans.push_back(p);
    return uint32_t(plans.size() - 1);
}

template <typename T>
static int grow_upload(DeviceBuf<T>& d, const std::vector<T>& src, hipStream_t s) {
    if (src.empty()) return HEC_OK;
    HEC_TRY(d.reserve(src.size() * sizeof(T)));
    HEC_HIP(hipMemcpyAsync(d, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice, s));
    return HEC_OK;
}

int DevicePlanSet::upload(const HostPlans& hp, const std::vector<uint32_t>* lut_host, hipStream_t s) {
    HEC_TRY(grow_upload(plans, hp.plans, s));
    HEC_TRY(grow_upload(tabs, hp.tabs, s));
    HEC_TRY(grow_upload(idx, hp.idx, s));
    if (lut_host) HEC_TRY(grow_upload(lut, *lut_host, s));
    // Host vectors may be freed by the caller right after: make the copies land.
    HEC_HIP(hipStreamSynchronize(s));
    return HEC_OK;
}

void DevicePlanSet::release() {
    plans.release();
    tabs.release();
    idx.release();
    lut.release();
}

// upstream reconstruct_internal: first k present shards -> sub-matrix ->
// inverse; missing data rows = inverse rows; missing parity rows = parity
// row x inverse (composed, bit-identical to upstream's second pass since the
// reconstructed data bytes are unique).
int decode_plan(const hec_rs* rs, const uint8_t* present, const uint8_t* required, Mat& coefs,
                std::vector<uint32_t>& in_ids, std::vector<uint32_t>& out_ids, bool* noop) {
    const int k = rs->k, n = rs->n;
    int npresent = 0;
    for (int i = 0; i < n; ++i) npresent += present[i] ? 1 : 0;
    *noop = false;
    in_ids.clear();
    out_ids.clear();
    if (npresent == n) {
        *noop = true;
        return HEC_OK;
    }
    if (npresent < k) return fail(HEC_ERR_TOO_FEW_SHARDS_PRESENT, "");
    std::vector<uint32_t> miss;
    for (int i = 0; i < n; ++i) {
        if (present[i]) {
            if (int(in_ids.size()) < k) in_ids.push_back(uint32_t(i));
        } else {
            miss.push_back(uint32_t(i));
        }
    }
    Mat sub(k, k);
    for (int r = 0; r < k; ++r)
        for (int c = 0; c < k; ++c) sub.at(r, c) = rs->matrix.at(int(in_ids[r]), c);
    Mat inv;
    if (!mat_invert(sub, inv)) return fail(HEC_ERR_INVALID_ARGUMENT, "singular decode matrix");
    for (uint32_t i : miss)
        if (!required || required[i]) out_ids.push_back(i);
    coefs = Mat(int(out_ids.size()), k);
    const Gf& g = gf();
    for (size_t r = 0; r < out_ids.size(); ++r) {
        const int id = int(out_ids[r]);
        if (id < k) {
            for (int c = 0; c < k; ++c) coefs.at(int(r), c) = inv.at(id, c);
        } else {
            for (int c = 0; c < k; ++c) {
                uint8_t acc = 0;
                for (int t = 0; t < k; ++t) acc ^= g.mul[rs->matrix.at(id, t)][inv.at(t, c)];
                coefs.at(int(r), c) = acc;
            }
        }
    }
    if (out_ids.empty()) *noop = true;
    return HEC_OK;
}

// ---------------------------------------------------------------------------
// Per-device geometry state
// ---------------------------------------------------------------------------
static std::mutex g_geom_mu;
static std::map<std::tuple<int, int, int>, std::unique_ptr<GeomDevice>> g_geom;

int geom_device(const hec_rs* rs, GeomDevice** out) {
    int dev;
    int rc = current_device(&dev);
    if (rc) return rc;
    std::lock_guard<std::mutex> lk(g_geom_mu);
    auto key = std::make_tuple(dev, rs->k, rs->m);
    auto it = g_geom.find(key);
    if (it != g_geom.end()) {
        *out = it->second.get();
        return HEC_OK;
    }
    std::unique_ptr<GeomDevice> gd(new GeomDevice());
    gd->k = uint32_t(rs->k);
    const bool is104 = rs->k == 10 && rs->m == 4;
    HostPlans hp;
    if (is104) hp.fixed_rows = 4;
    Mat par(rs->m, rs->k);
    for (int r = 0; r < rs->m; ++r)
        for (int c = 0; c < rs->k; ++c) par.at(r, c) = rs->matrix.at(rs->k + r, c);
    std::vector<uint32_t> in_ids, out_ids;
    for (int i = 0; i < rs->k; ++i) in_ids.push_back(uint32_t(i));
    for (int j = 0; j < rs->m; ++j) out_ids.push_back(uint32_t(j));
    hp.add(par, in_ids, out_ids);
    if ((rc = gd->encode.upload(hp, nullptr, nullptr))) return rc;
    gd->encode.fast104 = is104;
    if (is104) {
        // the locate kernel's constants: P[j][c] / P[0][c] for j = 1..3 (a
        // syndrome v * P[:,c] has s[j] = s[0] times that ratio)
        const Gf& g = gf();
        Mat ratio(rs->m - 1, rs->k);
        for (int c = 0; c < rs->k; ++c) {
            if (par.at(0, c) == 0) return fail(HEC_ERR_INVALID_ARGUMENT, "zero entry in the parity matrix");
            for (int j = 1; j < rs->m; ++j) ratio.at(j - 1, c) = g.mul[par.at(j, c)][g.inv(par.at(0, c))];
        }
        HostPlans rp;
        rp.add(ratio, in_ids, {1, 2, 3});
        if ((rc = gd->locate.upload(rp, nullptr, nullptr))) return rc;
        // the pair search's constants. Shard i of a codeword is p(alpha_i),
        // alpha_i = the byte i, deg p < k, so H'[j][i] = u_i * alpha_i^j with
        // u_i = 1 / prod_{l != i} (alpha_i ^ alpha_l) annihilates the code
        // and H' = T * [P | I], T = H'[:, k..n): checked here, not assumed.
        const int n = rs->n, m = rs->m;
        Mat dual(m, n);
        for (int i = 0; i < n; ++i) {
            uint8_t prod = 1;
            for (int l = 0; l < n; ++l)
                if (l != i) prod = g.mul[prod][uint8_t(i ^ l)];
            for (int j = 0; j < m; ++j) dual.at(j, i) = g.mul[g.inv(prod)][g.pow(uint8_t(i), unsigned(j))];
        }
        Mat t(m, m);
        for (int j = 0; j < m; ++j)
            for (int i = 0; i < m; ++i) t.at(j, i) = dual.at(j, rs->k + i);
        const Mat tp = mat_mul(t, par);
        for (int j = 0; j < m; ++j)
            for (int c = 0; c < rs->k; ++c)
                if (tp.at(j, c) != dual.at(j, c))
                    return fail(HEC_ERR_INVALID_ARGUMENT, "the encoding matrix is not the evaluation code");
        // plan 0: S = T * syn; plan 1: D * alpha_c^2 ^ N1 * alpha_c, one row per shard c
        Mat roots(n, 2);
        for (int c = 0; c < n; ++c) {
            roots.at(c, 0) = g.mul[uint8_t(c)][uint8_t(c)];
            roots.at(c, 1) = uint8_t(c);
        }
        std::vector<uint32_t> all_ids;
        for (int c = 0; c < n; ++c) all_ids.push_back(uint32_t(c));
        HostPlans pp;
        pp.add(t, {0, 1, 2, 3}, {0, 1, 2, 3});
        pp.add(roots, {0, 1}, all_ids);
        if ((rc = gd->locate_pairs.upload(pp, nullptr, nullptr))) return rc;
        // the correct kernel's constants (rs_kernels.hpp CorrectArgs::fix_tabs):
        // 1 / P[0][c], the value of a wrong data shard from s[0], and 1 / u_c,
        // the pair values' last factor. Both checked by multiplying back.
        Mat inv_p0(1, rs->k), inv_u(1, n);
        for (int c = 0; c < rs->k; ++c) {
            inv_p0.at(0, c) = g.inv(par.at(0, c));
            if (g.mul[par.at(0, c)][inv_p0.at(0, c)] != 1)
                return fail(HEC_ERR_INVALID_ARGUMENT, "1 / P[0][c] does not multiply back to 1");
        }
        for (int c = 0; c < n; ++c) {
            inv_u.at(0, c) = g.inv(dual.at(0, c));  // H'[0][c] = u_c
            if (g.mul[dual.at(0, c)][inv_u.at(0, c)] != 1)
                return fail(HEC_ERR_INVALID_ARGUMENT, "1 / u_c does not multiply back to 1");
        }
        HostPlans cp;
        cp.add(inv_p0, in_ids, {0});
        if (cp.add(inv_u, all_ids, {0}) != 1 || cp.plans[1].tab_off != uint32_t(kFixInvU))
            return fail(HEC_ERR_INVALID_ARGUMENT, "correct plan layout");
        if ((rc = gd->correct.upload(cp, nullptr, nullptr))) return rc;
    }
    *out = gd.get();
    g_geom[key] = std::move(gd);
    return HEC_OK;
}

int ensure_dense_decode(const hec_rs* rs, GeomDevice* gd, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_geom_mu);
    if (gd->decode_ready) return HEC_OK;
    const int n = rs->n, k = rs->k;
    if (n > 16) return fail(HEC_ERR_INVALID_ARGUMENT, "device-mask reconstruct needs total shards <= 16");
    HostPlans hp;
    const bool is104 = k == 10 && rs->m == 4;
    if (is104) hp.fixed_rows = 4;
    std::vector<uint32_t> lut(size_t(1) << n, kNoPlan);
    const uint32_t noop = hp.add_noop(uint32_t(k));
    uint8_t present[16];
    Mat coefs;
    std::vector<uint32_t> in_ids, out_ids;
    for (uint32_t mask = 0; mask < (1u << n); ++mask) {
        const int pc = __builtin_popcount(mask);
        if (pc < k) continue;
        if (pc == n) {
            lut[mask] = noop;
            continue;
        }
        for (int i = 0; i < n; ++i) present[i] = (mask >> i) & 1;
        bool is_noop = false;
        int rc = decode_plan(rs, present, nullptr, coefs, in_ids, out_ids, &is_noop);
        if (rc) return rc;
        lut[mask] = hp.add(coefs, in_ids, out_ids);
    }
    int rc = gd->decode_dense.upload(hp, &lut, s);
    if (rc) return rc;
    gd->decode_dense.fast104 = is104;
    gd->decode_dense.lut_bits = uint32_t(n);
    gd->decode_ready = true;
    return HEC_OK;
}

// decode_plan's sibling for the degraded scrub: the inputs are the same first
// k present shards (B), but the outputs are the OTHER present shards (E), so
// coefs = A_m, what the reconstruct would apply to B had E been erased.
int check_plan(const hec_rs* rs, const uint8_t* present, Mat& coefs, std::vector<uint32_t>& in_ids,
               std::vector<uint32_t>& out_ids) {
    const int k = rs->k, n = rs->n;
    in_ids.clear();
    out_ids.clear();
    for (int i = 0; i < n; ++i) {
        if (!present[i]) continue;
        if (int(in_ids.size()) < k) in_ids.push_back(uint32_t(i));
        else out_ids.push_back(uint32_t(i));
    }
    if (int(in_ids.size()) < k) return fail(HEC_ERR_TOO_FEW_SHARDS_PRESENT, "");
    Mat sub(k, k), rows(int(out_ids.size()), k);
    for (int r = 0; r < k; ++r)
        for (int c = 0; c < k; ++c) sub.at(r, c) = rs->matrix.at(int(in_ids[r]), c);
    Mat inv;
    if (!mat_invert(sub, inv)) return fail(HEC_ERR_INVALID_ARGUMENT, "singular decode matrix");
    for (size_t r = 0; r < out_ids.size(); ++r)
        for (int c = 0; c < k; ++c) rows.at(int(r), c) = rs->matrix.at(int(out_ids[r]), c);
    coefs = mat_mul(rows, inv);
    return HEC_OK;
}

int ensure_check_plans(const hec_rs* rs, GeomDevice* gd, hipStream_t s) {
    std::lock_guard<std::mutex> lk(g_geom_mu);
    if (gd->check_ready) return HEC_OK;
    const int n = rs->n, k = rs->k;
    if (k != 10 || rs->m != 4) return fail(HEC_ERR_INVALID_ARGUMENT, "check plans are RS(10,4) only");
    // plan ids count the masks with a spare shard in ascending order, in all
    // three sets: the tables of plan p start at p * 200 (check), p * 150
    // (ratio) and p * 50 (fix) words
    HostPlans hp, rp, fp;
    hp.fixed_rows = 4;
    rp.fixed_rows = 3;
    fp.fixed_rows = 1;
    std::vector<uint32_t> lut(size_t(1) << n, kNoPlan);
    uint8_t present[16];
    Mat coefs;
    std::vector<uint32_t> in_ids, out_ids;
    const Gf& g = gf();
    for (uint32_t mask = 0; mask < (1u << n); ++mask) {
        if (__builtin_popcount(mask) <= k) continue;
        for (int i = 0; i < n; ++i) present[i] = (mask >> i) & 1;
        HEC_TRY(check_plan(rs, present, coefs, in_ids, out_ids));
        lut[mask] = hp.add(coefs, in_ids, out_ids);
        // the masked locate's constants: A_m[j][c] / A_m[0][c], j = 1..r-1 (zero past r)
        Mat ratio(3, k);
        for (int c = 0; c < k; ++c) {
            if (coefs.at(0, c) == 0) return fail(HEC_ERR_INVALID_ARGUMENT, "zero entry in a check matrix");
            for (int j = 1; j < coefs.rows; ++j) ratio.at(j - 1, c) = g.mul[coefs.at(j, c)][g.inv(coefs.at(0, c))];
        }
        rp.add(ratio, in_ids, {1, 2, 3});
        // the masked correct's constants (rs_kernels.hpp CorrectPresentArgs::
        // fix_tabs): 1 / A_m[0][c], the value of a wrong shard B[c] from
        // syn[0]. Checked by multiplying back.
        Mat inv_a0(1, k);
        for (int c = 0; c < k; ++c) {
            inv_a0.at(0, c) = g.inv(coefs.at(0, c));
            if (g.mul[coefs.at(0, c)][inv_a0.at(0, c)] != 1)
                return fail(HEC_ERR_INVALID_ARGUMENT, "1 / A_m[0][c] does not multiply back to 1");
        }
        if (fp.add(inv_a0, in_ids, {0}) != lut[mask] || fp.plans.back().tab_off != lut[mask] * uint32_t(k * kTabWords))
            return fail(HEC_ERR_INVALID_ARGUMENT, "check fix plan layout");
    }
    HEC_TRY(gd->check.upload(hp, &lut, s));
    HEC_TRY(gd->check_ratio.upload(rp, nullptr, s));
    HEC_TRY(gd->check_fix.upload(fp, nullptr, s));
    gd->check.fast104 = true;
    gd->check.lut_bits = uint32_t(n);
    gd->check_ready = true;
    return HEC_OK;
}

// The coding arguments every strided launch shares, from a plan set and the
// batch's layout.
static void fill_args(ApplyArgs& a, const DevicePlanSet& ps, const Batch& b, uint32_t* bad) {
    a.in_base = b.in.base;
    a.in_stripe = b.in.stripe;
    a.in_shard = b.in.shard;
    a.out_base = b.out.base;
    a.out_stripe = b.out.stripe;
    a.out_shard = b.out.shard;
    a.len = b.len;
    a.n_stripes = b.n_stripes;
    a.plans = ps.plans;
    a.tabs = ps.tabs;
    a.idx = ps.idx;
    a.bad_count = bad;
    a.fast104 = ps.fast104 ? 1u : 0u;
}
// ... of a launch that picks each stripe's plan from its mask word.
static void fill_mask_args(ApplyArgs& a, const DevicePlanSet& ps, const Batch& b, const uint32_t* masks,
                           uint32_t* bad) {
    fill_args(a, ps, b, bad);
    a.masks = masks;
    a.lut = ps.lut;
    a.mask_limit = ps.lut_bits ? ((1u << ps.lut_bits) - 1u) : 0u;
}

int run_apply(const DevicePlanSet& ps, uint32_t nin, const Batch& b, const uint32_t* masks, uint32_t* bad,
              hipStream_t s, Completion* done, bool over_pcie) {
    ApplyArgs a{};
    if (done) HEC_TRY(done->arm(s, &a.done_count, &a.done_flag, &a.done_seq));
    fill_mask_args(a, ps, b, masks, bad);
    if (masks && !ps.lut) return fail(HEC_ERR_INVALID_ARGUMENT, "per-stripe masks need a decode LUT");
    HEC_HIP(launch_apply(a, int(nin), b.aligned(), over_pcie && !masks, s));
    return HEC_OK;
}

int run_some(const DevicePlanSet& ps, uint32_t nin, const Batch& b, const uint32_t* masks, const uint32_t* wants,
             uint32_t* bad, hipStream_t s) {
    if (!wants) return run_apply(ps, nin, b, masks, bad, s);  // "all": the decode's own launches
    SomeArgs v{};
    fill_mask_args(v.a, ps, b, masks, bad);
    v.wants = wants;
    if (!ps.lut || !ps.fast104) return fail(HEC_ERR_INVALID_ARGUMENT, "reconstruct some needs the RS(10,4) decode LUT");
    HEC_HIP(launch_some(v, b.aligned(), s));
    return HEC_OK;
}

int run_update(const DevicePlanSet& enc, const Strided& old, const Batch& b, const uint32_t* masks, hipStream_t s,
               Completion* done) {
    if (!enc.fast104) return fail(HEC_ERR_INVALID_ARGUMENT, "update needs the RS(10,4) encode plan");
    UpdateArgs v{};
    if (done) HEC_TRY(done->arm(s, &v.a.done_count, &v.a.done_flag, &v.a.done_seq));
    fill_args(v.a, enc, b, nullptr);
    v.a.masks = masks;
    v.old_base = old.base;
    v.old_stripe = old.stripe;
    v.old_shard = old.shard;
    HEC_HIP(launch_update(v, b.aligned() && (!old.base || old.low_bits() % 16 == 0), s));
    return HEC_OK;
}

// Pass 2 of a scrub, the part every kernel argument type shares: pass 1's
// arguments with its counters nulled (the counts are pass 1's), the words to
// name the shards in, cleared, and the locate's constants.
template <typename Args>
static int second_pass(Args& v, const DevicePlanSet& ratio, const Batch& b, const ScrubOut& out, hipStream_t s) {
    v.a.bad_count = nullptr;
    v.suspects = out.suspects;
    v.ratio_tabs = ratio.tabs;
    HEC_HIP(hipMemsetAsync(out.suspects, 0, size_t(b.n_stripes) * 4, s));
    return HEC_OK;
}
// ... and what a correcting pass 2 adds.
template <typename Args>
static void correct_pass(Args& v, const DevicePlanSet& fix, const ScrubOut& out) {
    v.fix_tabs = fix.tabs;
    v.uncorrected = out.left;
    v.corrected_bytes = out.corrected_bytes;
}

int run_scrub(const GeomDevice& gd, const Batch& b, const ScrubSpec& spec, const ScrubOut& out, hipStream_t s) {
    if (b.n_stripes == 0) return HEC_OK;
    const bool aligned = b.aligned();
    // the kernels only ever OR bits in: stale words must not leak through
    HEC_HIP(hipMemsetAsync(out.words, 0, size_t(b.n_stripes) * 4, s));
    if (!spec.masks) {
        // pass 1: the verify (bit-sliced where it applies), at its own rate
        CorrectArgs v{};
        fill_args(v.a, gd.encode, b, out.bad);
        v.mismatch = out.words;
        HEC_HIP(launch_verify(v, int(gd.k), aligned, s));
        if (spec.pass2 == Pass2::None) return HEC_OK;
        // pass 2: only the stripes pass 1 flagged are read again
        HEC_TRY(second_pass(v, gd.locate, b, out, s));
        v.pair_tabs = gd.locate_pairs.tabs;
        if (spec.pass2 == Pass2::Locate) {
            HEC_HIP(launch_locate(v, aligned, spec.pairs, s));
            return HEC_OK;
        }
        correct_pass(v, gd.correct, out);
        HEC_HIP(launch_correct(v, aligned, spec.pairs, s));
        return HEC_OK;
    }
    // pass 1: the masked check. out = in: the check kernels only read, the
    // masked correct writes through in_base (fix_shard)
    CorrectPresentArgs v{};
    fill_mask_args(v.a, gd.check, b, spec.masks, out.bad);
    v.check = out.words;
    v.unchecked = out.unchecked;
    HEC_HIP(launch_check(v, aligned, s));
    if (spec.pass2 == Pass2::None) return HEC_OK;
    HEC_TRY(second_pass(v, gd.check_ratio, b, out, s));
    v.unchecked = nullptr;
    if (spec.pass2 == Pass2::Locate) {
        HEC_HIP(launch_locate_present(v, aligned, s));
        return HEC_OK;
    }
    correct_pass(v, gd.check_fix, out);
    v.min_spares = spec.min_spares;
    HEC_HIP(launch_correct_present(v, aligned, s));
    return HEC_OK;
}

}  // namespace hec
