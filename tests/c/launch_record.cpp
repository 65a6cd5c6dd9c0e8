// Recorder of the kernel launch layer of helyim_amd/csrc/rs_kernels.hip. The
// object compiled from that file needs nothing from the HIP runtime but the
// registration and launch entry points; this program defines them itself, is
// linked against the object WITHOUT the runtime, calls every launch_* function
// on a CPU and prints one line per launch: which kernel, on what grid, with
// which launcher-computed arguments. No device is opened.
//   * __hipRegisterFunction gives host stub -> kernel symbol (demangled here);
//   * hipLaunchKernel gives the grid and pointers to the by-value arguments.
// Pointers are fixed fake addresses and are printed as stripe offsets from the
// values put in, fields only (never struct bytes: padding is not defined).
// `launch_record --registered` prints the registered kernel names instead.
// tests/test_launch_record.py builds and runs it against the product object
// and the small-grid object and lists the shapes.
#include <cxxabi.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "rs_kernels.hpp"

using namespace hec;

#ifdef HEC_MAX_LAUNCH_BLOCKS
extern "C" void hec_test_launch_limits(uint64_t* max_launch_blocks, uint32_t* locate_max_blocks);
#endif

// ---------------------------------------------------------------------------
// What the test put in: the bases the recorded pointers are measured from.
// ---------------------------------------------------------------------------
static uint8_t* const kIn = reinterpret_cast<uint8_t*>(0x100000000000ull);
static uint8_t* const kOut = reinterpret_cast<uint8_t*>(0x200000000000ull);
static uint8_t* const kOld = reinterpret_cast<uint8_t*>(0x300000000000ull);
static uint32_t* const kMasks = reinterpret_cast<uint32_t*>(0x400000000000ull);
static uint32_t* const kWords = reinterpret_cast<uint32_t*>(0x500000000000ull);  // wants / mismatch / check
static uint32_t* const kFake = reinterpret_cast<uint32_t*>(0x600000000000ull);   // everything never advanced

static std::map<const void*, std::string>& registered() {
    static std::map<const void*, std::string> m;  // built during static initialisation of the object
    return m;
}

// (p - base) / stride when that is whole, "-" for a null pointer.
static std::string offset_of(const void* p, const void* base, uint64_t stride) {
    if (!p) return "-";
    const int64_t d = reinterpret_cast<const char*>(p) - reinterpret_cast<const char*>(base);
    if (stride == 0 || d % int64_t(stride) != 0) return "?" + std::to_string(d);
    return std::to_string(d / int64_t(stride));
}

static void print_apply(const ApplyArgs& a) {
    std::printf(" ns=%u in=%s out=%s m=%s cps=%u ni=%llu q=%u r=%u mul=%u sh=%u", a.n_stripes,
                offset_of(a.in_base, kIn, a.in_stripe).c_str(),
                offset_of(a.out_base, a.out_base < kOut ? kIn : kOut, a.out_stripe).c_str(),  // in place: from kIn
                offset_of(a.masks, kMasks, 4).c_str(), a.chunks_per_stripe, (unsigned long long)a.n_items, a.map_q8,
                a.map_r8, a.cps_mul, a.cps_shift);
}

static void print_ragged(const RaggedArgs& a) {
    std::printf(" nb=%u base=%u q=%u r=%u", a.n_blocks, a.block_base, a.map_q8, a.map_r8);
}

static bool has(const std::string& s, const char* what) { return s.find(what) != std::string::npos; }

static const char* g_tag = "";  // the launcher call being recorded, and its launches so far
static int g_launches = 0;

// One line: the call's tag, the kernel (the parameter list is left to
// --registered: a template-id has one), the grid, the decoded fields.
static void record(const std::string& name, dim3 grid, dim3 block, void** args) {
    // the kernel's parameter list tells which struct to decode; the locate
    // kernels spell theirs as a std::conditional over their template flags
    const std::string fn = name.substr(0, name.find('(')), params = name.substr(name.find('('));
    ++g_launches;
    std::printf(" %s: %s g=%u", g_tag, fn.c_str(), grid.x);
    if (grid.y != 1 || grid.z != 1 || block.x != unsigned(kThreads) || block.y != 1 || block.z != 1)
        std::printf(" !dims");
    const bool ragged_walk = has(fn, "rs104_locate_present_kernel<") && has(fn, ", true>");
    if (has(fn, "_masks_")) {  // n_stripes is the last parameter of all four
        int n = 0;
        for (char c : params) n += c == ',';
        std::printf(" ns=%u\n", *static_cast<const uint32_t*>(args[n]));
        return;
    }
    const void* v = args[0];
    const uint32_t* done = nullptr;
    if (params == "(hec::RaggedArgs)" || params == "(hec::RaggedScrubArgs)" || ragged_walk) {
        const RaggedArgs& a = *static_cast<const RaggedArgs*>(v);
        print_ragged(a);
        if (params != "(hec::RaggedArgs)") std::printf(" half=%u", static_cast<const RaggedScrubArgs*>(v)->half_shift);
        done = a.done_flag;
    } else {
        const ApplyArgs& a = *static_cast<const ApplyArgs*>(v);  // every strided struct begins with one
        print_apply(a);
        if (params == "(hec::SomeArgs)") {
            std::printf(" wants=%s", offset_of(static_cast<const SomeArgs*>(v)->wants, kWords, 4).c_str());
        } else if (params == "(hec::UpdateArgs)") {
            const UpdateArgs& u = *static_cast<const UpdateArgs*>(v);
            std::printf(" old=%s", offset_of(u.old_base, kOld, u.old_stripe).c_str());
        } else if (params == "(hec::VerifyArgs)" || has(fn, "rs104_locate_kernel<")) {
            std::printf(" mis=%s", offset_of(static_cast<const VerifyArgs*>(v)->mismatch, kWords, 4).c_str());
        } else if (params == "(hec::CheckArgs)" || has(fn, "rs104_locate_present_kernel<")) {
            std::printf(" chk=%s", offset_of(static_cast<const CheckArgs*>(v)->check, kWords, 4).c_str());
        } else if (params != "(hec::ApplyArgs)") {
            std::printf(" !unknown-parameter");
        }
        done = a.done_flag;
    }
    std::printf(" done=%d\n", done ? 1 : 0);  // the completion flag: null, or still set
}

// ---------------------------------------------------------------------------
// The HIP entry points the object links against.
// ---------------------------------------------------------------------------
static struct {
    dim3 grid, block;
    size_t shared;
    hipStream_t stream;
} g_config;

extern "C" {
void** __hipRegisterFatBinary(const void*) {
    static void* handle = nullptr;
    return &handle;
}
void __hipUnregisterFatBinary(void**) {}
void __hipRegisterFunction(void**, const void* host_function, char*, const char* device_name, unsigned, void*, void*,
                           void*, void*, int*) {
    int status = 0;
    char* d = abi::__cxa_demangle(device_name, nullptr, nullptr, &status);
    std::string name = status == 0 && d ? d : device_name;
    std::free(d);
    for (const char* drop : {"void ", "hec::"})  // every kernel is a void function of namespace hec
        if (name.rfind(drop, 0) == 0) name.erase(0, std::strlen(drop));
    registered()[host_function] = name;
}
hipError_t __hipPushCallConfiguration(dim3 grid, dim3 block, size_t shared, hipStream_t stream) {
    g_config = {grid, block, shared, stream};
    return hipSuccess;
}
hipError_t __hipPopCallConfiguration(dim3* grid, dim3* block, size_t* shared, hipStream_t* stream) {
    *grid = g_config.grid;
    *block = g_config.block;
    *shared = g_config.shared;
    *stream = g_config.stream;
    return hipSuccess;
}
hipError_t hipLaunchKernel(const void* function, dim3 grid, dim3 block, void** args, size_t, hipStream_t) {
    const auto it = registered().find(function);
    record(it == registered().end() ? "!unregistered" : it->second, grid, block, args);
    return hipSuccess;
}
hipError_t hipGetLastError() { return hipSuccess; }
}

// ---------------------------------------------------------------------------
// The shapes.
// ---------------------------------------------------------------------------
struct Shape {
    uint64_t len;
    uint64_t n;
};

constexpr uint64_t kBig = (1ull << 32) + 8192;  // a shard of 4 GiB and more, a multiple of 8 KiB
constexpr uint64_t kPast = kMaxLaunchBlocks + 5;
constexpr uint64_t kLong = (kMaxLaunchBlocks + 2) * 4096;  // one stripe's 4 KiB chunks pass a launch (102 x 4096)

// Every length with one stripe and with a count past the small-grid limits
// (trimmed where a stripe is a launch of its own); every count with 4096 and
// 4096 + 16 bytes (one and two 4 KiB chunks per stripe); then the stripes past
// the limits of the 8 KiB and 2 KiB kernels, kMaxLaunchBlocks + 5 stripes of
// one chunk each under every sizing, and the empty batches.
static std::vector<Shape> family() {
    std::vector<Shape> s;
    for (uint64_t len : {1ull, 2048ull, 4096ull, 4112ull, 8192ull}) s.insert(s.end(), {{len, 1}, {len, 130}});
    s.insert(s.end(), {{101 * 2048, 1}, {101 * 2048, 3}, {kLong, 1}, {kLong, 3}});
    s.insert(s.end(), {{kBig, 1}, {kBig, 9}, {kBig + 16, 1}});
    for (uint64_t n : {50, 51, 100, 101}) s.insert(s.end(), {{4096, n}, {4112, n}});
    s.insert(s.end(), {{8192, 101}, {2048, 101}});
    s.insert(s.end(), {{2048, kPast}, {8192, kPast}});
    s.insert(s.end(), {{4096, 0}, {0, 130}});
    return s;
}

// The few shapes of a launcher with no branch on the count (grid-stride only).
static std::vector<Shape> few() { return {{1, 1}, {4112, 130}, {kLong, 3}, {kBig, 1}, {2048, kPast}, {4096, 0}, {0, 130}}; }

static ApplyArgs apply_of(Shape s, bool masks, bool in_place, bool fast104 = true) {
    ApplyArgs a{};
    const uint64_t pitch = (s.len + 15) / 16 * 16 + 16;
    a.in_base = kIn;
    a.in_stripe = 14 * pitch;
    a.in_shard = pitch;
    a.out_base = in_place ? kIn : kOut;
    a.out_stripe = in_place ? a.in_stripe : 4 * pitch;
    a.out_shard = pitch;
    a.len = s.len;
    a.n_stripes = uint32_t(s.n);
    a.plans = reinterpret_cast<const DevPlan*>(kFake);
    a.tabs = a.idx = a.lut = kFake;
    a.masks = masks ? kMasks : nullptr;
    a.mask_limit = (1u << 14) - 1;
    a.bad_count = kFake;
    a.fast104 = fast104 ? 1 : 0;
    a.done_count = a.done_flag = kFake;  // set on every batch: only the last launch may keep it
    a.done_seq = 7;
    return a;
}

static UpdateArgs update_of(Shape s, bool old) {
    UpdateArgs u;
    u.a = apply_of(s, true, false);
    if (old) {
        u.old_base = kOld;
        u.old_stripe = u.a.in_stripe;
        u.old_shard = u.a.in_shard;
    }
    return u;
}

// One launcher call under a tag; a call that launches nothing says so.
template <typename F>
static void run(const char* tag, F call) {
    g_tag = tag;
    g_launches = 0;
    const hipError_t e = call();
    if (e != hipSuccess) {
        std::printf("%s: the launcher returned error %d\n", tag, int(e));
        std::exit(1);
    }
    if (g_launches == 0) std::printf(" %s: no launch\n", tag);
}

static void title(const char* what, Shape s) {
    std::printf("%s len=%llu n=%llu\n", what, (unsigned long long)s.len, (unsigned long long)s.n);
}

static void strided() {
    for (Shape s : family()) {
        title("strided", s);
        run("encode", [&] { return launch_apply(apply_of(s, false, false), 10, true, false, nullptr); });
        run("encode over_pcie", [&] { return launch_apply(apply_of(s, false, false), 10, true, true, nullptr); });
        run("decode", [&] { return launch_apply(apply_of(s, true, true), 10, true, false, nullptr); });
        run("some", [&] { return launch_some(SomeArgs{apply_of(s, true, true), kWords}, true, nullptr); });
        run("update old", [&] { return launch_update(update_of(s, true), true, nullptr); });
        run("verify", [&] { return launch_verify(VerifyArgs{apply_of(s, false, false), kWords}, 10, true, nullptr); });
        run("check", [&] { return launch_check(CheckArgs{apply_of(s, true, true), kWords}, true, nullptr); });
    }
    // ten ranges of launch_apply (the other launchers' longest above is three)
    title("strided", {4096, 1000});
    run("encode", [&] { return launch_apply(apply_of({4096, 1000}, false, false), 10, true, false, nullptr); });
    run("decode", [&] { return launch_apply(apply_of({4096, 1000}, true, true), 10, true, false, nullptr); });
    for (Shape s : few()) {
        title("strided, other layouts", s);
        run("decode over_pcie", [&] { return launch_apply(apply_of(s, true, true), 10, true, true, nullptr); });
        run("encode unaligned", [&] { return launch_apply(apply_of(s, false, false), 10, false, false, nullptr); });
        run("decode unaligned", [&] { return launch_apply(apply_of(s, true, true), 10, false, false, nullptr); });
        run("encode nin=6", [&] { return launch_apply(apply_of(s, false, false, false), 6, true, false, nullptr); });
        run("decode nin=6 unaligned",
            [&] { return launch_apply(apply_of(s, true, true, false), 6, false, false, nullptr); });
        run("encode nin=10 not fast104",
            [&] { return launch_apply(apply_of(s, false, false, false), 10, true, false, nullptr); });
        run("some unaligned", [&] { return launch_some(SomeArgs{apply_of(s, true, true), kWords}, false, nullptr); });
        run("update", [&] { return launch_update(update_of(s, false), true, nullptr); });
        run("update unaligned", [&] { return launch_update(update_of(s, false), false, nullptr); });
        run("update old unaligned", [&] { return launch_update(update_of(s, true), false, nullptr); });
        run("verify unaligned",
            [&] { return launch_verify(VerifyArgs{apply_of(s, false, false), kWords}, 10, false, nullptr); });
        run("verify nin=10 not fast104",
            [&] { return launch_verify(VerifyArgs{apply_of(s, false, false, false), kWords}, 10, true, nullptr); });
        run("verify nin=6",
            [&] { return launch_verify(VerifyArgs{apply_of(s, false, false, false), kWords}, 6, true, nullptr); });
        run("verify nin=6 unaligned",
            [&] { return launch_verify(VerifyArgs{apply_of(s, false, false, false), kWords}, 6, false, nullptr); });
        run("check unaligned", [&] { return launch_check(CheckArgs{apply_of(s, true, true), kWords}, false, nullptr); });
    }
}

// Item counts below, at and above kLocateMaxBlocks in either build; the
// unaligned and the pairs forms take the same path on fewer shapes.
static void locates() {
    const std::vector<Shape> shapes = {{4096, 3}, {4112, 2},    {4096, 2049}, {4096, 1}, {4096, 4}, {4096, 5},
                                       {1, 130},  {4096, 2047}, {kBig, 1},    {4096, 0}, {0, 5}};
    for (size_t i = 0; i < shapes.size(); ++i) {
        const Shape s = shapes[i];
        title("locate", s);
        for (bool aligned : {true, false})
            for (bool pairs : {false, true}) {
                if ((!aligned || pairs) && i >= 3) continue;
                CorrectArgs c;
                c.a = apply_of(s, false, false);
                c.mismatch = kWords;
                c.suspects = kFake;
                c.ratio_tabs = c.pair_tabs = c.fix_tabs = kFake;
                const std::string form = std::string(aligned ? "" : " unaligned") + (pairs ? " pairs" : "");
                run(("locate" + form).c_str(), [&] { return launch_locate(c, aligned, pairs, nullptr); });
                run(("correct" + form).c_str(), [&] { return launch_correct(c, aligned, pairs, nullptr); });
                if (pairs) continue;
                CorrectPresentArgs p;
                p.a = apply_of(s, true, true);
                p.check = kWords;
                p.suspects = kFake;
                p.ratio_tabs = p.fix_tabs = kFake;
                run(("locate_present" + form).c_str(), [&] { return launch_locate_present(p, aligned, nullptr); });
                run(("correct_present" + form).c_str(), [&] { return launch_correct_present(p, aligned, nullptr); });
            }
    }
}

static void ragged() {
    for (uint64_t n : {0ull, 1ull, 99ull, 100ull, 101ull, 257ull, (unsigned long long)kPast}) {
        RaggedCorrectArgs c;
        RaggedArgs& a = c.a;
        a = RaggedArgs{};
        a.base = kIn;
        a.items = reinterpret_cast<const RaggedItem*>(kFake);
        a.block_item = a.tabs = a.lut = kFake;
        a.n_blocks = uint32_t(n);
        a.bad_count = kFake;
        a.done_count = a.done_flag = kFake;  // only the last launch may keep it
        a.done_seq = 7;
        c.check = kWords;
        c.suspects = c.uncorrected = kFake;
        c.ratio_tabs = c.fix_tabs = kFake;
        std::printf("ragged blocks=%llu\n", (unsigned long long)n);
        run("encode", [&] { return launch_rs104_ragged(a, false, nullptr); });
        run("bit-sliced encode", [&] { return launch_rs104_bs_ragged(a, nullptr); });
        if (n == 0 || n == 101) {  // the other users of the same block-launch loop
            run("decode", [&] { return launch_rs104_ragged(a, true, nullptr); });
            run("some", [&] { return launch_rs104_ragged_some(a, nullptr); });
            a.compact = 1;
            run("decode compact", [&] { return launch_rs104_ragged(a, true, nullptr); });
            run("some compact", [&] { return launch_rs104_ragged_some(a, nullptr); });
            a.compact = 0;
        }
        run("check", [&] { return launch_ragged_check(c, false, nullptr); });
        run("locate", [&] { return launch_ragged_locate(c, false, nullptr); });
        run("correct", [&] { return launch_ragged_correct(c, false, nullptr); });
        run("check bitslice", [&] { return launch_ragged_check(c, true, nullptr); });
        run("locate bitslice", [&] { return launch_ragged_locate(c, true, nullptr); });
        run("correct bitslice", [&] { return launch_ragged_correct(c, true, nullptr); });
    }
}

static void masks() {
    RaggedItem* items = reinterpret_cast<RaggedItem*>(kFake);
    for (uint32_t n : {0u, 1u, 1024u, 1025u, 5000u}) {
        std::printf("masks n=%u\n", n);
        run("repair", [&] { return launch_repair_masks(kFake, kMasks, kFake, n, nullptr); });
        run("use", [&] { return launch_use_masks(kMasks, kWords, kFake, kMasks, kFake, n, nullptr); });
        run("use corrected",
            [&] { return launch_use_masks_corrected(kMasks, kWords, kFake, kMasks, kFake, 2, n, nullptr); });
        run("ragged use corrected", [&] {
            return launch_ragged_use_masks_corrected(items, items, kWords, kFake, kMasks, kFake, 2, n, nullptr);
        });
    }
}

int main(int argc, char** argv) {
    if (argc > 1 && std::strcmp(argv[1], "--registered") == 0) {
        for (const auto& kv : registered()) std::printf("%s\n", kv.second.c_str());
        return 0;
    }
    uint64_t max_launch = kMaxLaunchBlocks;
    uint32_t locate_max = kLocateMaxBlocks;
#ifdef HEC_MAX_LAUNCH_BLOCKS
    hec_test_launch_limits(&max_launch, &locate_max);  // the object's own: it must agree with this program's header
    if (max_launch != kMaxLaunchBlocks || locate_max != kLocateMaxBlocks) {
        std::printf("the object was compiled with other limits than this program\n");
        return 1;
    }
#endif
    std::printf("limits max_launch_blocks=%llu locate_max_blocks=%u\n", (unsigned long long)max_launch, locate_max);
    strided();
    locates();
    ragged();
    masks();
    return 0;
}
