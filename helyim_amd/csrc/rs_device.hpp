// Device helpers and the ragged launch loop shared by the kernel files
// (rs_kernels.hip, rs_update_ragged.hip): vector access, the table multiply,
// the completion signal and the ragged workgroup map. Each file compiles its
// own copy; nothing here is a kernel.
#pragma once
#include "rs_kernels.hpp"
#include "launch_split.hpp"

namespace hec {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// Scalar-cache view of plan metadata: uniform loads through the constant
// address space become s_load (SGPR) instead of per-lane vector loads.
template <typename T>
__device__ __forceinline__ const __attribute__((address_space(4))) T* as_const(const T* p) {
    return (const __attribute__((address_space(4))) T*)(p);
}
typedef const __attribute__((address_space(4))) uint32_t* cu32p;

// Global-address-space views: the nontemporal hint on a flat (generic)
// pointer is dropped by the backend (plain global_load_dwordx4), so the
// streamed shards -- each byte touched exactly once -- are accessed through
// address_space(1) pointers to get `nt` (+2-4%, profiles/r01/tune11_*.jsonl;
// other cache policies through raw buffer instructions measured no better,
// profiles/r02/ab_cache_policy_buffer_*.txt).
typedef const __attribute__((address_space(1))) u32x4* gcu32x4p;
typedef __attribute__((address_space(1))) u32x4* gu32x4p;
typedef const __attribute__((address_space(1))) uint8_t* gcu8p;
typedef __attribute__((address_space(1))) uint8_t* gu8p;

__device__ __forceinline__ u32x4 load_full(const uint8_t* p, bool aligned) {
    if (aligned) return __builtin_nontemporal_load((gcu32x4p)(p));
    u32x4 v;
    __builtin_memcpy(&v, p, 16);
    return v;
}

__device__ __forceinline__ void store_full(uint8_t* p, u32x4 v, bool aligned) {
    if (aligned)
        __builtin_nontemporal_store(v, (gu32x4p)(p));
    else
        __builtin_memcpy(p, &v, 16);
}

// Streamed access at (uniform shard base) + (lane offset): the base is moved
// to the global address space before the offset is added, so a 32-bit offset
// becomes the saddr form (SGPR base + VGPR offset) with no 64-bit VALU math.
template <typename OffT>
__device__ __forceinline__ u32x4 load_at(const uint8_t* base, OffT o) {
    return __builtin_nontemporal_load((gcu32x4p)((gcu8p)(base) + o));
}
template <typename OffT>
__device__ __forceinline__ void store_at(uint8_t* base, OffT o, u32x4 v) {
    __builtin_nontemporal_store(v, (gu32x4p)((gu8p)(base) + o));
}

__device__ __noinline__ u32x4 load_tail(const uint8_t* p, uint64_t avail) {
    uint8_t b[16];
    for (int i = 0; i < 16; ++i) b[i] = (uint64_t(i) < avail) ? p[i] : 0;
    u32x4 v;
    __builtin_memcpy(&v, b, 16);
    return v;
}

__device__ __noinline__ void store_tail(uint8_t* p, u32x4 v, uint64_t avail) {
    uint8_t b[16];
    __builtin_memcpy(b, &v, 16);
    for (int i = 0; i < 16; ++i)
        if (uint64_t(i) < avail) p[i] = b[i];
}

// acc[r] ^= coef(r) * d for R output rows; tab -> [rows][5] words of this input.
template <int R>
__device__ __forceinline__ void gf_mac(u32x4 (&acc)[R], const u32x4 d, cu32p tab) {
    uint32_t s0[4], s1[4], s2[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const uint32_t x = d[w];
        s0[w] = x & 0x07070707u;
        s1[w] = (x >> 3) & 0x07070707u;
        s2[w] = (x >> 6) & 0x03030303u;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t t0l = tab[r * 5 + 0], t0h = tab[r * 5 + 1];
        const uint32_t t1l = tab[r * 5 + 2], t1h = tab[r * 5 + 3];
        const uint32_t t2 = tab[r * 5 + 4];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t a = __builtin_amdgcn_perm(t0h, t0l, s0[w]);
            const uint32_t b = __builtin_amdgcn_perm(t1h, t1l, s1[w]);
            const uint32_t c = __builtin_amdgcn_perm(t2, t2, s2[w]);
            acc[r][w] = __builtin_amdgcn_bitop3_b32(acc[r][w], a, b, 0x96) ^ c;
        }
    }
}

// gf_mac with accumulator r taking table row `row[r]` (reconstruct some, the
// byte-wise tail of a shard).
template <int R>
__device__ __forceinline__ void gf_mac_rows(u32x4 (&acc)[R], const u32x4 d, cu32p tab, const uint32_t (&row)[R]) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
        u32x4 one[1] = {acc[r]};
        gf_mac<1>(one, d, tab + row[r] * 5);
        acc[r] = one[0];
    }
}

// The rows a reconstruct-some decode computes, all wave-uniform scalar work:
// w = want & erased, out[q] = the q-th set bit of w (ascending), row[q] = that
// shard's row in the mask's plan (its rank among the erased shards). Entries
// at or past nout = popcount(w) are 0, a valid row that is computed by nobody
// (gf_mac2's prefix break) and never stored.
struct SomeRows {
    uint32_t nout;
    uint32_t out[4], row[4];
};
__device__ __forceinline__ SomeRows some_rows(uint32_t erased, uint32_t want) {
    SomeRows s;
    uint32_t w = want & erased;
    s.nout = __builtin_popcount(w);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        s.out[q] = w ? __builtin_ctz(w) : 0;
        s.row[q] = w ? __builtin_popcount(erased & ((1u << s.out[q]) - 1)) : 0;
        w &= w - 1;
    }
    return s;
}

// Two inputs at once: the six lookups of a row are folded into the
// accumulator by three 3-input XORs (v_bitop3) instead of four ops.
// nrows (wave-uniform, <= R): rows at or past it skip their math (a decode
// with e < 4 erasures; scalar branches, the tables keep their 4-row stride).
// ROWS (reconstruct some): accumulator r takes table row `row[r]` of the set
// instead of row r; the prefix break at nrows stays.
template <int R, typename V = u32x4, bool ROWS = false>
__device__ __forceinline__ void gf_mac2(V (&acc)[R], const V d0, const V d1, cu32p tab0, cu32p tab1,
                                        uint32_t nrows = R, const uint32_t* row = nullptr) {
    constexpr int W = int(sizeof(V) / 4);  // dwords per lane vector
    uint32_t s[2][3][W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const uint32_t x0 = d0[w], x1 = d1[w];
        s[0][0][w] = x0 & 0x07070707u;
        s[0][1][w] = (x0 >> 3) & 0x07070707u;
        s[0][2][w] = (x0 >> 6) & 0x03030303u;
        s[1][0][w] = x1 & 0x07070707u;
        s[1][1][w] = (x1 >> 3) & 0x07070707u;
        s[1][2][w] = (x1 >> 6) & 0x03030303u;
    }
    // both inputs' table words for every row, requested before the row
    // branches (the empty asm keeps the loads from sinking into them, where
    // each row would wait on its own scalar round trip)
    uint32_t ta[R * 5], tbw[R * 5];
#pragma unroll
    for (int j = 0; j < R * 5; ++j) {
        const uint32_t at = ROWS ? row[j / 5] * 5 + uint32_t(j % 5) : uint32_t(j);
        ta[j] = tab0[at];
        tbw[j] = tab1[at];
    }
    if (R < 4 || nrows < uint32_t(R)) {
#pragma unroll
        for (int j = 0; j < R * 5; ++j) asm volatile("" ::"s"(ta[j]), "s"(tbw[j]));
    }
#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (r > 0 && uint32_t(r) >= nrows) break;
        const uint32_t a0l = ta[r * 5 + 0], a0h = ta[r * 5 + 1], a1l = ta[r * 5 + 2], a1h = ta[r * 5 + 3],
                       a2 = ta[r * 5 + 4];
        const uint32_t b0l = tbw[r * 5 + 0], b0h = tbw[r * 5 + 1], b1l = tbw[r * 5 + 2], b1h = tbw[r * 5 + 3],
                       b2 = tbw[r * 5 + 4];
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t p0 = __builtin_amdgcn_perm(a0h, a0l, s[0][0][w]);
            const uint32_t p1 = __builtin_amdgcn_perm(a1h, a1l, s[0][1][w]);
            const uint32_t p2 = __builtin_amdgcn_perm(a2, a2, s[0][2][w]);
            const uint32_t q0 = __builtin_amdgcn_perm(b0h, b0l, s[1][0][w]);
            const uint32_t q1 = __builtin_amdgcn_perm(b1h, b1l, s[1][1][w]);
            const uint32_t q2 = __builtin_amdgcn_perm(b2, b2, s[1][2][w]);
            uint32_t x = __builtin_amdgcn_bitop3_b32(acc[r][w], p0, p1, 0x96);
            x = __builtin_amdgcn_bitop3_b32(x, p2, q0, 0x96);
            acc[r][w] = __builtin_amdgcn_bitop3_b32(x, q1, q2, 0x96);
        }
    }
}

// Completion signal of a launch for a host that spins on pinned memory
// (small host calls): every wave drains its stores, the
// workgroup meets at a barrier, lane 0 releases at system scope and counts
// itself in; the last workgroup resets the counter and stores the sequence
// number into the host flag. Every workgroup of the grid reaches this (the
// kernels call it after their body, early exits included).
__device__ __forceinline__ void signal_done(uint32_t* count, uint32_t* flag, uint32_t seq) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (threadIdx.x == 0) {
        __threadfence_system();
        const uint32_t blocks = gridDim.x * gridDim.y * gridDim.z;
        if (__hip_atomic_fetch_add(count, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) == blocks - 1) {
            __hip_atomic_store(count, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __threadfence_system();
            __hip_atomic_store(flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// Map entry of this workgroup: XCD x = blockIdx % 8 takes the x-th eighth of
// the launch's entries, so the workgroups sharing an XCD (and its L2) stream
// consecutive chunks, as in the strided kernels. The ragged decode +2% on the
// bench batch (with the no-op skip +10% on the mixed workload,
// profiles/r02/ab_ragged_remap_skip.jsonl); the bit-sliced ragged encode +2%
// at 512 mixed stripes, +7% at 4096 and +9% on uniform 4 MiB stripes
// (profiles/r03/sweep_mixed2.jsonl).
__device__ __forceinline__ uint32_t ragged_block(const RaggedArgs& a) {
    const uint32_t b = blockIdx.x, x = b & 7u;
    return x * a.map_q8 + (x < a.map_r8 ? x : a.map_r8) + (b >> 3) + a.block_base;
}

// The batch of any ragged kernel argument struct.
inline RaggedArgs& ragged_args(RaggedArgs& a) { return a; }
inline RaggedArgs& ragged_args(RaggedScrubArgs& v) { return v.a; }
inline RaggedArgs& ragged_args(RaggedUpdateArgs& v) { return v.a; }

// A ragged batch through `kern`, in launches of at most kMaxLaunchBlocks
// workgroups (launch_split.hpp).
template <typename Args>
static hipError_t launch_ragged(void (*kern)(Args), const Args& v, hipStream_t stream) {
    Args w = v;
    RaggedArgs& r = ragged_args(w);
    const RaggedArgs a = r;
    for (uint64_t i = 0, n = n_ranges(a.n_blocks, kMaxLaunchBlocks); i < n; ++i) {
        const BlockLaunch l = block_launch(a.n_blocks, kMaxLaunchBlocks, i);
        r = a;
        r.block_base = l.block_base;
        r.map_q8 = l.map_q8;
        r.map_r8 = l.map_r8;
        if (!l.last) r.done_flag = nullptr;  // the last launch signals
        hipLaunchKernelGGL(kern, dim3(l.n_blocks), dim3(kThreads), 0, stream, w);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace hec
