"""Reconstruct some on the GPU (include/hec.h hec_gpu_reconstruct_some_batch and
its ragged, host, per-call and batch forms): whole arenas of seeded random
bytes with 4 KiB of slack, erased slots holding random bytes too, compared byte
for byte -- and the counters -- with tests/some_model.py: exactly the wanted
erased shards change, to the C oracle's bytes."""
import ctypes

import numpy as np
import pytest

import footprint as F
import some_model as M
from footprint import HOST_PATHS, HostArenas, host_path, present_of, stream_ptr, to_device, to_host

pytestmark = pytest.mark.gpu

K, MP, N = 10, 4, 14
FULL = 0x3FFF
INVALID_ARGUMENT, EMPTY_SHARD = 66, 11
NARROW, TABLE, GENERIC = "rs104_narrow_some_kernel", "rs104_some_kernel", "rs_some_kernel"


def erase(rng, e):
    return FULL & ~sum(1 << int(i) for i in rng.choice(N, e, replace=False))


def noisy(rng, mask, w):
    """w with bits of present shards and bits 14 to 31 set at random: W = w & ~mask stays."""
    return (w | (int(rng.integers(0, 1 << 32)) & (mask | ~FULL))) & 0xFFFFFFFF


def full_pair_set(rng):
    """Every (mask, W) pair, then stripes with 9 present (W non-empty: counted;
    W empty: not counted) and all-present stripes; noisy want words."""
    pairs = list(M.every_pair())
    counted = 0
    for _ in range(6):
        m = erase(rng, 5)
        gone = [i for i in range(N) if not (m >> i) & 1]
        pairs.append((m, 1 << gone[int(rng.integers(0, 5))]))
        pairs.append((m, sum(1 << i for i in gone)))
        pairs.append((m, 0))
        counted += 2
    pairs += [(FULL, 0), (FULL, FULL), (FULL | 0x7FFFC000, 1 << 3)]
    return [(m, noisy(rng, m, w)) for m, w in pairs], counted


def random_pairs(rng, S):
    """S seeded pairs: 0 to 5 erasures, any subset of the erased shards."""
    out = []
    for _ in range(S):
        m = erase(rng, int(rng.integers(0, 6)))
        gone = [i for i in range(N) if not (m >> i) & 1]
        w = sum(1 << i for i in gone if rng.integers(0, 2))
        out.append((m, noisy(rng, m, w)))
    return out


def gpu_some(rs, devs, lay, masks, wants):
    """-> (status, counter) of hec_gpu_reconstruct_some_batch on the device arena"""
    import torch
    import helyim_amd as H
    dm = torch.from_numpy(np.array(masks, dtype=np.uint32).view(np.int32)).cuda()
    dw = torch.from_numpy(np.array(wants, dtype=np.uint32).view(np.int32)).cuda()
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    rc = H.lib.hec_gpu_reconstruct_some_batch(rs.handle, devs[0].data_ptr() + lay.base, lay.stripe_stride,
                                              lay.shard_stride, lay.L, lay.S, dm.data_ptr(), dw.data_ptr(),
                                              bad.data_ptr(), stream_ptr())
    torch.cuda.synchronize()
    return rc, int(bad.item())


def batch_name(devs, lay):
    import helyim_amd as H
    return H.lib.hec_reconstruct_some_batch_kernel_name(devs[0].data_ptr() + lay.base, lay.stripe_stride,
                                                        lay.shard_stride, lay.L, lay.S).decode()


def check_gpu_some(rs, rng, lay, pairs, kernel, n_counted=None):
    import helyim_amd as H
    masks, wants = [m for m, _ in pairs], [w for _, w in pairs]
    stripes = F.stripes_of(lay)
    arenas = [F.random_arena(sz, rng) for sz in F.arena_sizes(stripes)]
    plan = M.plan_reconstruct_some(arenas, stripes, K, MP, present_of(masks, N), wants)
    if n_counted is not None:
        assert plan.n_bad == n_counted and plan.n_noop_short > 0
    devs = to_device(arenas)
    # the launcher's choice for this base and these strides: the generic kernel exactly on the odd ones
    # (which of the two aligned kernels a stripe range runs also depends on the launch limit of the build)
    assert batch_name(devs, lay).startswith(GENERIC) == (kernel == GENERIC), (batch_name(devs, lay), lay)
    if kernel != GENERIC:
        assert H.lib.hec_reconstruct_some_kernel_name(lay.L).decode().startswith(kernel)
    if lay.L == 2048:
        assert batch_name(devs, lay).startswith(NARROW)
    rc, bad = gpu_some(rs, devs, lay, masks, wants)
    assert rc == 0
    F.assert_footprint(plan, to_host(devs), (kernel, lay))
    M.assert_counted(plan, bad, (kernel, lay))


@pytest.mark.parametrize("L,kernel", [(2048, NARROW), (1040, TABLE), (1000, TABLE)])
def test_every_mask_and_want_pair(gpu, L, kernel):
    """1. Every (mask, W) pair in one batch: the 8-byte narrow kernel at 2048;
    the table kernel with full vectors and a second wave of one live lane at
    1040, and with the byte-wise tail at 1000."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(100 + L)
    pairs, counted = full_pair_set(rng)
    assert len(pairs) == 19320 + 21
    check_gpu_some(rs, rng, F.stripe_major(N, L, len(pairs), F.r16(L)), pairs, kernel, counted)


@pytest.mark.parametrize("L,kernel", [(4096, NARROW), (4096 + 1000, TABLE)])
def test_two_chunks_per_stripe(gpu, L, kernel):
    """2. 200 seeded pairs on stripes of two column ranges per workgroup map."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(200 + L)
    check_gpu_some(rs, rng, F.stripe_major(N, L, 200, F.r16(L) + 16, 48), random_pairs(rng, 200), kernel)


LAYOUTS = {
    "stripe-major, pads and gaps": lambda S: (F.stripe_major(N, 301, S, F.r16(301) + 48, 4096 + 32), TABLE),
    "shard-major": lambda S: (F.shard_major(N, 301, S, F.r16(301) + 16, 48), TABLE),
    "odd base": lambda S: (F.stripe_major(N, 301, S, F.r16(301) + 16, 16, base=F.SLACK + 3), GENERIC),
    "odd strides": lambda S: (F.stripe_major(N, 301, S, 301 + 3, 5), GENERIC),
    "odd shard-major strides": lambda S: (F.shard_major(N, 301, S, 301 + 3, 7), GENERIC),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_layouts(gpu, layout):
    """3. The full pair set at L = 301 on strided layouts; odd bases and
    strides take the generic kernel and keep the footprint."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(300 + len(layout))
    pairs, counted = full_pair_set(rng)
    lay, kernel = LAYOUTS[layout](len(pairs))
    check_gpu_some(rs, rng, lay, pairs, kernel, counted)


def ragged_batch(rng, lens):
    """descs rows, stripes and (mask, want) pairs of a ragged batch with
    16-byte-aligned gaps between shards and between stripes."""
    descs, off = [], F.SLACK
    pairs = random_pairs(rng, len(lens))
    for j, L in enumerate(lens):
        stride = F.r16(L) + 16 * (j % 3)
        off += 16 * int(rng.integers(0, 4))
        descs.append([off, stride, L, pairs[j][0]])
        off += 13 * stride + F.r16(L)
    stripes = [F.Stripe(L, tuple((0, o + i * st) for i in range(N))) for o, st, L, _ in descs]
    return descs, stripes, pairs


@pytest.mark.parametrize("L", [2048, 1000])
def test_want_all_equals_reconstruct_batch(gpu, L):
    """4. With every want bit set the device call gives the arena and counter
    of hec_gpu_reconstruct_batch on a clone."""
    import torch
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(400 + L)
    S = 300
    lay = F.stripe_major(N, L, S, F.r16(L) + 16, 32)
    masks = [m for m, _ in random_pairs(rng, S)]
    arenas = [F.random_arena(sz, rng) for sz in F.arena_sizes(F.stripes_of(lay))]
    for wants in ([0xFFFFFFFF] * S, [FULL] * S):
        devs, clone = to_device(arenas), to_device(arenas)
        rc, bad = gpu_some(rs, devs, lay, masks, wants)
        dm = torch.from_numpy(np.array(masks, dtype=np.uint32).view(np.int32)).cuda()
        bad2 = torch.zeros(1, dtype=torch.int32, device="cuda")
        assert H.lib.hec_gpu_reconstruct_batch(rs.handle, clone[0].data_ptr() + lay.base, lay.stripe_stride,
                                               lay.shard_stride, L, S, dm.data_ptr(), bad2.data_ptr(),
                                               stream_ptr()) == 0
        assert rc == 0 and bad == int(bad2.item()) > 0
        assert torch.equal(devs[0], clone[0])


def test_want_all_equals_the_ragged_and_host_calls(gpu):
    """4. The same for hec_gpu_reconstruct_some_ragged against
    hec_gpu_reconstruct_ragged, and for the host call on pinned memory."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(450)
    lens = [int(x) for x in rng.choice([16, 1000, 2048, 4096, 8192 + 16], 60)]
    descs, stripes, _ = ragged_batch(rng, lens)
    arenas = [F.random_arena(sz, rng) for sz in F.arena_sizes(stripes)]
    devs, clone = to_device(arenas), to_device(arenas)
    bad, bad2 = (torch.zeros(1, dtype=torch.int32, device="cuda") for _ in range(2))
    B.reconstruct_some_ragged(rs, devs[0], descs, [0xFFFFFFFF] * len(descs), bad)
    B.reconstruct_ragged(rs, clone[0], descs, bad2)
    torch.cuda.synchronize()
    assert torch.equal(devs[0], clone[0]) and int(bad.item()) == int(bad2.item()) > 0
    # host, pinned in place
    S, L = 64, 1000
    lay = F.stripe_major(N, L, S, F.r16(L) + 16, 32)
    masks = [m for m, _ in random_pairs(rng, S)]
    size = F.arena_sizes(F.stripes_of(lay))[0]
    a = torch.from_numpy(F.random_arena(size, rng)).pin_memory()
    b = a.clone().pin_memory()
    va, vb = (t[lay.base:lay.base + S * lay.stripe_stride].view(S, lay.stripe_stride)[:, :N * lay.shard_stride]
              .view(S, N, lay.shard_stride)[:, :, :L] for t in (a, b))
    n1 = B.host_reconstruct_some_batch(rs, va, masks, [0xFFFFFFFF] * S)
    n2 = B.host_reconstruct_batch(rs, vb, masks)
    assert n1 == n2 > 0 and torch.equal(a, b)


def test_ragged(gpu):
    """5. 300 seeded ragged stripes of mixed lengths, masks and wants; many
    want nothing of what they lost and own no workgroup."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(500)
    choice = [16, 1000, 2048, 4096, 8192 + 16, 65536]
    lens = choice + [int(x) for x in rng.choice(choice, 294, p=[.25, .25, .2, .15, .1, .05])]
    descs, stripes, pairs = ragged_batch(rng, lens)
    for j in range(0, 300, 7):  # whole stripes without a wanted shard, short ones among them
        pairs[j] = (pairs[j][0], noisy(rng, pairs[j][0], 0))
    wants = [w for _, w in pairs]
    arenas = [F.random_arena(sz, rng) for sz in F.arena_sizes(stripes)]
    plan = M.plan_reconstruct_some(arenas, stripes, K, MP, present_of([m for m, _ in pairs], N), wants)
    assert plan.n_bad > 0 and plan.n_noop_short > 0
    assert sum(r == [M.NOOP] * N for r in plan.roles) >= 30
    devs = to_device(arenas)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_some_ragged(rs, devs[0], descs, wants, bad)
    F.assert_footprint(plan, to_host(devs), "ragged")
    M.assert_counted(plan, int(bad.item()), "ragged")
    # a batch in which nobody wants anything launches nothing and changes nothing
    devs = to_device(arenas)
    B.reconstruct_some_ragged(rs, devs[0], descs, [noisy(rng, m, 0) for m, _ in pairs], bad)
    F.assert_unchanged(arenas, to_host(devs), stripes, "ragged, nothing wanted")


@pytest.fixture(scope="module")
def host_arenas(gpu):
    return HostArenas()


def host_some(rs, live, lay, masks, wants):
    import helyim_amd as H
    m, w = np.array(masks, dtype=np.uint32), np.array(wants, dtype=np.uint32)
    bad = ctypes.c_uint32(12345)
    rc = H.lib.hec_host_reconstruct_some_batch(rs.handle, live[lay.arena].ctypes.data + lay.base, lay.stripe_stride,
                                               lay.shard_stride, lay.L, lay.S, m.ctypes.data, w.ctypes.data,
                                               ctypes.byref(bad))
    return rc, bad.value


HOST_S, HOST_LENGTHS = 64, (1000, 2048)


@pytest.mark.parametrize("path", HOST_PATHS[1:2] + HOST_PATHS[:1] + HOST_PATHS[2:])
def test_host_batch(gpu, host_arenas, path):
    """6. The three host paths at L = 1000 and 2048, 64 stripes. The
    pinned-slot path comes first, after longer random stripes went through
    the slots it then reuses: what they left there must not come back."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(600 + HOST_PATHS.index(path))
    with host_path(path) as hp:
        if path == HOST_PATHS[1]:
            lay = F.stripe_major(N, 3000, 64, 3008)
            live, _ = host_arenas.take(path, F.stripes_of(lay), rng)
            pairs = random_pairs(rng, 64)
            assert host_some(rs, live, lay, [m for m, _ in pairs], [w for _, w in pairs])[0] == 0
        for L in HOST_LENGTHS:
            for lay in (F.stripe_major(N, L, HOST_S, F.r16(L) + 16, 48),
                        F.shard_major(N, L, HOST_S, F.r16(L) + 16, 48), F.stripe_major(N, L, HOST_S, L + 3, 5)):
                stripes = F.stripes_of(lay)
                live, before = host_arenas.take(path, stripes, rng)
                pairs = random_pairs(rng, HOST_S)
                short = erase(rng, 5)  # 9 present: counted when it wants a lost shard, a no-op when not
                pairs[:3] = [(pairs[0][0], noisy(rng, pairs[0][0], 0)), (short, 0xFFFFFFFF),
                             (short, noisy(rng, short, 0))]
                masks, wants = [m for m, _ in pairs], [w for _, w in pairs]
                plan = M.plan_reconstruct_some(before, stripes, K, MP, present_of(masks, N), wants)
                hp.check_view(live, lay)
                rc, bad = host_some(rs, live, lay, masks, wants)
                assert rc == 0
                F.assert_footprint(plan, live, (path, lay))
                M.assert_counted(plan, bad, (path, lay))


EDGE_S, EDGE_L = 64, 1000  # 22 chunks in the small-chunk build: 21 of 3 stripes and one of 1


def edge_pairs(rng, S):
    """A (mask, want) pair of its own per stripe, five kinds in turn: all lost
    shards wanted, one of several wanted, 9 present and none wanted (a no-op,
    not counted), 9 present and one lost shard wanted (counted), all present.
    Five kinds against chunks of three stripes: every kind falls on either side
    of a chunk edge and at every position of a chunk, with its neighbours of
    other kinds. -> (pairs, stripes counted)"""
    pairs = []
    for s in range(S):
        kind = s % 5
        m = erase(rng, (1 + s % 4, 2 + s % 3, 5, 5, 0)[kind])
        gone = [i for i in range(N) if not (m >> i) & 1]
        w = (0xFFFFFFFF, 1 << gone[s % len(gone)] if gone else 0, 0, 1 << gone[s % len(gone)] if gone else 0,
             0xFFFFFFFF)[kind]
        pairs.append((m, noisy(rng, m, w)))
    return pairs, sum(1 for s in range(S) if s % 5 == 3)


@pytest.mark.parametrize("path", HOST_PATHS)
def test_host_batch_across_chunk_edges(gpu, host_arenas, path):
    """6b. 64 stripes of 1000 bytes whose masks and wants differ from stripe to
    stripe (edge_pairs), on the three host paths, stripe-major and shard-major:
    footprint and counter against some_model. The product takes the batch in
    one chunk; in the small-chunk build (tests/test_gpu_small_chunk.py) every
    stripe lies at a chunk edge, so the want words must advance with the masks
    (wants + s0), each slot's launch must take its own words, and a stripe
    that wants nothing must stay uncounted past chunk 0."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(650 + HOST_PATHS.index(path))
    S, L = EDGE_S, EDGE_L
    with host_path(path) as hp:
        for lay in (F.stripe_major(N, L, S, F.r16(L) + 16, 48), F.shard_major(N, L, S, F.r16(L) + 16, 48)):
            stripes = F.stripes_of(lay)
            live, before = host_arenas.take(path, stripes, rng)
            pairs, counted = edge_pairs(rng, S)
            masks, wants = [m for m, _ in pairs], [w for _, w in pairs]
            plan = M.plan_reconstruct_some(before, stripes, K, MP, present_of(masks, N), wants)
            assert plan.n_bad == counted and plan.n_noop_short == sum(1 for s in range(S) if s % 5 == 2)
            hp.check_view(live, lay)
            rc, bad = host_some(rs, live, lay, masks, wants)
            assert rc == 0
            F.assert_footprint(plan, live, (path, lay))
            M.assert_counted(plan, bad, (path, lay))


PINNED_COPY_S, PINNED_COPY_L = 10, 1000  # chunks of 3, 3, 3 and 1 stripes in the small-chunk build
PINNED_COPY_LOST = (1, 2, 5, 0, 3, 4, 0, 1, 2, 5)  # shards lost per stripe: 5 | 0 at the first chunk edge, 5 alone last


def test_host_batch_pinned_memory_on_the_copy_pipeline(gpu, host_arenas):
    """6c. Pinned memory with zero copy off: the copy pipeline's 2-D copies
    read and write the caller's pinned arena (the three paths above give it
    pageable memory only). Ten stripes of 1000 bytes with a mask of its own
    each, against some_model: two stripes with 5 shards lost (one wants a lost
    shard, one everything: both counted, both untouched), two with none lost,
    one that wants nothing, the others all or one of their lost shards. In the
    small-chunk build the chunks are 3, 3, 3 and 1 stripes: all three streams
    and device slots reused, a short last chunk, and 1000 is a multiple of
    neither 16 nor 256."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(680)
    S, L = PINNED_COPY_S, PINNED_COPY_L
    lay = F.stripe_major(N, L, S, F.r16(L) + 16, 48)
    stripes = F.stripes_of(lay)
    masks, wants = [], []
    for s, e in enumerate(PINNED_COPY_LOST):
        m = erase(rng, e)
        gone = [i for i in range(N) if not (m >> i) & 1]
        kind = "all one one none none all one all none all".split()[s]
        w = {"all": 0xFFFFFFFF, "one": 1 << gone[s % len(gone)] if gone else 0, "none": 0}[kind]
        masks.append(m)
        wants.append(noisy(rng, m, w))
    with host_path(HOST_PATHS[2]) as hp:  # zero copy off ...
        live, before = host_arenas.take(HOST_PATHS[0], stripes, rng)  # ... on the pinned buffers
        plan = M.plan_reconstruct_some(before, stripes, K, MP, present_of(masks, N), wants)
        assert plan.n_bad == 2 and plan.n_noop_short == 0
        hp.check_view(live, lay)
        rc, bad = host_some(rs, live, lay, masks, wants)
        assert rc == 0
        F.assert_footprint(plan, live, ("pinned copy2d", lay))
        M.assert_counted(plan, bad, ("pinned copy2d", lay))


def per_call_stripe(rng, k, m, L, base):
    n = k + m
    stride = F.r16(L) + 16
    return F.Stripe(L, tuple((0, base + i * stride) for i in range(n))), base + n * stride + 32


@pytest.mark.parametrize("staging", [1 << 62, 0], ids=["staged", "unstaged"])
def test_per_call_and_batch(gpu, staging):
    """7. hec_rs_reconstruct_some_batch over stripes of eight lengths with
    random masks and flags, NULL pointers in the unrequired absent slots; the
    per-call form on RS(5,3) and RS(17,3); all flags = reconstruct, the data
    flags = reconstruct_data."""
    import helyim_amd as H
    lib = H.lib
    rng = np.random.default_rng(700)
    assert lib.hec_set_host_staging(staging) == 0
    try:
        lens = [1, 15, 16, 17, 1000, 4096, 4097, 65543]
        rs = H.ReedSolomon(K, MP)
        stripes, base = [], F.SLACK
        for L in lens * 2:
            st, base = per_call_stripe(rng, K, MP, L, base)
            stripes.append(st)
        arena = F.random_arena(F.arena_sizes(stripes)[0], rng)
        pairs = random_pairs(rng, len(stripes))
        pairs = [(m, w) if bin(m & FULL).count("1") >= K else (erase(rng, 4), w) for m, w in pairs]  # no failing stripe
        masks, wants = [m for m, _ in pairs], [w & FULL for _, w in pairs]
        plan = M.plan_reconstruct_some([arena], stripes, K, MP, present_of(masks, N), wants)
        ptrs, ln, pr, rq = [], [], [], []
        for st, mk, w in zip(stripes, masks, wants):
            for i, (_, o) in enumerate(st.locs):
                present, required = (mk >> i) & 1, (w >> i) & 1
                ptrs.append(None if not present and not required else arena.ctypes.data + o)
                ln.append(st.L if present else 0)
                pr.append(present)
                rq.append(required)
        c = len(ptrs)
        bad = ctypes.c_size_t(0)
        assert lib.hec_rs_reconstruct_some_batch(rs.handle, (ctypes.c_void_p * c)(*ptrs), (ctypes.c_size_t * c)(*ln),
                                                 (ctypes.c_uint8 * c)(*pr), (ctypes.c_uint8 * c)(*rq), len(stripes),
                                                 ctypes.byref(bad)) == 0
        assert bad.value == len(stripes)
        F.assert_footprint(plan, [arena], ("hec_rs_reconstruct_some_batch", staging))
        # per call, other codecs too (their plan's rows are filtered by the flags)
        for k, m in ((K, MP), (5, 3), (17, 3)):
            rsx, n = H.ReedSolomon(k, m), k + m
            for L in (17, 4097):
                for _ in range(4):
                    st, _ = per_call_stripe(rng, k, m, L, F.SLACK)
                    arena = F.random_arena(F.arena_sizes([st])[0], rng)
                    gone = [int(i) for i in rng.choice(n, int(rng.integers(1, m + 1)), replace=False)]
                    req = [int(rng.integers(0, 2)) for _ in range(n)]
                    present = [i not in gone for i in range(n)]
                    want = sum(1 << i for i in range(n) if req[i])
                    plan = M.plan_reconstruct_some([arena], [st], k, m, [present], [want])
                    ptrs = [None if not present[i] and not req[i] else arena.ctypes.data + o
                            for i, (_, o) in enumerate(st.locs)]
                    assert lib.hec_rs_reconstruct_some(rsx.handle, (ctypes.c_void_p * n)(*ptrs),
                                                       (ctypes.c_size_t * n)(*[L] * n),
                                                       (ctypes.c_uint8 * n)(*present), (ctypes.c_uint8 * n)(*req),
                                                       n) == 0
                    F.assert_footprint(plan, [arena], ("hec_rs_reconstruct_some", k, m, L, gone, req))
            # the two equivalences, through the Python wrapper
            shards = [rng.integers(0, 256, 1000, dtype=np.uint8) for _ in range(k)] + [np.zeros(1000, np.uint8)
                                                                                       for _ in range(m)]
            rsx.encode(shards)
            lost = [0, k - 1, k][:m]
            holes = lambda: [None if i in lost else s.copy() for i, s in enumerate(shards)]
            a, b = holes(), holes()
            rsx.reconstruct_some(a, [1] * n)
            rsx.reconstruct(b)
            assert all(np.array_equal(x, y) and np.array_equal(x, s) for x, y, s in zip(a, b, shards))
            a, b = holes(), holes()
            rsx.reconstruct_some(a, [1] * k + [0] * m)
            rsx.reconstruct_data(b)
            assert [x is None for x in a] == [y is None for y in b] == [i in lost and i >= k for i in range(n)]
            assert all(x is None or np.array_equal(x, y) for x, y in zip(a, b))
    finally:
        lib.hec_set_host_staging(16 << 20)


def test_refused_calls_leave_the_arena_unchanged(gpu):
    """8. Argument errors, an unsupported codec and an empty shard: nothing is written."""
    import torch
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    rng = np.random.default_rng(800)
    L, S = 1000, 5
    lay = F.stripe_major(N, L, S, F.r16(L) + 16, 48)
    stripes = F.stripes_of(lay)
    arenas = [F.random_arena(sz, rng) for sz in F.arena_sizes(stripes)]
    devs = to_device(arenas)
    dm = torch.full((S,), 0x3FF0, dtype=torch.int32, device="cuda")
    dw = torch.full((S,), 0xF, dtype=torch.int32, device="cuda")
    base = devs[0].data_ptr() + lay.base
    call = H.lib.hec_gpu_reconstruct_some_batch
    good = (base, lay.stripe_stride, lay.shard_stride, L, S, dm.data_ptr(), dw.data_ptr(), None, stream_ptr())
    for i, value, status in ((0, None, INVALID_ARGUMENT), (5, None, INVALID_ARGUMENT), (6, None, INVALID_ARGUMENT),
                             (3, 0, EMPTY_SHARD), (2, L - 1, INVALID_ARGUMENT), (1, L - 1, INVALID_ARGUMENT)):
        args = list(good)
        args[i] = value
        assert call(rs.handle, *args) == status, (i, value)
    assert call(H.ReedSolomon(10, 2).handle, *good) == INVALID_ARGUMENT
    assert call(None, *good) == INVALID_ARGUMENT
    F.assert_unchanged(arenas, to_host(devs), stripes, "refused device calls")
    # the ragged call: a null want list, a misaligned stripe
    descs = [[lay.off(s, 0), lay.shard_stride, L, 0x3FF0] for s in range(S)]
    import helyim_amd.batch as B
    d = np.array([tuple(r) for r in descs], dtype=B.desc_dtype())
    w = np.full(S, 0xF, dtype=np.uint32)
    ragged = H.lib.hec_gpu_reconstruct_some_ragged
    assert ragged(rs.handle, devs[0].data_ptr(), d.ctypes.data, None, S, None, stream_ptr()) == INVALID_ARGUMENT
    d["offset"][S - 1] += 8
    assert ragged(rs.handle, devs[0].data_ptr(), d.ctypes.data, w.ctypes.data, S, None,
                  stream_ptr()) == INVALID_ARGUMENT
    F.assert_unchanged(arenas, to_host(devs), stripes, "refused ragged calls")
    # the host call, and a batch with a failing stripe
    live = [a.copy() for a in arenas]
    m = np.full(S, 0x3FF0, dtype=np.uint32)
    host = H.lib.hec_host_reconstruct_some_batch
    hb = live[0].ctypes.data + lay.base
    assert host(rs.handle, hb, lay.stripe_stride, lay.shard_stride, L, S, m.ctypes.data, None, None) == INVALID_ARGUMENT
    assert host(rs.handle, hb, lay.stripe_stride, L - 8, L, S, m.ctypes.data, w.ctypes.data, None) == INVALID_ARGUMENT
    st = stripes[:2]
    c = 2 * N
    ptrs = (ctypes.c_void_p * c)(*[live[0].ctypes.data + o for s in st for _, o in s.locs])
    ln = (ctypes.c_size_t * c)(*[L] * c)
    pr = (ctypes.c_uint8 * c)(*([0, 0] + [1] * 12 + [0] * 5 + [1] * 9))
    rq = (ctypes.c_uint8 * c)(*[1] * c)
    bad = ctypes.c_size_t(9)
    assert H.lib.hec_rs_reconstruct_some_batch(rs.handle, ptrs, ln, pr, rq, 2, ctypes.byref(bad)) == 10
    assert bad.value == 1
    F.assert_unchanged(arenas, live, stripes, "refused host calls")
