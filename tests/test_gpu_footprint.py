"""Write footprint of every coding entry point on strided layouts: each call
runs on shards inside a flat arena of seeded random bytes (gaps, slack, erased
slots and outputs included) and the WHOLE arena afterwards must equal the
image tests/footprint.py builds from the arena's own bytes with the C oracle.
A 16-byte store where fewer bytes were due, a write one chunk too far, swapped
or mixed-up strides, a touched survivor or skipped stripe: any of them changes
a byte the image keeps.

Layout families (strides of the aligned ones are the shard length rounded up
to 16 plus a pad, so odd lengths reach the fast kernels' byte-wise tails):
A stripe-major, B shard-major ([shards][S][L], stripe stride < shard stride),
C data and parity apart in different families (parity also in a second arena),
D odd bases or strides (the generic kernel's unaligned path)."""
import ctypes

import numpy as np
import pytest

import footprint as F
from footprint import HOST_PATHS, HostArenas, host_path, present_of, stream_ptr, to_device, to_host

pytestmark = pytest.mark.gpu

SIZES = (1, 3, 9)  # nine 2-4 KiB items give the XCD-eighths map a quotient and a remainder
INVALID_ARGUMENT, INCORRECT_SHARD_SIZE, TOO_FEW_SHARDS_PRESENT = 66, 9, 10


# ---- layout families -----------------------------------------------------------
def family_a(n, L, S, pads=(0, 16, 48), gaps=(0, 16, 4096 + 32)):
    for pad in pads:
        for gap in gaps:
            yield f"A pad {pad} gap {gap}", F.stripe_major(n, L, S, F.r16(L) + pad, gap)


def family_b(n, L, S, pads=((0, 0), (16, 48), (48, 16))):
    for pad, pad2 in pads:
        yield f"B pad {pad} pad2 {pad2}", F.shard_major(n, L, S, F.r16(L) + pad, pad2)


def family_d(n, L, S):
    yield "D base + 3", F.stripe_major(n, L, S, F.r16(L) + 16, 16, base=F.SLACK + 3)
    yield "D stripe-major stride L + 3", F.stripe_major(n, L, S, L + 3, 5)
    yield "D shard-major stride L + 3", F.shard_major(n, L, S, L + 3, 7)


def family_c(k, m, L, S):
    """(name, data layout, parity layout): different families, one or two arenas."""
    da = F.stripe_major(k, L, S, F.r16(L) + 48, 16)
    db = F.shard_major(k, L, S, F.r16(L) + 16, 48)
    pa = F.stripe_major(m, L, S, F.r16(L) + 16, 4096 + 32)
    pb = F.shard_major(m, L, S, F.r16(L) + 16, 48)
    yield "C data A, parity B", da, pb.moved(F.r16(da.end) + 48)
    yield "C data B, parity A", db, pa.moved(F.r16(db.end) + 16)
    yield "C data A, parity B in a second arena", da, pb.moved(F.SLACK, arena=1)
    yield "C data B, parity A in a second arena", db, pa.moved(F.SLACK + 16, arena=1)


def family_cd(k, m, L, S):
    """C with an odd parity base: aligned data, unaligned parity."""
    da = F.stripe_major(k, L, S, F.r16(L) + 16, 0)
    yield "D data A, parity B at base + 3 in a second arena", da, \
        F.shard_major(m, L, S, L + 3, 7, base=F.SLACK + 3, arena=1)


def in_place(k, m, layouts):
    for name, lay in layouts:
        yield name + ", in place", lay.sub(0, k), lay.sub(k, m)


def masks_for(rng, S, k, m):
    """Per stripe a seeded erasure count of 0..m; with three stripes or more,
    stripe 0 has k - 1 present (skipped and counted), stripe 1 every shard
    present, stripe 2 an erasure and stray bits above the shard count."""
    n = k + m
    full = (1 << n) - 1

    def erase(e):
        return full & ~sum(1 << int(i) for i in rng.choice(n, e, replace=False))

    if S < 3:
        return [erase(int(rng.integers(1, m + 1))) for _ in range(S)]
    masks = [erase(int(rng.integers(0, m + 1))) for _ in range(S)]
    masks[0] = erase(m + 1)
    masks[1] = full
    masks[2] = erase(int(rng.integers(1, m + 1))) | (0x7FFFFFFF & ~full)
    return masks


def fresh_arenas(stripes, rng):
    arenas = [F.random_arena(sz, rng) for sz in F.arena_sizes(stripes)]
    assert sum(len(a) for a in arenas) <= 6 << 20
    return arenas


# ---- device strided batches ----------------------------------------------------
def gpu_encode(rs, devs, data, par):
    import helyim_amd as H
    return H.lib.hec_gpu_encode_batch(rs.handle, devs[data.arena].data_ptr() + data.base, data.stripe_stride,
                                      data.shard_stride, devs[par.arena].data_ptr() + par.base, par.stripe_stride,
                                      par.shard_stride, data.L, data.S, stream_ptr())


def check_gpu_encode(rs, k, m, rng, name, data, par):
    stripes = F.stripes_of(data, par)
    arenas = fresh_arenas(stripes, rng)
    plan = F.plan_encode(arenas, stripes, k, m)
    devs = to_device(arenas)
    assert gpu_encode(rs, devs, data, par) == 0, name
    F.assert_footprint(plan, to_host(devs), (name, data, par))


def check_gpu_reconstruct(rs, k, m, rng, name, lay):
    import torch
    import helyim_amd as H
    stripes = F.stripes_of(lay)
    arenas = fresh_arenas(stripes, rng)
    masks = masks_for(rng, lay.S, k, m)
    plan = F.plan_reconstruct(arenas, stripes, k, m, present_of(masks, k + m))
    devs = to_device(arenas)
    dmasks = torch.tensor(masks, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert H.lib.hec_gpu_reconstruct_batch(rs.handle, devs[0].data_ptr() + lay.base, lay.stripe_stride,
                                           lay.shard_stride, lay.L, lay.S, dmasks.data_ptr(), bad.data_ptr(),
                                           stream_ptr()) == 0, name
    F.assert_footprint(plan, to_host(devs), (name, lay, [hex(x) for x in masks]))
    assert int(bad.item()) == plan.n_bad == (1 if lay.S >= 3 else 0), name


ENCODE_KERNEL = {8192: "rs104_bs_encode_kernel", 16384: "rs104_bs_encode_kernel"}  # every other length: the table kernel


@pytest.mark.parametrize("L", [8192, 16384, 16, 4096 + 16, 1, 15, 17, 4095, 4097, 8192 + 5])
def test_device_encode_footprint(gpu, L):
    """hec_gpu_encode_batch, in place and with data and parity apart: 8 KiB
    multiples take the bit-sliced kernel, the rest the 16-byte table kernel
    (byte-wise tail where L is no multiple of 16), family D the generic one."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    name = H.lib.hec_encode_kernel_name(L).decode()
    assert name.startswith(ENCODE_KERNEL.get(L, "rs104_kernel<DEC=false>")), name
    rng = np.random.default_rng(1000 + L)
    for S in SIZES:
        layouts = [*family_a(14, L, S), *family_b(14, L, S), *family_d(14, L, S)]
        for case in [*in_place(10, 4, layouts), *family_c(10, 4, L, S), *family_cd(10, 4, L, S)]:
            check_gpu_encode(rs, 10, 4, rng, *case)


@pytest.mark.parametrize("L,kernel", [(2048, "rs104_narrow_kernel<DEC=true, 8 B per lane>"),
                                      (6144, "rs104_narrow_kernel<DEC=true, 8 B per lane>"),
                                      (4096 + 16, "rs104_kernel<DEC=true>"), (17, "rs104_kernel<DEC=true>"),
                                      (4097, "rs104_kernel<DEC=true>")])
def test_device_reconstruct_footprint(gpu, L, kernel):
    """hec_gpu_reconstruct_batch in place: erased slots hold random bytes, the
    surplus survivors too; a 9-present stripe is counted and keeps its bytes,
    an all-present stripe is a no-op, stray mask bits above bit 13 are ignored."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    name = H.lib.hec_decode_kernel_name(L).decode()
    assert name.startswith(kernel), name
    rng = np.random.default_rng(2000 + L)
    for S in SIZES:
        for case in [*family_a(14, L, S), *family_b(14, L, S), *family_d(14, L, S)]:
            check_gpu_reconstruct(rs, 10, 4, rng, *case)


@pytest.mark.parametrize("k,m", [(3, 2), (12, 4), (10, 6)])
@pytest.mark.parametrize("L", [17, 4096 + 3])
def test_device_footprint_other_geometries(gpu, k, m, L):
    """The same two calls on geometries the generic plan interpreter runs."""
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    n = k + m
    rng = np.random.default_rng(3000 + 100 * k + L)
    for S in SIZES:
        layouts = [*family_a(n, L, S, pads=(0, 48), gaps=(0, 4096 + 32)), *family_b(n, L, S)]
        for case in [*in_place(k, m, layouts), *family_c(k, m, L, S)]:
            check_gpu_encode(rs, k, m, rng, *case)
        for case in layouts:
            check_gpu_reconstruct(rs, k, m, rng, *case)


def test_device_batches_rejected_by_contract_write_nothing(gpu):
    """Overlapping shards (stride below the shard length) are refused before
    any device work: INVALID_ARGUMENT, and no byte of the arena changes."""
    import torch
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(7)
    L, S = 4096 + 16, 3
    lay = F.stripe_major(14, L, S, L + 16, 16)
    stripes = F.stripes_of(lay)
    arenas = fresh_arenas(stripes, rng)
    devs = to_device(arenas)
    data, par = lay.sub(0, 10), lay.sub(10, 4)
    assert gpu_encode(rs, devs, data._replace(shard_stride=L - 16), par) == INVALID_ARGUMENT
    assert gpu_encode(rs, devs, data, par._replace(shard_stride=L - 16)) == INVALID_ARGUMENT
    assert gpu_encode(rs, devs, data, par._replace(stripe_stride=L - 16)) == INVALID_ARGUMENT
    masks = torch.tensor([0x3FFE] * S, dtype=torch.int32, device="cuda")
    assert H.lib.hec_gpu_reconstruct_batch(rs.handle, devs[0].data_ptr() + lay.base, lay.stripe_stride, L - 16, L, S,
                                           masks.data_ptr(), None, stream_ptr()) == INVALID_ARGUMENT
    F.assert_unchanged(arenas, to_host(devs), stripes)


# ---- ragged device batches -----------------------------------------------------
@pytest.mark.parametrize("lengths,kernel", [("8k multiples", "rs104_bs_ragged_kernel"),
                                            ("mixed", "rs104_ragged_kernel<DEC=false>")])
def test_ragged_footprint(gpu, lengths, kernel):
    """hec_gpu_encode_ragged / hec_gpu_reconstruct_ragged: 6-12 stripes with
    16-byte-aligned gaps between shards and between stripes; the decode has
    0-5 erasures per stripe, and skipped and all-present stripes are compared
    like everything else."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(4000 + len(lengths))
    for n_stripes in (6, 9, 12):
        if lengths == "mixed":
            lens = [1, 17, 4096, 5000, 8192 + 16] + [int(x) for x in
                                                     rng.choice([1, 17, 4096, 5000, 8192 + 16], n_stripes - 5)]
        else:
            lens = [8192 * int(x) for x in rng.integers(1, 4, n_stripes)]
        descs, off = [], F.SLACK
        for j, L in enumerate(lens):
            stride = F.r16(L) + 16 * (j % 3)
            off += 16 * int(rng.integers(0, 4))
            descs.append([off, stride, L, 0x3FFF])
            off += 13 * stride + F.r16(L)
        stripes = [F.Stripe(L, tuple((0, o + i * st) for i in range(14))) for o, st, L, _ in descs]
        assert B.ragged_kernel_name(descs, decode=False).startswith(kernel)
        assert B.ragged_kernel_name(descs, decode=True).startswith("rs104_ragged_kernel<DEC=true>")
        # encode
        arenas = fresh_arenas(stripes, rng)
        plan = F.plan_encode(arenas, stripes, 10, 4)
        devs = to_device(arenas)
        B.encode_ragged(rs, devs[0], descs)
        F.assert_footprint(plan, to_host(devs), ("ragged encode", descs))
        # reconstruct: 0-5 erasures; stripe 0 skipped, 1 all present, 2 with stray bits
        arenas = fresh_arenas(stripes, rng)
        for j, d in enumerate(descs):
            e = {0: 5, 1: 0, 2: 4}.get(j, int(rng.integers(0, 6)))
            d[3] = 0x3FFF & ~sum(1 << int(i) for i in rng.choice(14, e, replace=False))
        descs[2][3] |= 0x7FFFC000
        plan = F.plan_reconstruct(arenas, stripes, 10, 4, present_of([d[3] for d in descs], 14))
        devs = to_device(arenas)
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        B.reconstruct_ragged(rs, devs[0], descs, bad)
        F.assert_footprint(plan, to_host(devs), ("ragged reconstruct", descs))
        assert int(bad.item()) == plan.n_bad >= 1


# ---- host batches ----------------------------------------------------------------
@pytest.fixture(scope="module")
def host_arenas(gpu):
    return HostArenas()


def host_encode(rs, live, data, par, devices=None):
    import helyim_amd as H
    args = (live[data.arena].ctypes.data + data.base, data.stripe_stride, data.shard_stride,
            live[par.arena].ctypes.data + par.base, par.stripe_stride, par.shard_stride, data.L, data.S)
    if devices is None:
        return H.lib.hec_host_encode_batch(rs.handle, *args)
    devs = (ctypes.c_int * len(devices))(*devices)
    return H.lib.hec_host_encode_batch_multi(rs.handle, devs, len(devices), *args)


def host_reconstruct(rs, live, lay, masks, devices=None):
    """-> (status, stripes counted as skipped)"""
    import helyim_amd as H
    m = np.array(masks, dtype=np.uint32)
    bad = ctypes.c_uint32(12345)
    args = (live[lay.arena].ctypes.data + lay.base, lay.stripe_stride, lay.shard_stride, lay.L, lay.S,
            m.ctypes.data, ctypes.byref(bad))
    if devices is None:
        return H.lib.hec_host_reconstruct_batch(rs.handle, *args), bad.value
    devs = (ctypes.c_int * len(devices))(*devices)
    return H.lib.hec_host_reconstruct_batch_multi(rs.handle, devs, len(devices), *args), bad.value


def check_host_encode(rs, k, m, rng, hp, host_arenas, name, data, par, devices=None):
    stripes = F.stripes_of(data, par)
    live, before = host_arenas.take(hp.path, stripes, rng)
    plan = F.plan_encode(before, stripes, k, m)
    hp.check_view(live, data)
    hp.check_view(live, par)
    assert host_encode(rs, live, data, par, devices) == 0, name
    F.assert_footprint(plan, live, (hp.path, name, data, par))


def check_host_reconstruct(rs, k, m, rng, hp, host_arenas, name, lay, devices=None, masks=None):
    stripes = F.stripes_of(lay)
    live, before = host_arenas.take(hp.path, stripes, rng)
    n_bad = (1 if lay.S >= 3 else 0) if masks is None else sum(bin(mk & ((1 << (k + m)) - 1)).count("1") < k
                                                                for mk in masks)
    masks = masks_for(rng, lay.S, k, m) if masks is None else masks
    plan = F.plan_reconstruct(before, stripes, k, m, present_of(masks, k + m))
    hp.check_view(live, lay)
    rc, bad = host_reconstruct(rs, live, lay, masks, devices)
    assert rc == 0, name
    F.assert_footprint(plan, live, (hp.path, name, lay, [hex(x) for x in masks]))
    assert bad == plan.n_bad == n_bad, name


HOST_LENGTHS = [17, 2048, 4096 + 3, 8192]
MIXED = (1000, [0, 1, 4, 5, 0, 5, 4, 1, 1, 0, 5])  # shard length, shards lost per stripe


@pytest.mark.parametrize("L", HOST_LENGTHS)
@pytest.mark.parametrize("path", HOST_PATHS)
def test_host_batch_footprint(gpu, host_arenas, path, L):
    """hec_host_encode_batch with distinct data and parity pointers and
    hec_host_reconstruct_batch on the three host paths: padded and shard-major
    host strides, parity in a buffer of its own, odd host bases and pitches
    (the pack / unpack address math and the 2D copies' pitches)."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(5000 + 10 * L + HOST_PATHS.index(path))
    # the aligned zero-copy encodes: 8 bytes per lane at 2 KiB multiples, else the 16-byte table kernel
    name = H.lib.hec_host_encode_kernel_name(L).decode()
    assert name.startswith("rs104_narrow_kernel<DEC=false, 8 B per lane>" if L % 2048 == 0
                           else "rs104_kernel<DEC=false>"), name
    name = H.lib.hec_decode_kernel_name(L).decode()
    assert name.startswith("rs104_narrow_kernel<DEC=true" if L % 2048 == 0 else "rs104_kernel<DEC=true>"), name
    with host_path(path) as hp:
        for S in SIZES:
            layouts = [*family_a(14, L, S), *family_b(14, L, S), *family_d(14, L, S)]
            for case in [*in_place(10, 4, layouts), *family_c(10, 4, L, S), *family_cd(10, 4, L, S)]:
                check_host_encode(rs, 10, 4, rng, hp, host_arenas, *case)
            for case in layouts:
                check_host_reconstruct(rs, 10, 4, rng, hp, host_arenas, *case)


@pytest.mark.parametrize("path", HOST_PATHS)
def test_host_reconstruct_footprint_mixed_erasure_counts(gpu, host_arenas, path):
    """hec_host_reconstruct_batch with 0, 1, 4 and 5 shards lost in stripes
    next to each other (masks_for's counts vary from stripe to stripe too, but
    by seed, and its shapes are one stripe or all stripes per chunk in either
    build). Eleven stripes of 1000 bytes: chunks of 3, 3, 3 and 2 stripes in
    the small-chunk build, with 4 | 5, 5 | 4 and 1 | 0 lost at the chunk edges;
    a mask or a rebuilt shard taken from the neighbouring stripe or from the
    slot's first changes a byte the image keeps, or the count."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    L, lost = MIXED
    S = len(lost)
    rng = np.random.default_rng(5500 + HOST_PATHS.index(path))
    with host_path(path) as hp:
        for name, lay in [*family_a(14, L, S, pads=(16,), gaps=(48,)), *family_b(14, L, S, pads=((16, 48),)),
                          *family_d(14, L, S)]:
            masks = [0x3FFF & ~sum(1 << int(i) for i in rng.choice(14, e, replace=False)) for e in lost]
            masks[4] |= 0x7FFFC000  # stray bits above the shard count
            check_host_reconstruct(rs, 10, 4, rng, hp, host_arenas, name, lay, masks=masks)


@pytest.mark.parametrize("L", [2048, 4096 + 3])
@pytest.mark.parametrize("path", HOST_PATHS)
def test_host_batch_multi_footprint_shard_major(gpu, host_arenas, path, L):
    """The _multi calls over devices [0, 0] on a shard-major batch of seven
    stripes: the range boundary (stripe 3) falls inside the interleaved
    layout, every range's base is the batch base plus s0 stripe strides."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(6000 + L)
    with host_path(path) as hp:
        for name, lay in family_b(14, L, 7, pads=((16, 48),)):
            check_host_encode(rs, 10, 4, rng, hp, host_arenas, name, lay.sub(0, 10), lay.sub(10, 4), devices=[0, 0])
            check_host_reconstruct(rs, 10, 4, rng, hp, host_arenas, name, lay, devices=[0, 0])
        for name, data, par in family_c(10, 4, L, 7):
            check_host_encode(rs, 10, 4, rng, hp, host_arenas, name, data, par, devices=[0, 0])


@pytest.mark.parametrize("path", HOST_PATHS)
def test_host_batches_rejected_by_contract_write_nothing(gpu, host_arenas, path):
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(8)
    L, S = 4096 + 3, 3
    lay = F.shard_major(14, L, S, F.r16(L) + 16, 48)
    stripes = F.stripes_of(lay)
    with host_path(path):
        live, before = host_arenas.take(path, stripes, rng)
        data, par = lay.sub(0, 10), lay.sub(10, 4)
        assert host_encode(rs, live, data._replace(stripe_stride=L - 1), par) == INVALID_ARGUMENT
        assert host_encode(rs, live, data, par._replace(shard_stride=L - 1)) == INVALID_ARGUMENT
        assert host_encode(rs, live, data, par._replace(shard_stride=L - 1), devices=[0, 0]) == INVALID_ARGUMENT
        assert host_reconstruct(rs, live, lay._replace(stripe_stride=L - 1), [0x3FFE] * S)[0] == INVALID_ARGUMENT
        assert host_reconstruct(rs, live, lay._replace(shard_stride=L - 1), [0x3FFE] * S,
                                devices=[0, 0])[0] == INVALID_ARGUMENT
        F.assert_unchanged(before, live, stripes)


# ---- per-call C ABI ----------------------------------------------------------------
def scattered_stripe(L, n, start):
    """n shards of L bytes in one arena at odd offsets with uneven gaps;
    -> (stripe, first free offset after it)."""
    locs, o = [], start | 1
    for i in range(n):
        locs.append((0, o))
        o += L + 3 + 2 * (i % 3)
        o |= 1
    return F.Stripe(L, tuple(locs)), o


def call_args(arena, stripes, present=None, lens=None):
    """shards / lens / present arrays of the C ABI, stripe-major."""
    flat = [(st, a, o) for st in stripes for a, o in st.locs]
    ptrs = (ctypes.c_void_p * len(flat))(*[arena.ctypes.data + o for _, _, o in flat])
    ln = (ctypes.c_size_t * len(flat))(*(lens if lens is not None else [st.L for st, _, _ in flat]))
    if present is None:
        return ptrs, ln
    pr = (ctypes.c_uint8 * len(flat))(*[1 if p else 0 for row in present for p in row])
    return ptrs, ln, pr


def erased_flags(rng, n, e):
    gone = set(int(i) for i in rng.choice(n, e, replace=False))
    return [i not in gone for i in range(n)]


@pytest.mark.parametrize("zero_copy", [1, 0])
@pytest.mark.parametrize("staging", [0, 1 << 40])
@pytest.mark.parametrize("k,m", [(10, 4), (3, 2)])
def test_per_call_abi_footprint(gpu, k, m, staging, zero_copy):
    """hec_rs_encode / _reconstruct / _reconstruct_data / _reconstruct_batch
    through the library itself, every shard pointer aimed into one host arena
    at an odd offset: an overrun that separately allocated shards would take
    into the heap lands in a gap here. Staging off (one copy per shard) and on
    (packed pinned staging), zero copy on and off."""
    import helyim_amd as H
    lib = H.lib
    rs = H.ReedSolomon(k, m)
    n = k + m
    rng = np.random.default_rng(7000 + 10 * k + zero_copy + (1 if staging else 0) * 2)
    lib.hec_set_host_staging(staging)
    lib.hec_set_host_zero_copy(zero_copy)
    try:
        for L in (17, 4096 + 3):
            st, _ = scattered_stripe(L, n, F.SLACK)
            # encode
            arena, = fresh_arenas([st], rng)
            plan = F.plan_encode([arena], [st], k, m)
            assert lib.hec_rs_encode(rs.handle, *call_args(arena, [st]), n) == 0
            F.assert_footprint(plan, [arena], ("hec_rs_encode", L))
            # reconstruct and reconstruct_data: 1..m erasures, then parity-only and data-only losses
            for data_only, fn in ((False, lib.hec_rs_reconstruct), (True, lib.hec_rs_reconstruct_data)):
                rows = [erased_flags(rng, n, e) for e in range(1, m + 1)]
                rows.append([i < k or i == n - 1 for i in range(n)])       # parity lost, one survivor
                rows.append([i != 0 for i in range(n)])                      # surplus survivors: all of the parity
                for pr in rows:
                    arena, = fresh_arenas([st], rng)
                    plan = F.plan_reconstruct([arena], [st], k, m, [pr], data_only=data_only)
                    assert fn(rs.handle, *call_args(arena, [st], [pr]), n) == 0
                    F.assert_footprint(plan, [arena], (fn.__name__, L, pr))
                # too few present: the error, and nothing written
                pr = erased_flags(rng, n, m + 1)
                arena, = fresh_arenas([st], rng)
                before = arena.copy()
                assert fn(rs.handle, *call_args(arena, [st], [pr]), n) == TOO_FEW_SHARDS_PRESENT
                F.assert_unchanged([before], [arena], [st], (fn.__name__, "too few present"))
        # reconstruct_batch: three stripes of different lengths in one arena
        stripes, o = [], F.SLACK
        for L in (17, 4096 + 3, 1000):
            st, o = scattered_stripe(L, n, o + 16)
            stripes.append(st)
        for data_only in (0, 1):
            present = [erased_flags(rng, n, m), erased_flags(rng, n, 1), [i != n - 1 for i in range(n)]]
            arena, = fresh_arenas(stripes, rng)
            plan = F.plan_reconstruct([arena], stripes, k, m, present, data_only=bool(data_only))
            bad = ctypes.c_size_t(99)
            assert lib.hec_rs_reconstruct_batch(rs.handle, *call_args(arena, stripes, present), 3, data_only,
                                                ctypes.byref(bad)) == 0
            assert bad.value == 3  # no failing stripe
            F.assert_footprint(plan, [arena], ("hec_rs_reconstruct_batch", data_only, present))
            # the middle stripe has a survivor of the wrong size: its error and index, and nothing
            # written -- not even stripe 0's erased shards, which were valid
            arena, = fresh_arenas(stripes, rng)
            before = arena.copy()
            lens = [s.L for s in stripes for _ in range(n)]
            lens[n + present[1].index(True, 1)] += 1
            bad = ctypes.c_size_t(99)
            assert lib.hec_rs_reconstruct_batch(rs.handle, *call_args(arena, stripes, present, lens), 3, data_only,
                                                ctypes.byref(bad)) == INCORRECT_SHARD_SIZE
            assert bad.value == 1
            F.assert_unchanged([before], [arena], stripes, ("hec_rs_reconstruct_batch", "wrong-size shard"))
    finally:
        lib.hec_set_host_staging(16 << 20)
        lib.hec_set_host_zero_copy(1)
