"""Update on the GPU (include/hec.h hec_gpu_update_batch, hec_rs_update) against
tests/update_model.py: the parity before the call XOR gfref's encode of the
masked delta, never the library's own encode. The strided cases run on whole
arenas of seeded random bytes -- gaps, pads, slack, and a parity that is no
codeword's -- and compare every byte with an expected image (tests/footprint.py):
the old and new arenas unchanged, the parity arena different only in [0, L) of
the parity shards of the stripes whose mask names a shard."""
import ctypes

import numpy as np
import pytest

import footprint as F
import update_model as M
from oracle import corc

pytestmark = pytest.mark.gpu

K, MP = 10, 4
HIGH = 0xFFFFFC00  # mask bits that mean nothing
# every mask: stripe s with mask s, two 4 KiB column ranges a stripe, the second partial
EVERY_S, EVERY_L = 1 << K, 4096 + 48
LENGTHS = (1, 15, 16, 17, 2047, 2048, 4095, 4096, 4097, 8192 + 16, 12288 + 5)
ALIGNED_KERNEL = "rs104_update_kernel"


def gather(arenas, lay):
    """[S, shards, L] copy of a layout's shards."""
    return np.stack([np.stack([arenas[lay.arena][lay.off(s, i):lay.off(s, i) + lay.L] for i in range(lay.shards)])
                     for s in range(lay.S)])


def plan_update(arenas, old_lay, new_lay, par_lay, masks):
    """Expected image of an update: the arenas as they are, with exactly the
    parity shards of the stripes with a non-empty U set to the model's bytes."""
    lays = [la for la in (old_lay, new_lay, par_lay) if la is not None]
    plan = F.Plan(arenas, F.stripes_of(*lays))
    want = M.updated_parity(gather(arenas, par_lay), None if old_lay is None else gather(arenas, old_lay),
                            gather(arenas, new_lay), masks)
    first = sum(la.shards for la in lays) - MP
    for s in range(par_lay.S):
        if int(masks[s]) & 0x3FF:
            for j in range(MP):
                plan.shard(plan.expected, s, first + j)[:] = want[s, j]
                plan.roles[s][first + j] = F.OUTPUT
    return plan


def device_words(masks):
    import torch
    return torch.from_numpy(np.asarray(masks, dtype=np.uint32).view(np.int32).copy()).cuda()


def launch(rs, devs, old_lay, new_lay, par_lay, words):
    import helyim_amd as H

    def where(lay):
        return devs[lay.arena].data_ptr() + lay.base, lay.stripe_stride, lay.shard_stride

    old = (None, 0, 0) if old_lay is None else where(old_lay)
    rc = H.lib.hec_gpu_update_batch(rs.handle, *old, *where(new_lay), *where(par_lay), par_lay.L, par_lay.S,
                                    words.data_ptr(), F.stream_ptr())
    assert rc == 0, H._lib.last_detail()


def aligned(*lays):
    return all((la.base | la.stripe_stride | la.shard_stride) % 16 == 0 for la in lays if la is not None)


def check(lays, masks, seed, note):
    """One call on fresh random arenas, every byte of every arena against the plan."""
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    old_lay, new_lay, par_lay = lays
    rng = np.random.default_rng(seed)
    stripes = F.stripes_of(*[la for la in lays if la is not None])
    arenas = [F.random_arena(sz, rng) for sz in F.arena_sizes(stripes)]
    plan = plan_update(arenas, old_lay, new_lay, par_lay, masks)
    devs = F.to_device(arenas)
    launch(rs, devs, old_lay, new_lay, par_lay, device_words(masks))
    F.assert_footprint(plan, F.to_host(devs), note)
    return plan, arenas


def in_place(L, S, pitch, gap=0, new_gap=0):
    """Old data and parity in one [S][14][pitch] arena, the new data apart."""
    lay = F.stripe_major(14, L, S, pitch, gap)
    return lay.sub(0, K), F.stripe_major(K, L, S, F.r16(L), new_gap, arena=1), lay.sub(K, MP)


@pytest.mark.parametrize("has_old", [True, False], ids=["old", "no old"])
def test_every_mask(gpu, has_old):
    """1024 stripes, stripe s with mask s: every subset of the ten data shards,
    the empty one included, on both column ranges of a stripe."""
    old_lay, new_lay, par_lay = in_place(EVERY_L, EVERY_S, EVERY_L)
    masks = np.arange(EVERY_S, dtype=np.uint32)
    plan, arenas = check((old_lay if has_old else None, new_lay, par_lay), masks, 0x0A110 + has_old, "every mask")
    # the expected image moves every stripe's parity but stripe 0's
    before, after = gather(arenas, par_lay), gather(plan.expected, par_lay)
    assert np.array_equal(before[0], after[0]) and (before[1:] != after[1:]).any(axis=(1, 2)).all()


@pytest.mark.parametrize("has_old", [True, False], ids=["old", "no old"])
@pytest.mark.parametrize("L", LENGTHS)
def test_lengths_across_lane_tail_and_range_edges(gpu, L, has_old):
    import helyim_amd as H
    old_lay, new_lay, par_lay = in_place(L, 3, F.r16(L) + 16)
    assert aligned(old_lay, new_lay, par_lay)
    assert H.lib.hec_update_kernel_name(L).decode().startswith(ALIGNED_KERNEL)
    check((old_lay if has_old else None, new_lay, par_lay), [0x001, 0x200, 0x3FF], 0x1E00 + L, L)


def layouts(L, S):
    p = F.r16(L)
    return {
        "stripe-major in place": in_place(L, S, p + 16),
        "separate arenas, different strides": (F.stripe_major(K, L, S, p + 32), F.stripe_major(K, L, S, p, 48, arena=1),
                                               F.stripe_major(MP, L, S, p + 16, arena=2)),
        "shard-major parity": (F.stripe_major(K, L, S, p), F.stripe_major(K, L, S, p + 16, arena=1),
                               F.shard_major(MP, L, S, p + 16, 32, arena=2)),
        "gap between stripes": in_place(L, S, p, gap=4096 + 112, new_gap=208),
        "odd bases and strides": (F.stripe_major(K, L, S, L + 3, base=F.SLACK + 1),
                                  F.stripe_major(K, L, S, L + 7, 5, base=F.SLACK + 3, arena=1),
                                  F.stripe_major(MP, L, S, L + 1, base=F.SLACK + 5, arena=2)),
        "odd parity base alone": (F.stripe_major(K, L, S, p), F.stripe_major(K, L, S, p, arena=1),
                                  F.stripe_major(MP, L, S, p, base=F.SLACK + 8, arena=2)),
    }


LAYOUT_NAMES = tuple(layouts(16, 1))


@pytest.mark.parametrize("has_old", [True, False], ids=["old", "no old"])
@pytest.mark.parametrize("L", [4096 + 48, 4099, 1000])
@pytest.mark.parametrize("name", LAYOUT_NAMES)
def test_layouts_and_footprint(gpu, name, L, has_old):
    S = 5
    old_lay, new_lay, par_lay = layouts(L, S)[name]
    assert aligned(old_lay, new_lay, par_lay) == (not name.startswith("odd"))
    assert par_lay.stripe_stride < par_lay.shard_stride or name != "shard-major parity"
    check((old_lay if has_old else None, new_lay, par_lay), [0x3FF, 0x000, 0x001, 0x2A5, 0x200],
          0x1A70 + L + 7 * LAYOUT_NAMES.index(name), (name, L, has_old))


GENERIC_S = 64  # two column ranges a stripe: 128 items for the grid-stride kernel


@pytest.mark.parametrize("has_old", [True, False], ids=["old", "no old"])
def test_generic_kernel_over_many_stripes(gpu, has_old):
    """Odd bases and strides over enough stripes that a small grid loops."""
    old_lay, new_lay, par_lay = layouts(EVERY_L, GENERIC_S)["odd bases and strides"]
    masks = np.random.default_rng(0x6E0).integers(0, 1 << K, GENERIC_S).astype(np.uint32)
    masks[[0, 17, GENERIC_S - 1]] = 0
    check((old_lay if has_old else None, new_lay, par_lay), masks, 0x6E1 + has_old, "generic, many stripes")


def test_mask_bits_from_ten_up_are_ignored(gpu):
    lays = in_place(4096 + 48, 5, 4096 + 64)
    masks = [HIGH | 0x005, HIGH, HIGH | 0x3FF, 0x005, HIGH | 0x200]
    plan, arenas = check(lays, masks, 0xB175, "high bits")
    # stripes 0 and 3 differ in the high bits alone; stripe 1 is a no-op
    assert np.array_equal(gather(plan.expected, lays[2])[1], gather(arenas, lays[2])[1])
    plain = plan_update(arenas, *lays, [m & 0x3FF for m in masks])
    assert all(np.array_equal(a, b) for a, b in zip(plain.expected, plan.expected))


def random_batch(S, L, seed):
    import torch
    g = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randint(0, 256, (S, K + MP, L), dtype=torch.uint8, device="cuda", generator=g)


def test_progressive_encode_from_zero_parity(gpu):
    """Three calls without an old arena over a partition of the data shards give the encode's bytes."""
    import torch

    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(K, MP)
    S, L = 6, 4096 + 48
    t = random_batch(S, L, 0x9E06)
    t[:, K:] = 0
    for word in (0x007, 0x0F8, 0x300):
        B.update_batch_sep(rs, None, t[:, :K], t[:, K:], torch.full((S,), word, dtype=torch.int32, device="cuda"))
    ref = t.clone()
    B.encode_batch(rs, ref)
    torch.cuda.synchronize()
    assert torch.equal(t, ref)
    assert np.array_equal(t[:, K:].cpu().numpy(), corc.encode_stripes(np.ascontiguousarray(t[:, :K].cpu().numpy())))
    assert not B.verify_batch(rs, t).cpu().numpy().any()


def test_round_trip_with_the_scrub(gpu):
    """Encode, update shard 2 or shards 0 and 9 of two stripes in three, commit
    new over old: the scrub finds every stripe clean, and the untouched
    stripes' parity never moved."""
    import torch

    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(K, MP)
    S, L = 9, 4096 + 48
    t = random_batch(S, L, 0x5C4B)
    B.encode_batch(rs, t)
    before = t.clone()
    new = random_batch(S, L, 0x5C4C)[:, :K].contiguous()
    words = [(0x004, 0x201, 0x000)[s % 3] for s in range(S)]
    B.update_batch(rs, t, new, device_words(words))
    torch.cuda.synchronize()
    assert torch.equal(t[:, :K], before[:, :K])  # the call does not commit
    assert B.verify_batch(rs, t).cpu().numpy()[[s for s in range(S) if words[s]]].all()
    sel = torch.from_numpy(M.changed(words, K)).cuda()
    t[:, :K] = torch.where(sel[:, :, None], new, t[:, :K])
    assert not B.verify_batch(rs, t).cpu().numpy().any()
    idle = [s for s in range(S) if not words[s]]
    assert torch.equal(t[idle], before[idle])
    host = t.cpu().numpy()
    assert np.array_equal(host[:, K:], corc.encode_stripes(np.ascontiguousarray(host[:, :K])))


def test_two_updates_back_to_back_on_one_stream(gpu):
    """Both read and write the same parity: queued on one non-default stream and
    synchronised once, they equal the model applied twice."""
    import torch

    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(K, MP)
    S, L = 256, 4096 + 48
    a, b, c = (random_batch(S, L, 0x57E0 + i) for i in range(3))
    old, new1, new2, parity = a[:, :K], b[:, :K], c[:, :K], a[:, K:]
    rng = np.random.default_rng(0x57E3)
    m1, m2 = (rng.integers(0, 1 << K, S).astype(np.uint32) for _ in range(2))
    w1, w2 = device_words(m1), device_words(m2)
    h_old, h_new1, h_new2, h_par = (x.cpu().numpy() for x in (old, new1, new2, parity))
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    B.update_batch_sep(rs, old, new1, parity, w1, stream=stream)
    B.update_batch_sep(rs, new1, new2, parity, w2, stream=stream)
    stream.synchronize()
    want = M.updated_parity(M.updated_parity(h_par, h_old, h_new1, m1), h_new1, h_new2, m2)
    assert np.array_equal(parity.cpu().numpy(), want)
    assert np.array_equal(old.cpu().numpy(), h_old) and np.array_equal(new1.cpu().numpy(), h_new1)


def per_call(rs, k, m, L, changed, rng):
    old, new = (rng.integers(0, 256, (k, L), dtype=np.uint8) for _ in range(2))
    parity = rng.integers(0, 256, (m, L), dtype=np.uint8)
    live_old, live_new, live_par = old.copy(), new.copy(), parity.copy()
    # the old slots of unchanged shards are not needed
    shards = [live_old[i] if i in changed else None for i in range(k)] + [live_par[j] for j in range(m)]
    rs.update(shards, [live_new[c] if c in changed else None for c in range(k)])
    want = M.updated_parity(parity[None], old[None], new[None], [sum(1 << c for c in changed)], k, m)[0]
    assert np.array_equal(live_par, want), (k, m, L, changed)
    assert np.array_equal(live_old, old) and np.array_equal(live_new, new)


@pytest.mark.parametrize("L", [1, 1000, 65536 + 7])
@pytest.mark.parametrize("k,m", [(10, 4), (5, 5), (3, 2)])
def test_per_call(gpu, k, m, L):
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    rng = np.random.default_rng(0xCA11 + 100 * k + L)
    for changed in ([k // 2], list(range(k)), []):
        per_call(rs, k, m, L, changed, rng)


@pytest.mark.parametrize("k,m", [(10, 4), (5, 5)])
def test_per_call_through_device_staging(gpu, k, m):
    """The same with zero copy off: H2D, the kernel over device staging, D2H."""
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    rng = np.random.default_rng(0xCA12 + k)
    assert H.lib.hec_set_host_zero_copy(0) == 0
    try:
        for changed in ([0], [1, k - 1], list(range(k))):
            per_call(rs, k, m, 1000, changed, rng)
    finally:
        assert H.lib.hec_set_host_zero_copy(1) == 0


def test_wide_codec_per_call(gpu):
    """More than four parity rows: the generic path's second row group re-reads
    the rows the first one stored, with coefficient zero."""
    import helyim_amd as H
    rs = H.ReedSolomon(6, 7)
    rng = np.random.default_rng(0xCA13)
    for changed in ([3], [0, 5], list(range(6))):
        per_call(rs, 6, 7, 4096 + 17, changed, rng)


def test_empty_batch_and_an_all_empty_mask_batch_write_nothing(gpu):
    import helyim_amd as H
    rs = H.ReedSolomon(K, MP)
    lays = in_place(4096 + 48, 3, 4096 + 64)
    check(lays, [0, HIGH, 0], 0xE3B7, "no stripe changes")
    rng = np.random.default_rng(0xE3B8)
    arenas = [F.random_arena(sz, rng) for sz in F.arena_sizes(F.stripes_of(*lays))]
    devs = F.to_device(arenas)
    old_lay, new_lay, par_lay = lays
    rc = H.lib.hec_gpu_update_batch(rs.handle, devs[0].data_ptr() + old_lay.base, old_lay.stripe_stride,
                                    old_lay.shard_stride, devs[1].data_ptr() + new_lay.base, new_lay.stripe_stride,
                                    new_lay.shard_stride, devs[0].data_ptr() + par_lay.base, par_lay.stripe_stride,
                                    par_lay.shard_stride, par_lay.L, 0, device_words([0x3FF]).data_ptr(),
                                    ctypes.c_void_p(F.stream_ptr()))
    assert rc == 0
    F.assert_unchanged(arenas, F.to_host(devs), F.stripes_of(*lays))
