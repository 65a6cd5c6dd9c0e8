"""The degraded scrub on the GPU: hec_gpu_verify_present_batch,
hec_gpu_locate_corrupt_present_batch, hec_gpu_reconstruct_checked_batch and
hec_locate_corrupt_ec_files_present.

Every expected word comes from tests/check_model.py (the contracts by brute
force) applied to the batch as it is; where the test built the corruption
itself the word is asserted by construction too. Stripes live in one
tests/footprint.py layout inside an arena filled with a sentinel byte: absent
shards, shard gaps and stripe gaps hold it, so a kernel that reads an absent
shard or a byte at or past shard_len computes a wrong word here. Every device
call is also a footprint check: the arena comes back byte for byte (or, for the
checked reconstruct, equals the expected image), word S keeps its sentinel."""
import itertools
import os

import numpy as np
import pytest

import check_model as C
import locate_model as M
import scrub_harness as SH
from oracle import corc
from scrub_harness import (ALL, BLOCK, Batch, FILL, LAUNCH_LIMIT, MASK_ROUND, R1, R2, R3, UNEXPLAINED, assert_words,
                           checksum, clean_stripes, expect_words, flip, hexes, i32, lost,
                           masked_block_words as block_words, read_words, result_words, with_stray_bits, write_volume)

pytestmark = pytest.mark.gpu

LENGTHS = (2048, 8192 + 2048, 1000, 4096 + 16)  # one fast chunk, five, generic with an 8-byte tail, generic


def device_locate(rs, b, locate=True, preset=(7, 5)):
    """The masked locate (or verify alone) on batch b -> (check, suspects,
    bad_stripes, unchecked), the counters without their presets. Asserts the
    footprint."""
    call = "hec_gpu_locate_corrupt_present_batch" if locate else "hec_gpu_verify_present_batch"
    ws, (bad, unchecked) = SH.device_masked(call, rs, b, 2 if locate else 1, preset)
    return ws[0], ws[1] if locate else None, bad - preset[0], unchecked - preset[1]


def check_batch(rs, b, by_construction=None, note=None):
    """Verify alone and locate on b against the model -> (check, suspects)."""
    got = b.gather()
    want_chk, want_sus = C.check_words(got, b.masks), C.suspect_words(got, b.masks)
    if by_construction is not None:
        assert want_sus == by_construction, (note, hexes(want_sus), hexes(by_construction))
    assert [w != 0 for w in want_chk] == [w != 0 for w in want_sus], note
    chk, sus, bad, unchecked = device_locate(rs, b)
    assert chk == want_chk, (note, hexes(chk), hexes(want_chk))
    assert sus == want_sus, (note, hexes(sus), hexes(want_sus))
    assert bad == sum(1 for w in want_chk if w) and unchecked == C.unchecked_count(b.masks), note
    chk1, _, bad1, unchecked1 = device_locate(rs, b, locate=False)
    assert (chk1, bad1, unchecked1) == (chk, bad, unchecked), note
    return chk, sus


# ---- every mask ------------------------------------------------------------------
def test_every_mask(gpu):
    """All 470 masks with a spare shard, and a few without, in one batch of one
    fast chunk per stripe. Clean: every word 0 over stale words, the unchecked
    count exact. Then one flipped byte per stripe, in a shard of B for the even
    stripes and of E for the odd ones."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    L = 2048
    assert "rs104_check_kernel" in H.check_kernel_name(L)
    masks = C.checkable_masks() + [0x3FF, 0x3FF << 4, lost(0, 5, 9, 13), 0x1FF, 0x2AAA, 0]
    S = len(masks)
    assert S == 476 and C.unchecked_count(masks) == 6
    clean = clean_stripes(S, L)
    b = Batch(clean, masks)
    chk, sus = check_batch(rs, b, [0] * S, "clean")
    assert chk == [0] * S
    want_sus, want_chk = [], []
    for s, m in enumerate(masks):
        B, E = C.split(m)
        if len(B) < 10 or not E:
            if B:
                b.shard(s, B[0])[s % L] ^= 0x40
            want_sus.append(0)
            want_chk.append(0)
            continue
        group = B if s % 2 == 0 else E
        shard = group[(s // 2) % len(group)]
        b.shard(s, shard)[(37 * s) % L] ^= 1 + s % 255
        want_sus.append(1 << shard if len(E) >= 2 else UNEXPLAINED)
        want_chk.append(sum(1 << e for e in E) if shard in B else 1 << shard)  # no entry of A_m is zero
    chk, sus = check_batch(rs, b, want_sus, "one flip per stripe")
    assert chk == want_chk, (hexes(chk), hexes(want_chk))


@pytest.mark.parametrize("mask", [R2, R3, ALL], ids=["r2", "r3", "r4"])
def test_every_error_value(gpu, mask):
    """Stripe v - 1 gets ^= v in a shard of B, stripe 254 + v in a shard of E."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 510, 2048
    B, E = C.split(mask)
    b = Batch(clean_stripes(S, L), [mask] * S)
    for v in range(1, 256):
        b.shard(v - 1, B[4])[(9 * v) % L] ^= v
        b.shard(254 + v, E[-1])[L - v] ^= v
    check_batch(rs, b, [1 << B[4]] * 255 + [1 << E[-1]] * 255, hex(mask))


@pytest.mark.parametrize("L", [8192 + 2048, 1000])
def test_two_shards_in_different_columns(gpu, L):
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    masks = [R3, R2, R3, R2, R3]
    b = Batch(clean_stripes(5, L), masks)
    b.shard(1, 1)[L - 1] ^= 0x80        # R2: B shard 1 and E shard 13
    b.shard(1, 13)[3] ^= 0x01
    b.shard(2, 9)[L // 2] ^= 0xFF       # R3: B shards 9 and 2 in neighbouring bytes of one dword
    b.shard(2, 2)[L // 2 + 1] ^= 0x07
    b.shard(4, 12)[0] ^= 0x10           # R3: E shards 12 and 13, different chunks where L allows
    b.shard(4, 13)[L - 1] ^= 0x10
    check_batch(rs, b, [0, 1 << 1 | 1 << 13, 1 << 9 | 1 << 2, 0, 1 << 12 | 1 << 13], L)


def test_same_column_pairs_with_three_spares_are_unexplained(gpu):
    """All 78 pairs of the 13 present shards wrong in one byte column: exactly
    bit 31. Then a single wrong shard in another column: bit 31 plus its bit."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    B, E = C.split(R3)
    pairs = list(itertools.combinations(B + E, 2))
    S, L = len(pairs), 1000
    assert S == 78
    rng = np.random.default_rng(78)
    b = Batch(clean_stripes(S, L), [R3] * S)
    for s, pair in enumerate(pairs):
        for c in pair:
            b.shard(s, c)[11 * s] ^= int(rng.integers(1, 256))
    check_batch(rs, b, [UNEXPLAINED] * S, "pairs")
    want = []
    for s in range(S):
        single = (B + E)[(5 * s + 3) % 13]
        b.shard(s, single)[11 * s + 1] ^= int(rng.integers(1, 256))
        want.append(UNEXPLAINED | 1 << single)
    check_batch(rs, b, want, "pairs and a single")


def test_one_spare_only_detects(gpu):
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    masks = [R1, lost(0, 1, 2), lost(11, 12, 13), lost(4, 10, 13), R1, lost(9, 10, 11)]
    S = len(masks)
    for L in (2048, 1000):
        b = Batch(clean_stripes(S, L), masks)
        want = []
        for s, m in enumerate(masks):
            B, E = C.split(m)
            assert len(E) == 1
            if s == 4:
                want.append(0)
                continue
            b.shard(s, (B + E)[(3 * s) % 11] if s % 2 else E[0])[L - 1 - s] ^= 0x01 << s
            want.append(UNEXPLAINED)
        chk, _ = check_batch(rs, b, want, L)
        assert chk == [1 << C.split(m)[1][0] if s != 4 else 0 for s, m in enumerate(masks)]


def test_shard_end(gpu):
    """The last byte of a shard at L = 1000 (the 8-byte tail of the last
    vector) is seen; garbage in the pads past shard_len changes nothing."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    L, masks = 1000, [R3, R2, R1, ALL, R3]
    clean = clean_stripes(5, L)
    results = []
    for fill in (FILL, None):  # None: random bytes in every gap and pad
        b = Batch(clean, masks, fill=fill)
        assert check_batch(rs, b, [0] * 5, "clean")[0] == [0] * 5
        b.shard(0, 13)[L - 1] ^= 0x80
        b.shard(1, 0 + 1)[L - 1] ^= 0x01
        b.shard(2, 5)[L - 1] ^= 0x55
        b.shard(3, 9)[L - 1] ^= 0xFF
        results.append(check_batch(rs, b, [1 << 13, 1 << 1, UNEXPLAINED, 1 << 9, 0], fill))
    assert results[0] == results[1]


LAYOUT_MASKS = [R3, R2, R1, ALL, lost(13), lost(0, 1), 0x3FF, R3]


def layouts_batch(L, kind, masks=LAYOUT_MASKS):
    """Every r, flips at the ends of chunks in all stripes but the last; bits
    of `masks` above bit 13 take no part in where the shards are."""
    b = Batch(clean_stripes(len(masks), L), masks, kind)
    positions = sorted({p for p in (0, 2047, 2048, 4095, 4096, L - 1) if p < L})
    for s, m in enumerate(masks[:-1]):
        B, E = C.split(m)
        shard = (B + E)[(4 * s + 1) % len(B + E)]
        for n, p in enumerate(positions):
            b.shard(s, shard)[p] ^= 0x11 * (n + 1)
    return b


@pytest.mark.parametrize("L", LENGTHS)
def test_layouts_give_the_same_words(gpu, L):
    """Odd base and odd strides, and the shard-major layout, against the
    aligned run, over a batch with every r and flips at the ends of chunks."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    runs = []
    for kind in ("aligned", "odd", "shard-major"):
        runs.append(check_batch(rs, layouts_batch(L, kind), note=(kind, L)))
        assert runs[-1][0][-1] == 0 and runs[-1][0][6] == 0 and all(runs[-1][0][:6])
    assert runs[0] == runs[1] == runs[2]


@pytest.mark.parametrize("L", LENGTHS)
def test_stray_mask_bits_change_nothing(gpu, L):
    """The batches of test_layouts_give_the_same_words (the fast and the
    grid-stride kernels, aligned and odd) with bits 14..31 set in every mask:
    the model's words for the masks & 0x3FFF, and words, counts and footprint
    equal to the run with clean masks. A kernel that indexes its plan table
    or counts present shards with the raw word gives other words or faults."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    stray = with_stray_bits(LAYOUT_MASKS, L)
    for kind in ("aligned", "odd"):
        # check_batch: both calls' words and counts against the model, the footprint
        runs = [check_batch(rs, layouts_batch(L, kind, masks), note=(kind, L, masks is stray))
                for masks in (LAYOUT_MASKS, stray)]
        assert runs[0] == runs[1] and any(runs[0][0]), (kind, L)


@pytest.mark.parametrize("L", [8192 + 2048, 4096 + 16])
def test_full_masks_reproduce_locate(gpu, L):
    import torch
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 6
    b = Batch(clean_stripes(S, L), [ALL] * S)
    b.shard(0, 3)[L - 1] ^= 0x21
    b.shard(1, 12)[0] ^= 0x01
    b.shard(2, 6)[77] ^= 0x80
    b.shard(2, 9)[77] ^= 0x80
    b.shard(4, 0)[4095] ^= 0xFF
    b.shard(4, 13)[4096] ^= 0x02
    chk, sus = check_batch(rs, b, [1 << 3, 1 << 12, UNEXPLAINED, 0, 1 | 1 << 13, 0], L)
    la = b.layout
    dev = torch.from_numpy(b.arena).cuda()
    mis_t, sus_t = result_words(2, S)
    base = dev.data_ptr() + la.base
    rc = H.lib.hec_gpu_locate_corrupt_batch(rs.handle, base, la.stripe_stride, la.shard_stride,
                                            base + 10 * la.shard_stride, la.stripe_stride, la.shard_stride, L, S,
                                            mis_t.data_ptr(), sus_t.data_ptr(), None,
                                            torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert chk == [w << 10 for w in read_words(mis_t, S)] and sus == read_words(sus_t, S)
    assert sus == M.suspect_words(b.gather())


def test_more_items_than_the_locate_grid(gpu):
    """2048 + 5 one-chunk stripes: more items than pass 2's 2048 workgroups, so
    some workgroups take a second item, with the masks array in step."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 2048 + 5, 16
    cycle = [R3, R2, ALL, lost(13), lost(5, 6), 0x3FF, R1]
    masks = [cycle[s % len(cycle)] for s in range(S)]
    b = Batch(clean_stripes(S, L), masks)
    want = [0] * S
    for s, pos in ((0, 0), (1, 3), (2047, 15), (2048, 7), (2051, 1), (S - 1, 15)):
        B, E = C.split(masks[s])
        shard = (B + E)[s % len(B + E)]
        assert len(E) >= 2
        b.shard(s, shard)[pos] ^= 0x5A
        want[s] = 1 << shard
    assert len(C.split(masks[1000])[1]) == 1       # R1
    b.shard(1000, 0)[4] ^= 0x01
    want[1000] = UNEXPLAINED
    assert masks[1006] == 0x3FF                     # nothing to check: not even read
    b.shard(1006, 4)[4] ^= 0x01
    check_batch(rs, b, want, "grid")


def test_encode_corrupt_locate_in_stream_order(gpu):
    """encode_batch, a corrupting write and the masked locate on one non-default
    stream with no synchronise between; then the Python mirror's shapes."""
    import torch
    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    g = torch.Generator(device="cuda").manual_seed(12)
    t = torch.randint(0, 256, (6, 14, 16384), dtype=torch.uint8, device="cuda", generator=g)
    host_masks = [ALL, lost(0), lost(4, 13), lost(1, 2, 3), lost(12), 0x3FF]
    masks = torch.tensor(host_masks, dtype=torch.int32, device="cuda")
    chk = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    sus = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    unchecked = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        batch.encode_batch(rs, t, stream=s)
        t[1, 11, 9000] ^= 0x10
        t[2, 2, 16383] ^= 0x01
        t[3, 13, 5] ^= 0x01
        t[5, 3, 5] ^= 0x01
        out = H.locate_corrupt_present_batch(rs, t, masks, check=chk, suspects=sus, bad_stripes=bad,
                                             unchecked=unchecked, stream=s)
    s.synchronize()
    assert out[0] is chk and out[1] is sus
    host = t.cpu().numpy()
    assert C.suspect_words(host, host_masks) == [0, 1 << 11, 1 << 2, UNEXPLAINED, 0, 0]
    assert sus.cpu().numpy().view(np.uint32).tolist() == C.suspect_words(host, host_masks)
    assert chk.cpu().numpy().view(np.uint32).tolist() == C.check_words(host, host_masks)
    assert (int(bad.item()), int(unchecked.item())) == (3, 1)
    assert H.verify_present_batch(rs, t, masks).cpu().numpy().view(np.uint32).tolist() == \
        C.check_words(host, host_masks)
    with pytest.raises(ValueError, match="suspects"):
        H.locate_corrupt_present_batch(rs, t, masks, suspects=torch.zeros(5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="present_masks"):
        H.verify_present_batch(rs, t, masks[:5])


@pytest.mark.parametrize("L", [(1 << 32) - 2048, (1 << 32) + 4096 + 16])
def test_shard_len_near_4gib(gpu, L):
    """Two degraded stripes (112 GiB in HBM) at the edge of the 32-bit lane
    offsets: 2^32 - 2 KiB is the longest shard the fast kernel takes, its last
    chunks at offsets past 2^31; 2^32 + 4 KiB + 16 runs the grid-stride kernels
    with chunk offsets above 2^32 and a 16-byte last chunk. The absent shards
    hold a sentinel. The model is applied to 32-byte windows around the flips
    (everything else is clean: the first run says so). A wrapped or
    sign-extended offset would read other bytes: a clean word or a wrong bit."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    S, W = 2, 32
    assert ("rs104_check_kernel" in H.check_kernel_name(L)) == (L < 1 << 32)
    host_masks = [lost(2), lost(0, 13)]
    torch.cuda.empty_cache()
    t = torch.empty((S, 14, L), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(t, 10 * L, 0x5EED7000)
    B.encode_batch(rs, t)
    for s, m in enumerate(host_masks):
        for i in range(14):
            if not m >> i & 1:
                t[s, i].fill_(FILL)
    masks = torch.tensor(host_masks, dtype=torch.int32, device="cuda")
    chk = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    sus = torch.full((S,), -1, dtype=torch.int32, device="cuda")

    def locate():
        H.locate_corrupt_present_batch(rs, t, masks, check=chk, suspects=sus)
        torch.cuda.synchronize()
        return chk.cpu().numpy().view(np.uint32).tolist(), sus.cpu().numpy().view(np.uint32).tolist()

    assert locate() == ([0, 0], [0, 0])
    far = (1 << 32) + 5 if L > 1 << 32 else (1 << 31) + 2048 * 3 + 5
    flips = [(0, 12, L - 1), (0, 4, (1 << 31) - 1), (1, 5, far), (1, 12, 0)]
    for s, i, o in flips:
        t[s, i, o] ^= 0x08
    torch.cuda.synchronize()
    windows = [[], []]
    for s, _, o in flips:
        lo = min(max(o - W // 2, 0), L - W)
        windows[s].append(t[s, :, lo:lo + W].cpu().numpy())
    small = np.stack([np.concatenate(w, axis=1) for w in windows])
    want = (C.check_words(small, host_masks), C.suspect_words(small, host_masks))
    assert want == ([1 << 11 | 1 << 12 | 1 << 13, 1 << 11 | 1 << 12], [1 << 12 | 1 << 4, 1 << 5 | 1 << 12])
    assert locate() == want
    del t
    torch.cuda.empty_cache()


# ---- checked reconstruct ---------------------------------------------------------
def checked_reconstruct(L, kind, stray=False):
    """stray: the call is given the masks with bits 14..31 set; everything
    expected is built from the masks & 0x3FFF."""
    import torch
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    cases = [  # (present mask, flips [(shard, pos)])
        (lost(6), []), (lost(0, 10), []), (lost(1, 2, 13), []), (lost(3, 4, 5, 6), []),  # clean, f = 1..4
        (lost(13), [(2, 7), (2, L - 1)]),          # f = 1, a corrupt B shard: named and rebuilt with the hole
        (lost(0, 5), [(13, L // 2)]),              # f = 2, a corrupt E shard
        (lost(1, 8, 12), [(4, 9)]),                # f = 3 dirty: detected only, left alone
        (0x3FF, []),                               # p = 10: the plain reconstruct
        (lost(0, 1, 2, 3, 4), []),                 # p < 10: skipped and counted by the reconstruct
        (ALL, []),                                 # clean full stripe
        (ALL, [(11, 0)]),                          # full stripe, one corrupt shard
        (lost(9), [(0, 33), (12, 33)]),            # r = 3, a same-column pair: left alone
        (lost(2, 3), [(7, 1), (10, L - 2), (13, 5)]),  # r = 2, three named: fewer than ten would remain
    ]
    S = len(cases)
    masks = [m for m, _ in cases]
    given = with_stray_bits(masks, L) if stray else masks
    clean = clean_stripes(S, L, seed=3)
    b = Batch(clean, masks, kind)
    for s, (_, flips) in enumerate(cases):
        for n, (shard, pos) in enumerate(flips):
            b.shard(s, shard)[pos] ^= 0x21 + n
    got = b.gather()
    want_chk, want_sus = C.check_words(got, masks), C.suspect_words(got, masks)
    want_use, want_left = C.use_masks(masks, want_chk, want_sus)
    assert want_use == [masks[0], masks[1], masks[2], masks[3], lost(13, 2), lost(0, 5, 13), ALL, 0x3FF,
                        masks[8], ALL, lost(11), ALL, ALL]
    assert want_left == 3
    # the expected image: repaired stripes are the clean originals, the others as they are
    expected = Batch(clean, masks, kind)
    expected.arena[:] = b.arena
    repaired = [s for s in range(S) if want_use[s] != ALL and bin(want_use[s]).count("1") >= 10]
    assert repaired == [0, 1, 2, 3, 4, 5, 7, 10]
    for s in repaired:
        for i in range(14):
            expected.shard(s, i)[:] = clean[s, i]
    la = b.layout
    dev = torch.from_numpy(b.arena).cuda()
    chk, sus, use = result_words(3, S)
    mt = SH.masks_tensor(given)
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    left = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    base = dev.data_ptr() + la.base
    rc = H.lib.hec_gpu_reconstruct_checked_batch(rs.handle, base, la.stripe_stride, la.shard_stride, L, S,
                                                 mt.data_ptr(), chk.data_ptr(), sus.data_ptr(), use.data_ptr(),
                                                 bad.data_ptr(), left.data_ptr(), stream)
    assert rc == 0, (rc, H._lib.last_detail())
    torch.cuda.synchronize()
    after = dev.cpu().numpy()
    # every byte: only shards outside the use mask changed, and to the original bytes
    SH.assert_arenas([expected.arena], [after], b.stripes, masks=masks)
    assert read_words(chk, S) == want_chk and read_words(sus, S) == want_sus
    assert read_words(use, S) == want_use, hexes(read_words(use, S))
    SH.assert_masks(mt.cpu().numpy(), given + [ALL])
    assert int(left.item()) == 5 + want_left and int(bad.item()) == 7 + 1
    for s in range(S):
        for i in range(14):
            if want_use[s] >> i & 1 or s == 8:
                o = la.off(s, i)
                assert np.array_equal(after[o:o + L], b.arena[o:o + L]), (s, i)
    # the proof: the repaired stripes verify clean
    ver, = result_words(1, S)
    rc = H.lib.hec_gpu_verify_batch(rs.handle, base, la.stripe_stride, la.shard_stride, base + 10 * la.shard_stride,
                                    la.stripe_stride, la.shard_stride, L, S, ver.data_ptr(), None, stream)
    assert rc == 0
    torch.cuda.synchronize()
    assert [w == 0 for w in read_words(ver, S)] == [s in repaired or s == 9 for s in range(S)]


@pytest.mark.parametrize("L,kind", [(8192 + 2048, "aligned"), (1000, "aligned"), (1000, "odd")])
def test_checked_reconstruct(gpu, L, kind):
    checked_reconstruct(L, kind)


@pytest.mark.parametrize("L,kind", [(8192 + 2048, "aligned"), (1000, "odd")])
def test_checked_reconstruct_with_stray_mask_bits(gpu, L, kind):
    """Bits 14..31 set in every present mask: the check, the locate, the use
    masks (built from m & 0x3FFF, so none of the stray bits may come through)
    and the reconstruct give what the clean masks give."""
    checked_reconstruct(L, kind, stray=True)


def test_checked_reconstruct_python_mirror(gpu):
    """What the call prevents: reconstruct_batch multiplies a corrupt survivor
    into the shard it rebuilds; the checked call names the survivor and
    restores the original bytes of both."""
    import torch
    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    L = 4096
    clean = torch.from_numpy(np.array(clean_stripes(2, L, seed=9)))
    masks = torch.tensor([lost(12), lost(12)], dtype=torch.int32, device="cuda")
    bad_copy, good_copy = clean.clone().cuda(), clean.clone().cuda()
    for t in (bad_copy, good_copy):
        t[:, 12] = FILL
        t[1, 3, 100] ^= 0x44
    batch.reconstruct_batch(rs, bad_copy, masks)
    assert torch.equal(bad_copy[0].cpu(), clean[0])
    assert not torch.equal(bad_copy[1, 12].cpu(), clean[1, 12])           # rebuilt from the corrupt shard 3
    left = torch.zeros(1, dtype=torch.int32, device="cuda")
    chk, sus, use = H.reconstruct_checked_batch(rs, good_copy, masks, unrepaired=left)
    assert sus.cpu().tolist() == [0, 1 << 3] and use.cpu().tolist() == [lost(12), lost(12, 3)]
    assert chk.cpu().tolist() == [0, 1 << 10 | 1 << 11 | 1 << 13] and int(left.item()) == 0
    assert torch.equal(good_copy.cpu(), clean)


# ---- big batches: built, corrupted and compared on the device ----------------------
CYCLE = [ALL, R3, R2, R1, 0x3FF]  # r = 4, 3, 2, 1 and p = 10, over the whole batch


def edge_hits(edge):
    """stripe -> (present mask, flips [(shard, pos, value)], suspects word by
    construction) of a batch of edge + 5 stripes of 16 bytes: one-shard flips
    (named and rebuilt) in the first and last stripe, on both sides of a wave
    and of `edge`; same-column pairs and one-spare stripes (left alone) on both
    sides of `edge` and in the last, partial wave; clean stripes with nine
    shards (skipped and counted by the reconstruct)."""
    S = edge + 5
    assert edge % 64 == 0 and edge // 2 > 1000
    return {
        0: (lost(13), [(2, 7, 0x21)], 1 << 2),
        77: (lost(0, 1, 2, 3, 4), [], 0),
        255: (R2, [(13, 0, 0x01)], 1 << 13),
        256: (ALL, [(11, 15, 0x80)], 1 << 11),
        1000: (R1, [(5, 4, 0x01)], UNEXPLAINED),
        edge // 2 + 1: (lost(1, 10), [(12, 9, 0x5A)], 1 << 12),
        edge - 3: (lost(9, 10, 11, 12, 13), [], 0),
        edge - 2: (R3, [(4, 5, 0x33), (8, 5, 0x44)], UNEXPLAINED),
        edge - 1: (R3, [(9, 3, 0xFF)], 1 << 9),
        edge: (R2, [(1, 8, 0x10)], 1 << 1),
        edge + 1: (R3, [(0, 11, 0x07), (13, 11, 0x70)], UNEXPLAINED),
        S - 3: (ALL, [(6, 9, 0x11), (12, 9, 0x22)], UNEXPLAINED),
        S - 2: (R1, [(0, 0, 0x01)], UNEXPLAINED),
        S - 1: (lost(5), [(0, 15, 0x42)], 1 << 0),
    }


def masked_scrub_big(edge):
    """The masked verify, the masked locate and the checked reconstruct over
    edge + 5 stripes of 16 bytes with CYCLE's masks and edge_hits' corruption.
    Expected words of the dirty stripes from check_model on those stripes, and
    by construction; every other stripe is a codeword of gfref's torch twin
    with its absent shards holding FILL, so its words are zero, its use mask
    its present mask and its image the codeword: whole arrays and the whole
    image are compared on the device."""
    import torch
    import gfref
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = edge + 5, 16
    hits = edge_hits(edge)
    order = sorted(hits)
    idx = torch.tensor(order, device="cuda")
    hit_masks = [hits[s][0] for s in order]
    expected = gfref.device_codewords(10, 4, S, L, seed=edge)
    masks = i32(CYCLE)[torch.arange(S, device="cuda") % len(CYCLE)]
    masks[idx] = i32(hit_masks)
    t = expected.clone()
    for i in range(14):
        t[:, i][(masks >> i & 1) == 0] = FILL  # absent shards
    for s in order:
        for shard, pos, value in hits[s][1]:
            t[s, shard, pos] ^= value
    dirty = t[idx].cpu().numpy()
    want_chk, want_sus = C.check_words(dirty, hit_masks), C.suspect_words(dirty, hit_masks)
    assert want_sus == [hits[s][2] for s in order], hexes(want_sus)
    want_use, want_left = C.use_masks(hit_masks, want_chk, want_sus)
    n_dirty = sum(1 for w in want_chk if w)
    assert n_dirty == sum(1 for s in order if hits[s][1]) and want_left == 5
    present = sum(masks >> i & 1 for i in range(14))
    n_unchecked, n_few = int((present <= 10).sum()), int((present < 10).sum())
    assert n_few == 2 and n_unchecked > S // len(CYCLE)
    chk_want, sus_want = expect_words(S, idx, want_chk), expect_words(S, idx, want_sus)
    use_want = expect_words(S, idx, want_use, rest=masks)
    given, before = masks.clone(), checksum(t)

    # pass 1 alone, then both passes: words and counts, nothing else written
    for locate in (False, True):
        chk, sus = result_words(2, S)
        bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        unchecked = torch.full((1,), 5, dtype=torch.int32, device="cuda")
        if locate:
            H.locate_corrupt_present_batch(rs, t, masks, check=chk, suspects=sus, bad_stripes=bad, unchecked=unchecked)
        else:
            H.verify_present_batch(rs, t, masks, check=chk, bad_stripes=bad, unchecked=unchecked)
        torch.cuda.synchronize()
        assert_words(chk, chk_want, ("check", locate))
        if locate:
            assert_words(sus, sus_want, "suspects")
        assert (int(bad.item()), int(unchecked.item())) == (7 + n_dirty, 5 + n_unchecked), locate
        assert checksum(t) == before and torch.equal(masks, given)

    # the checked reconstruct: stripes it must leave byte for byte keep what they hold now
    kept = [n for n, u in enumerate(want_use) if u == ALL or bin(u).count("1") < 10]
    assert len(kept) == want_left + n_few
    kept_idx = idx[torch.tensor(kept, device="cuda")]
    expected[kept_idx] = t[kept_idx]
    chk, sus, use = result_words(3, S)
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    left = torch.full((1,), 5, dtype=torch.int32, device="cuda")
    H.reconstruct_checked_batch(rs, t, masks, check=chk, suspects=sus, use_masks=use, bad_stripes=bad,
                                unrepaired=left)
    torch.cuda.synchronize()
    assert_words(chk, chk_want, "check of the reconstruct")
    assert_words(sus, sus_want, "suspects of the reconstruct")
    assert_words(use, use_want, "use masks")
    assert (int(left.item()), int(bad.item())) == (5 + want_left, 7 + n_few)
    assert torch.equal(masks, given)
    if not torch.equal(t, expected):
        wrong = torch.nonzero((t != expected).flatten(1).any(dim=1)).flatten()
        pytest.fail(f"image: {wrong.numel()} wrong stripes, the first {wrong[:8].cpu().tolist()}")
    # the proof: every stripe but the ones left alone verifies clean
    ver, = result_words(1, S)
    H.verify_batch(rs, t, mismatch=ver)
    torch.cuda.synchronize()
    assert torch.nonzero(ver[:S]).flatten().cpu().tolist() == [order[n] for n in kept]
    del t, expected
    torch.cuda.empty_cache()


def test_checked_reconstruct_second_mask_round(gpu):
    """2^19 + 5 stripes (117 MB): use_masks_kernel runs 2048 workgroups of 256
    lanes, so the stripes from 2^19 on are its second round, the last five in
    a partial wave whose ballot counts the stripes left alone."""
    masked_scrub_big(MASK_ROUND)


def test_masked_scrub_past_one_launch(gpu):
    """2^23 + 5 stripes (1.9 GB and one clone): the last five items are the
    second pass of rs104_check_stride_kernel's and rs104_locate_present_kernel's
    grid-stride loops, the mask kernel's 17th round, and the second stripe
    range of the reconstruct, driven by the use masks written just before."""
    masked_scrub_big(LAUNCH_LIMIT)


# ---- shard files -----------------------------------------------------------------
@pytest.fixture(scope="module")
def volume(tmp_path_factory):
    return SH.degraded_volume(str(tmp_path_factory.mktemp("degraded") / "9"))


def test_files_one_missing_one_corrupt_then_rebuild(gpu, volume, tmp_path):
    import helyim_amd as H
    files, size = volume
    base = write_volume(tmp_path, files, absent=(3,))
    n_blocks = -(-size // BLOCK)
    assert H.locate_corrupt_ec_files_present(base, BLOCK) == (n_blocks, 0, [], 0x3FF7)
    with pytest.raises(H.ShardNotFound):
        H.locate_corrupt_ec_files(base, BLOCK)
    x7, x_last = 5 * BLOCK + 1234, size - 1
    flip(base, 7, x7)
    now = [bytearray(f) for f in files]
    now[7][x7] ^= 0x5A
    lo = x7 // BLOCK * BLOCK
    want = [(lo, BLOCK) + block_words(now, 0x3FF7, lo, lo + BLOCK)]
    assert want[0][3] == 1 << 7 and want[0][2] == 1 << 11 | 1 << 12 | 1 << 13
    present = [i for i in range(14) if i != 3]
    for i in present:
        os.utime(base + ".ec%02d" % i, ns=(10**18, 10**18 + i))
    assert H.locate_corrupt_ec_files_present(base, BLOCK) == (n_blocks, 1, want, 0x3FF7)
    assert H.locate_corrupt_ec_files_present(base, BLOCK, cap=0) == (n_blocks, 1, [], 0x3FF7)
    # the last, short block, in a second corrupt file: its own entry with its own length
    flip(base, 12, x_last, 0x01)
    now[12][x_last] ^= 0x01
    os.utime(base + ".ec12", ns=(10**18, 10**18 + 12))
    lo2 = x_last // BLOCK * BLOCK
    want.append((lo2, size - lo2) + block_words(now, 0x3FF7, lo2, size))
    assert want[1][2:] == (1 << 12, 1 << 12)
    assert H.locate_corrupt_ec_files_present(base, BLOCK) == (n_blocks, 2, want, 0x3FF7)
    # one block over the whole volume names both files
    assert H.locate_corrupt_ec_files_present(base)[2] == [(0, size) + block_words(now, 0x3FF7, 0, size)]
    assert block_words(now, 0x3FF7, 0, size)[1] == 1 << 7 | 1 << 12
    # nothing was written, and the missing file was not created
    assert [os.stat(base + ".ec%02d" % i).st_mtime_ns for i in present] == [10**18 + i for i in present]
    assert [open(base + ".ec%02d" % i, "rb").read() for i in present] == [bytes(now[i]) for i in present]
    assert not os.path.exists(base + ".ec03")
    # the recipe: delete the named files too, rebuild, scrub again
    os.remove(base + ".ec07")
    os.remove(base + ".ec12")
    assert H.rebuild_ec_files(base) == [3, 7, 12]
    assert [open(base + ".ec%02d" % i, "rb").read() for i in range(14)] == files
    assert H.locate_corrupt_ec_files_present(base, BLOCK) == (n_blocks, 0, [], 0x3FFF)


def test_files_three_missing_only_detects(gpu, volume, tmp_path):
    import helyim_amd as H
    files, size = volume
    base = write_volume(tmp_path, files, absent=(0, 6, 13))
    mask = lost(0, 6, 13)
    x = 2 * BLOCK + 5
    flip(base, 9, x)
    now = [bytearray(f) for f in files]
    now[9][x] ^= 0x5A
    lo = x // BLOCK * BLOCK
    want = (lo, BLOCK) + block_words(now, mask, lo, lo + BLOCK)
    assert want[2:] == (1 << 12, UNEXPLAINED)
    assert H.locate_corrupt_ec_files_present(base, BLOCK) == (-(-size // BLOCK), 1, [want], mask)


def test_files_all_present_equal_the_full_locate(gpu, volume, tmp_path):
    import helyim_amd as H
    files, size = volume
    base = write_volume(tmp_path, files)
    flip(base, 2, 7 * BLOCK + 1)
    flip(base, 11, 9 * BLOCK)
    flip(base, 5, size - 2)
    flip(base, 8, 3 * BLOCK + 9)
    flip(base, 10, 3 * BLOCK + 9)
    for block in (BLOCK, 2 * BLOCK):
        n_blocks, n_bad, full = H.locate_corrupt_ec_files(base, block)
        assert n_bad == 4 and [e[3] for e in full] == [UNEXPLAINED, 1 << 2, 1 << 11, 1 << 5]
        assert H.locate_corrupt_ec_files_present(base, block) == \
            (n_blocks, n_bad, [(o, ln, pm << 10, sus) for o, ln, pm, sus in full], 0x3FFF)


def test_files_longer_than_the_two_slots(gpu, tmp_path):
    """Shards of 8 MiB and a ragged rest with two files missing: three chunks
    of the scrub's 4 MiB column range, both pinned slots reused. A missing
    file's row of a slot is never read into, so it holds what an earlier call
    left there: a full locate of another volume, 14 files of random bytes, runs
    first in this process, and only "the kernel never reads an absent shard"
    keeps the words right. Flips in the first, a middle and the last, short
    block and on both sides of the chunk edges; the words of every listed block
    from check_model, at 64 KiB blocks and at the default block size."""
    import helyim_amd as H
    size = (8 << 20) + 300_007
    absent, mask = (3, 12), lost(3, 12)
    rng = np.random.default_rng(2026)
    stale = str(tmp_path / "stale")
    for i in range(14):
        rng.integers(0, 256, size, dtype=np.uint8).tofile(stale + ".ec%02d" % i)
    bufs = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(10)] + [np.zeros(size, np.uint8) for _ in range(4)]
    corc.CReedSolomon(10, 4).encode(bufs)
    hits = [(11, 5), (2, (4 << 20) - 1), (13, 4 << 20), (6, (6 << 20) + 99), (9, (6 << 20) + 99),
            (0, (8 << 20) - 1), (10, 8 << 20), (4, size - 1)]
    for shard, off in hits:
        assert shard not in absent
        bufs[shard][off] ^= 0x33
    base = str(tmp_path / "big")
    for i in range(14):
        if i not in absent:
            bufs[i].tofile(base + ".ec%02d" % i)
    # 5 MiB blocks are larger than a chunk's 4 MiB: one block per chunk, and the
    # last chunk is a short block alone, whose words are the slot's first
    for block in (65536, 0, 5 << 20):
        width = block or 1 << 20  # HEC_SMALL_BLOCK_SIZE
        n_blocks = -(-size // width)
        # every block of the random volume is bad, so both slots and all 14 rows were filled
        assert H.locate_corrupt_ec_files(stale, block, cap=0)[:2] == (n_blocks, n_blocks)
        want = []
        for lo in sorted({off // width * width for _, off in hits}):
            hi = min(lo + width, size)
            want.append((lo, hi - lo) + block_words(bufs, mask, lo, hi))
        assert all(w[2] and w[3] for w in want)
        assert want[-1][:2] == (size // width * width, size % width)
        if block == 65536:
            assert [w[3] for w in want] == [1 << 11, 1 << 2, 1 << 13, want[3][3], 1 << 0, 1 << 10, 1 << 4]
        assert H.locate_corrupt_ec_files_present(base, block) == (n_blocks, len(want), want, mask), hex(block)
    assert not any(os.path.exists(base + ".ec%02d" % i) for i in absent)
