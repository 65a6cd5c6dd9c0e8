"""Correct in place with shards missing, on the GPU:
hec_gpu_correct_present_batch, hec_gpu_reconstruct_corrected_batch and
hec_correct_ec_files_present.

Every expected image, word and count comes from tests/correct_present_model.py
(the contract by brute force, on top of tests/check_model.py) applied to the
batch as it is; where the test built the damage itself the words and the
restored image are asserted by construction too. The arena harness is that of
tests/scrub_harness.py (Batch): absent shards, shard gaps and stripe gaps hold a
sentinel byte, result word S a sentinel word, and every device call is also a
whole-arena comparison against the model's image -- an absent shard, a gap or a
byte at or past shard_len that was read or written shows."""
import os
import stat

import numpy as np
import pytest

import check_model as C
import correct_present_model as CP
import scrub_harness as SH
from scrub_harness import (ALL, BLOCK, Batch, FILL, R1, R2, R3, UNEXPLAINED, clean_stripes, flip, hexes, lost,
                           masked_block_words as block_words, read_words, result_words, with_stray_bits, write_volume)

pytestmark = pytest.mark.gpu

LENGTHS = (2048, 8192 + 2048, 1000, 4096 + 16)  # one fast chunk, five, generic with an 8-byte tail, generic
KINDS = ("aligned", "odd", "shard-major")
BAD0, UNCHECKED0, UNC0, BYTES0 = 7, 5, 3, 11  # presets of the four accumulated counters


def image_arena(b, image):
    """b's arena with the present shards of every stripe replaced by image[S, 14, L]."""
    out = b.arena.copy()
    for s in range(b.S):
        for i in range(14):
            if b.masks[s] >> i & 1:
                o = b.layout.off(s, i)
                out[o:o + b.L] = image[s, i]
    return out


def device_correct(rs, b, expected, min_spares=2, given=None):
    """hec_gpu_correct_present_batch on b -> (check, suspects, bad_stripes,
    unchecked, uncorrected, corrected_bytes), the counters without their
    presets. Asserts that the arena afterwards equals `expected` in every byte."""
    presets = [BAD0, UNCHECKED0, UNC0, BYTES0]
    (chk, sus), got = SH.device_masked("hec_gpu_correct_present_batch", rs, b, 2, presets, wide_last=True,
                                       min_spares=min_spares, given=given, expected=expected, note=min_spares)
    return (chk, sus) + tuple(g - p0 for g, p0 in zip(got, presets))


def check_correct(rs, b, min_spares=2, note=None, want_sus=None, restored=None, given=None, want_counts=None):
    """The call on b against the model -> (expected arena, check, suspects).
    want_sus: the words by construction; restored: the arena the result must
    equal as a whole (the clean original's); want_counts: (uncorrected,
    corrected_bytes) by construction."""
    image, want_chk, sus_model, uncorrected, changed = CP.correct(b.gather(), b.masks, min_spares)
    expected = image_arena(b, image)
    if want_counts is not None:
        assert (uncorrected, changed) == want_counts, (note, uncorrected, changed)
    if want_sus is not None:
        assert sus_model == want_sus, (note, hexes(sus_model), hexes(want_sus))
    if restored is not None:
        assert np.array_equal(expected, restored), note
    chk, sus, bad, unchecked, unc, nbytes = device_correct(rs, b, expected, min_spares, given)
    assert chk == want_chk, (note, hexes(chk), hexes(want_chk))
    assert sus == sus_model, (note, hexes(sus), hexes(sus_model))
    assert bad == sum(1 for w in want_chk if w) and unchecked == C.unchecked_count(b.masks), (note, bad, unchecked)
    assert unc == uncorrected, (note, unc, uncorrected)
    assert nbytes == changed, (note, nbytes, changed)
    return expected, chk, sus


def device_reconstruct(rs, b, expected, corrected, min_spares=2):
    """hec_gpu_reconstruct_corrected_batch (or the checked one) on b -> (check,
    suspects, use masks, bad_stripes, unrepaired, corrected_bytes)."""
    if corrected:
        (chk, sus, use), (bad, left, nbytes) = SH.device_masked(
            "hec_gpu_reconstruct_corrected_batch", rs, b, 3, [BAD0, UNC0, BYTES0], wide_last=True,
            min_spares=min_spares, expected=expected, note="corrected")
    else:
        (chk, sus, use), (bad, left) = SH.device_masked("hec_gpu_reconstruct_checked_batch", rs, b, 3, [BAD0, UNC0],
                                                        expected=expected, note="checked")
        nbytes = BYTES0
    return chk, sus, use, bad - BAD0, left - UNC0, nbytes - BYTES0


def positions_of_interest(L):
    """The first byte, the ends of the 1 KiB wave ranges and 4 KiB chunks, the
    first byte of the last (tail) vector and the last byte."""
    return sorted({p for p in (0, 1023, 1024, 2047, 2048, 4095, 4096, (L - 1) // 16 * 16, L - 1) if p < L})


# ---- device batches --------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_clean_batch(gpu, L):
    """Nothing is written, the words are 0 and the counters keep their presets."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    masks = [R3, R2, R1, ALL, lost(13)]
    for kind in KINDS:
        b = Batch(clean_stripes(5, L), masks, kind)
        for min_spares in (2, 4):
            got = device_correct(rs, b, b.arena, min_spares)
            assert got == ([0] * 5, [0] * 5, 0, 0, 0, 0), (kind, min_spares, got)


def test_every_mask(gpu):
    """All 470 masks with a spare shard and a few without, one flipped byte per
    stripe in a seeded present shard: stripes with two or more spares are
    restored, those with one are untouched, carry bit 31 and are counted,
    those with none are neither read nor written and count as unchecked."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    L = 2048
    masks = C.checkable_masks() + [0x3FF, 0x3FF << 4, lost(0, 5, 9, 13), 0x1FF, 0x2AAA, 0]
    S = len(masks)
    assert S == 476
    clean = clean_stripes(S, L)
    b = Batch(clean, masks)
    restored = Batch(clean, masks).arena
    rng = np.random.default_rng(476)
    want_sus, n_r1 = [], 0
    for s, m in enumerate(masks):
        ids = [i for i in range(14) if m >> i & 1]
        r = len(ids) - 10
        if not ids:
            want_sus.append(0)
            continue
        shard = ids[int(rng.integers(len(ids)))]
        pos = int(rng.integers(L))
        b.shard(s, shard)[pos] ^= 1 + s % 255
        if r < 2:  # stays as it is
            o = b.layout.off(s, shard) + pos
            restored[o] = b.arena[o]
        want_sus.append(0 if r <= 0 else UNEXPLAINED if r == 1 else 1 << shard)
        n_r1 += r == 1
    expected, chk, sus = check_correct(rs, b, note="every mask", want_sus=want_sus, restored=restored)
    assert n_r1 == 364 and sum(1 for w in sus if w == UNEXPLAINED) == 364
    # the restored stripes verify clean under their masks, the others still differ
    _, chk2, sus2 = check_correct(rs, Batch(b.gather(expected), masks), note="second pass")
    assert [w != 0 for w in chk2] == [w == UNEXPLAINED for w in want_sus] and sus2 == [w & UNEXPLAINED for w in want_sus]


@pytest.mark.parametrize("L", LENGTHS)
def test_one_flipped_byte_in_every_present_shard(gpu, L):
    """Stripe n has its n-th present shard wrong at every position of interest
    -- the first byte, the last byte and, on the odd base, the tail vector
    among them; one more stripe is clean. The arena must equal the clean
    original. Fixes of the spare shards 10..13 land in those shards (not in
    shards 0..3: every shard id is addressed from the batch's one base)."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for mask in (R3, R2, ALL):
        ids = [i for i in range(14) if mask >> i & 1]
        S = len(ids) + 1
        clean = clean_stripes(S, L, seed=2)
        for kind in KINDS:
            b = Batch(clean, [mask] * S, kind)
            restored = b.arena.copy()
            for s, shard in enumerate(ids):
                for k, pos in enumerate(positions_of_interest(L)):
                    b.shard(s, shard)[pos] ^= (0x01, 0xFF, 0x40, 0x9C, 0x80)[(s + k) % 5]
            _, chk, sus = check_correct(rs, b, note=(hex(mask), kind, L), want_sus=[1 << i for i in ids] + [0],
                                        restored=restored)
            assert all(chk[:-1]) and chk[-1] == 0


@pytest.mark.parametrize("mask", [R2, R3, ALL], ids=["r2", "r3", "r4"])
def test_every_error_value(gpu, mask):
    """Stripe v - 1 gets ^= v in a shard of B, stripe 254 + v in a shard of E:
    a wrong fix table (another column's, another plan's) restores none of them."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 510, 1000
    B, E = C.split(mask)
    b = Batch(clean_stripes(S, L), [mask] * S, "odd" if mask == R3 else "aligned")
    restored = b.arena.copy()
    for v in range(1, 256):
        b.shard(v - 1, B[(v + 4) % 10])[(9 * v) % L] ^= v
        b.shard(254 + v, E[v % len(E)])[L - v] ^= v
    want = [1 << B[(v + 4) % 10] for v in range(1, 256)] + [1 << E[v % len(E)] for v in range(1, 256)]
    check_correct(rs, b, note=hex(mask), want_sus=want, restored=restored)


@pytest.mark.parametrize("L", [8192 + 2048, 1000])
def test_scattered_damage_with_a_shard_lost(gpu, L):
    """One shard lost and five survivors each wrong at another offset (stripe
    0), two lost and three survivors wrong (stripe 1), a clean degraded stripe
    (stripe 2). hec_gpu_reconstruct_checked_batch leaves the damaged stripes
    byte for byte and counts them: 13 - 5 = 8 and 12 - 3 = 9 trusted shards.
    hec_gpu_correct_present_batch restores the survivors, and
    hec_gpu_reconstruct_corrected_batch all 14 shards of the clean original."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    masks = [R3, R2, R3]
    hits = {0: [(0, 3, 0x10), (4, L // 3, 0xFF), (9, L // 2, 0x01), (10, L - 1, 0x80), (13, L - 17, 0x5A)],
            1: [(1, 0, 0x01), (7, L // 2 + 1, 0x77), (13, L - 1, 0xC3)]}
    clean = clean_stripes(3, L, seed=4)
    for kind in KINDS:
        b = Batch(clean, masks, kind)
        survivors = b.arena.copy()               # the survivors restored, the holes as they are
        whole = Batch(clean, [ALL] * 3, kind).arena  # all 14 shards of every stripe
        for s, flips in hits.items():
            for shard, pos, value in flips:
                b.shard(s, shard)[pos] ^= value
        named = [sum(1 << h[0] for h in hits[0]), sum(1 << h[0] for h in hits[1]), 0]
        # the checked reconstruct: the gap this call closes
        left_alone = b.arena.copy()
        o = b.layout.off(2, 3)
        left_alone[o:o + L] = clean[2, 3]         # the clean stripe is rebuilt
        chk, sus, use, bad, left, _ = device_reconstruct(rs, b, left_alone, corrected=False)
        assert sus == named and use == [ALL, ALL, R3] and (bad, left) == (0, 2), (kind, hexes(sus), hexes(use))
        # the masked correct: the survivors
        check_correct(rs, b, note=(kind, L), want_sus=named, restored=survivors)
        # the corrected reconstruct on a fresh copy: everything
        chk2, sus2, use2, bad, left, nbytes = device_reconstruct(rs, b, whole, corrected=True)
        assert (chk2, sus2) == (chk, sus) and use2 == masks and (bad, left, nbytes) == (0, 0, 8), kind
        want_use, want_left = CP.use_masks(masks, chk2, sus2)
        assert (use2, left) == (want_use, want_left)


def test_two_wrong_survivors_in_one_column(gpu):
    """r = 3: pairs in several columns of stripe 0 that different waves and
    chunks hold stay untouched, set bit 31 and count the stripe once; a single
    in the same stripe is still fixed. r = 2: one seeded pair the model takes
    for an intact shard (which is then written) and one it leaves unexplained:
    the device equals the model in both."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    L = 8192 + 2048
    rng = np.random.default_rng(32)
    ids2 = [i for i in range(14) if R2 >> i & 1]
    taken = unexplained = None
    while taken is None or unexplained is None:
        a, c = (ids2[i] for i in rng.choice(len(ids2), 2, replace=False))
        errors = {a: int(rng.integers(1, 256)), c: int(rng.integers(1, 256))}
        word = C.column_word(C.syndrome_of(R2, errors), R2)
        if word == UNEXPLAINED:
            unexplained = unexplained or errors
        else:
            assert word.bit_length() - 1 not in errors
            taken = taken or (errors, word)
    for kind in ("aligned", "odd"):
        b = Batch(clean_stripes(4, L, seed=5), [R3, R2, R2, R3], kind)
        for n, pos in enumerate((5, 1024 + 5, 4096 + 7, 8192 + 2047)):
            for shard, v in ((0 + n, 0x21), (13 - n, 0x9C)):
                b.shard(0, shard if shard != 3 else 4)[pos] ^= v
        b.shard(0, 6)[6] ^= 0x3C
        for shard, v in taken[0].items():
            b.shard(1, shard)[77] ^= v
        for shard, v in unexplained.items():
            b.shard(2, shard)[L - 1] ^= v
        before = b.arena.copy()
        expected, chk, sus = check_correct(rs, b, note=kind,
                                           want_sus=[UNEXPLAINED | 1 << 6, taken[1], UNEXPLAINED, 0])
        changed = np.flatnonzero(expected != before)
        intact = taken[1].bit_length() - 1
        assert sorted(changed) == sorted([b.layout.off(0, 6) + 6, b.layout.off(1, intact) + 77]), kind
        # with min_spares = 3 the r = 2 stripes are left alone and counted
        expected3, _, _ = check_correct(rs, b, 3, note=kind)
        assert np.flatnonzero(expected3 != before).tolist() == [b.layout.off(0, 6) + 6]


@pytest.mark.parametrize("L", [2048, 1000])
def test_min_spares(gpu, L):
    """min_spares = 3: stripes with two spares and one wrong byte are not
    written, their words are the locate's, and they are counted in
    *d_uncorrected; min_spares = 4: only full-mask stripes are written."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    masks = [R2, R3, ALL, R1, R2, lost(5, 6), R3, 0x3FF]
    S = len(masks)
    clean = clean_stripes(S, L, seed=6)
    for kind in ("aligned", "odd"):
        b = Batch(clean, masks, kind)
        restored = {}
        for s, m in enumerate(masks):
            if s == 4:
                continue  # a clean stripe with two spares
            shard = [i for i in range(14) if m >> i & 1][(5 * s + 9) % bin(m).count("1")]
            pos = (L - 1, 0, L // 2)[s % 3]
            o = b.layout.off(s, shard) + pos
            restored[s] = (o, b.arena[o])
            b.arena[o] ^= 0x11 * (s + 1)
        want_sus = C.suspect_words(b.gather(), masks)
        assert [bin(w).count("1") for w in want_sus] == [1, 1, 1, 1, 0, 1, 1, 0] and want_sus[3] == UNEXPLAINED
        for min_spares, written in ((2, (0, 1, 2, 5, 6)), (3, (1, 2, 6)), (4, (2,))):
            want = b.arena.copy()
            for s in written:
                want[restored[s][0]] = restored[s][1]
            check_correct(rs, b, min_spares, note=(kind, min_spares), want_sus=want_sus, restored=want,
                          want_counts=(6 - len(written), len(written)))


@pytest.mark.parametrize("L", [8192 + 2048, 4096 + 16])
def test_full_masks_reproduce_correct(gpu, L):
    """With every shard present the arena, the suspects and the byte count equal
    hec_gpu_correct_batch's on the same bytes, the check word its mismatch word << 10."""
    import torch
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 6
    for kind in ("aligned", "odd"):
        b = Batch(clean_stripes(S, L), [ALL] * S, kind)
        b.shard(0, 3)[L - 1] ^= 0x21
        b.shard(1, 12)[0] ^= 0x01
        b.shard(2, 6)[77] ^= 0x80
        b.shard(2, 9)[77] ^= 0x80
        b.shard(2, 11)[78] ^= 0x44
        b.shard(4, 0)[4095] ^= 0xFF
        b.shard(4, 13)[4096] ^= 0x02
        expected, chk, sus = check_correct(rs, b, note=(kind, L),
                                           want_sus=[1 << 3, 1 << 12, UNEXPLAINED | 1 << 11, 0, 1 | 1 << 13, 0])
        la = b.layout
        dev = torch.from_numpy(b.arena).cuda()
        mis_t, sus_t = result_words(2, S)
        unc = torch.zeros(1, dtype=torch.int32, device="cuda")
        nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
        base = dev.data_ptr() + la.base
        rc = H.lib.hec_gpu_correct_batch(rs.handle, base, la.stripe_stride, la.shard_stride,
                                         base + 10 * la.shard_stride, la.stripe_stride, la.shard_stride, L, S,
                                         mis_t.data_ptr(), sus_t.data_ptr(), None, unc.data_ptr(), nbytes.data_ptr(),
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(dev.cpu().numpy(), expected), kind
        assert chk == [w << 10 for w in read_words(mis_t, S)] and sus == read_words(sus_t, S)
        assert (int(unc.item()), int(nbytes.item())) == (1, 5)


@pytest.mark.parametrize("L", [2048, 4096 + 16])
def test_stray_mask_bits_change_nothing(gpu, L):
    """Bits 14..31 set in every mask given to the call: the model's image, words
    and counts for the masks & 0x3FFF."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    masks = [R3, R2, R1, ALL, lost(13), lost(0, 1), 0x3FF, R3]
    stray = with_stray_bits(masks, L)
    for kind in ("aligned", "odd"):
        runs = []
        for given in (masks, stray):
            b = Batch(clean_stripes(len(masks), L), masks, kind)
            for s, m in enumerate(masks[:-1]):
                ids = [i for i in range(14) if m >> i & 1]
                b.shard(s, ids[(4 * s + 1) % len(ids)])[(L - 1, 0, 1024)[s % 3]] ^= 0x11 * (s + 1)
            expected, chk, sus = check_correct(rs, b, note=(kind, given is stray), given=given)
            runs.append((expected.tobytes(), chk, sus))
        assert runs[0] == runs[1] and any(runs[0][1])


def test_shard_end(gpu):
    """An error in the last byte with shard_len % 16 != 0 (the 8-byte tail of
    the last vector) is fixed through the tail store; the random bytes past
    shard_len, in every gap and pad, take no part and stay."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    L, masks = 1000, [R3, R2, R1, ALL, R3]
    clean = clean_stripes(5, L)
    for kind in KINDS:
        b = Batch(clean, masks, kind, fill=None)
        restored = b.arena.copy()
        b.shard(0, 13)[L - 1] ^= 0x80
        b.shard(1, 1)[L - 1] ^= 0x01
        b.shard(2, 5)[L - 1] ^= 0x55
        b.shard(3, 12)[L - 1] ^= 0xFF
        b.shard(3, 9)[L - 2] ^= 0xFE
        o = b.layout.off(2, 5) + L - 1
        restored[o] = b.arena[o]  # one spare: detected only
        check_correct(rs, b, note=kind, want_sus=[1 << 13, 1 << 1, UNEXPLAINED, 1 << 9 | 1 << 12, 0], restored=restored)


def test_more_items_than_the_locate_grid(gpu):
    """2048 + 5 stripes of one 4 KiB chunk: more items than pass 2's 2048
    workgroups, so some take a second item, with fixes in the first and the
    last stripes and the masks array in step."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 2048 + 5, 4096
    cycle = [R3, R2, ALL, lost(13), lost(5, 6), 0x3FF, R1]
    masks = [cycle[s % len(cycle)] for s in range(S)]
    clean = clean_stripes(S, L)
    b = Batch(clean, masks)
    restored = b.arena.copy()
    want = [0] * S
    for s, pos in ((0, 0), (1, 3), (2047, 4095), (2048, 7), (2051, 1024), (S - 1, 4095)):
        B, E = C.split(masks[s])
        shard = (B + E)[s % len(B + E)]
        assert len(E) >= 2
        b.shard(s, shard)[pos] ^= 0x5A
        want[s] = 1 << shard
    assert masks[1000] == R1 and masks[1006] == 0x3FF
    b.shard(1000, 0)[4] ^= 0x01     # one spare: detected, left
    b.shard(1006, 4)[4] ^= 0x01     # nothing to check: not even read
    for s, i in ((1000, 0), (1006, 4)):
        restored[b.layout.off(s, i) + 4] ^= 0x01
    want[1000] = UNEXPLAINED
    check_correct(rs, b, note="grid", want_sus=want, restored=restored)


def test_encode_corrupt_correct_verify_in_stream_order_and_python_mirrors(gpu):
    """encode_batch, corrupting writes, the masked correct and the masked verify
    on one non-default stream with no synchronise between; then the mirrors'
    shapes, counters and argument checks, and reconstruct_corrected_batch."""
    import torch
    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    g = torch.Generator(device="cuda").manual_seed(21)
    t = torch.randint(0, 256, (6, 14, 16384), dtype=torch.uint8, device="cuda", generator=g)
    host_masks = [ALL, lost(0), lost(4, 13), lost(1, 2, 3), lost(12), 0x3FF]
    masks = torch.tensor(host_masks, dtype=torch.int32, device="cuda")
    chk = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    sus = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    unc = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        batch.encode_batch(rs, t, stream=s)
        good = t.clone()
        t[1, 11, 9000] ^= 0x10
        t[1, 2, 16383] ^= 0x7F
        t[2, 2, 16383] ^= 0x01
        t[3, 13, 5] ^= 0x01
        t[5, 3, 5] ^= 0x01
        damaged = t.clone()
        out = H.correct_present_batch(rs, t, masks, check=chk, suspects=sus, uncorrected=unc, corrected_bytes=nbytes,
                                      stream=s)
        after = H.verify_present_batch(rs, t, masks, stream=s)
    s.synchronize()
    assert out[0] is chk and out[1] is sus
    host = damaged.cpu().numpy()
    image, want_chk, want_sus, uncorrected, changed = CP.correct(host, host_masks)
    assert want_sus == [0, 1 << 11 | 1 << 2, 1 << 2, UNEXPLAINED, 0, 0] and (uncorrected, changed) == (1, 3)
    assert sus.cpu().numpy().view(np.uint32).tolist() == want_sus
    assert chk.cpu().numpy().view(np.uint32).tolist() == want_chk
    assert (int(unc.item()), int(nbytes.item())) == (1, 3)
    assert np.array_equal(t.cpu().numpy(), image)
    assert torch.equal(t[:3], good[:3]) and torch.equal(t[3:], damaged[3:])
    assert after.cpu().numpy().view(np.uint32).tolist() == [0, 0, 0, want_chk[3], 0, 0]
    # min_spares = 3 on the damaged batch: the stripe with two spares stays
    t3 = damaged.clone()
    H.correct_present_batch(rs, t3, masks, min_spares=3, uncorrected=unc)
    assert torch.equal(t3[2], damaged[2]) and torch.equal(t3[1], good[1]) and int(unc.item()) == 1 + 2
    # the corrected reconstruct: holes filled where the survivors are consistent
    t4 = damaged.clone()
    for st, m in enumerate(host_masks):
        for i in range(14):
            if not m >> i & 1:
                t4[st, i] = FILL
    holes = t4.clone()
    left = torch.zeros(1, dtype=torch.int32, device="cuda")
    c4, s4, use = H.reconstruct_corrected_batch(rs, t4, masks, unrepaired=left, corrected_bytes=nbytes)
    assert s4.cpu().numpy().view(np.uint32).tolist() == want_sus
    assert use.cpu().tolist() == [ALL, lost(0), lost(4, 13), ALL, lost(12), 0x3FF]
    assert int(left.item()) == 1 and int(nbytes.item()) == 6
    assert torch.equal(t4[:3], good[:3]) and torch.equal(t4[4], good[4]) and torch.equal(t4[3], holes[3])
    assert torch.equal(t4[5, :10], damaged[5, :10]) and not torch.equal(t4[5, 10:], good[5, 10:])  # decoded on faith
    with pytest.raises(ValueError, match="corrected_bytes"):
        H.correct_present_batch(rs, t, masks, corrected_bytes=torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="suspects"):
        H.correct_present_batch(rs, t, masks, suspects=torch.zeros(5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="present_masks"):
        H.reconstruct_corrected_batch(rs, t, masks[:5])
    with pytest.raises(H.DeviceError, match="min_spares"):
        H.correct_present_batch(rs, t, masks, min_spares=1)


# ---- shard files -----------------------------------------------------------------
@pytest.fixture(scope="module")
def volume(tmp_path_factory):
    return SH.degraded_volume(str(tmp_path_factory.mktemp("degraded") / "9"))


def read_files(base, ids=range(14)):
    return {i: open(base + ".ec%02d" % i, "rb").read() for i in ids}


def test_files_one_missing_five_scattered_then_rebuild(gpu, volume, tmp_path):
    """File 3 is missing and five others carry scattered flips (two of them in
    one block, one in the short last block, two files in one column of another
    block). The entries equal the locate's; only the named files' rows of bad
    blocks change, to the model's image; rebuild_ec_files then yields the
    original 14 files where no column stayed unexplained, and a second scrub
    reports that block alone."""
    import helyim_amd as H
    files, size = volume
    base = write_volume(tmp_path, files, absent=(3,))
    n_blocks = -(-size // BLOCK)
    present = [i for i in range(14) if i != 3]
    assert H.correct_ec_files_present(base, BLOCK) == (n_blocks, 0, [], 0x3FF7)
    hits = [(0, BLOCK + 1, 0x40), (7, 5 * BLOCK + 1234, 0x5A), (9, 5 * BLOCK + 4000, 0x01), (10, 2 * BLOCK - 1, 0xFF),
            (12, size - 1, 0x01), (13, 8 * BLOCK + 9, 0x21)]
    now = [bytearray(f) for f in files]
    for shard, off, value in hits:
        flip(base, shard, off, value)
        now[shard][off] ^= value
    want = []
    for lo in sorted({off // BLOCK * BLOCK for _, off, _ in hits}):
        hi = min(lo + BLOCK, size)
        want.append((lo, hi - lo) + block_words(now, 0x3FF7, lo, hi))
    assert [w[3] for w in want] == [1 | 1 << 10, 1 << 7 | 1 << 9, 1 << 13, 1 << 12]
    assert H.locate_corrupt_ec_files_present(base, BLOCK) == (n_blocks, 4, want, 0x3FF7)
    untouched = [i for i in present if i not in (0, 7, 9, 10, 12, 13)]
    for i in present:
        os.utime(base + ".ec%02d" % i, ns=(10**18, 10**18 + i))
    assert H.correct_ec_files_present(base, BLOCK, cap=3) == (n_blocks, 4, want[:3], 0x3FF7)
    assert read_files(base, present) == {i: files[i] for i in present}
    assert [os.stat(base + ".ec%02d" % i).st_mtime_ns for i in untouched] == [10**18 + i for i in untouched]
    assert not os.path.exists(base + ".ec03")
    assert H.correct_ec_files_present(base, BLOCK) == (n_blocks, 0, [], 0x3FF7)
    assert H.rebuild_ec_files(base) == [3]
    assert [open(base + ".ec%02d" % i, "rb").read() for i in range(14)] == files
    assert H.locate_corrupt_ec_files_present(base, BLOCK) == (n_blocks, 0, [], 0x3FFF)
    # two wrong files in one column (three spares: unexplained) beside a single: the single is fixed, the block stays
    os.remove(base + ".ec03")
    now = [bytearray(f) for f in files]
    for shard, off, value in ((1, 3 * BLOCK + 9, 0x11), (11, 3 * BLOCK + 9, 0x22), (5, 3 * BLOCK + 10, 0x33)):
        flip(base, shard, off, value)
        now[shard][off] ^= value
    entry = (3 * BLOCK, BLOCK) + block_words(now, 0x3FF7, 3 * BLOCK, 4 * BLOCK)
    assert entry[3] == UNEXPLAINED | 1 << 5
    assert H.correct_ec_files_present(base, BLOCK) == (n_blocks, 1, [entry], 0x3FF7)
    now[5][3 * BLOCK + 10] ^= 0x33
    assert read_files(base, present) == {i: bytes(now[i]) for i in present}
    left = (3 * BLOCK, BLOCK) + block_words(now, 0x3FF7, 3 * BLOCK, 4 * BLOCK)
    assert left[3] == UNEXPLAINED
    assert H.correct_ec_files_present(base, BLOCK) == (n_blocks, 1, [left], 0x3FF7)
    # min_spares above the volume's three spares: the locate, nothing written
    flip(base, 5, 3 * BLOCK + 10, 0x33)
    before = read_files(base, present)
    assert H.correct_ec_files_present(base, BLOCK, min_spares=4) == (n_blocks, 1, [entry], 0x3FF7)
    assert read_files(base, present) == before


def test_files_three_missing_only_detects(gpu, volume, tmp_path):
    import helyim_amd as H
    files, size = volume
    base = write_volume(tmp_path, files, absent=(0, 6, 13))
    mask = lost(0, 6, 13)
    present = [i for i in range(14) if mask >> i & 1]
    x = 2 * BLOCK + 5
    flip(base, 9, x)
    now = [bytearray(f) for f in files]
    now[9][x] ^= 0x5A
    lo = x // BLOCK * BLOCK
    want = (lo, BLOCK) + block_words(now, mask, lo, lo + BLOCK)
    assert want[2:] == (1 << 12, UNEXPLAINED)
    for i in present:
        os.utime(base + ".ec%02d" % i, ns=(10**18, 10**18 + i))
    assert H.correct_ec_files_present(base, BLOCK) == (-(-size // BLOCK), 1, [want], mask)
    assert read_files(base, present) == {i: bytes(now[i]) for i in present}
    assert [os.stat(base + ".ec%02d" % i).st_mtime_ns for i in present] == [10**18 + i for i in present]
    assert not any(os.path.exists(base + ".ec%02d" % i) for i in (0, 6, 13))


def test_files_a_read_only_present_file_is_an_io_error(gpu, volume, tmp_path):
    import errno
    import helyim_amd as H
    files, size = volume
    base = write_volume(tmp_path, files, absent=(3,))
    flip(base, 7, 100)
    damaged = read_files(base, [i for i in range(14) if i != 3])
    os.remove(base + ".ec05")
    os.mkdir(base + ".ec05")  # cannot be opened for writing by anybody
    with pytest.raises(H.Io):
        H.correct_ec_files_present(base, BLOCK)
    assert H._lib.last_values()[2] == errno.EISDIR
    os.rmdir(base + ".ec05")
    open(base + ".ec05", "wb").write(files[5])
    os.chmod(base + ".ec09", stat.S_IRUSR)
    if not os.access(base + ".ec09", os.W_OK):  # file modes bind this user
        with pytest.raises(H.Io):
            H.correct_ec_files_present(base, BLOCK)
        assert H._lib.last_values()[2] == errno.EACCES and ".ec09" in H._lib.last_detail()
        assert read_files(base, damaged) == damaged
        assert H.locate_corrupt_ec_files_present(base, BLOCK)[1] == 1  # reading is still possible


def test_files_longer_than_the_two_slots(gpu, tmp_path):
    """Shards of 8 MiB and a ragged rest with two files missing: three chunks
    of the scrub's 4 MiB column range, both pinned slots reused and written
    back from. Flips in the first, a middle and the last, short block and on
    both sides of the chunk edges, at 64 KiB blocks and at the default block
    size: the entries are the locate's, the files come back to the original."""
    import helyim_amd as H
    from oracle import corc
    size = (8 << 20) + 300_007
    absent, mask = (3, 12), lost(3, 12)
    present = [i for i in range(14) if i not in absent]
    rng = np.random.default_rng(2027)
    bufs = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(10)] + [np.zeros(size, np.uint8) for _ in range(4)]
    corc.CReedSolomon(10, 4).encode(bufs)
    hits = [(11, 5), (2, (4 << 20) - 1), (13, 4 << 20), (6, (6 << 20) + 99), (9, (6 << 20) + 100),
            (0, (8 << 20) - 1), (10, 8 << 20), (4, size - 1)]
    base = str(tmp_path / "big")
    for i in present:
        bufs[i].tofile(base + ".ec%02d" % i)
    good = read_files(base, present)
    # 5 MiB blocks are larger than a chunk's 4 MiB: one block per chunk, and the
    # last chunk is a short block alone, whose words are the slot's first
    for block in (65536, 0, 5 << 20):
        width = block or 1 << 20  # HEC_SMALL_BLOCK_SIZE
        n_blocks = -(-size // width)
        for shard, off in hits:
            flip(base, shard, off, 0x33)
            bufs[shard][off] ^= 0x33
        want = []
        for lo in sorted({off // width * width for _, off in hits}):
            hi = min(lo + width, size)
            want.append((lo, hi - lo) + block_words(bufs, mask, lo, hi))
        assert all(w[2] and w[3] and not w[3] & UNEXPLAINED for w in want)
        for shard, off in hits:
            bufs[shard][off] ^= 0x33
        assert H.correct_ec_files_present(base, block) == (n_blocks, len(want), want, mask), hex(block)
        assert read_files(base, present) == good, hex(block)
        assert H.locate_corrupt_ec_files_present(base, block) == (n_blocks, 0, [], mask)
    assert not any(os.path.exists(base + ".ec%02d" % i) for i in absent)
