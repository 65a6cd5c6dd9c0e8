"""The ragged correct on the GPU: hec_gpu_correct_ragged and
hec_gpu_reconstruct_corrected_ragged over stripes of mixed lengths and present
masks.

Every expected value comes from tests/correct_present_model.py (correct,
use_masks) and tests/check_model.py, applied stripe by stripe to that stripe's
own [1, 14, L] bytes as they are in the arena. The arena harness is
tests/scrub_harness.py's Ragged: absent shards, the slack after each shard up
to its stride and the gaps between stripes hold a sentinel byte. Every device
call is also a footprint check: the arena that comes back equals the model's
image byte for byte (slack, gaps and absent shards included), the result
arrays start stale with a sentinel in word S that must survive, and the
counters start non-zero and advance by exactly the model's amounts.

The shapes are the ragged scrub suite's LENGTHS and MASKS: one vector, a
tail, a second map entry, one and three bit-sliced entries, every value of r."""
import numpy as np
import pytest

import check_model as C
import correct_present_model as M
import scrub_harness as SH
from scrub_harness import (ALL, FILL, NINE, R1, R2, R3, R4, RAGGED_LENGTHS as LENGTHS, RAGGED_MASKS as MASKS, Ragged,
                           TEN, UNEXPLAINED, hexes, ragged_flip_cases as flip_cases,
                           ragged_kernel_name as kernel_name, ragged_stripe as clean_stripe, read_words, result_words,
                           rs104)

pytestmark = pytest.mark.gpu

PRESET = (7, 5, 3, 11)  # bad_stripes, unchecked, uncorrected / unrepaired, corrected_bytes before a call


def model(b, min_spares=2):
    """-> (arena image, check, suspects, uncorrected, bytes changed) of correct_ragged on b."""
    img = b.arena.copy()
    chk, sus, left, changed = [], [], 0, 0
    for s, (L, m) in enumerate(b.shapes):
        out, c, w, u, n = M.correct(b.gather(s)[None], [m], min_spares)
        for i in range(14):
            if m >> i & 1:
                o = b.offs[s] + i * b.strides[s]
                img[o:o + L] = out[0, i]
            else:
                assert np.array_equal(out[0, i], b.gather(s)[i])  # the model leaves absent shards alone
        chk += c
        sus += w
        left += u
        changed += n
    return img, chk, sus, left, changed


def counters():
    return SH.preset_counters(PRESET, wide_last=True)


def advanced(ts):
    return [int(t.item()) - p for t, p in zip(ts, PRESET)]


def check_correct(rs, b, min_spares=2, note=None, want_sus=None):
    """correct_ragged on b against the model -> (image, check, suspects)."""
    import helyim_amd as H
    img, want_chk, want, left, changed = model(b, min_spares)
    if want_sus is not None:
        assert want == want_sus, (note, hexes(want), hexes(want_sus))
    (chk, sus), got, _ = SH.device_ragged(H.correct_ragged, rs, b, ("check", "suspects"),
                                          ("bad_stripes", "unchecked", "uncorrected", "corrected_bytes"), PRESET,
                                          wide_last=True, min_spares=min_spares, expected=img, note=note)
    cs = [g - p for g, p in zip(got, PRESET)]
    assert chk == want_chk, (note, hexes(chk), hexes(want_chk))
    assert sus == want, (note, hexes(sus), hexes(want))
    assert cs == [sum(1 for w in want_chk if w), C.unchecked_count(b.masks()), left, changed], \
        (note, cs, left, changed)
    check_correct.counted = (left, changed)  # the model's, which the device's equal
    return img, chk, sus


def check_reconstruct(rs, b, min_spares=2, note=None):
    """reconstruct_corrected_ragged on b against the models -> (arena, use masks).
    A rebuilt stripe's survivors must be their originals after the correct
    (asserted on the CPU), so its holes are expected to hold the originals."""
    import helyim_amd as H
    img, want_chk, want_sus, _, changed = model(b, min_spares)
    want_use, want_left = M.use_masks(b.masks(), want_chk, want_sus, min_spares)
    short = 0
    for s, (L, m) in enumerate(b.shapes):
        p = bin(want_use[s]).count("1")
        if p < 10:
            short += 1
        elif p < 14:
            for i in range(14):
                o = b.offs[s] + i * b.strides[s]
                if m >> i & 1:
                    assert np.array_equal(img[o:o + L], clean_stripe(L, s)[i]), (note, s, i)
                else:
                    img[o:o + L] = clean_stripe(L, s)[i]
    presets = (PRESET[0], PRESET[2], PRESET[3])
    (chk, sus, use), got, dev = SH.device_ragged(H.reconstruct_corrected_ragged, rs, b, ("check", "suspects", "use_masks"),
                                                 ("bad_stripes", "unrepaired", "corrected_bytes"), presets,
                                                 wide_last=True, min_spares=min_spares, expected=img, note=note)
    assert chk == want_chk and sus == want_sus, note
    assert use == want_use, (note, hexes(use), hexes(want_use))
    cs = [g - p for g, p in zip(got, presets)]
    assert cs == [short, want_left, changed], (note, cs, short, want_left, changed)
    return dev, use


# ---- 1. clean mixed batch ------------------------------------------------------
def clean_shapes():
    return [(L, m) for L in LENGTHS for m in MASKS] + [(24576, m) for m in (R3, R2, R1) * 3]


def test_clean_mixed_batch(gpu):
    """Every length with every mask, and 24576-byte stripes until the map has
    more than 100 entries: nothing is written, all words 0 over stale words,
    no byte counted. The bit-sliced pick on its own clean batch too."""
    b = Ragged(clean_shapes())
    assert b.entries() > 100 and "rs104_ragged_check_kernel" in kernel_name(b)
    img, chk, sus = check_correct(rs104(), b, note="clean", want_sus=[0] * b.S)
    assert np.array_equal(img, b.arena) and chk == [0] * b.S
    b = Ragged([(8192, ALL), (24576, ALL), (8192, ALL)])
    assert "bit-sliced" in kernel_name(b)
    img, chk, sus = check_correct(rs104(), b, note="clean bit-sliced", want_sus=[0] * 3)
    assert np.array_equal(img, b.arena) and chk == [0] * 3


# ---- 2. single wrong bytes -----------------------------------------------------
def single_flip_cases(form):
    return flip_cases(LENGTHS, (R4, R3, R2, R1)) if form == "table" else flip_cases((8192, 24576), (R4,))


@pytest.mark.parametrize("form", ["table", "bit-sliced"])
def test_single_wrong_bytes(gpu, form):
    """One wrong byte per stripe, the first or the last, in a shard of B or of
    E: with r >= 2 the byte is restored (the image is the clean arena), the
    words name the shard and corrected_bytes counts the flips; an r = 1 stripe
    keeps its bytes, sets bit 31 and is counted uncorrected. A flip of the
    byte at shard_len, in an absent shard, or in a stripe with p <= 10 changes
    nothing and is still there afterwards, in a clean stripe (which pass 2
    never reads) and in one with a wrong byte in the same last vector."""
    cases = single_flip_cases(form)
    extra = [(1000, R3), (4096 + 16, R2), (16, TEN), (2048, NINE), (1000, R3), (4096 + 16, R2)] \
        if form == "table" else []
    shapes = [(L, m) for L, m, _, _ in cases] + extra
    b, clean = Ragged(shapes), Ragged(shapes)
    want_sus, fixed, r1 = [], 0, 0
    for s, (L, m, shard, pos) in enumerate(cases):
        b.flip(s, shard, pos)
        if len(C.split(m)[1]) == 1:
            clean.flip(s, shard, pos)  # stays
            want_sus.append(UNEXPLAINED)
            r1 += 1
        else:
            want_sus.append(1 << shard)
            fixed += 1
    if extra:
        s = len(cases)
        stay = [(s, 5, 1000), (s, 13, 1001),                        # the byte at shard_len, and slack
                (s + 1, 0, 17), (s + 1, 12, 4096 + 15),             # absent shards of lost(0, 12)
                (s + 1, 6, 4096 + 16),                              # the byte at shard_len of a second-entry tail
                (s + 2, 2, 3), (s + 3, 1, 0)]                       # stripes that are not read at all
        # the same slack and absent-shard flips again in stripes that pass 1 does flag: a wrong
        # byte in the last vector of a present shard is fixed, its neighbours past the end stay
        stay += [(s + 4, 5, 1000), (s + 4, 13, 1001), (s + 5, 12, 4096 + 15), (s + 5, 6, 4096 + 16)]
        for where in stay:
            b.flip(*where)
            clean.flip(*where)
        b.flip(s + 4, 1, 999)
        b.flip(s + 5, 5, 4096 + 15)
        fixed += 2
        want_sus += [0] * 4 + [1 << 1, 1 << 5]
    assert ("rs104_bs_ragged_verify_kernel" if form == "bit-sliced" else "rs104_ragged_check_kernel") in kernel_name(b)
    img, chk, sus = check_correct(rs104(), b, note=form, want_sus=want_sus)
    assert np.array_equal(img, clean.arena)
    assert check_correct.counted == (r1, fixed) and fixed > 0 and (r1 > 0) == (form == "table")


# ---- 3. min_spares -------------------------------------------------------------
@pytest.mark.parametrize("min_spares", [2, 3, 4])
def test_min_spares(gpu, min_spares):
    """R2, R3 and R4 stripes with one wrong byte each: a stripe with r <
    min_spares is classified (the locate's words) but not written, and counted
    uncorrected once."""
    shapes = [(L, m) for L in (1000, 4096 + 16, 8192) for m in (R2, R3, R4)]
    b, want = Ragged(shapes), Ragged(shapes)
    named, left = [], 0
    for s, (L, m) in enumerate(shapes):
        ids = C.split(m)[0] + C.split(m)[1]
        shard, pos = ids[(3 * s + 1) % len(ids)], (L - 1, 0, L // 2)[s % 3]
        b.flip(s, shard, pos, 0x6B)
        b.flip(s, shard, (pos + 4095) % L, 0x6B)  # a second column, another wave or entry: still once
        named.append(1 << shard)
        if M.spares(m) < min_spares:
            want.flip(s, shard, pos, 0x6B)
            want.flip(s, shard, (pos + 4095) % L, 0x6B)
            left += 1
    img, chk, sus = check_correct(rs104(), b, min_spares, note=min_spares, want_sus=named)
    assert np.array_equal(img, want.arena)
    assert check_correct.counted[0] == left == {2: 0, 3: 3, 4: 6}[min_spares]


# ---- 4. scattered damage across entries -----------------------------------------
@pytest.mark.parametrize("mask", [R3, ALL], ids=["table", "bit-sliced"])
def test_scattered_damage_across_entries(gpu, mask):
    """A 24576-byte stripe with a wrong byte in each of its six 4 KiB ranges, in
    five different survivors (the bit-sliced map is walked as two halves per
    entry): everything is restored, bad_stripes is 1."""
    shapes = [(8192, mask), (24576, mask), (8192, mask)]
    b = Ragged(shapes)
    assert ("bit-sliced" in kernel_name(b)) == (mask == ALL)
    ids = C.split(mask)[0] + C.split(mask)[1]
    hit = [ids[1], ids[4], ids[8], ids[10], ids[-1], ids[4]]
    assert len(set(hit)) == 5
    for k in range(6):
        b.flip(1, hit[k], 4096 * k + 1024 * (k % 4) + 7 * k + 1, 0x11 * (k + 1))
    img, chk, sus = check_correct(rs104(), b, note=hex(mask), want_sus=[0, sum(1 << c for c in set(hit)), 0])
    assert np.array_equal(img, Ragged(shapes).arena)
    assert check_correct.counted == (0, 6)


# ---- 5. two wrong shards in one column -------------------------------------------
R2_PAIR = {2: 0x17, 9: 0xC3}  # shard -> error value, in one column of an R2 = lost(0, 12) stripe


def test_two_wrong_shards_in_one_column(gpu):
    """r = 4 and r = 3: the columns with two wrong shards keep their bytes and
    set bit 31, a single wrong byte elsewhere in the same stripe is fixed, and
    the stripe is counted uncorrected once although four columns in different
    waves and entries report it. r = 2, errors 0x17 in shard 2 and 0xC3 in
    shard 9 of one column of a lost(0, 12) stripe: the model finds no single
    shard that explains the column (asserted below, on the CPU), so the column
    keeps its bytes too and the stripe is counted uncorrected."""
    shapes = [(L, m) for m in (R4, R3) for L in (1000, 4096 + 16, 24576)] + [(2048, R2)]
    b, want = Ragged(shapes), Ragged(shapes)
    sus = []
    for s, (L, m) in enumerate(shapes[:-1]):
        B, E = C.split(m)
        for pos in sorted({0, L // 3, L // 2 + 300, L - 1}):
            for shard, v in ((B[2], 0x17), ((B[7], E[1])[s % 2], 0xC3)):
                b.flip(s, shard, pos, v)
                want.flip(s, shard, pos, v)
        b.flip(s, (E[0], B[5])[s % 2], L // 4 + 1, 0x3C)  # a single, fixed
        sus.append(UNEXPLAINED | 1 << (E[0], B[5])[s % 2])
    s = len(shapes) - 1
    for shard, v in R2_PAIR.items():
        b.flip(s, shard, 77, v)
    # what the model makes of the r = 2 pair, from the bytes themselves
    out, _, w, left2, changed2 = M.correct(b.gather(s)[None], [R2], 2)
    assert (w, left2, changed2) == ([UNEXPLAINED], 1, 0) and np.array_equal(out[0], b.gather(s))
    for shard, v in R2_PAIR.items():
        want.flip(s, shard, 77, v)
    img, chk, got = check_correct(rs104(), b, note="pairs", want_sus=sus + [UNEXPLAINED])
    assert np.array_equal(img, want.arena)
    assert check_correct.counted == (len(shapes), len(shapes) - 1)


# ---- 6. no leakage between neighbours -------------------------------------------
@pytest.mark.parametrize("shapes", [[(2048, R2), (4096 + 16, R3), (1000, R4), (24576, R3), (16, R2)],
                                    [(8192, ALL), (24576, ALL), (8192, ALL), (24576, ALL)]],
                         ids=["table", "bit-sliced"])
def test_no_leakage_between_neighbours(gpu, shapes):
    """Only the last chunk of stripe j, or only the first chunk of stripe
    j + 1, corrupt: exactly that stripe changes, back to its original."""
    rs, clean = rs104(), Ragged(shapes)
    for j in range(len(shapes) - 1):
        for s, pos in ((j, shapes[j][0] - 1), (j + 1, 0)):
            b = Ragged(shapes)
            shard = C.split(shapes[s][1])[0][4]
            b.flip(s, shard, pos)
            want = [0] * b.S
            want[s] = 1 << shard
            img, chk, sus = check_correct(rs, b, note=(j, s, pos), want_sus=want)
            assert np.array_equal(img, clean.arena)
            assert [w != 0 for w in chk] == [w != 0 for w in want]


# ---- 7. agreement with the strided call -------------------------------------------
def test_agrees_with_the_strided_call(gpu):
    """Eight uniform 8192-byte stripes with mixed masks: correct_ragged and
    correct_present_batch give equal words, equal counters and byte-equal
    images."""
    import torch
    import helyim_amd as H
    rs, S, L = rs104(), 8, 8192
    masks = [R3, R2, ALL, R1, TEN, R3, R2, NINE]
    host = np.stack([clean_stripe(L, s) for s in range(S)]).copy()
    host[0, C.split(masks[0])[0][6], 100] ^= 1
    host[1, C.split(masks[1])[1][1], 8191] ^= 0x55
    host[2, 13, 8191] ^= 0x55
    host[2, 2, 4096] ^= 3
    host[3, 4, 0] ^= 9
    host[5, 2, 4096] ^= 3
    host[5, 8, 4096] ^= 3
    host[5, 8, 5000] ^= 7
    host[6, 1, 77] ^= 0xFF
    host[7, 1, 78] ^= 0xFF
    a, t = torch.from_numpy(host).cuda(), torch.from_numpy(host).cuda()
    descs = [(s * 14 * L, L, L, masks[s]) for s in range(S)]
    md = torch.tensor(np.array(masks, dtype=np.uint32).view(np.int32), device="cuda")
    ca, cb = counters(), counters()
    chk, sus = H.correct_ragged(rs, a.view(-1), descs, 2, bad_stripes=ca[0], unchecked=ca[1], uncorrected=ca[2],
                                corrected_bytes=ca[3])
    chk_s, sus_s = H.correct_present_batch(rs, t, md, 2, bad_stripes=cb[0], unchecked=cb[1], uncorrected=cb[2],
                                           corrected_bytes=cb[3])
    torch.cuda.synchronize()
    assert chk.tolist() == chk_s.tolist() and sus.tolist() == sus_s.tolist()
    assert advanced(ca) == advanced(cb)
    assert torch.equal(a, t)
    want, want_chk, want_sus, left, changed = M.correct(host, masks, 2)
    assert np.array_equal(a.cpu().numpy(), want)
    assert chk.cpu().numpy().view(np.uint32).tolist() == want_chk
    assert sus.cpu().numpy().view(np.uint32).tolist() == want_sus
    assert advanced(ca)[2:] == [left, changed] and changed == 6 and left == 2


# ---- 8. corrected reconstruct ---------------------------------------------------
def test_corrected_reconstruct(gpu):
    """The shapes of the ragged scrub's repair recipe with a wrong survivor
    each, then: one lost shard plus five survivors wrong at five offsets (the
    checked recipe must leave that one alone), an R1 stripe with damage (left
    alone: use mask 0x3FFF, holes still holding the sentinel, unrepaired plus
    one), a clean TEN stripe (decoded on faith), a NINE stripe (counted in
    bad_stripes), a clean full stripe. Every rebuilt stripe equals its whole
    original, and verify_ragged with full masks on the rebuilt stripes is 0."""
    import torch
    import helyim_amd as H
    rs = rs104()
    shapes = [(L, m) for L, m in zip(LENGTHS * 2, (R4, R3, R2) * 4)]
    shapes += [(24576, R3), (4096 + 16, R1), (1000, TEN), (2048, NINE), (8192, ALL)]
    b = Ragged(shapes)
    for s, (L, m) in enumerate(shapes[:12]):
        ids = C.split(m)[0] + C.split(m)[1]
        for pos in sorted({0, L // 3, L - 1}):
            b.flip(s, ids[(5 * s + 2) % len(ids)], pos, 0x99)
    ids = C.split(R3)[0] + C.split(R3)[1]
    for k, shard in enumerate((ids[0], ids[3], ids[6], ids[9], ids[12])):
        b.flip(12, shard, 4096 * k + 1000 * k + 5, 0x10 + k)
    b.flip(13, C.split(R1)[0][3], 4096 + 3, 0x77)
    dev, use = check_reconstruct(rs, b, note="reconstruct")
    assert use[12] == R3 and use[13] == ALL and use[14] == TEN and use[15] == NINE and use[16] == ALL
    # the checked recipe would have left stripe 12 alone: five shards named, eight would remain
    sus12 = C.suspect_words(b.gather(12)[None], [R3])[0]
    assert bin(sus12).count("1") == 5 and bin(R3 & ~sus12).count("1") < 10
    got = dev.cpu().numpy()
    whole = Ragged(shapes, present=[ALL] * b.S)
    rebuilt = [s for s in range(b.S) if s not in (13, 15)]
    for s in rebuilt:
        assert np.array_equal(b.gather(s, got), whole.gather(s)), s
    for i in (2, 7, 11):  # the R1 stripe's holes
        o = b.offs[13] + i * b.strides[13]
        assert (got[o:o + shapes[13][0]] == FILL).all()
    full = [d[:3] + (ALL,) for d in b.descs()]
    again = H.verify_ragged(rs, dev, [full[s] for s in rebuilt])
    torch.cuda.synchronize()
    assert again.tolist() == [0] * len(rebuilt)


@pytest.mark.parametrize("min_spares", [3, 4])
def test_corrected_reconstruct_min_spares(gpu, min_spares):
    """With min_spares above a dirty stripe's r the stripe is classified, left
    alone and counted unrepaired; its neighbours are rebuilt."""
    shapes = [(1000, R2), (4096 + 16, R3), (8192, R3), (2048, R2), (16, TEN)]
    b = Ragged(shapes)
    for s, (L, m) in enumerate(shapes[:3]):
        b.flip(s, C.split(m)[0][s + 2], L - 1, 0x42)
    dev, use = check_reconstruct(rs104(), b, min_spares, note=min_spares)
    assert use == [ALL, R3 if min_spares == 3 else ALL, R3 if min_spares == 3 else ALL, R2, TEN]


# ---- 9. metadata slots ----------------------------------------------------------
def test_five_calls_back_to_back(gpu):
    """Five calls on one stream, different batches, one synchronise at the
    end: the calls pass through the reuse of the four metadata slots and every
    result is the model's."""
    import torch
    import helyim_amd as H
    rs = rs104()
    runs = []
    for n in range(5):
        shapes = [(LENGTHS[(n + k) % 6], (R4, R3, R2, R1, TEN)[(2 * n + k) % 5]) for k in range(4 + n)]
        b = Ragged(shapes)
        for s, (L, m) in enumerate(shapes):
            if s % 2 == 0 and M.spares(m) >= 1:
                b.flip(s, C.split(m)[0][(n + s) % 10], (L - 1) * (s % 4 == 0), 0x21 + n)
        recon = n % 2 == 1
        img, want_chk, want_sus, left, changed = model(b)
        want_use, want_left = M.use_masks(b.masks(), want_chk, want_sus)
        if recon:
            for s, (L, m) in enumerate(shapes):
                if want_use[s] != ALL:
                    for i in range(14):
                        if not m >> i & 1:
                            o = b.offs[s] + i * b.strides[s]
                            img[o:o + L] = clean_stripe(L, s)[i]
        runs.append((b, recon, img, want_chk, want_sus, want_use, want_left if recon else left, changed))
    state = []
    for b, recon, *_ in runs:
        dev = torch.from_numpy(b.arena).cuda()
        state.append((dev, result_words(3, b.S), counters()))
    torch.cuda.synchronize()
    for (b, recon, *_), (dev, (chk, sus, use), cs) in zip(runs, state):
        if recon:
            H.reconstruct_corrected_ragged(rs, dev, b.descs(), 2, check=chk, suspects=sus, use_masks=use,
                                           unrepaired=cs[2], corrected_bytes=cs[3])
        else:
            H.correct_ragged(rs, dev, b.descs(), 2, check=chk, suspects=sus, uncorrected=cs[2], corrected_bytes=cs[3])
    torch.cuda.synchronize()
    for n, ((b, recon, img, want_chk, want_sus, want_use, left, changed), (dev, (chk, sus, use), cs)) in \
            enumerate(zip(runs, state)):
        assert np.array_equal(dev.cpu().numpy(), img), n
        assert read_words(chk, b.S) == want_chk and read_words(sus, b.S) == want_sus, n
        if recon:
            assert read_words(use, b.S) == want_use, n
        assert advanced(cs)[2:] == [left, changed], n
