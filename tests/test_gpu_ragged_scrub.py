"""The ragged scrub on the GPU: hec_gpu_verify_ragged and
hec_gpu_locate_corrupt_ragged over stripes of mixed lengths and present masks.

Every expected word comes from tests/check_model.py (the masked contracts by
brute force), applied stripe by stripe to that stripe's own [1, 14, L] bytes as
they are in the arena; where the test built the corruption itself the word is
asserted by construction too. Stripes sit back to back in one arena filled with
a sentinel byte: absent shards, the slack after each shard up to its stride and
the gaps between stripes hold it, so a kernel that reads an absent shard or a
byte at or past shard_len computes a wrong word here. Every device call is also
a footprint check: the arena comes back byte for byte, the result arrays start
stale with a sentinel in word S that must survive, the counters start non-zero.

The shapes are the smallest that reach each path: 16 bytes (one lane's vector),
1000 (a tail with an 8-byte remainder), 2048, 4096 + 16 (a second map entry of
one vector), 8192 (one bit-sliced entry), 24576 (three)."""
import numpy as np
import pytest

import check_model as C
import scrub_harness as SH
from scrub_harness import (ALL, NINE, R1, R2, R3, R4, RAGGED_LENGTHS as LENGTHS, RAGGED_MASKS as MASKS, Ragged, TEN,
                           UNEXPLAINED, hexes, ragged_flip_cases as flip_cases, ragged_kernel_name as kernel_name,
                           ragged_stripe as clean_stripe, rs104)

pytestmark = pytest.mark.gpu

def device_scrub(rs, b, locate=True, preset=(7, 5), masks=None):
    """The ragged locate (or the verify alone) on b -> (check, suspects,
    bad_stripes, unchecked), the counters without their presets. Asserts the
    footprint."""
    import helyim_amd as H
    fn, names = (H.locate_corrupt_ragged, ("check", "suspects")) if locate else (H.verify_ragged, ("check",))
    ws, (bad, unchecked), _ = SH.device_ragged(fn, rs, b, names, ("bad_stripes", "unchecked"), preset, masks=masks)
    return ws[0], ws[1] if locate else None, bad - preset[0], unchecked - preset[1]


def check_batch(rs, b, by_construction=None, note=None):
    """Verify alone and locate on b against the model -> (check, suspects)."""
    want_chk, want_sus = b.model()
    if by_construction is not None:
        assert want_sus == by_construction, (note, hexes(want_sus), hexes(by_construction))
    assert [w != 0 for w in want_chk] == [w != 0 for w in want_sus], note
    chk, sus, bad, unchecked = device_scrub(rs, b)
    assert chk == want_chk, (note, hexes(chk), hexes(want_chk))
    assert sus == want_sus, (note, hexes(sus), hexes(want_sus))
    assert bad == sum(1 for w in want_chk if w) and unchecked == C.unchecked_count(b.masks()), (note, bad, unchecked)
    chk1, _, bad1, unchecked1 = device_scrub(rs, b, locate=False)
    assert (chk1, bad1, unchecked1) == (chk, bad, unchecked), note
    return chk, sus


# ---- 1. clean mixed batch ------------------------------------------------------
def test_clean_mixed_batch(gpu):
    """Every length with every mask, and 24576-byte stripes until the map has
    more than 100 entries (several pass-1 launches under the small-grid
    build). All words 0 over stale words, nothing counted bad, the stripes
    without a spare shard counted unchecked and not read."""
    shapes = [(L, m) for L in LENGTHS for m in MASKS] + [(24576, m) for m in (R3, R2, R1) * 3]
    b = Ragged(shapes)
    assert b.S == 45 and b.entries() > 100
    assert "rs104_ragged_check_kernel" in kernel_name(b)
    chk, sus = check_batch(rs104(), b, [0] * b.S, "clean")
    assert chk == [0] * b.S
    assert C.unchecked_count(b.masks()) == 12
    # the bit-sliced pick on its own clean batch
    b = Ragged([(8192, ALL), (24576, ALL), (8192, ALL)])
    assert "bit-sliced" in kernel_name(b)
    assert check_batch(rs104(), b, [0] * 3, "clean bit-sliced")[0] == [0] * 3


# ---- 2. single flipped bytes ---------------------------------------------------
@pytest.mark.parametrize("form", ["table", "bit-sliced"])
def test_single_flipped_bytes(gpu, form):
    """One flipped byte per stripe names its shard (r >= 2) or sets bit 31
    (r = 1); the check word has the one bit of a flipped spare shard, or every
    spare bit for a flipped shard of B (no entry of A_m is zero). A flip of
    the byte at shard_len, or in an absent shard, changes nothing."""
    if form == "table":
        cases = flip_cases(LENGTHS, (R4, R3, R2, R1))
    else:
        cases = flip_cases((8192, 24576), (R4,))
    b = Ragged([(L, m) for L, m, _, _ in cases] + ([(1000, R3), (4096 + 16, R2), (16, TEN)] if form == "table" else []))
    want_sus, want_chk = [], []
    for s, (L, m, shard, pos) in enumerate(cases):
        b.flip(s, shard, pos)
        E = C.split(m)[1]
        want_sus.append(UNEXPLAINED if len(E) == 1 else 1 << shard)
        want_chk.append(1 << shard if shard in E else sum(1 << e for e in E))
    if form == "table":
        s = len(cases)
        b.flip(s, 5, 1000)             # the byte at shard_len (slack)
        b.flip(s, 13, 1001)
        b.flip(s + 1, 0, 17)           # an absent shard of lost(0, 12)
        b.flip(s + 1, 12, 4096 + 15)
        b.flip(s + 1, 6, 4096 + 16)    # the byte at shard_len of a second-entry tail
        b.flip(s + 2, 2, 3)            # a stripe that is not read at all
        want_sus += [0, 0, 0]
        want_chk += [0, 0, 0]
    assert ("rs104_bs_ragged_verify_kernel" if form == "bit-sliced" else "rs104_ragged_check_kernel") in kernel_name(b)
    chk, sus = check_batch(rs104(), b, want_sus, form)
    assert chk == want_chk, (hexes(chk), hexes(want_chk))


# ---- 3. no leakage between neighbours ----------------------------------------
@pytest.mark.parametrize("shapes", [[(2048, R2), (4096 + 16, R3), (1000, R4), (24576, R3), (16, R2)],
                                    [(8192, ALL), (24576, ALL), (8192, ALL), (24576, ALL)]],
                         ids=["table", "bit-sliced"])
def test_no_leakage_between_neighbours(gpu, shapes):
    """Only the last chunk of stripe j, or only the first chunk of stripe
    j + 1, corrupt: exactly that stripe's word pair is non-zero (an off-by-one
    in first_block or in the map would move it)."""
    rs = rs104()
    for j in range(len(shapes) - 1):
        for s, pos in ((j, shapes[j][0] - 1), (j + 1, 0)):
            b = Ragged(shapes)
            shard = C.split(shapes[s][1])[0][4]
            b.flip(s, shard, pos)
            want = [0] * b.S
            want[s] = 1 << shard
            chk, sus = check_batch(rs, b, want, (j, s, pos))
            assert [w != 0 for w in chk] == [w != 0 for w in want]


# ---- 4. bad_stripes counts once -----------------------------------------------
@pytest.mark.parametrize("mask", [ALL, R3], ids=["bit-sliced", "table"])
def test_bad_stripes_counts_a_stripe_once(gpu, mask):
    """A flip in each of the six 4 KiB ranges of a 24576-byte stripe (all four
    waves of some, three shards in all): six map entries (three bit-sliced
    ones) report the stripe, bad_stripes gets exactly one."""
    b = Ragged([(8192, mask), (24576, mask), (8192, mask)])
    for k in range(6):
        b.flip(1, (1, 5, 11)[k % 3], 4096 * k + 1024 * (k % 4) + 7 * k)
    b.flip(1, 5, 4096 + 3000)
    want = [0, 1 << 1 | 1 << 5 | 1 << 11, 0]
    chk, sus, bad, unchecked = device_scrub(rs104(), b)
    assert (b.model()[1], sus) == (want, want)
    assert (bad, unchecked) == (1, 0)
    assert device_scrub(rs104(), b, locate=False)[2] == 1


# ---- 5. two wrong shards in one column ------------------------------------------
def test_two_wrong_shards_in_one_column(gpu):
    """r = 4 and r = 3: bit 31, and no shard -- intact or not -- is named."""
    shapes = [(L, m) for m in (R4, R3) for L in (1000, 4096 + 16, 8192)]
    b = Ragged(shapes)
    for s, (L, m) in enumerate(shapes):
        B, E = C.split(m)
        for pos in (0, L // 2, L - 1):
            b.flip(s, B[2], pos, 0x17)
            b.flip(s, (B[7], E[1])[s % 2], pos, 0xC3)
    check_batch(rs104(), b, [UNEXPLAINED] * b.S, "two in a column")


# ---- 6. both picks give the same words ------------------------------------------
def test_both_picks_give_the_same_words(gpu):
    shapes = [(8192, ALL), (24576, ALL), (8192, ALL), (24576, ALL), (8192, ALL)]

    def corrupt(b):
        b.flip(0, 13, 8191)
        b.flip(1, 4, 8192)
        b.flip(1, 4, 24575, 0x80)
        b.flip(3, 0, 12288)
        b.flip(3, 9, 12288)
        b.flip(3, 12, 5)
        return b

    rs = rs104()
    a = corrupt(Ragged(shapes))
    t = corrupt(Ragged(shapes + [(16, ALL)]))
    assert "bit-sliced" in kernel_name(a) and "rs104_ragged_check_kernel" in kernel_name(t)
    chk_a, sus_a = check_batch(rs, a, [1 << 13, 1 << 4, 0, UNEXPLAINED | 1 << 12, 0], "bit-sliced")
    chk_t, sus_t = check_batch(rs, t, [1 << 13, 1 << 4, 0, UNEXPLAINED | 1 << 12, 0, 0], "table")
    assert (chk_t[:5], sus_t[:5]) == (chk_a, sus_a)


# ---- 7. agreement with the strided calls ----------------------------------------
@pytest.mark.parametrize("masks", [[ALL] * 8, [R3, R2, ALL, R1, TEN, R3, R2, NINE]], ids=["full", "mixed"])
def test_agrees_with_the_strided_calls(gpu, masks):
    """A uniform batch, 8 stripes of 8192 bytes, gives the words of the masked
    strided calls; with full masks also hec_gpu_locate_corrupt_batch's, the
    check word its mismatch word shifted left by 10."""
    import torch
    import helyim_amd as H
    rs, S, L = rs104(), 8, 8192
    host = np.stack([clean_stripe(L, s) for s in range(S)]).copy()
    host[1, C.split(masks[1])[0][6], 100] ^= 1
    host[2, 13, 8191] ^= 0x55
    host[3, 4, 0] ^= 9
    host[5, 2, 4096] ^= 3
    host[5, 8, 4096] ^= 3
    host[6, 1, 77] ^= 0xFF
    t = torch.from_numpy(host).cuda()
    descs = [(s * 14 * L, L, L, masks[s]) for s in range(S)]
    md = torch.tensor(np.array(masks, dtype=np.uint32).view(np.int32), device="cuda")
    bad = torch.zeros(4, dtype=torch.int32, device="cuda")
    chk, sus = H.locate_corrupt_ragged(rs, t.view(-1), descs, bad_stripes=bad[0:1], unchecked=bad[1:2])
    chk_s, sus_s = H.locate_corrupt_present_batch(rs, t, md, bad_stripes=bad[2:3], unchecked=bad[3:4])
    only = H.verify_ragged(rs, t.view(-1), descs)
    torch.cuda.synchronize()
    assert chk.tolist() == chk_s.tolist() == only.tolist() and sus.tolist() == sus_s.tolist()
    assert chk.cpu().numpy().view(np.uint32).tolist() == C.check_words(host, masks)
    assert sus.cpu().numpy().view(np.uint32).tolist() == C.suspect_words(host, masks)
    assert bad[0].item() == bad[2].item() > 0 and bad[1].item() == bad[3].item() == C.unchecked_count(masks)
    if masks == [ALL] * S:
        assert "bit-sliced" in H.ragged_scrub_kernel_name(descs)
        mis, sus_f = H.locate_corrupt_batch(rs, t)
        torch.cuda.synchronize()
        assert [w << 10 for w in mis.tolist()] == chk.tolist() and sus_f.tolist() == sus.tolist()
    assert np.array_equal(t.cpu().numpy(), host)


# ---- 8. the repair recipe closes -----------------------------------------------
def test_repair_recipe_closes(gpu):
    """Locate, drop the named shards from the masks on the host, reconstruct:
    verify_ragged with the original masks is clean and every shard holds its
    original bytes."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = rs104()
    shapes = [(L, m) for L, m in zip(LENGTHS * 2, (R4, R3, R2) * 4)]
    b = Ragged(shapes)
    named = []
    for s, (L, m) in enumerate(shapes):
        ids = C.split(m)[0] + C.split(m)[1]
        shard = ids[(5 * s + 2) % len(ids)]  # survivors of B and of E
        named.append(shard)
        for pos in sorted({0, L // 3, L - 1}):
            b.flip(s, shard, pos, 0x99)
    dev = torch.from_numpy(b.arena).cuda()
    chk, sus = H.locate_corrupt_ragged(rs, dev, b.descs())
    torch.cuda.synchronize()
    sus = sus.cpu().numpy().view(np.uint32).tolist()
    assert sus == [1 << c for c in named] == b.model()[1]
    use = [m & ~w for m, w in zip(b.masks(), sus)]
    assert all(bin(u).count("1") >= 10 for u in use)
    left = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_ragged(rs, dev, b.descs(use), bad_stripes=left)
    bad = torch.zeros(2, dtype=torch.int32, device="cuda")
    again = H.verify_ragged(rs, dev, b.descs(), bad_stripes=bad[0:1], unchecked=bad[1:2])
    torch.cuda.synchronize()
    assert again.tolist() == [0] * b.S and bad.tolist() == [0, 0] and left.item() == 0
    whole = Ragged(shapes, present=[ALL] * b.S)  # every shard, the lost ones too, with its original bytes
    assert np.array_equal(dev.cpu().numpy(), whole.arena)
