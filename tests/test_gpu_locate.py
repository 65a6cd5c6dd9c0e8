"""Locate and repair on the GPU: hec_gpu_locate_corrupt_batch,
hec_gpu_repair_batch and hec_locate_corrupt_ec_files.

Every expected suspects word comes from tests/locate_model.py (the result
contract by brute force) applied to the arenas as they are, every expected
mismatch word from the C oracle as in tests/test_gpu_verify.py; where the test
built the corruption itself the word is asserted by construction too. Shards
live in tests/footprint.py arenas of seeded random bytes, so a compare at or
past shard_len shows up as a false suspect. Every device call is also a
footprint check: the arenas come back byte for byte (or, for a repair, equal
the expected image), the result words at index S untouched."""
import itertools
import os

import numpy as np
import pytest

import locate_model as M
from oracle import corc
import scrub_harness as SH
from scrub_harness import (ALL, BLOCK, LAUNCH_LIMIT, MASK_ROUND, assert_words, clean_case, copies, expect_words, flip,
                           flip_positions, gather, hexes, in_place_layout, oracle_words, result_words, shard_of)

pytestmark = pytest.mark.gpu

UNEXPLAINED = M.UNEXPLAINED
LENGTHS = (8192, 8192 + 2048, 4096 + 16, 1000, 17, 1)
LAYOUTS = (0, 3)  # scrub_harness.layouts: aligned stripe-major with gaps, odd base


def model_words(arenas, stripes):
    return M.suspect_words(gather(arenas, stripes))


def device_locate(rs, arenas, stripes, data, par, preset_bad=7):
    """hec_gpu_locate_corrupt_batch on the arenas -> (mismatch [S], suspects
    [S], bad_stripes). Asserts the footprint."""
    (mis, sus), (bad,) = SH.device_words("hec_gpu_locate_corrupt_batch", rs, arenas, stripes, data, par, 2,
                                         [preset_bad])
    return mis, sus, bad


def check_locate(rs, work, stripes, data, par, by_construction=None, note=None):
    """Locate on `work` against the model and the oracle; -> the suspects words."""
    want_sus = model_words(work, stripes)
    want_mis = oracle_words(work, stripes, 10, 4)
    if by_construction is not None:
        assert want_sus == by_construction, (note, [hex(w) for w in want_sus], [hex(w) for w in by_construction])
    assert [w != 0 for w in want_mis] == [w != 0 for w in want_sus], note
    mis, sus, bad = device_locate(rs, work, stripes, data, par)
    assert sus == want_sus, (note, [hex(w) for w in sus], [hex(w) for w in want_sus])
    assert mis == want_mis, (note, [hex(w) for w in mis], [hex(w) for w in want_mis])
    assert bad == 7 + sum(1 for w in want_mis if w), note
    return sus


# ---- device batches --------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_clean_batch(gpu, L):
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, 5, which)
        mis, sus, bad = device_locate(rs, copies(arenas), stripes, data, par)
        assert mis == [0] * 5 and sus == [0] * 5, (name, hexes(mis), hexes(sus))
        assert bad == 7, name


@pytest.mark.parametrize("L", LENGTHS)
def test_one_flipped_byte_names_its_shard(gpu, L):
    """One flipped byte per stripe, one stripe of each launch left clean: every
    shard 0..13 at every position of interest, suspects exactly 1 << shard."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 5
    combos = [(shard, pos) for shard in range(14) for pos in flip_positions(L)]
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        for b0 in range(0, len(combos), S - 1):
            batch = combos[b0:b0 + S - 1]
            clean_stripe = (b0 // (S - 1)) % S
            targets = [s for s in range(S) if s != clean_stripe][:len(batch)]
            work = copies(arenas)
            want = [0] * S
            for s, (shard, pos) in zip(targets, batch):
                shard_of(work, stripes, s, shard)[pos] ^= 0x40
                want[s] = 1 << shard
            check_locate(rs, work, stripes, data, par, want, (name, batch))


@pytest.mark.parametrize("shard", [4, 12])
def test_every_error_value(gpu, shard):
    """Stripe v - 1 gets ^= v at byte 16 (the last one, in the tail vector) of
    one shard: all 255 error values name it."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 255, 17
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        work = copies(arenas)
        for v in range(1, 256):
            shard_of(work, stripes, v - 1, shard)[16] ^= v
        check_locate(rs, work, stripes, data, par, [1 << shard] * S, name)


@pytest.mark.parametrize("L", [8192, 8192 + 2048])
def test_many_columns_of_one_shard(gpu, L):
    """Bytes 0, 4095, 4096 and L - 1 of one shard of one stripe: several chunks,
    waves and lanes report, the word is the one bit."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, 5, which)
        for stripe, shard in ((1, 7), (3, 10)):
            work = copies(arenas)
            for n, pos in enumerate((0, 4095, 4096, L - 1)):
                shard_of(work, stripes, stripe, shard)[pos] ^= 0x11 * (n + 1)
            want = [0] * 5
            want[stripe] = 1 << shard
            check_locate(rs, work, stripes, data, par, want, (name, shard))


@pytest.mark.parametrize("L", [8192 + 2048, 1000])
def test_two_shards_in_different_columns(gpu, L):
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, 5, which)
        work = copies(arenas)
        shard_of(work, stripes, 2, 0)[L - 1] ^= 0x80
        shard_of(work, stripes, 2, 13)[3] ^= 0x01
        shard_of(work, stripes, 4, 9)[L // 2] ^= 0xFF
        shard_of(work, stripes, 4, 2)[L // 2 + 1] ^= 0x07   # the neighbouring byte of the same dword
        want = [0, 0, 1 << 0 | 1 << 13, 0, 1 << 9 | 1 << 2]
        check_locate(rs, work, stripes, data, par, want, name)


@pytest.mark.parametrize("size", [2, 3])
def test_same_column_pairs_and_triples_are_unexplained(gpu, size):
    """All 91 pairs / 364 triples of shards wrong in one byte column: exactly
    HEC_SUSPECT_UNEXPLAINED. Then with a single wrong shard in another column
    of every stripe: bit 31 plus that shard."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    groups = list(itertools.combinations(range(14), size))
    S, L = len(groups), 17
    assert S == (91 if size == 2 else 364)
    rng = np.random.default_rng(size)
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        work = copies(arenas)
        for s, group in enumerate(groups):
            for c in group:
                shard_of(work, stripes, s, c)[s % L] ^= int(rng.integers(1, 256))
        check_locate(rs, work, stripes, data, par, [UNEXPLAINED] * S, name)
        want = []
        for s in range(S):
            single = (5 * s + 3) % 14
            shard_of(work, stripes, s, single)[(s + 1 + s % 7) % L] ^= int(rng.integers(1, 256))
            want.append(UNEXPLAINED | 1 << single)
        assert all((s + 1 + s % 7) % L != s % L for s in range(S))
        check_locate(rs, work, stripes, data, par, want, name)


def test_more_items_than_the_grid(gpu):
    """2048 + 5 one-chunk stripes: more items than pass 2's 2048 workgroups, so
    some workgroups take a second item. Flips in the first and last stripe and
    on both sides of the cap."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 2048 + 5, 16
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        work = copies(arenas)
        want = [0] * S
        for s, shard, pos in ((0, 1, 0), (2047, 11, 15), (2048, 8, 7), (2049, 13, 1), (S - 1, 5, 15)):
            shard_of(work, stripes, s, shard)[pos] ^= 0x5A
            want[s] = 1 << shard
        shard_of(work, stripes, 1000, 3)[4] ^= 0x01
        shard_of(work, stripes, 1000, 6)[4] ^= 0x01
        want[1000] = UNEXPLAINED
        check_locate(rs, work, stripes, data, par, want, name)


def test_more_items_than_the_grid_with_three_chunks_per_stripe(gpu):
    """700 stripes of 8 KiB + 16: three chunks per stripe, 2100 items on 2048
    workgroups, and 2048 is no multiple of 3, so a workgroup's second item is
    another chunk index than its first. Flips in chunks 0, 1 and 2 (the 16-byte
    last one) of stripes whose items fall in the first iteration, around the
    cap (item 2048 = stripe 682 chunk 2) and in the last item."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 700, 8192 + 16
    assert -(-L // 4096) == 3 and 2048 < 3 * S and 2048 % 3 != 0
    name, data, par, stripes, arenas = clean_case(10, 4, L, S, 0)
    work = copies(arenas)
    want = [0] * S
    hits = {0: [(2, 5), (2, 4096 + 77), (2, 8192 + 15)],        # items 0, 1, 2
            350: [(11, 4095), (11, 4096), (11, 8192)],
            682: [(7, 8192 + 3)],                               # item 2048: the first second-iteration item
            683: [(0, 0), (0, 8191), (0, L - 1)],               # items 2049, 2050, 2051
            698: [(13, 4097)],                                  # item 2095
            699: [(9, L - 1)]}                                  # item 2099, the last
    for s, flips in hits.items():
        for shard, pos in flips:
            shard_of(work, stripes, s, shard)[pos] ^= 0x3C
        want[s] = 1 << flips[0][0]
    # one chunk of a stripe unexplained, another naming a shard
    shard_of(work, stripes, 690, 4)[8192 + 1] ^= 0x01
    shard_of(work, stripes, 690, 5)[8192 + 1] ^= 0x02
    shard_of(work, stripes, 690, 12)[100] ^= 0x80
    want[690] = UNEXPLAINED | 1 << 12
    check_locate(rs, work, stripes, data, par, want, name)


def test_encode_then_locate_in_stream_order(gpu):
    """encode_batch then locate_corrupt_batch on one non-default stream with no
    synchronise between: the parity slots start as random bytes, so a locate
    that ran early would flag every stripe. Then the Python mirror's shapes."""
    import torch
    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    g = torch.Generator(device="cuda").manual_seed(12)
    t = torch.randint(0, 256, (6, 14, 16384), dtype=torch.uint8, device="cuda", generator=g)
    mis = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    sus = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    batch.encode_batch(rs, t, stream=s)
    out = H.locate_corrupt_batch(rs, t, mismatch=mis, suspects=sus, stream=s)
    s.synchronize()
    assert out[0] is mis and out[1] is sus
    assert mis.cpu().tolist() == [0] * 6 and sus.cpu().tolist() == [0] * 6
    t[3, 11, 9000] ^= 0x10
    t[5, 2, 16383] ^= 0x01
    torch.cuda.synchronize()
    want = M.suspect_words(t.cpu().numpy())
    assert want == [0, 0, 0, 1 << 11, 0, 1 << 2]
    m2, s2 = H.locate_corrupt_batch(rs, t)
    assert s2.cpu().tolist() == want and m2.cpu().tolist() == [0, 0, 0, 2, 0, 15]
    data, par = t[:, :10].contiguous(), t[:, 10:].contiguous()
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    m3, s3 = H.locate_corrupt_batch_sep(rs, data, par, bad_stripes=bad)
    assert s3.cpu().tolist() == want and m3.cpu().tolist() == [0, 0, 0, 2, 0, 15] and int(bad.item()) == 2
    with pytest.raises(ValueError, match="suspects"):
        H.locate_corrupt_batch(rs, t, suspects=torch.zeros(5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        H.locate_corrupt_batch(rs, t, mismatch=torch.zeros(6, dtype=torch.int64, device="cuda"))
    # repair through the mirror: both stripes come back clean
    left = torch.zeros(1, dtype=torch.int32, device="cuda")
    m4, s4, masks = H.repair_batch(rs, t, unrepaired=left)
    assert s4.cpu().tolist() == want and int(left.item()) == 0
    assert masks.cpu().tolist() == [ALL, ALL, ALL, ALL & ~(1 << 11), ALL, ALL & ~(1 << 2)]
    assert H.verify_batch(rs, t).cpu().tolist() == [0] * 6


# ---- repair ----------------------------------------------------------------------
def device_repair(rs, arenas, stripes, layout, expected, preset_left=7):
    return SH.device_repair("hec_gpu_repair_batch", rs, arenas, stripes, layout, expected, preset_left)


def expected_masks(sus):
    return [ALL & ~w if not w & UNEXPLAINED and 1 <= bin(w & ALL).count("1") <= 4 else ALL for w in sus]


@pytest.mark.parametrize("L", [8192 + 2048, 1000])
def test_repair(gpu, L):
    """Stripes with 1, 2 and 4 wrong shards (each in columns of its own) are
    rebuilt to the clean originals; the stripe with a same-column pair stays
    byte for byte as corrupted and is the one counted; the clean stripe and
    every gap are untouched."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 6
    hits = {0: [(3, 0), (3, L - 1), (3, L // 3)],
            1: [(0, 5), (13, L - 2)],
            2: [(2, 1), (7, L - 1), (10, 40), (12, L // 2)],
            3: [(5, 77), (11, 77)],            # a pair in one column: not repairable
            5: [(11, L - 1)]}                  # stripe 4 stays clean
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        layout = in_place_layout(data, par)
        work = copies(arenas)
        for s, flips in hits.items():
            for n, (shard, pos) in enumerate(flips):
                shard_of(work, stripes, s, shard)[pos] ^= 0x21 + n
        want_sus = model_words(work, stripes)
        assert want_sus == [1 << 3, 1 << 0 | 1 << 13, 1 << 2 | 1 << 7 | 1 << 10 | 1 << 12, UNEXPLAINED, 0, 1 << 11]
        want_mis = oracle_words(work, stripes, 10, 4)
        expected = copies(arenas)
        for shard, pos in hits[3]:
            shard_of(expected, stripes, 3, shard)[pos] = shard_of(work, stripes, 3, shard)[pos]
        mis, sus, masks, left, after = device_repair(rs, work, stripes, layout, expected)
        assert sus == want_sus and mis == want_mis, (name, hexes(sus), hexes(mis))
        assert masks == expected_masks(want_sus), (name, hexes(masks))
        assert masks[3] == ALL and masks[4] == ALL and masks[2] == ALL & ~(1 << 2 | 1 << 7 | 1 << 10 | 1 << 12)
        assert left == 7 + 1, name
        assert after == [0, 0, 0, want_mis[3], 0, 0], (name, hexes(after))


def test_repair_leaves_five_suspects_alone(gpu):
    """Five shards wrong in five different columns: every bit is right, but a
    stripe has only four parity shards, so it is left alone and counted."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 3, 1000
    name, data, par, stripes, arenas = clean_case(10, 4, L, S, 0)
    layout = in_place_layout(data, par)
    work = copies(arenas)
    five = (1, 4, 8, 10, 13)
    for n, shard in enumerate(five):
        shard_of(work, stripes, 1, shard)[100 * n + 9] ^= 0x80 >> n
    want_sus = model_words(work, stripes)
    assert want_sus == [0, sum(1 << c for c in five), 0]
    mis, sus, masks, left, after = device_repair(rs, work, stripes, layout, copies(work))
    assert sus == want_sus and masks == [ALL] * 3 and left == 8
    assert after == mis == oracle_words(work, stripes, 10, 4) and after[1] != 0


# ---- big batches: built, corrupted and compared on the device ----------------------
def edge_hits(edge):
    """stripe -> (flips [(shard, pos, value)], suspects word by construction)
    of a batch of edge + 5 stripes of 16 bytes: one-shard flips (repaired) in
    the first and last stripe, on both sides of a wave and of `edge`; two
    shards in two columns (both repaired); same-column pairs and five wrong
    shards (left alone) on both sides of `edge` and in the last, partial wave."""
    S = edge + 5
    assert edge % 64 == 0 and edge // 2 > 1000
    return {
        0: ([(2, 7, 0x21)], 1 << 2),
        255: ([(13, 0, 0x01)], 1 << 13),
        256: ([(11, 15, 0x80)], 1 << 11),
        1000: ([(1, 0, 0x80), (4, 3, 0x40), (8, 6, 0x20), (10, 9, 0x10), (13, 12, 0x08)],
               1 << 1 | 1 << 4 | 1 << 8 | 1 << 10 | 1 << 13),
        edge // 2 + 1: ([(0, 2, 0x5A), (12, 9, 0x5A)], 1 << 0 | 1 << 12),
        edge - 2: ([(4, 5, 0x33), (8, 5, 0x44)], UNEXPLAINED),
        edge - 1: ([(9, 3, 0xFF)], 1 << 9),
        edge: ([(1, 8, 0x10)], 1 << 1),
        edge + 1: ([(0, 11, 0x07), (13, 11, 0x70)], UNEXPLAINED),
        S - 3: ([(6, 9, 0x11), (12, 9, 0x22)], UNEXPLAINED),
        S - 2: ([(3, 1, 0x01), (3, 14, 0xFE)], 1 << 3),
        S - 1: ([(10, 15, 0x42)], 1 << 10),
    }


def locate_and_repair_big(edge):
    """hec_gpu_locate_corrupt_batch, then hec_gpu_repair_batch, over edge + 5
    stripes of 16 bytes with edge_hits' corruption. Expected words of the dirty
    stripes from locate_model on those stripes, and by construction; every
    other stripe is a codeword of gfref's torch twin, so its words are zero
    and its mask 0x3FFF: whole arrays and the whole image are compared on the
    device."""
    import torch
    import gfref
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = edge + 5, 16
    hits = edge_hits(edge)
    order = sorted(hits)
    idx = torch.tensor(order, device="cuda")
    expected = gfref.device_codewords(10, 4, S, L, seed=edge + 1)
    t = expected.clone()
    for s in order:
        for shard, pos, value in hits[s][0]:
            t[s, shard, pos] ^= value
    dirty = t[idx].cpu().numpy()
    want_sus, want_mis = M.suspect_words(dirty), M.mismatch_words(dirty)
    assert want_sus == [hits[s][1] for s in order], hexes(want_sus)
    assert all(want_mis)
    want_masks = expected_masks(want_sus)
    kept = [n for n, m in enumerate(want_masks) if m == ALL]  # dirty and left alone
    assert [order[n] for n in kept] == [1000, edge - 2, edge + 1, S - 3]
    sus_want, mis_want = expect_words(S, idx, want_sus), expect_words(S, idx, want_mis)
    masks_want = expect_words(S, idx, want_masks, rest=ALL)
    before = int(t.view(torch.int64).sum().item())

    mis, sus = result_words(2, S)
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    H.locate_corrupt_batch(rs, t, mismatch=mis, suspects=sus, bad_stripes=bad)
    torch.cuda.synchronize()
    assert_words(mis, mis_want, "mismatch")
    assert_words(sus, sus_want, "suspects")
    assert int(bad.item()) == 7 + len(order)
    assert int(t.view(torch.int64).sum().item()) == before  # nothing written: one reduction over every byte

    kept_idx = idx[torch.tensor(kept, device="cuda")]
    expected[kept_idx] = t[kept_idx]
    mis, sus, masks = result_words(3, S)
    left = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    H.repair_batch(rs, t, mismatch=mis, suspects=sus, present_masks=masks, unrepaired=left)
    torch.cuda.synchronize()
    assert_words(mis, mis_want, "mismatch of the repair")
    assert_words(sus, sus_want, "suspects of the repair")
    assert_words(masks, masks_want, "present masks")
    assert int(left.item()) == 7 + len(kept)
    if not torch.equal(t, expected):
        wrong = torch.nonzero((t != expected).flatten(1).any(dim=1)).flatten()
        pytest.fail(f"image: {wrong.numel()} wrong stripes, the first {wrong[:8].cpu().tolist()}")
    # the proof: every stripe but the ones left alone verifies clean
    ver, = result_words(1, S)
    H.verify_batch(rs, t, mismatch=ver)
    torch.cuda.synchronize()
    assert_words(ver, expect_words(S, kept_idx, [want_mis[n] for n in kept]), "verify after the repair")
    del t, expected
    torch.cuda.empty_cache()


def test_repair_second_mask_round(gpu):
    """2^19 + 5 stripes (117 MB): repair_masks_kernel runs 2048 workgroups of
    256 lanes, so the stripes from 2^19 on are its second round, the last five
    in a partial wave whose ballot counts the stripes left alone."""
    locate_and_repair_big(MASK_ROUND)


def test_locate_and_repair_past_one_launch(gpu):
    """2^23 + 5 stripes (1.9 GB and one clone): rs104_locate_kernel's loop far
    past 2^23 items, the mask kernel's 17th round, and the second stripe range
    of the reconstruct, driven by the masks written just before."""
    locate_and_repair_big(LAUNCH_LIMIT)


# ---- shard files -----------------------------------------------------------------
@pytest.fixture(scope="module")
def shard_files(tmp_path_factory):
    """Oracle-written shard files of a seeded .dat (as test_gpu_verify's): each
    shard 250250 bytes, not a multiple of the 4096-byte block."""
    d = tmp_path_factory.mktemp("locate")
    base = str(d / "7")
    large, small = 64 * 1001, 1001
    files = SH.oracle_volume(base, 77, large, small, 123)
    size = len(files[0])
    assert all(len(f) == size for f in files) and size % BLOCK > 1
    return base, files, size


def block_words(files, lo, hi):
    """(mismatch, suspects) of the column block [lo, hi) by the model."""
    return SH.block_words(files, lo, hi, M.mismatch_words, M.suspect_words)


def test_files_locate_then_rebuild(gpu, shard_files, tmp_path):
    import helyim_amd as H
    src, files, size = shard_files
    base = str(tmp_path / "v")
    for i, f in enumerate(files):
        open(base + ".ec%02d" % i, "wb").write(f)
    n_blocks = -(-size // BLOCK)
    assert H.locate_corrupt_ec_files(base, BLOCK) == (n_blocks, 0, [])
    x7, x12 = 5 * BLOCK + 1234, 9 * BLOCK + 17
    flip(base, 7, x7)
    flip(base, 12, x12)
    now = [bytearray(f) for f in files]
    now[7][x7] ^= 0x5A
    now[12][x12] ^= 0x5A
    for i in range(14):
        os.utime(base + ".ec%02d" % i, ns=(10**18, 10**18 + i))
    before = [os.stat(base + ".ec%02d" % i).st_mtime_ns for i in range(14)]
    want = []
    for x in (x7, x12):
        lo = x // BLOCK * BLOCK
        want.append((lo, BLOCK) + block_words(now, lo, lo + BLOCK))
    assert [w[3] for w in want] == [1 << 7, 1 << 12] and want[1][2] == 1 << 2
    assert H.locate_corrupt_ec_files(base, BLOCK) == (n_blocks, 2, want)
    assert H.locate_corrupt_ec_files(base, BLOCK, cap=1) == (n_blocks, 2, want[:1])
    assert H.locate_corrupt_ec_files(base, BLOCK, cap=0) == (n_blocks, 2, [])
    assert H.verify_ec_files(base, BLOCK) == (n_blocks, 2, [w[:3] for w in want])
    # 8 KiB blocks: pass 1 runs bit-sliced on the whole blocks; one 1 MiB block names both files
    got = H.locate_corrupt_ec_files(base, 2 * BLOCK)
    assert [(b[0], b[3]) for b in got[2]] == [(x7 // 8192 * 8192, 1 << 7), (x12 // 8192 * 8192, 1 << 12)]
    assert H.locate_corrupt_ec_files(base) == (1, 1, [(0, size) + block_words(now, 0, size)])
    assert block_words(now, 0, size)[1] == 1 << 7 | 1 << 12
    # nothing was written
    assert [os.stat(base + ".ec%02d" % i).st_mtime_ns for i in range(14)] == before
    assert [open(base + ".ec%02d" % i, "rb").read() for i in range(14)] == [bytes(f) for f in now]
    # the use of the result: delete the named file, rebuild it from the others
    os.remove(base + ".ec07")
    assert H.rebuild_ec_files(base) == [7]
    assert open(base + ".ec07", "rb").read() == files[7]
    assert H.verify_ec_files(base, BLOCK) == (n_blocks, 1, [want[1][:3]])
    assert H.locate_corrupt_ec_files(base, BLOCK) == (n_blocks, 1, [want[1]])


def test_files_longer_than_the_two_slots(gpu, tmp_path):
    """Shards of 8 MiB and a ragged rest: three chunks of the scrub's 4 MiB
    column range, both pinned slots reused, a flip in the last, short block,
    and one block with a same-column pair."""
    import helyim_amd as H
    block, size = 65536, (8 << 20) + 300_000 + 7
    rng = np.random.default_rng(2025)
    bufs = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(10)] + [np.zeros(size, np.uint8) for _ in range(4)]
    corc.CReedSolomon(10, 4).encode(bufs)
    hits = [(11, 5), (2, (4 << 20) - 1), (13, (4 << 20)), (6, (6 << 20) + 99), (9, (6 << 20) + 99),
            (10, (8 << 20) + 12345), (4, size - 1)]
    for shard, off in hits:
        bufs[shard][off] ^= 0x33
    syn = M.syndromes(np.stack(bufs))
    base = str(tmp_path / "big")
    for i in range(14):
        bufs[i].tofile(base + ".ec%02d" % i)
    # 5 MiB blocks are larger than a chunk's 4 MiB: one block per chunk, and the
    # last chunk is a short block alone, whose words are the slot's first
    for block in (65536, 5 << 20):
        want = []
        for lo in sorted({off // block * block for _, off in hits}):
            hi = min(lo + block, size)
            s = syn[:, lo:hi]
            want.append((lo, hi - lo, sum(1 << j for j in range(4) if s[j].any()), M.syndrome_word(s)))
        if block == 65536:
            assert [w[3] for w in want] == [1 << 11, 1 << 2, 1 << 13, UNEXPLAINED, 1 << 10, 1 << 4]
        else:
            assert [w[3] for w in want] == [1 << 11 | 1 << 2 | 1 << 13, UNEXPLAINED | 1 << 10 | 1 << 4]
        assert want[-1][:2] == (size // block * block, size % block)
        assert H.locate_corrupt_ec_files(base, block) == (-(-size // block), len(want), want), block
