"""Locate and repair out to two wrong shards per byte column on the GPU:
hec_gpu_locate_corrupt_pairs_batch, hec_gpu_repair_pairs_batch and
hec_locate_corrupt_pairs_ec_files.

Every expected suspects word comes from tests/locate_pairs_model.py (the
result contract by brute force) applied to the arenas as they are, every
expected mismatch word from the C oracle as in tests/test_gpu_verify.py; where
the test built the corruption itself the word is asserted by construction
too. Shards live in tests/footprint.py arenas of seeded random bytes, and
every device call is also a footprint check: the arenas come back byte for
byte (or, for a repair, equal the expected image), the result words at index S
untouched."""
import itertools
import os

import numpy as np
import pytest

import locate_model as M
import locate_pairs_model as PM
import scrub_harness as SH
from scrub_harness import (ALL, BIG_BLOCKS, BIG_SIZE, BLOCK, EDGE, TRIPLE_AT, big_entries, big_volume, bits,
                           clean_case, copies, ec_names, flip_positions, gather, hexes, in_place_layout, oracle_words,
                           shard_of)

pytestmark = pytest.mark.gpu

UNEXPLAINED = PM.UNEXPLAINED
LENGTHS = (8192, 8192 + 2048, 4096 + 16, 1000, 17, 1)
LAYOUTS = (0, 3)  # scrub_harness.layouts: aligned stripe-major with gaps, odd base
PAIRS_CALL, SINGLE_CALL = "hec_gpu_locate_corrupt_pairs_batch", "hec_gpu_locate_corrupt_batch"


def device_locate(call, rs, arenas, stripes, data, par, preset_bad=7):
    """`call` (one of the two locate entry points) on the arenas -> (mismatch
    [S], suspects [S], bad_stripes). Asserts the footprint."""
    (mis, sus), (bad,) = SH.device_words(call, rs, arenas, stripes, data, par, 2, [preset_bad])
    return mis, sus, bad


def check_pairs(rs, work, stripes, data, par, by_construction=None, note=None, single=None):
    """The pairs call on `work` against the model and the oracle; -> the
    suspects words. single: what the existing call must say on the same arenas
    (a list of words, or "same")."""
    shards = gather(work, stripes)
    want_sus = PM.suspect_words(shards)
    want_mis = oracle_words(work, stripes, 10, 4)
    if by_construction is not None:
        assert want_sus == by_construction, (note, hexes(want_sus), hexes(by_construction))
    assert [w != 0 for w in want_mis] == [w != 0 for w in want_sus], note
    mis, sus, bad = device_locate(PAIRS_CALL, rs, work, stripes, data, par)
    assert sus == want_sus, (note, hexes(sus), hexes(want_sus))
    assert mis == want_mis, (note, hexes(mis), hexes(want_mis))
    assert bad == 7 + sum(1 for w in want_mis if w), note
    if single is not None:
        mis1, sus1, bad1 = device_locate(SINGLE_CALL, rs, work, stripes, data, par)
        assert sus1 == (sus if single == "same" else single), (note, hexes(sus1))
        assert sus1 == M.suspect_words(shards), note
        assert (mis1, bad1) == (mis, bad), note
    return sus


# ---- device batches --------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_clean_batch(gpu, L):
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, 5, which)
        mis, sus, bad = device_locate(PAIRS_CALL, rs, copies(arenas), stripes, data, par)
        assert mis == [0] * 5 and sus == [0] * 5, (name, hexes(mis), hexes(sus))
        assert bad == 7, name


@pytest.mark.parametrize("L", LENGTHS)
def test_single_wrong_shards_give_the_existing_words(gpu, L):
    """One flipped byte per stripe (one stripe of each launch clean), and two
    shards wrong in different columns of one stripe: the pairs call and the
    existing call return the same words on the same arenas."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 5
    combos = [((3 * n + 1) % 14, pos) for n, pos in enumerate(flip_positions(L))]
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        for b0 in range(0, len(combos), S - 1):
            batch = combos[b0:b0 + S - 1]
            work = copies(arenas)
            want = [0] * S
            for s, (shard, pos) in zip(range(1, S), batch):
                shard_of(work, stripes, s, shard)[pos] ^= 0x40
                want[s] = 1 << shard
            if L > 1:
                shard_of(work, stripes, 1, 13)[(batch[0][1] + 1) % L] ^= 0x07  # the neighbouring column
                want[1] |= 1 << 13
            check_pairs(rs, work, stripes, data, par, want, (name, batch), single="same")


@pytest.mark.parametrize("L", [17, 8192 + 2048])
def test_all_91_pairs(gpu, L):
    """Stripe s has pair s of the 91 wrong in one byte column: exactly those two
    bits. The existing call gives bit 31 on the same arenas."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = len(PM.PAIRS)
    assert S == 91
    rng = np.random.default_rng(L)
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        work = copies(arenas)
        for s, (a, b) in enumerate(PM.PAIRS):
            pos = (s * 113 + 5) % L
            shard_of(work, stripes, s, a)[pos] ^= int(rng.integers(1, 256))
            shard_of(work, stripes, s, b)[pos] ^= int(rng.integers(1, 256))
        check_pairs(rs, work, stripes, data, par, [bits(a, b) for a, b in PM.PAIRS], name, single=[UNEXPLAINED] * S)


@pytest.mark.parametrize("L", LENGTHS)
def test_pairs_at_every_position(gpu, L):
    """(2,7), (5,12) and (10,13) at every position of interest of every length."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 5
    combos = [(pair, pos) for pair in ((2, 7), (5, 12), (10, 13)) for pos in flip_positions(L)]
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        for b0 in range(0, len(combos), S - 1):
            batch = combos[b0:b0 + S - 1]
            clean_stripe = (b0 // (S - 1)) % S
            targets = [s for s in range(S) if s != clean_stripe][:len(batch)]
            work = copies(arenas)
            want = [0] * S
            for n, (s, ((a, b), pos)) in enumerate(zip(targets, batch)):
                shard_of(work, stripes, s, a)[pos] ^= 0x40 >> n
                shard_of(work, stripes, s, b)[pos] ^= 0x11 * (n + 1)
                want[s] = bits(a, b)
            check_pairs(rs, work, stripes, data, par, want, (name, batch))


@pytest.mark.parametrize("pair", [(0, 9), (4, 12), (11, 13)])
def test_every_error_value(gpu, pair):
    """Stripe v - 1 gets ^= v at byte 16 (the last one, in the tail vector) of
    one shard of the pair and a fixed w on the other; then the roles swapped;
    then v on both."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L, W = 255, 17, 0xA7
    a, b = pair
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        for how in ("v on a", "v on b", "v on both"):
            work = copies(arenas)
            for v in range(1, 256):
                shard_of(work, stripes, v - 1, a)[16] ^= W if how == "v on b" else v
                shard_of(work, stripes, v - 1, b)[16] ^= W if how == "v on a" else v
            check_pairs(rs, work, stripes, data, par, [bits(a, b)] * S, (name, how))


@pytest.mark.parametrize("L", [17, 8192 + 2048])
def test_bytes_of_one_dword_are_independent(gpu, L):
    """The four bytes of one aligned dword hold, in order, a pair, a single
    wrong shard, a clean column and an unexplained triple; then two different
    pairs sit in adjacent bytes. The word is the OR."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(4)
    triple = PM.unexplained_triple(rng)
    o = (L - 1) // 4 * 4 - 4  # 12 at L = 17, 10232 at 10 KiB: the second dword from the end
    assert o % 4 == 0 and o + 4 <= L
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, 5, which)
        work = copies(arenas)
        shard_of(work, stripes, 1, 3)[o] ^= 0x5A
        shard_of(work, stripes, 1, 11)[o] ^= 0xC3
        shard_of(work, stripes, 1, 8)[o + 1] ^= 0x01
        for c, v in triple.items():
            shard_of(work, stripes, 1, c)[o + 3] ^= v
        shard_of(work, stripes, 3, 0)[o + 1] ^= 0x80
        shard_of(work, stripes, 3, 6)[o + 1] ^= 0x7F
        shard_of(work, stripes, 3, 9)[o + 2] ^= 0x02
        shard_of(work, stripes, 3, 13)[o + 2] ^= 0xFF
        want = [0, bits(3, 11, 8) | UNEXPLAINED, 0, bits(0, 6, 9, 13), 0]
        check_pairs(rs, work, stripes, data, par, want, name, single=[0, bits(8) | UNEXPLAINED, 0, UNEXPLAINED, 0])


def test_three_wrong_shards_are_unexplained(gpu):
    """Seeded triples for which the model says bit 31: so does the device."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 60, 17
    rng = np.random.default_rng(3)
    triples = [PM.unexplained_triple(rng) for _ in range(S)]
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        work = copies(arenas)
        for s, errors in enumerate(triples):
            for c, v in errors.items():
                shard_of(work, stripes, s, c)[s % L] ^= v
        check_pairs(rs, work, stripes, data, par, [UNEXPLAINED] * S, name, single="same")


def test_three_wrong_shards_named_as_an_intact_pair(gpu):
    """The documented limit of the contract (include/hec.h): a column with three
    wrong shards that a pair explains. Such a column is found by a search on
    the CPU; the pair holds an intact shard, and the device names it, as the
    model does."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(33)
    triples = np.array(list(itertools.combinations(range(14), 3)))
    n = 20_000  # 0.138 % of them: about 28
    which_t = triples[rng.integers(0, len(triples), n)]
    values = rng.integers(1, 256, (n, 3), dtype=np.uint8)
    syn = np.zeros((4, n), dtype=np.uint8)
    for t in range(3):
        for r in range(4):
            syn[r] ^= PM.MUL[PM.H[r, which_t[:, t]], values[:, t]]
    found = np.flatnonzero(PM.pair_of(syn))
    assert len(found) > 0
    o = int(found[0])
    errors = {int(c): int(v) for c, v in zip(which_t[o], values[o])}
    word = PM.column_word(PM.syndrome_of(errors))
    assert bin(word).count("1") == 2 and word & ~bits(*errors), (errors, hex(word))  # an intact shard is blamed
    S, L = 5, 1000
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        work = copies(arenas)
        for c, v in errors.items():
            shard_of(work, stripes, 2, c)[L - 1] ^= v
        check_pairs(rs, work, stripes, data, par, [0, 0, word, 0, 0], name, single=[0, 0, UNEXPLAINED, 0, 0])


def test_more_items_than_the_grid(gpu):
    """2048 + 5 stripes of one 4 KiB chunk: more items than pass 2's 2048
    workgroups, so some take a second item. Pairs in the first and last stripe
    and on both sides of the cap."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 2048 + 5, 4096
    name, data, par, stripes, arenas = clean_case(10, 4, L, S, 0)
    work = copies(arenas)
    want = [0] * S
    for s, (a, b), pos in ((0, (1, 4), 0), (2047, (11, 12), 4095), (2048, (0, 8), 2049), (2052, (9, 13), 1023)):
        shard_of(work, stripes, s, a)[pos] ^= 0x5A
        shard_of(work, stripes, s, b)[pos] ^= 0x21
        want[s] = bits(a, b)
    check_pairs(rs, work, stripes, data, par, want, name)


def test_python_mirror(gpu):
    """locate_corrupt_pairs_batch, _sep and repair_pairs_batch on torch tensors."""
    import torch
    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    g = torch.Generator(device="cuda").manual_seed(14)
    t = torch.randint(0, 256, (6, 14, 16384), dtype=torch.uint8, device="cuda", generator=g)
    batch.encode_batch(rs, t)
    t[3, 11, 9000] ^= 0x10
    t[3, 4, 9000] ^= 0x99
    t[5, 2, 16383] ^= 0x01
    torch.cuda.synchronize()
    want = PM.suspect_words(t.cpu().numpy())
    assert want == [0, 0, 0, bits(4, 11), 0, bits(2)]
    mis = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    sus = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    out = H.locate_corrupt_pairs_batch(rs, t, mismatch=mis, suspects=sus)
    assert out[0] is mis and out[1] is sus
    assert sus.cpu().tolist() == want and mis.cpu().tolist() == [0, 0, 0, 15, 0, 15]
    data, par = t[:, :10].contiguous(), t[:, 10:].contiguous()
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    m3, s3 = H.locate_corrupt_pairs_batch_sep(rs, data, par, bad_stripes=bad)
    assert s3.cpu().tolist() == want and m3.cpu().tolist() == [0, 0, 0, 15, 0, 15] and int(bad.item()) == 2
    with pytest.raises(ValueError, match="suspects"):
        H.locate_corrupt_pairs_batch(rs, t, suspects=torch.zeros(5, dtype=torch.int32, device="cuda"))
    left = torch.zeros(1, dtype=torch.int32, device="cuda")
    m4, s4, masks = H.repair_pairs_batch(rs, t, unrepaired=left)
    assert s4.cpu().tolist() == want and int(left.item()) == 0
    assert masks.cpu().tolist() == [ALL, ALL, ALL, ALL & ~bits(4, 11), ALL, ALL & ~bits(2)]
    assert H.verify_batch(rs, t).cpu().tolist() == [0] * 6


# ---- repair ----------------------------------------------------------------------
def device_repair(rs, arenas, stripes, layout, expected, preset_left=7):
    return SH.device_repair("hec_gpu_repair_pairs_batch", rs, arenas, stripes, layout, expected, preset_left)


@pytest.mark.parametrize("L", [8192 + 2048, 1000])
def test_repair(gpu, L):
    """Stripe 0: one column names {1, 2} and another {7}: rebuilt to the clean
    original. Stripe 1: two pairs and a single, five shards in all: every bit
    is right, but left byte for byte and counted. Stripe 2: an unexplained
    triple, left alone and counted. Stripe 3 clean; stripe 4 a pair in the last
    column, rebuilt."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 5
    triple = PM.unexplained_triple(np.random.default_rng(5))
    hits = {0: [(1, 40, 0x21), (2, 40, 0x84), (7, L - 2, 0x01)],
            1: [(0, 3, 0x10), (3, 3, 0x20), (5, L // 2, 0x30), (9, L // 2, 0x40), (12, L - 1, 0x50)],
            2: [(c, L // 3, v) for c, v in triple.items()],
            4: [(6, L - 1, 0xFF), (13, L - 1, 0xFF)]}
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        layout = in_place_layout(data, par)
        work = copies(arenas)
        for s, flips in hits.items():
            for shard, pos, value in flips:
                shard_of(work, stripes, s, shard)[pos] ^= value
        want_sus = PM.suspect_words(gather(work, stripes))
        assert want_sus == [bits(1, 2, 7), bits(0, 3, 5, 9, 12), UNEXPLAINED, 0, bits(6, 13)], hexes(want_sus)
        want_mis = oracle_words(work, stripes, 10, 4)
        expected = copies(arenas)
        for s in (1, 2):  # left as corrupted
            for shard, pos, _ in hits[s]:
                shard_of(expected, stripes, s, shard)[pos] = shard_of(work, stripes, s, shard)[pos]
        mis, sus, masks, left, after = device_repair(rs, work, stripes, layout, expected)
        assert sus == want_sus and mis == want_mis, (name, hexes(sus), hexes(mis))
        assert masks == [ALL & ~bits(1, 2, 7), ALL, ALL, ALL, ALL & ~bits(6, 13)], (name, hexes(masks))
        assert left == 7 + 2, name
        assert after == [0, want_mis[1], want_mis[2], 0, 0], (name, hexes(after))
        assert want_mis[1] and want_mis[2]


# ---- shard files -----------------------------------------------------------------
def test_files(gpu, tmp_path):
    """A small volume written by the library itself with small blocks. .ec03
    and .ec11 are corrupted over the same 100-byte run, .ec05 elsewhere: the
    entries equal the model on the file bytes, and the existing file locate
    reports bit 31 for the block of the run."""
    import helyim_amd as H
    base = str(tmp_path / "9")
    large, small = 16 * 1001, 1001
    files = [bytearray(f) for f in SH.library_volume(base, 99, 10 * large * 2 + 10 * small * 7 + 55)]
    size = len(files[0])
    n_blocks = -(-size // BLOCK)
    assert all(len(f) == size for f in files) and n_blocks >= 8 and size % BLOCK
    assert H.locate_corrupt_pairs_ec_files(base, BLOCK) == (n_blocks, 0, [])
    run, x5 = 2 * BLOCK + 700, 6 * BLOCK + 9
    assert run // BLOCK == (run + 99) // BLOCK
    rng = np.random.default_rng(9)
    for shard in (3, 11):
        for o in range(run, run + 100):
            files[shard][o] ^= int(rng.integers(1, 256))
    files[5][x5] ^= 0x5A
    for shard in (3, 5, 11):
        open(base + ".ec%02d" % shard, "wb").write(files[shard])

    def block_words(model, lo):
        return (lo, BLOCK) + SH.block_words(files, lo, lo + BLOCK, M.mismatch_words, model.suspect_words)

    lows = [run // BLOCK * BLOCK, x5 // BLOCK * BLOCK]
    want = [block_words(PM, lo) for lo in lows]
    assert [w[3] for w in want] == [bits(3, 11), bits(5)]
    before = [os.stat(base + ".ec%02d" % i).st_mtime_ns for i in range(14)]
    assert H.locate_corrupt_pairs_ec_files(base, BLOCK) == (n_blocks, 2, want)
    assert H.locate_corrupt_pairs_ec_files(base, BLOCK, cap=1) == (n_blocks, 2, want[:1])
    single = [block_words(M, lo) for lo in lows]
    assert [w[3] for w in single] == [UNEXPLAINED, bits(5)]
    assert H.locate_corrupt_ec_files(base, BLOCK) == (n_blocks, 2, single)
    # nothing was written
    assert [os.stat(base + ".ec%02d" % i).st_mtime_ns for i in range(14)] == before
    # the recipe: three files named in all, bit 31 nowhere -> delete and rebuild them
    for shard in (3, 5, 11):
        os.remove(base + ".ec%02d" % shard)
    assert H.rebuild_ec_files(base) == [3, 5, 11]
    assert H.locate_corrupt_pairs_ec_files(base, BLOCK) == (n_blocks, 0, [])


# ---- shard files longer than the two slots -----------------------------------------
def test_files_longer_than_the_two_slots(gpu, tmp_path):
    """hec_locate_corrupt_pairs_ec_files over three chunks (64 KiB and 1 MiB
    blocks: slot 0 is used twice, its words collected while later chunks are
    in flight) and with a block larger than a chunk: the entries equal the
    model's at every block size, and no file is written."""
    import helyim_amd as H
    good, bad, cols, triple = big_volume(2028)
    base = str(tmp_path / "big")
    for i, name in enumerate(ec_names(base)):
        bad[i].tofile(name)
        os.utime(name, ns=(10**18, 10**18 + i))
    for block in BIG_BLOCKS:
        width = block or 1 << 20  # HEC_SMALL_BLOCK_SIZE
        want = big_entries(PM, bad, cols, width)
        if block == 65536:
            assert [(w[0], w[3]) for w in want] == [
                (0, bits(11)), (EDGE - 65536, bits(2, 13)), (EDGE, bits(2, 13)), (6 << 20, bits(6, 9)),
                ((8 << 20) - 65536, bits(0)), (8 << 20, bits(10)), (TRIPLE_AT // 65536 * 65536, UNEXPLAINED),
                (BIG_SIZE // 65536 * 65536, bits(4))]
            assert want[-1][1] == BIG_SIZE % 65536
        if block == 5 << 20:
            assert [w[:2] for w in want] == [(0, 5 << 20), (5 << 20, BIG_SIZE - (5 << 20))]
        assert H.locate_corrupt_pairs_ec_files(base, block) == (-(-BIG_SIZE // width), len(want), want), hex(block)
    assert [os.stat(name).st_mtime_ns for name in ec_names(base)] == [10**18 + i for i in range(14)]
    assert all(np.array_equal(np.fromfile(name, np.uint8), bad[i]) for i, name in enumerate(ec_names(base)))
