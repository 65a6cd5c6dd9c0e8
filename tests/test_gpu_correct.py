"""Correct in place, per byte column, on the GPU: hec_gpu_correct_batch,
hec_gpu_correct_pairs_batch, hec_correct_ec_files and
hec_correct_pairs_ec_files.

Every expected image, suspects word and byte count comes from
tests/correct_model.py (the contract by brute force) applied to the arenas as
they are, every expected mismatch word from the C oracle as in
tests/test_gpu_verify.py. The arenas, layouts and helpers are those of
tests/scrub_harness.py, and every device call is also a footprint
check: the arenas afterwards equal the model's image byte for byte -- slack,
gaps and the bytes past shard_len included -- and result word S is untouched."""
import os

import numpy as np
import pytest

import correct_model as CM
import locate_model as M
import locate_pairs_model as PM
import scrub_harness as SH
from scrub_harness import (ALL, BIG_BLOCKS, BIG_SIZE, EDGE, NEIGHBOURS, RUN, SINGLES, TRIPLE_AT, UNEXPLAINED,
                           big_entries, big_volume, bits, clean_case, copies, ec_names, flip_positions, gather, hexes,
                           in_place_layout, oracle_words, shard_of)

pytestmark = pytest.mark.gpu

LENGTHS = (8192, 8192 + 2048, 4096 + 16, 1000, 17, 1)
LAYOUTS = (0, 3)  # scrub_harness.layouts: aligned stripe-major with gaps, odd base
BAD0, UNC0, BYTES0 = 7, 5, 11  # presets of the three accumulated counters


def device_correct(rs, arenas, stripes, data, par, expected, pairs):
    """One of the two calls on the arenas -> (mismatch [S], suspects [S],
    bad_stripes, uncorrected, corrected_bytes). Asserts that the arenas
    afterwards equal `expected` in every byte."""
    call = "hec_gpu_correct_pairs_batch" if pairs else "hec_gpu_correct_batch"
    (mis, sus), (bad, unc, nbytes) = SH.device_words(call, rs, arenas, stripes, data, par, 2, [BAD0, UNC0, BYTES0],
                                                     wide_last=True, expected=expected,
                                                     note="pairs" if pairs else "single")
    return mis, sus, bad, unc, nbytes


def model_image(work, stripes, pairs):
    """correct_model on the arenas -> (expected arenas, suspects, bytes changed)."""
    image, _, suspects, changed = CM.correct(gather(work, stripes), pairs)
    expected = copies(work)
    for s in range(len(stripes)):
        for i in range(14):
            shard_of(expected, stripes, s, i)[:] = image[s, i]
    return expected, suspects, changed


def check_correct(rs, work, stripes, data, par, pairs, note=None, want_sus=None, restored=None):
    """The call on `work` against the model and the oracle -> the expected
    arenas. want_sus: the words by construction; restored: arenas the result
    must equal as a whole (the clean original)."""
    expected, sus_model, changed = model_image(work, stripes, pairs)
    want_mis = oracle_words(work, stripes, 10, 4)
    if want_sus is not None:
        assert sus_model == want_sus, (note, hexes(sus_model), hexes(want_sus))
    if restored is not None:
        assert all(np.array_equal(e, r) for e, r in zip(expected, restored)), note
    mis, sus, bad, unc, nbytes = device_correct(rs, copies(work), stripes, data, par, expected, pairs)
    assert sus == sus_model, (note, pairs, hexes(sus), hexes(sus_model))
    assert mis == want_mis, (note, pairs, hexes(mis), hexes(want_mis))
    assert bad == BAD0 + sum(1 for w in want_mis if w), (note, pairs)
    assert unc == UNC0 + sum(1 for w in sus_model if w & UNEXPLAINED), (note, pairs, unc)
    assert nbytes == BYTES0 + changed, (note, pairs, nbytes, changed)
    return expected


# ---- device batches --------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_clean_batch(gpu, L):
    """Nothing is written, the words are 0 and the counters keep their presets."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, 5, which)
        for pairs in (False, True):
            got = device_correct(rs, copies(arenas), stripes, data, par, arenas, pairs)
            assert got == ([0] * 5, [0] * 5, BAD0, UNC0, BYTES0), (name, pairs, got)


@pytest.mark.parametrize("L", LENGTHS)
def test_one_flipped_byte_in_every_shard(gpu, L):
    """One flipped byte per stripe (one stripe of each launch clean), in every
    shard 0..13 at every position of interest -- the last byte and, on the odd
    base, the tail vector among them: the arenas equal the original, the words
    are locate's, and corrected_bytes counts the flips."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 5
    combos = [(shard, pos) for pos in flip_positions(L) for shard in range(14)]
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        for n, b0 in enumerate(range(0, len(combos), S - 1)):
            batch = combos[b0:b0 + S - 1]
            clean_stripe = n % S
            targets = [s for s in range(S) if s != clean_stripe][:len(batch)]
            work = copies(arenas)
            want = [0] * S
            for k, (s, (shard, pos)) in enumerate(zip(targets, batch)):
                shard_of(work, stripes, s, shard)[pos] ^= (0x01, 0xFF, 0x40, 0x9C)[k]
                want[s] = 1 << shard
            check_correct(rs, work, stripes, data, par, bool(n % 2), (name, batch), want, restored=arenas)


@pytest.mark.parametrize("L", [8192 + 2048, 1000])
def test_five_shards_at_five_offsets(gpu, L):
    """Scattered bit rot: five shards of stripe 1 each carry one wrong byte at
    five different offsets. hec_gpu_repair_batch leaves the stripe byte for
    byte and counts it; hec_gpu_correct_batch restores the original."""
    import torch
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 5
    hits = [(0, 3, 0x10), (4, L // 3, 0xFF), (9, L // 2, 0x01), (10, L - 1, 0x80), (13, L - 17, 0x5A)]
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        layout = in_place_layout(data, par)
        work = copies(arenas)
        for shard, pos, value in hits:
            shard_of(work, stripes, 1, shard)[pos] ^= value
        named = bits(*(h[0] for h in hits))
        # the repair on a copy: left alone, unrepaired + 1
        _, sus, masks, left, _ = SH.device_repair("hec_gpu_repair_batch", rs, copies(work), stripes, layout, work)
        assert sus == [0, named, 0, 0, 0] and left == 7 + 1, name
        assert masks == [ALL] * S, name
        # the correct
        for pairs in (False, True):
            check_correct(rs, work, stripes, data, par, pairs, name, [0, named, 0, 0, 0], restored=arenas)


@pytest.mark.parametrize("L", [17, 8192 + 2048])
def test_all_91_pairs_with_singles_elsewhere(gpu, L):
    """Stripe s has pair s of the 91 (shard 0 in thirteen of them) wrong in one
    column and a single wrong shard in another. The single call leaves the
    pair's column, sets bit 31, fixes the single and counts every stripe into
    uncorrected; the pairs call restores everything."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = len(PM.PAIRS)
    rng = np.random.default_rng(L)
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        work = copies(arenas)
        left = copies(arenas)  # what the single call must leave: the pairs' columns
        want1, want2 = [], []
        for s, (a, b) in enumerate(PM.PAIRS):
            pos = (s * 113 + 5) % L
            va, vb = (0xFF, 0x01) if s % 7 == 0 else (int(rng.integers(1, 256)), int(rng.integers(1, 256)))
            for arr in (work, left):
                shard_of(arr, stripes, s, a)[pos] ^= va
                shard_of(arr, stripes, s, b)[pos] ^= vb
            c = (s * 5) % 14
            shard_of(work, stripes, s, c)[(pos + 1 + s % 3) % L] ^= int(rng.integers(1, 256))
            want1.append(bits(c) | UNEXPLAINED)
            want2.append(bits(*{a, b, c}))
        expected = check_correct(rs, work, stripes, data, par, False, name, want1)
        assert all(np.array_equal(e, r) for e, r in zip(expected, left)), name
        check_correct(rs, work, stripes, data, par, True, name, want2, restored=arenas)


@pytest.mark.parametrize("L", [8192 + 2048, 17])
def test_unexplained_triples_stay_and_count_once(gpu, L):
    """Three wrong shards in one column, chosen so that the model says bit 31,
    in several columns of stripe 2 that different waves and chunks hold, plus
    explainable columns in the same stripe: both calls leave the triples'
    columns, fix the others, and count the stripe into uncorrected once."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(6)
    triple_at = sorted({p % L for p in (5, 1024 + 5, 4096 + 7, 8192 + 2047)})
    triples = [PM.unexplained_triple(rng) for _ in triple_at]
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, 5, which)
        work = copies(arenas)
        left = copies(arenas)
        for pos, errors in zip(triple_at, triples):
            for c, v in errors.items():
                for arr in (work, left):
                    shard_of(arr, stripes, 2, c)[pos] ^= v
        free = [p for p in range(L) if p not in triple_at]
        shard_of(work, stripes, 2, 7)[free[free.index(triple_at[0] - 1) + 1]] ^= 0x3C  # the next free column
        shard_of(work, stripes, 2, 12)[free[-1]] ^= 0xFF                                # the last byte
        shard_of(work, stripes, 4, 0)[0] ^= 0x01
        want = [0, 0, bits(7, 12) | UNEXPLAINED, 0, bits(0)]
        for pairs in (False, True):
            expected = check_correct(rs, work, stripes, data, par, pairs, name, want)
            assert all(np.array_equal(e, r) for e, r in zip(expected, left)), name


def test_runs_and_a_whole_shard(gpu):
    """A 4 KiB run wrong in one shard (stripe 0) and in two shards at the same
    offset (stripe 1); a whole shard wrong (stripe 3), at L = 8192."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    L, S = 8192, 5
    rng = np.random.default_rng(8)
    for which in LAYOUTS:
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        work = copies(arenas)
        shard_of(work, stripes, 0, 6)[2048:2048 + 4096] ^= rng.integers(1, 256, 4096, dtype=np.uint8)
        shard_of(work, stripes, 1, 0)[4000:4000 + 4096] ^= rng.integers(1, 256, 4096, dtype=np.uint8)
        shard_of(work, stripes, 1, 11)[4000:4000 + 4096] ^= rng.integers(1, 256, 4096, dtype=np.uint8)
        shard_of(work, stripes, 3, 3)[:] ^= rng.integers(1, 256, L, dtype=np.uint8)
        check_correct(rs, work, stripes, data, par, False, name, [bits(6), UNEXPLAINED, 0, bits(3), 0])
        check_correct(rs, work, stripes, data, par, True, name, [bits(6), bits(0, 11), 0, bits(3), 0],
                      restored=arenas)


def test_more_items_than_the_grid(gpu):
    """2048 + 5 stripes of one 4 KiB chunk with scattered damage: more items
    than pass 2's 2048 workgroups, so some take a second item."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 2048 + 5, 4096
    name, data, par, stripes, arenas = clean_case(10, 4, L, S, 0)
    work = copies(arenas)
    rng = np.random.default_rng(2053)
    want = [0] * S
    for s in sorted({0, 1, 2047, 2048, 2052} | {int(x) for x in rng.integers(0, S, 40)}):
        a, b = (int(x) for x in rng.choice(14, 2, replace=False))
        pos = int(rng.integers(0, L))
        shard_of(work, stripes, s, a)[pos] ^= int(rng.integers(1, 256))
        shard_of(work, stripes, s, b)[pos] ^= int(rng.integers(1, 256))
        c = int(rng.integers(0, 14))
        shard_of(work, stripes, s, c)[(pos + 100) % L] ^= int(rng.integers(1, 256))
        want[s] = bits(*{a, b, c})
    check_correct(rs, work, stripes, data, par, True, name, want, restored=arenas)


def test_python_mirror(gpu):
    """correct_batch and correct_batch_sep on torch tensors."""
    import torch
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    g = torch.Generator(device="cuda").manual_seed(15)
    t = torch.randint(0, 256, (6, 14, 16384), dtype=torch.uint8, device="cuda", generator=g)
    from helyim_amd import batch
    batch.encode_batch(rs, t)
    good = t.clone()
    t[3, 11, 9000] ^= 0x10
    t[3, 4, 9000] ^= 0x99
    t[5, 2, 16383] ^= 0x01
    t[5, 13, 0] ^= 0x80
    bad_t = t.clone()
    torch.cuda.synchronize()
    unc = torch.zeros(1, dtype=torch.int32, device="cuda")
    nbytes = torch.zeros(1, dtype=torch.int64, device="cuda")
    mis, sus = H.correct_batch(rs, t, uncorrected=unc, corrected_bytes=nbytes)
    assert sus.cpu().numpy().view(np.uint32).tolist() == [0, 0, 0, UNEXPLAINED, 0, bits(2, 13)]
    assert mis.cpu().tolist() == [0, 0, 0, 15, 0, 15]
    assert (int(unc.item()), int(nbytes.item())) == (1, 2)
    assert torch.equal(t[5], good[5]) and torch.equal(t[3], bad_t[3])
    mis, sus = H.correct_batch(rs, t, uncorrected=unc, corrected_bytes=nbytes, pairs=True)
    assert sus.cpu().tolist() == [0, 0, 0, bits(4, 11), 0, 0]
    assert (int(unc.item()), int(nbytes.item())) == (1, 4) and torch.equal(t, good)
    data, par = bad_t[:, :10].contiguous(), bad_t[:, 10:].contiguous()
    count = torch.zeros(1, dtype=torch.int32, device="cuda")
    m3, s3 = H.correct_batch_sep(rs, data, par, bad_stripes=count, pairs=True)
    assert s3.cpu().tolist() == [0, 0, 0, bits(4, 11), 0, bits(2, 13)] and int(count.item()) == 2
    assert torch.equal(data, good[:, :10]) and torch.equal(par, good[:, 10:])
    assert H.verify_batch(rs, t).cpu().tolist() == [0] * 6
    with pytest.raises(ValueError, match="corrected_bytes"):
        H.correct_batch(rs, t, corrected_bytes=torch.zeros(1, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="suspects"):
        H.correct_batch(rs, t, suspects=torch.zeros(5, dtype=torch.int32, device="cuda"))


# ---- shard files -----------------------------------------------------------------
BLOCK = 4096


def names(base):
    return [base + ".ec%02d" % i for i in range(14)]


def test_files(gpu, tmp_path):
    """A small volume written by the library itself, with a short last block.
    Five files get one flipped byte each at five offsets of block 1; two files
    the same 4 KiB run wrong (blocks 3 and 4); one column of block 7 three
    wrong files the model calls unexplained; the short last block one flipped
    byte. After hec_correct_pairs_ec_files every file equals its original
    except the triple's column, the entries are the pair locate's from before,
    and a second scrub reports the triple's block alone. The single form on the
    same damage also leaves the run."""
    import helyim_amd as H
    from oracle import corc
    base = str(tmp_path / "9")
    large, small = 16 * 1001, 1001
    open(base + ".dat", "wb").write(corc.splitmix64_bytes(77, 10 * large * 2 + 10 * small * 7 + 55).tobytes())
    H.generate_ec_files(base, small, large, small)
    good = [open(n, "rb").read() for n in names(base)]
    size = len(good[0])
    n_blocks = -(-size // BLOCK)
    assert all(len(f) == size for f in good) and n_blocks >= 9 and size % BLOCK
    assert H.correct_ec_files(base, BLOCK, pairs=True) == (n_blocks, 0, [])
    assert [open(n, "rb").read() for n in names(base)] == good

    rng = np.random.default_rng(9)
    bad = [bytearray(f) for f in good]
    five = [(0, BLOCK + 1), (3, BLOCK + 700), (8, BLOCK + 2048), (10, 2 * BLOCK - 1), (12, BLOCK + 4000)]
    for shard, o in five:
        bad[shard][o] ^= 0x40
    run = 3 * BLOCK + 100
    for shard in (2, 13):
        for o in range(run, run + 4096):
            bad[shard][o] ^= int(rng.integers(1, 256))
    triple, t_at = PM.unexplained_triple(rng), 7 * BLOCK + 9
    for c, v in triple.items():
        bad[c][t_at] ^= v
    last = size - 1
    assert last // BLOCK == n_blocks - 1 and last // BLOCK > 7
    bad[5][last] ^= 0xFF

    def damage():
        for n, f in zip(names(base), bad):
            open(n, "wb").write(f)

    def block_words(model, lo):
        block = np.stack([np.frombuffer(bytes(f[lo:lo + BLOCK]), np.uint8) for f in bad])[None]
        return (lo, min(BLOCK, size - lo), M.mismatch_words(block)[0], model.suspect_words(block)[0])

    lows = [BLOCK, 3 * BLOCK, 4 * BLOCK, 7 * BLOCK, (n_blocks - 1) * BLOCK]
    # ---- pairs
    damage()
    want = [block_words(PM, lo) for lo in lows]
    assert [w[3] for w in want] == [bits(0, 3, 8, 10, 12), bits(2, 13), bits(2, 13), UNEXPLAINED, bits(5)]
    assert H.locate_corrupt_pairs_ec_files(base, BLOCK) == (n_blocks, 5, want)
    untouched = [i for i in range(14) if i not in (0, 3, 8, 10, 12, 2, 13, 5)]
    before = {i: os.stat(names(base)[i]).st_mtime_ns for i in untouched}
    assert H.correct_ec_files(base, BLOCK, pairs=True) == (n_blocks, 5, want)
    after = [bytearray(open(n, "rb").read()) for n in names(base)]
    expect = [bytearray(f) for f in good]
    for c in triple:
        expect[c][t_at] = bad[c][t_at]
    assert after == expect
    assert {i: os.stat(names(base)[i]).st_mtime_ns for i in untouched} == before  # files nobody named: not written
    left = (7 * BLOCK, BLOCK, want[3][2], UNEXPLAINED)
    assert H.correct_ec_files(base, BLOCK, pairs=True) == (n_blocks, 1, [left])
    assert H.locate_corrupt_pairs_ec_files(base, BLOCK) == (n_blocks, 1, [left])
    assert [bytearray(open(n, "rb").read()) for n in names(base)] == expect
    # ---- single, and the cap
    damage()
    single = [block_words(M, lo) for lo in lows]
    assert [w[3] for w in single] == [bits(0, 3, 8, 10, 12), UNEXPLAINED, UNEXPLAINED, UNEXPLAINED, bits(5)]
    assert H.correct_ec_files(base, BLOCK, cap=2) == (n_blocks, 5, single[:2])
    after = [bytearray(open(n, "rb").read()) for n in names(base)]
    for shard in (2, 13):
        expect[shard][run:run + 4096] = bad[shard][run:run + 4096]
    assert after == expect
    assert H.locate_corrupt_ec_files(base, BLOCK) == (n_blocks, 3, single[1:4])
    # ---- the default block (1 MiB: the whole volume is one short block)
    damage()
    whole = (0, size, 15, bits(0, 3, 8, 10, 12, 2, 13, 5) | UNEXPLAINED)
    assert H.correct_ec_files(base, pairs=True) == (1, 1, [whole])
    for shard in (2, 13):
        expect[shard][run:run + 4096] = good[shard][run:run + 4096]
    assert [bytearray(open(n, "rb").read()) for n in names(base)] == expect


def test_files_longer_than_the_two_slots(gpu, tmp_path):
    """hec_correct_pairs_ec_files and hec_correct_ec_files over three chunks
    (64 KiB and 1 MiB blocks: slot 0 is used twice, and a chunk's rows are
    written back from its slot while later chunks are in flight) and with a
    5 MiB block, larger than a chunk, whose last chunk is one short block. The
    volume and its damage are test_gpu_locate_pairs.big_volume's. Pairs: the
    entries are the pair locate's from before, every file equals its original
    but for the triple's column, files no word names are not written, and a
    second scrub reports the triple's block alone. Single: every column with
    one wrong file is restored, those at the chunk edge inside the run
    included, the run's pair columns and the triple keep their bytes; with
    cap = 2 every fix is still written."""
    import helyim_amd as H
    good, bad, cols, triple = big_volume(2029)
    base = str(tmp_path / "big")
    files = ec_names(base)
    named = {s for s, _ in SINGLES + NEIGHBOURS} | set(triple)
    assert {2, 13} <= named
    untouched = [i for i in range(14) if i not in named]
    assert untouched
    for i in untouched:
        good[i].tofile(files[i])
        os.utime(files[i], ns=(10**18, 10**18 + i))

    def damage():
        for i in sorted(named):
            bad[i].tofile(files[i])

    def on_disk():
        return [np.fromfile(name, np.uint8) for name in files]

    def same(got, expect):
        return all(np.array_equal(g, e) for g, e in zip(got, expect))

    after_pairs = [g.copy() for g in good]
    for c in triple:
        after_pairs[c][TRIPLE_AT] = bad[c][TRIPLE_AT]
    after_single = [a.copy() for a in after_pairs]
    pair_cols = np.array([o for o in range(*RUN) if o not in (EDGE - 1, EDGE)])
    for c in (2, 13):
        after_single[c][pair_cols] = bad[c][pair_cols]
    for block in BIG_BLOCKS:
        width = block or 1 << 20  # HEC_SMALL_BLOCK_SIZE
        n_blocks = -(-BIG_SIZE // width)
        # ---- pairs
        damage()
        want = big_entries(PM, bad, cols, width)
        assert H.locate_corrupt_pairs_ec_files(base, block) == (n_blocks, len(want), want), hex(block)
        assert H.correct_ec_files(base, block, pairs=True) == (n_blocks, len(want), want), hex(block)
        assert same(on_disk(), after_pairs), hex(block)
        left = big_entries(PM, after_pairs, cols, width)
        assert len(left) == 1 and left[0][3] == UNEXPLAINED and left[0][0] == TRIPLE_AT // width * width
        assert H.correct_ec_files(base, block, pairs=True) == (n_blocks, 1, left), hex(block)
        assert H.locate_corrupt_pairs_ec_files(base, block) == (n_blocks, 1, left), hex(block)
        assert same(on_disk(), after_pairs), hex(block)
        # ---- single, and once the cap
        damage()
        single = big_entries(M, bad, cols, width)
        assert all(w[3] & UNEXPLAINED for w in single if w[0] <= RUN[1] and RUN[0] < w[0] + w[1])
        if block == 65536:
            assert [(w[0], w[3]) for w in single] == [
                (0, bits(11)), (EDGE - 65536, bits(2) | UNEXPLAINED), (EDGE, bits(13) | UNEXPLAINED),
                (6 << 20, bits(6, 9)), ((8 << 20) - 65536, bits(0)), (8 << 20, bits(10)),
                (TRIPLE_AT // 65536 * 65536, UNEXPLAINED), (BIG_SIZE // 65536 * 65536, bits(4))]
            assert H.correct_ec_files(base, block, cap=2) == (n_blocks, len(single), single[:2])
        else:
            assert H.correct_ec_files(base, block) == (n_blocks, len(single), single), hex(block)
        assert same(on_disk(), after_single), hex(block)
    assert [os.stat(files[i]).st_mtime_ns for i in untouched] == [10**18 + i for i in untouched]
