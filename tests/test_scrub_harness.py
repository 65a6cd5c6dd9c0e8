"""The scrub suites' shared checks (tests/scrub_harness.py) against themselves
on the CPU: the compare functions the device wrappers call take numpy arrays,
an untouched result passes, and every planted fault, taken alone, raises."""
import numpy as np
import pytest

import scrub_harness as SH

S = 5


def words(*values):
    out = np.array(list(values) + [SH.SENTINEL], dtype=np.uint32)
    assert len(values) == S
    return out


def test_result_words():
    assert SH.check_words(words(0, 1 << 13, SH.UNEXPLAINED, 0, 0x3C00), S) == [0, 1 << 13, SH.UNEXPLAINED, 0, 0x3C00]
    over = words(0, 0, 0, 0, 0)
    over[S] = 0
    with pytest.raises(AssertionError, match="sentinel was overwritten"):
        SH.check_words(over, S)
    with pytest.raises(AssertionError, match=r"stale words left at \[3\]"):
        SH.check_words(words(0, 0, 0, SH.STALE, 0), S)
    with pytest.raises(AssertionError):     # an array of another length is not the one that was handed in
        SH.check_words(words(0, 0, 0, 0, 0)[1:], S)


def test_counters_advance_from_their_presets():
    assert SH.advance(9, 7) == 2 and SH.advance(7, 7, want=0) == 0 and SH.advance(11 + (1 << 33), 11) == 1 << 33
    with pytest.raises(AssertionError, match="advanced by 0 from 7, expected 2"):
        SH.advance(7, 7, want=2)            # a counter that did not advance
    with pytest.raises(AssertionError, match="below its preset"):
        SH.advance(2, 7)                    # set, not accumulated


def test_masks_come_back_unchanged():
    given = [SH.R3, SH.R2 | 1 << 31 | 5 << 14, SH.ALL]
    SH.assert_masks(np.array(given, dtype=np.uint32).view(np.int32), given)
    got = np.array(given, dtype=np.uint32)
    got[1] &= SH.ALL                        # a call that "cleaned" the stray bits in place
    with pytest.raises(AssertionError, match="present masks were written"):
        SH.assert_masks(got, given)


def planted(arena, offset):
    out = arena.copy()
    out[offset] ^= 0x01
    return out


def test_masked_batch_arena():
    b = SH.Batch(SH.clean_stripes(3, 17, seed=1), [SH.R3, SH.ALL, SH.R2])
    la = b.layout
    SH.assert_arenas([b.arena], [b.arena.copy()], b.stripes, masks=b.masks)
    for offset, what in ((la.off(1, 4) + 16, "present shard .stripe 1 shard 4 at byte 16"),
                         (la.off(0, 3) + 2, "absent shard .stripe 0 shard 3 at byte 2"),
                         (la.off(1, 4) + 17, "shard gap"),          # the byte at shard_len
                         (la.off(1, 0) - 1, "stripe gap"),
                         (la.base - 1, "slack"), (len(b.arena) - 1, "slack")):
        with pytest.raises(AssertionError, match=what):
            SH.assert_arenas([b.arena], [planted(b.arena, offset)], b.stripes, masks=b.masks)
    # the expected image of a writing call: the input no longer passes
    image = planted(b.arena, la.off(2, 13))
    SH.assert_arenas([image], [image.copy()], b.stripes, masks=b.masks)
    with pytest.raises(AssertionError, match="stripe 2 shard 13 at byte 0"):
        SH.assert_arenas([image], [b.arena], b.stripes, masks=b.masks)


def test_ragged_arena():
    b = SH.Ragged([(16, SH.R2), (1000, SH.R4), (17, SH.TEN)])
    assert [len(b.gather(s)[0]) for s in range(3)] == [16, 1000, 17] and b.entries() == 2
    assert all((b.shard(0, i) == SH.FILL).all() for i in (0, 12))
    assert np.array_equal(b.shard(1, 9), SH.ragged_stripe(1000, 1)[9])

    def check(got):
        SH.assert_arenas([b.arena], [got], b.stripes(), masks=b.masks(), slack=SH.Ragged.SLACK)

    check(b.arena.copy())
    for offset, what in ((b.offs[1] + 9 * b.strides[1] + 999, "present shard .stripe 1 shard 9 at byte 999"),
                         (b.offs[0] + 12 * b.strides[0], "absent shard .stripe 0 shard 12 at byte 0"),
                         (b.offs[1] + 1000, "shard gap"),
                         (b.offs[2] - 1, "stripe gap"), (0, "slack")):
        with pytest.raises(AssertionError, match=what):
            check(planted(b.arena, offset))


def test_separate_arenas():
    name, data, par, stripes, arenas = SH.clean_case(10, 4, 17, 3, 2)
    assert name == "separate arenas" and len(arenas) == 2 and SH.oracle_words(arenas, stripes, 10, 4) == [0, 0, 0]
    SH.assert_arenas(arenas, SH.copies(arenas), stripes)
    work = SH.copies(arenas)
    SH.shard_of(work, stripes, 2, 11)[16] ^= 0x80
    assert SH.oracle_words(work, stripes, 10, 4) == [0, 0, 1 << 1]
    assert np.array_equal(SH.gather(work, stripes)[2, 11], SH.shard_of(work, stripes, 2, 11))
    with pytest.raises(AssertionError, match="arena 1 .*stripe 2 shard 11 at byte 16"):
        SH.assert_arenas(arenas, work, stripes)


def test_clean_stripes_keep_each_suites_seed_rule():
    rng = np.random.default_rng(1000003 * 3 + 31 * 17 + 2)
    assert np.array_equal(SH.clean_stripes(2, 17, 3)[:, :10], rng.integers(0, 256, (2, 14, 17), dtype=np.uint8)[:, :10])
    rng = np.random.default_rng(7919 * 4 + 16)
    assert np.array_equal(SH.ragged_stripe(16, 4)[:10], rng.integers(0, 256, (1, 14, 16), dtype=np.uint8)[0, :10])
    assert not SH.clean_stripes(2, 17, 3).flags.writeable
