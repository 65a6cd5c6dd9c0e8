"""The guarantees of the pair-locate contract (include/hec.h,
hec_gpu_locate_corrupt_pairs_batch), pinned on the numpy model itself
(tests/locate_pairs_model.py): two wrong shards in a byte column are named
exactly, for every pair and every pair of values; one wrong shard keeps its
single bit; the word equals locate_model's wherever that names a shard; three
wrong shards never name a single shard but sometimes an intact pair."""
import itertools

import numpy as np

import locate_model as M
import locate_pairs_model as PM
from oracle import rs_oracle as O

VALUES = np.arange(1, 256, dtype=np.uint8)


def pair_syndromes(a, b):
    """Syndromes [4, 255 * 255] of shard a wrong by v and shard b by w, all v, w != 0."""
    v, w = np.repeat(VALUES, 255), np.tile(VALUES, 255)
    return np.stack([PM.MUL[int(PM.H[r, a])][v] ^ PM.MUL[int(PM.H[r, b])][w] for r in range(4)])


def single_explained(syn):
    """[n] bool: some single shard explains the column (locate_model's rule, vectorised)."""
    out = np.zeros(syn.shape[1], dtype=bool)
    for c in range(14):
        col = [int(x) for x in PM.H[:, c]]
        r0 = next(r for r in range(4) if col[r])
        v = PM.MUL[O.gf_div(1, col[r0])][syn[r0]]
        ok = v != 0
        for r in range(4):
            ok &= PM.MUL[col[r]][v] == syn[r]
        out |= ok
    return out


def test_every_pair_and_every_value_pair_is_named_exactly():
    assert len(PM.PAIRS) == 91
    for a, b in PM.PAIRS:
        syn = pair_syndromes(a, b)
        assert syn.shape == (4, 255 * 255)
        assert (PM.pair_of(syn) == (1 << a | 1 << b)).all(), (a, b)   # asserts uniqueness too
        assert not single_explained(syn).any(), (a, b)                # so column_word goes on to the pair
    # and through column_word itself, a few of each
    rng = np.random.default_rng(91)
    for a, b in PM.PAIRS:
        for _ in range(3):
            errors = {a: int(rng.integers(1, 256)), b: int(rng.integers(1, 256))}
            assert PM.column_word(PM.syndrome_of(errors)) == (1 << a | 1 << b), errors


def test_every_single_error_keeps_its_single_bit():
    for c in range(14):
        syn = np.stack([PM.MUL[int(PM.H[r, c])][VALUES] for r in range(4)])
        assert (PM.pair_of(syn) == 0).all(), c  # no pair explains a single error: three columns would be dependent
        for v in range(1, 256):
            assert PM.column_word(PM.syndrome_of({c: v})) == 1 << c, (c, v)
    assert PM.column_word([0, 0, 0, 0]) == 0


def test_equals_the_single_model_wherever_that_names_a_shard():
    rng = np.random.default_rng(31)
    syn = rng.integers(0, 256, (4, 1500), dtype=np.uint8)
    syn[:, :200] = 0
    syn[rng.integers(0, 4, 400), np.arange(200, 600)] = 0       # some with a zero row
    for c in range(14):                                          # and real single errors
        for n in range(8):
            syn[:, 600 + 8 * c + n] = PM.syndrome_of({c: int(rng.integers(1, 256))})
    pairs = PM.pair_of(syn)
    n_single = n_pair = 0
    for o in range(syn.shape[1]):
        single = M.column_word(syn[:, o])
        word = PM.column_word(syn[:, o])
        if single != M.UNEXPLAINED:
            assert word == single, (o, hex(word), hex(single))
            n_single += single != 0
        else:
            assert word == (int(pairs[o]) or PM.UNEXPLAINED), o
            n_pair += word != PM.UNEXPLAINED
    assert n_single >= 14 * 8


def test_three_wrong_shards_never_name_one_shard_but_may_name_an_intact_pair():
    """The documented limit: 91 * 255^2 of the 2^32 syndromes are pair-explainable
    (0.138 %), so about that share of triple errors comes back as a pair, and
    such a pair always holds an intact shard (else two or three columns of H
    plus the triple's would be dependent)."""
    rng = np.random.default_rng(333)
    n = 200_000
    triples = np.array(list(itertools.combinations(range(14), 3)))
    which = triples[rng.integers(0, len(triples), n)]                    # [n, 3]
    values = rng.integers(1, 256, (n, 3), dtype=np.uint8)
    syn = np.zeros((4, n), dtype=np.uint8)
    for t in range(3):
        for r in range(4):
            syn[r] ^= PM.MUL[PM.H[r, which[:, t]], values[:, t]]
    assert not single_explained(syn).any()
    pairs = PM.pair_of(syn)
    named = np.flatnonzero(pairs)
    assert 100 <= len(named) <= 500, len(named)                          # 0.138 % of 200,000 = 276
    for o in named:
        wrong = sum(1 << int(c) for c in which[o])
        assert int(pairs[o]) & ~wrong, (o, hex(int(pairs[o])), hex(wrong))  # an intact shard is blamed


def test_stripe_words_are_the_or_over_columns():
    rng = np.random.default_rng(8)
    data = rng.integers(0, 256, (3, 14, 40), dtype=np.uint8)
    data[:, 10:] = 0
    data[:, 10:] = M.syndromes(data)
    assert PM.suspect_words(data) == [0, 0, 0]
    data[0, 3, 5] ^= 0x21
    data[0, 12, 5] ^= 0x01            # a pair in column 5
    data[0, 7, 39] ^= 0x80            # a single elsewhere
    data[1, 11, 0] ^= 0xFF
    assert PM.suspect_words(data) == [1 << 3 | 1 << 12 | 1 << 7, 1 << 11, 0]
    assert M.suspect_words(data) == [M.UNEXPLAINED | 1 << 7, 1 << 11, 0]
