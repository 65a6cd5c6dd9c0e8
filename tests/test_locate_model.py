"""The guarantee of the locate contract (include/hec.h), pinned on the numpy
model itself (tests/locate_model.py): RS(10,4)'s check matrix H = [P | I4] has
any four columns independent, so one wrong shard in a byte column is named
uniquely and two or three wrong shards are recognised as no single shard."""
import itertools

import numpy as np

import locate_model as M
from oracle import rs_oracle as O


def syndrome_of(errors):
    """errors: {shard: value} in one byte column -> the 4 syndrome bytes."""
    syn = [0] * 4
    for c, v in errors.items():
        for r in range(4):
            syn[r] ^= O.gf_mul(v, int(M.H[r, c]))
    return syn


def test_every_four_columns_of_h_are_independent():
    subsets = list(itertools.combinations(range(14), 4))
    assert len(subsets) == 1001
    for sub in subsets:
        O.mat_invert(M.H[:, list(sub)])  # raises SingularMatrix


def test_parity_matrix_has_no_zero_and_distinct_ratios():
    assert M.P.shape == (4, 10) and (M.P != 0).all()
    ratios = {O.gf_div(int(M.P[1, c]), int(M.P[0, c])) for c in range(10)}
    assert len(ratios) == 10


def test_one_wrong_shard_is_named_for_every_value():
    for c in range(14):
        for v in range(1, 256):
            assert M.column_word(syndrome_of({c: v})) == 1 << c, (c, v)
    assert M.column_word([0, 0, 0, 0]) == 0


def test_two_or_three_wrong_shards_are_unexplained():
    rng = np.random.default_rng(104)
    pairs = list(itertools.combinations(range(14), 2))
    triples = list(itertools.combinations(range(14), 3))
    assert (len(pairs), len(triples)) == (91, 364)
    for group in pairs + triples:
        for _ in range(4):
            errors = {c: int(rng.integers(1, 256)) for c in group}
            assert M.column_word(syndrome_of(errors)) == M.UNEXPLAINED, errors


def test_stripe_words_are_the_or_over_columns():
    rng = np.random.default_rng(7)
    data = rng.integers(0, 256, (3, 14, 40), dtype=np.uint8)
    data[:, 10:] = 0
    data[:, 10:] = M.syndromes(data)  # parity of the data: XOR with zero parity
    assert M.suspect_words(data) == [0, 0, 0] and M.mismatch_words(data) == [0, 0, 0]
    data[0, 3, 5] ^= 0x21
    data[0, 12, 39] ^= 0x01
    data[1, 6, 9] ^= 0x80
    data[1, 9, 9] ^= 0x80
    data[1, 11, 0] ^= 0xFF
    assert M.suspect_words(data) == [1 << 3 | 1 << 12, M.UNEXPLAINED | 1 << 11, 0]
    assert M.mismatch_words(data) == [0b1111, 0b1111, 0]
