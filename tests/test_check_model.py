"""What the degraded scrub rests on (include/hec.h, "degraded scrub"), pinned on
the numpy model (tests/check_model.py): for every present mask with 11 to 13
shards the check matrix A_m has no zero entry and, with two or more spare
shards, no two columns of H_m = [A_m | I_r] are proportional, so the ratio
method of the locate kernel carries over and one wrong shard is named uniquely.
With the full mask the model is tests/locate_model.py."""
import itertools

import numpy as np

import check_model as C
import locate_model as M
from oracle import rs_oracle as O

DEGRADED = C.checkable_masks((1, 2, 3))


def test_there_are_469_degraded_masks_and_470_checkable():
    assert len(DEGRADED) == 469 and len(C.checkable_masks()) == 470
    assert [len([m for m in DEGRADED if bin(m).count("1") == p]) for p in (11, 12, 13)] == [364, 91, 14]


def test_no_check_matrix_has_a_zero_entry():
    for m in C.checkable_masks():
        B, E, A, _ = C.check_matrix(m)
        assert A.shape == (len(E), 10) and (A != 0).all(), hex(m)
        assert B == sorted(B) and E == sorted(E) and max(B) < min(E)


def test_no_two_columns_are_proportional():
    """Each column normalised by its first non-zero entry: all p are distinct."""
    for m in C.checkable_masks((2, 3, 4)):
        _, E, _, H = C.check_matrix(m)
        seen = set()
        for pos in range(H.shape[1]):
            col = [int(x) for x in H[:, pos]]
            lead = next(x for x in col if x)
            seen.add(tuple(O.gf_div(x, lead) for x in col))
        assert len(seen) == H.shape[1], hex(m)


def test_the_full_mask_is_the_locate_model():
    B, E, A, H = C.check_matrix(C.ALL)
    assert B == list(range(10)) and E == [10, 11, 12, 13]
    assert np.array_equal(A, M.P) and np.array_equal(H, M.H)
    rng = np.random.default_rng(14)
    data = rng.integers(0, 256, (6, 14, 48), dtype=np.uint8)
    data[:, 10:] = 0
    data[:, 10:] = M.syndromes(data)
    data[1, 3, 5] ^= 0x21
    data[2, 12, 47] ^= 0x01
    data[3, 6, 9] ^= 0x80
    data[3, 9, 9] ^= 0x80
    data[4, 0, 0] ^= 0xFF
    data[4, 13, 1] ^= 0x02
    masks = [C.ALL] * 6
    assert C.suspect_words(data, masks) == M.suspect_words(data)
    assert C.check_words(data, masks) == [w << 10 for w in M.mismatch_words(data)]
    assert C.suspect_words(data, masks) == [0, 1 << 3, 1 << 12, C.UNEXPLAINED, 1 << 0 | 1 << 13, 0]


def test_one_wrong_shard_is_named_for_every_mask():
    rng = np.random.default_rng(470)
    for m in C.checkable_masks((2, 3)):
        B, E, _, _ = C.check_matrix(m)
        for c in B + E:
            v = int(rng.integers(1, 256))
            assert C.column_word(C.syndrome_of(m, {c: v}), m) == 1 << c, (hex(m), c, v)
    for m in C.checkable_masks((1,))[::7]:
        B, E, _, _ = C.check_matrix(m)
        for c in B + E:
            assert C.column_word(C.syndrome_of(m, {c: 1}), m) == C.UNEXPLAINED


def test_pairs_with_three_spares_are_unexplained():
    """r = 3: the present shards are an MDS code of distance 4, so two wrong
    shards in a column never look like one."""
    rng = np.random.default_rng(3)
    for m in C.checkable_masks((3,)):
        B, E, _, _ = C.check_matrix(m)
        for pair in itertools.combinations(B + E, 2):
            errors = {c: int(rng.integers(1, 256)) for c in pair}
            assert C.column_word(C.syndrome_of(m, errors), m) == C.UNEXPLAINED, (hex(m), errors)


def test_pairs_with_two_spares_can_name_an_intact_shard():
    """r = 2's limit, stated in hec.h: distance 3 corrects one error and no more."""
    m = C.ALL & ~(1 << 4 | 1 << 11)
    B, E, _, H = C.check_matrix(m)
    ids = B + E
    # errors in B[0] and B[1] chosen so that the syndrome is column B[2]'s
    target = [int(x) for x in H[:, ids.index(B[2])]]
    sub = H[:, [0, 1]]
    v = O.mat_mul(O.mat_invert(sub), np.array(target, dtype=np.uint8).reshape(2, 1))
    errors = {B[0]: int(v[0, 0]), B[1]: int(v[1, 0])}
    assert all(errors.values())
    assert C.column_word(C.syndrome_of(m, errors), m) == 1 << B[2]


def test_use_masks_rule():
    U = C.UNEXPLAINED
    one_lost, two_lost, three_lost = C.ALL & ~1, C.ALL & ~(1 | 2), C.ALL & ~(1 | 2 | 4)
    masks = [one_lost, one_lost, two_lost, three_lost, 0x3FF, 0x1FF, C.ALL, C.ALL, one_lost, one_lost | 1 << 20]
    check = [0, 1 << 13, 1 << 12, 1 << 13, 0, 0, 0, 1 << 10, 1 << 11, 0]
    sus = [0, 1 << 5, 1 << 13, U, 0, 0, 0, 1 << 3, U | 1 << 5, 0]
    use, left = C.use_masks(masks, check, sus)
    assert use == [one_lost, one_lost & ~(1 << 5), two_lost & ~(1 << 13), C.ALL, 0x3FF, 0x1FF, C.ALL,
                   C.ALL & ~(1 << 3), C.ALL, one_lost]
    assert left == 2
    # naming leaves fewer than ten: left alone
    assert C.use_masks([three_lost], [1 << 13], [1 << 13 | 1 << 12]) == ([C.ALL], 1)
