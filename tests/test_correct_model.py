"""tests/correct_model.py against itself and against the kernel's formulas, on
the CPU: the model restores the codeword for every shard, every pair of the 91
(shard 0 included) and values that include 0x01 and 0xFF; the single form
leaves columns with 2 or 3 wrong shards untouched; a second application is the
identity; and the closed forms rs104_correct_kernel evaluates (s[0] / P[0][c],
and the classical syndromes' (D S1 ^ N1 S0 ^ alpha_c D S0) / (N1 u_c)) give
the values the model finds by enumeration."""
import numpy as np
import pytest

import correct_model as CM
import locate_model as M
import locate_pairs_model as PM
from oracle import rs_oracle as O

UNEXPLAINED = CM.UNEXPLAINED
VALUES = (0x01, 0xFF, 0x80, 0x5A)


def test_every_single_shard_is_restored():
    good = CM.codewords(14, 33, 1)
    bad = good.copy()
    for c in range(14):
        for n, v in enumerate(VALUES):
            bad[c, c, (5 * c + 8 * n) % 33] ^= v
    for pairs in (False, True):
        image, mismatch, suspects, changed = CM.correct(bad, pairs)
        assert np.array_equal(image, good)
        assert suspects == [1 << c for c in range(14)]
        assert mismatch == M.mismatch_words(bad) and all(mismatch)
        assert changed == 14 * len(VALUES)


def test_every_pair_is_restored():
    good = CM.codewords(91, 19, 2)
    bad = good.copy()
    rng = np.random.default_rng(22)
    for s, (a, b) in enumerate(PM.PAIRS):
        for n, v in enumerate(VALUES):
            bad[s, a, 4 * n] ^= v
            bad[s, b, 4 * n] ^= VALUES[(n + 1) % 4] if n < 3 else int(rng.integers(1, 256))
    image, mismatch, suspects, changed = CM.correct(bad, pairs=True)
    assert np.array_equal(image, good)
    assert suspects == [(1 << a) | (1 << b) for a, b in PM.PAIRS]
    assert changed == 91 * 2 * len(VALUES)
    # the single form: every such column is unexplained and stays
    image, _, suspects, changed = CM.correct(bad, pairs=False)
    assert np.array_equal(image, bad) and suspects == [UNEXPLAINED] * 91 and changed == 0


def test_single_form_leaves_two_and_three_wrong_shards_and_fixes_the_rest():
    good = CM.codewords(3, 40, 3)
    bad = good.copy()
    bad[0, 0, 7] ^= 0x11
    bad[0, 13, 7] ^= 0xFF   # two wrong in column 7
    bad[0, 4, 30] ^= 0x02   # a single elsewhere
    for c, v in ((2, 0x33), (6, 0x01), (11, 0xFF)):
        bad[1, c, 39] ^= v  # three wrong in the last column
    bad[1, 12, 0] ^= 0x80
    image, _, suspects, changed = CM.correct(bad, pairs=False)
    want = good.copy()
    want[0, :, 7] = bad[0, :, 7]
    want[1, :, 39] = bad[1, :, 39]
    assert np.array_equal(image, want)
    assert suspects == [(1 << 4) | UNEXPLAINED, (1 << 12) | UNEXPLAINED, 0] and changed == 2


def test_second_application_is_the_identity():
    good = CM.codewords(4, 25, 4)
    bad = good.copy()
    bad[0, 3, 1] ^= 0x44
    bad[1, 0, 24] ^= 0x10
    bad[1, 9, 24] ^= 0x20
    for c, v in ((1, 0x21), (5, 0x07), (10, 0x99)):
        bad[2, c, 12] ^= v
    for pairs in (False, True):
        once = CM.correct(bad, pairs)
        twice = CM.correct(once[0], pairs)
        assert np.array_equal(twice[0], once[0]) and twice[3] == 0
        # what is left names nothing but unexplained columns
        assert all(w in (0, UNEXPLAINED) for w in twice[2])


# ---- the kernel's closed forms -------------------------------------------------
def inv(x):
    return O.gf_div(1, x)


def dual_code():
    """u_c and T of DESIGN.md §4 "Locate, two per column": H'[j][c] = u_c *
    alpha_c^j with alpha_c = c, u_c = 1 / prod_{l != c} (c ^ l); T = H'[:, 10:]."""
    u = []
    for c in range(14):
        prod = 1
        for l in range(14):
            if l != c:
                prod = O.gf_mul(prod, c ^ l)
        u.append(inv(prod))
    dual = [[O.gf_mul(u[c], O.gf_exp(c, j)) if (c or j == 0) else 0 for c in range(14)] for j in range(4)]
    T = [[dual[j][10 + i] for i in range(4)] for j in range(4)]
    return u, T


def test_single_value_is_s0_over_p0():
    for c in range(10):
        for v in (1, 0xFF, 0x37):
            syn = PM.syndrome_of({c: v})
            assert O.gf_mul(syn[0], inv(int(M.P[0, c]))) == v
            assert CM._table((c,))[int(CM._pack(np.array([[x] for x in syn], dtype=np.uint8))[0])] == (v,)


@pytest.mark.parametrize("seed", [0, 1])
def test_pair_values_closed_form(seed):
    u, T = dual_code()
    rng = np.random.default_rng(seed)
    cases = [(a, b, int(rng.integers(1, 256)), int(rng.integers(1, 256))) for a, b in PM.PAIRS]
    cases += [(0, b, 0xFF, 0x01) for b in range(1, 14)]
    mul = O.gf_mul
    for a, b, v, w in cases:
        syn = PM.syndrome_of({a: v, b: w})
        S = [0] * 4
        for j in range(4):
            for i in range(4):
                S[j] ^= mul(T[j][i], syn[i])
        D = mul(S[0], S[2]) ^ mul(S[1], S[1])
        N1 = mul(S[0], S[3]) ^ mul(S[1], S[2])
        assert D and N1, (a, b)
        got = []
        for c in (a, b):
            num = mul(D, S[1]) ^ mul(N1, S[0]) ^ mul(c, mul(D, S[0]))
            got.append(mul(mul(num, inv(N1)), inv(u[c])))
        assert got == [v, w], (a, b, v, w, got)
        key = int(CM._pack(np.array([[x] for x in syn], dtype=np.uint8))[0])
        assert CM._table((a, b))[key] == (v, w)
