"""The pair-locate result contract of include/hec.h
(hec_gpu_locate_corrupt_pairs_batch) as numpy, by brute force -- TEST
INFRASTRUCTURE ONLY.

A column's word from its 4 syndrome bytes (H = [P | I4], locate_model's):
0 when the syndrome is 0; bit c when one shard explains it (locate_model's rule,
unchanged); else bits a and b when some shards a < b and bytes v, w != 0 have
syndrome == v * H[:,a] ^ w * H[:,b]; else UNEXPLAINED. For each of the 91 pairs
(v, w) is solved from two rows of the 4 x 2 system whose 2 x 2 minor is
invertible, and all four rows are checked (tabulated once over the 2^16 values
of those two rows, so that a batch of columns costs one lookup per pair).
Deliberately NOT the kernel's method (classical syndromes and an error-locator
polynomial): this is the statement, that the shortcut."""
import itertools

import numpy as np

import locate_model as M
from oracle import rs_oracle as O

UNEXPLAINED = M.UNEXPLAINED
N, R = M.N, M.M
H = M.H
MUL = np.asarray(O.MUL_TABLE, dtype=np.uint8)                      # MUL[a][b] = a * b
PAIRS = list(itertools.combinations(range(N), 2))


def _solver(a, b):
    """The pair (a, b) as a table over two syndrome rows. Rows (r0, r1) whose
    2 x 2 minor of H[:, (a, b)] is invertible give (v, w) for each of the 2^16
    values of (syn[r0], syn[r1]); where v, w != 0 and v * H[:,a] ^ w * H[:,b]
    reproduces those two rows, the table holds what the other two rows (r2, r3)
    must be, as r2 << 8 | r3, else a value no byte pair equals."""
    for r0, r1 in itertools.combinations(range(R), 2):
        minor = H[[r0, r1]][:, [a, b]]
        det = O.gf_mul(int(minor[0, 0]), int(minor[1, 1])) ^ O.gf_mul(int(minor[0, 1]), int(minor[1, 0]))
        if det:
            break
    else:
        raise AssertionError((a, b))  # any two columns of H are independent
    inv = O.mat_invert(minor)
    r2, r3 = (r for r in range(R) if r not in (r0, r1))
    s0, s1 = (np.arange(1 << 16) >> 8).astype(np.uint8), (np.arange(1 << 16) & 255).astype(np.uint8)
    v = MUL[int(inv[0, 0])][s0] ^ MUL[int(inv[0, 1])][s1]
    w = MUL[int(inv[1, 0])][s0] ^ MUL[int(inv[1, 1])][s1]
    row = lambda r: MUL[int(H[r, a])][v] ^ MUL[int(H[r, b])][w]
    ok = (v != 0) & (w != 0) & (row(r0) == s0) & (row(r1) == s1)
    rest = (row(r2).astype(np.uint32) << 8) | row(r3)
    return (r0, r1, r2, r3), np.where(ok, rest, np.uint32(1 << 16)).astype(np.uint32)


SOLVERS = {pair: _solver(*pair) for pair in PAIRS}


def pair_of(syn: np.ndarray) -> np.ndarray:
    """syn [4, n] uint8 -> [n] int64 words: (1 << a) | (1 << b) where a pair of
    shards with two non-zero values explains the column (all four rows), 0
    where none does. Asserts that no column has two explanations."""
    syn = np.asarray(syn, dtype=np.uint8).astype(np.uint32)
    out = np.zeros(syn.shape[1], dtype=np.int64)
    for (a, b), ((r0, r1, r2, r3), table) in SOLVERS.items():
        ok = table[(syn[r0] << 8) | syn[r1]] == ((syn[r2] << 8) | syn[r3])
        assert not (ok & (out != 0)).any(), (a, b)
        out[ok] = (1 << a) | (1 << b)
    return out


def column_word(syn) -> int:
    """Word of one byte column from its 4 syndrome bytes."""
    single = M.column_word(syn)
    if single != UNEXPLAINED:
        return single
    pair = int(pair_of(np.array([[int(x)] for x in syn], dtype=np.uint8))[0])
    return pair if pair else UNEXPLAINED


def syndrome_word(syn: np.ndarray) -> int:
    """Word of the columns syn [4, L]."""
    cols = np.flatnonzero(syn.any(axis=0))
    word, rest = 0, []
    for t in {tuple(int(x) for x in syn[:, o]) for o in cols}:
        single = M.column_word(t)
        if single != UNEXPLAINED:
            word |= single
        else:
            rest.append(t)
    if rest:  # the columns no single shard explains, all pairs at once
        for pair in pair_of(np.array(rest, dtype=np.uint8).T):
            word |= int(pair) or UNEXPLAINED
    return word


def suspect_words(stripes: np.ndarray):
    """stripes [S, 14, L] uint8 -> the S pair-locate suspects words."""
    return [syndrome_word(s) for s in M.syndromes(stripes)]


def syndrome_of(errors) -> list:
    """errors: {shard: value} in one byte column -> the 4 syndrome bytes."""
    syn = [0] * R
    for c, v in errors.items():
        for r in range(R):
            syn[r] ^= O.gf_mul(v, int(H[r, c]))
    return syn


def unexplained_triple(rng):
    """{shard: value} of three wrong shards in one column for which the model
    says bit 31 (nearly all do), and one it explains by a pair is skipped."""
    while True:
        group = sorted(int(c) for c in rng.choice(14, 3, replace=False))
        errors = {c: int(rng.integers(1, 256)) for c in group}
        if column_word(syndrome_of(errors)) == UNEXPLAINED:
            return errors
