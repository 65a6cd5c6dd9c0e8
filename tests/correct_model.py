"""The correct result contract of include/hec.h (hec_gpu_correct_batch and
hec_gpu_correct_pairs_batch) as numpy, by brute force -- TEST INFRASTRUCTURE
ONLY.

For stripes [S, 14, L]: the corrected image, verify's words, the suspects words
and the number of bytes changed. The names of a column come from locate_model
(single) or locate_pairs_model (pairs), unchanged. The error values come from
an enumeration: for a named shard c every v in 1..255, for a named pair (a, b)
every (v, w) in 1..255 squared, is multiplied into all four rows of H and the
one whose four bytes equal the column's syndrome is the answer (exactly one
is, asserted). Deliberately NOT the kernel's formulas (s[0] / P[0][c], the
classical syndromes' closed form): this is the statement, that the shortcut.
A column whose word is UNEXPLAINED keeps its bytes."""
import functools

import numpy as np

import locate_model as M
import locate_pairs_model as PM

UNEXPLAINED = M.UNEXPLAINED
H = M.H
MUL = PM.MUL
_VALUES = np.arange(1, 256, dtype=np.uint8)


def codewords(S, L, seed) -> np.ndarray:
    """[S, 14, L] seeded codewords, the parity from the model's own tables."""
    rng = np.random.default_rng(seed)
    data = rng.integers(0, 256, (S, 10, L), dtype=np.uint8)
    out = np.zeros((S, 14, L), dtype=np.uint8)
    out[:, :10] = data
    for j in range(4):
        for i in range(10):
            out[:, 10 + j] ^= MUL[int(M.P[j, i])][data[:, i]]
    assert not M.syndromes(out).any()
    return out


def _pack(syn) -> np.ndarray:
    """syn [4, n] uint8 -> [n] uint32 keys."""
    syn = np.asarray(syn, dtype=np.uint8).astype(np.uint32)
    return syn[0] | (syn[1] << 8) | (syn[2] << 16) | (syn[3] << 24)


def _unpack(key: int):
    return tuple((int(key) >> (8 * r)) & 255 for r in range(4))


@functools.lru_cache(maxsize=None)
def _table(shards):
    """Every syndrome the shards (one, or a pair) produce with non-zero values
    -> those values: {key: (v,)} or {key: (v, w)}."""
    if len(shards) == 1:
        c, = shards
        keys = _pack(np.stack([MUL[int(H[r, c])][_VALUES] for r in range(4)]))
        table = {int(k): (int(v),) for k, v in zip(keys, _VALUES)}
    else:
        a, b = shards
        v, w = (g.ravel() for g in np.meshgrid(_VALUES, _VALUES, indexing="ij"))
        keys = _pack(np.stack([MUL[int(H[r, a])][v] ^ MUL[int(H[r, b])][w] for r in range(4)]))
        table = {int(k): (int(x), int(y)) for k, x, y in zip(keys, v, w)}
    assert len(table) == 255 ** len(shards), shards  # no two value sets share a syndrome
    return table


_single_words = {}


def _column_words(keys, pairs: bool):
    """Keys of non-zero syndromes -> their words (the locate models')."""
    words = []
    for k in keys:
        k = int(k)
        if k not in _single_words:
            _single_words[k] = M.column_word(_unpack(k))
        words.append(_single_words[k])
    if pairs:
        rest = [n for n, w in enumerate(words) if w == UNEXPLAINED]
        if rest:
            syn = np.array([_unpack(keys[n]) for n in rest], dtype=np.uint8).T
            for n, pair in zip(rest, PM.pair_of(syn)):
                words[n] = int(pair) or UNEXPLAINED
    return words


def shards_of(word: int):
    return tuple(c for c in range(M.N) if (word >> c) & 1)


def correct(stripes, pairs: bool = False):
    """stripes [S, 14, L] uint8 -> (image [S, 14, L], mismatch words [S],
    suspects words [S], bytes changed). The words are those of the input."""
    out = np.array(stripes, dtype=np.uint8, copy=True)
    syn_all = M.syndromes(out)
    mismatch = [sum(1 << j for j in range(M.M) if syn[j].any()) for syn in syn_all]  # locate_model.mismatch_words
    suspects, changed = [], 0
    for s in range(len(out)):
        syn = syn_all[s]
        cols = np.flatnonzero(syn.any(axis=0))
        word = 0
        if cols.size:
            uniq, inverse = np.unique(_pack(syn[:, cols]), return_inverse=True)
            for u, name in enumerate(_column_words(uniq, pairs)):
                word |= name
                if name == UNEXPLAINED:
                    continue
                named = shards_of(name)
                assert len(named) in (1, 2), hex(name)
                values = _table(named)[int(uniq[u])]  # KeyError: the name does not explain the column
                where = cols[inverse == u]
                for c, v in zip(named, values):
                    out[s, c, where] ^= np.uint8(v)
                    changed += int(where.size)
        suspects.append(word)
    return out, mismatch, suspects, changed
