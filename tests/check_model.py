"""The degraded-scrub result contracts of include/hec.h
(hec_gpu_verify_present_batch, hec_gpu_locate_corrupt_present_batch,
hec_gpu_reconstruct_checked_batch) as numpy, by brute force -- TEST
INFRASTRUCTURE ONLY. Mirrors tests/locate_model.py.

Built from the oracle's GF(2^8) tables and encoding matrix alone. For a present
mask m with p >= 11 bits: B = its ten lowest set bits, E = the other r = p - 10,
A_m = rows E of the encoding matrix times the inverse of rows B (mat_invert,
mat_mul), H_m = [A_m | I_r] with columns labelled B then E. syn = stored E XOR
A_m times stored B. A column's suspects word: 0 when syn is 0; with r >= 2, bit
c when some byte v != 0 has syn == v * H_m[:,c], searched over every present c
(v solved from the first non-zero row of the column, all rows checked); else
UNEXPLAINED. Deliberately NOT the kernel's method (ratios of the first row)."""
from functools import lru_cache

import numpy as np

from oracle import rs_oracle as O

UNEXPLAINED = 0x80000000
K, N = 10, 14
ALL = (1 << N) - 1
ENC = O.build_matrix(K, N)  # 14 x 10, identity on top


def split(mask: int):
    """(B, E) of a present mask: its ten lowest set bits, and the rest."""
    ids = [i for i in range(N) if (int(mask) & ALL) >> i & 1]
    return ids[:K], ids[K:]


def checkable_masks(r_values=(1, 2, 3, 4)):
    return [m for m in range(1 << N) if bin(m).count("1") - K in r_values]


@lru_cache(maxsize=None)
def check_matrix(mask: int):
    """(B, E, A_m [r x 10], H_m [r x p]) for a mask with 11 or more bits."""
    B, E = split(mask)
    assert E, hex(mask)
    A = O.mat_mul(ENC[E, :], O.mat_invert(ENC[B, :]))
    H = np.concatenate([A, np.eye(len(E), dtype=np.uint8)], axis=1)
    return B, E, A, H


def syndrome_of(mask: int, errors: dict) -> list:
    """errors: {shard: value} in one byte column -> the r syndrome bytes."""
    B, E, _, H = check_matrix(mask)
    ids = B + E
    syn = [0] * len(E)
    for c, v in errors.items():
        for j in range(len(E)):
            syn[j] ^= O.gf_mul(v, int(H[j, ids.index(c)]))
    return syn


def syndrome(stripe: np.ndarray, mask: int) -> np.ndarray:
    """stripe [14, L] uint8 -> syn [r, L]; only present shards are looked at."""
    B, E, A, _ = check_matrix(int(mask) & ALL)
    out = np.array(stripe[E, :], copy=True)
    for j in range(len(E)):
        for i in range(K):
            out[j] ^= O.MUL_TABLE[int(A[j, i])][stripe[B[i], :]]
    return out


def column_word(syn, mask: int) -> int:
    """Suspects word of one byte column from its r syndrome bytes."""
    syn = [int(x) for x in syn]
    if not any(syn):
        return 0
    B, E, _, H = check_matrix(int(mask) & ALL)
    r = len(E)
    if r < 2:
        return UNEXPLAINED
    named = []
    for pos, c in enumerate(B + E):
        col = [int(x) for x in H[:, pos]]
        r0 = next(j for j in range(r) if col[j])
        v = O.gf_div(syn[r0], col[r0])
        if v and all(O.gf_mul(v, col[j]) == syn[j] for j in range(r)):
            named.append(c)
    assert len(named) <= 1, (hex(mask), syn, named)  # no two columns of H_m are proportional
    return 1 << named[0] if named else UNEXPLAINED


def _popcount(mask) -> int:
    return bin(int(mask) & ALL).count("1")


def check_words(stripes: np.ndarray, masks):
    """stripes [S, 14, L], masks [S] -> the S check words (bits by shard index)."""
    out = []
    for st, m in zip(stripes, masks):
        if _popcount(m) <= K:
            out.append(0)
            continue
        E = split(m)[1]
        syn = syndrome(st, m)
        out.append(sum(1 << e for j, e in enumerate(E) if syn[j].any()))
    return out


def suspect_words(stripes: np.ndarray, masks):
    """stripes [S, 14, L], masks [S] -> the S suspects words."""
    out = []
    for st, m in zip(stripes, masks):
        if _popcount(m) <= K:
            out.append(0)
            continue
        syn = syndrome(st, m)
        word = 0
        for t in {tuple(int(x) for x in syn[:, o]) for o in np.flatnonzero(syn.any(axis=0))}:
            word |= column_word(t, m)
        out.append(word)
    return out


def unchecked_count(masks) -> int:
    return sum(1 for m in masks if _popcount(m) <= K)


def use_masks(masks, check, suspects):
    """The checked reconstruct's use masks -> (use masks [S], unrepaired count)."""
    out, left = [], 0
    for m, c, w in zip(masks, check, suspects):
        m, w = int(m) & ALL, int(w)
        if int(c) == 0:
            out.append(m)
        elif not w & UNEXPLAINED and w & ALL and bin(m & ~w).count("1") >= K:
            out.append(m & ~w)
        else:
            out.append(ALL)
            left += 1
    return out, left
