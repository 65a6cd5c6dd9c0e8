"""The locate result contract of include/hec.h (hec_gpu_locate_corrupt_batch)
as numpy, by brute force -- TEST INFRASTRUCTURE ONLY.

Built from the oracle's GF(2^8) tables and encoding matrix alone. H = [P | I4]
is the 4 x 14 check matrix, P the parity rows of build_matrix(10, 14). The
syndrome of a byte column is stored parity XOR parity of the stored data (4
bytes). A column's word: 0 when the syndrome is 0; bit c when some byte v != 0
has syndrome == v * H[:,c] (for each c, v is solved from the first non-zero row
of the column and all four rows are checked); else UNEXPLAINED. A stripe's word
is the OR over its columns. Deliberately NOT the kernel's method (ratios of the
first row): this is the statement, that the shortcut."""
import numpy as np

from oracle import rs_oracle as O

UNEXPLAINED = 0x80000000
K, M, N = 10, 4, 14
P = O.build_matrix(K, N)[K:, :]                                # 4 x 10
H = np.concatenate([P, np.eye(M, dtype=np.uint8)], axis=1)     # 4 x 14


def column_word(syn) -> int:
    """Word of one byte column from its 4 syndrome bytes."""
    syn = [int(x) for x in syn]
    if not any(syn):
        return 0
    named = []
    for c in range(N):
        col = [int(x) for x in H[:, c]]
        r0 = next(r for r in range(M) if col[r])
        v = O.gf_div(syn[r0], col[r0])
        if v and all(O.gf_mul(v, col[r]) == syn[r] for r in range(M)):
            named.append(c)
    assert len(named) <= 1, (syn, named)  # any two columns of H are independent
    return 1 << named[0] if named else UNEXPLAINED


def syndromes(shards: np.ndarray) -> np.ndarray:
    """shards [..., 14, L] uint8 -> syndromes [..., 4, L]."""
    shards = np.asarray(shards, dtype=np.uint8)
    out = np.array(shards[..., K:, :], copy=True)
    for j in range(M):
        for i in range(K):
            out[..., j, :] ^= O.MUL_TABLE[int(P[j, i])][shards[..., i, :]]
    return out


def syndrome_word(syn: np.ndarray) -> int:
    """Word of the columns syn [4, L]."""
    cols = np.flatnonzero(syn.any(axis=0))
    word = 0
    for t in {tuple(int(x) for x in syn[:, o]) for o in cols}:
        word |= column_word(t)
    return word


def suspect_words(stripes: np.ndarray):
    """stripes [S, 14, L] uint8 -> the S suspects words."""
    return [syndrome_word(s) for s in syndromes(stripes)]


def mismatch_words(stripes: np.ndarray):
    """stripes [S, 14, L] -> verify's words (bit j = parity shard j differs somewhere)."""
    return [sum(1 << j for j in range(M) if s[j].any()) for s in syndromes(stripes)]
