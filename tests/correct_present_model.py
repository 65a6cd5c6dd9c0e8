"""The masked correct's result contract of include/hec.h
(hec_gpu_correct_present_batch, and the use masks of
hec_gpu_reconstruct_corrected_batch) as numpy, by brute force -- TEST
INFRASTRUCTURE ONLY. Sits on top of tests/check_model.py as
tests/correct_model.py sits on tests/locate_model.py.

For stripes [S, 14, L] and present masks [S]: the corrected image, the check
and suspects words (of the input), the number of stripes the call leaves
inconsistent and the number of bytes changed. A column's name comes from
check_model.column_word, unchanged. Its error value comes from an enumeration:
every v in 1..255 is multiplied into all r rows of the named shard's column of
H_m, and the one whose r bytes equal the column's syndrome is the answer
(exactly one is, asserted). Deliberately NOT the kernel's formula (syn[0] /
A_m[0][c]): this is the statement, that the shortcut. A column whose word is
UNEXPLAINED keeps its bytes, and so does every column of a stripe with fewer
than min_spares spare shards."""
import numpy as np

import check_model as C
from oracle import rs_oracle as O

UNEXPLAINED, K, N, ALL = C.UNEXPLAINED, C.K, C.N, C.ALL


def spares(mask) -> int:
    """r = p - 10 of a present mask (negative or zero: nothing to check)."""
    return bin(int(mask) & ALL).count("1") - K


def column_value(syn, mask: int, shard: int) -> int:
    """The v in 1..255 with syn == v * H_m[:, shard], by enumeration over all r rows."""
    B, E, _, H = C.check_matrix(int(mask) & ALL)
    col = [int(x) for x in H[:, (B + E).index(shard)]]
    syn = [int(x) for x in syn]
    hits = [v for v in range(1, 256) if all(O.gf_mul(v, col[j]) == syn[j] for j in range(len(E)))]
    assert len(hits) == 1, (hex(mask), shard, syn, hits)
    return hits[0]


def correct(stripes, masks, min_spares: int = 2):
    """-> (image [S, 14, L], check words [S], suspects words [S], uncorrected
    stripes, bytes changed). The words are those of the input."""
    assert min_spares in (2, 3, 4)
    out = np.array(stripes, dtype=np.uint8, copy=True)
    check, suspects, uncorrected, changed = [], [], 0, 0
    for s, m in enumerate(masks):
        m = int(m) & ALL
        r = spares(m)
        if r <= 0:
            check.append(0)
            suspects.append(0)
            continue
        E = C.split(m)[1]
        syn = C.syndrome(out[s], m)
        check.append(sum(1 << e for j, e in enumerate(E) if syn[j].any()))
        cols = np.flatnonzero(syn.any(axis=0))
        word = 0
        by_tuple = {}
        for o in cols:
            by_tuple.setdefault(tuple(int(x) for x in syn[:, o]), []).append(int(o))
        for t, where in by_tuple.items():
            name = C.column_word(t, m)
            word |= name
            if name == UNEXPLAINED or r < min_spares:
                continue
            shard = name.bit_length() - 1
            assert name == 1 << shard and m >> shard & 1, hex(name)
            out[s, shard, where] ^= np.uint8(column_value(t, m, shard))
            changed += len(where)
        suspects.append(word)
        if word & UNEXPLAINED or (check[-1] and r < min_spares):
            uncorrected += 1
    return out, check, suspects, uncorrected, changed


def use_masks(masks, check, suspects, min_spares: int = 2):
    """The corrected reconstruct's use masks -> (use masks [S], unrepaired count)."""
    out, left = [], 0
    for m, c, w in zip(masks, check, suspects):
        m = int(m) & ALL
        if int(c) == 0 or (spares(m) >= min_spares and not int(w) & UNEXPLAINED):
            out.append(m)
        else:
            out.append(ALL)
            left += 1
    return out, left
