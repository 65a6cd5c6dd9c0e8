"""tests/update_model.py against the C oracle's encode, without a GPU: the
model over a codeword's parity gives the parity of the merged data for every
mask, it holds for any parity, and accumulating from zero parity over any split
of the data shards is the encode."""
import numpy as np

import update_model as M
from oracle import corc

K, MP, L = 10, 4, 33


def rand(rng, *shape):
    return rng.integers(0, 256, shape, dtype=np.uint8)


def test_every_mask_over_a_codeword_is_the_encode_of_the_merged_data():
    rng = np.random.default_rng(0x0DD0)
    S = 1 << K
    masks = np.arange(S, dtype=np.uint32)
    old, new = rand(rng, S, K, L), rand(rng, S, K, L)
    before = corc.encode_stripes(old)
    after = M.updated_parity(before, old, new, masks)
    assert np.array_equal(after, corc.encode_stripes(np.ascontiguousarray(M.merged(old, new, masks))))
    assert np.array_equal(after[0], before[0])  # mask 0: nothing changes
    assert (after[1:] != before[1:]).any(axis=(1, 2)).all()  # 33 random bytes: every other stripe's parity moves


def test_bits_from_ten_up_mean_nothing():
    rng = np.random.default_rng(0x0DD1)
    S = 64
    masks = rng.integers(0, 1 << K, S).astype(np.uint32)
    old, new, parity = rand(rng, S, K, L), rand(rng, S, K, L), rand(rng, S, MP, L)
    want = M.updated_parity(parity, old, new, masks)
    assert np.array_equal(M.updated_parity(parity, old, new, masks | np.uint32(0xFFFFFC00)), want)
    assert np.array_equal(M.updated_parity(parity, old, new, np.full(S, 0xFFFFFC00, np.uint32)), parity)


def test_linearity_holds_for_any_parity():
    """Random parity before the call: the change is the encode of the masked delta, whatever the parity was."""
    rng = np.random.default_rng(0x0DD2)
    S = 128
    masks = rng.integers(0, 1 << K, S).astype(np.uint32)
    old, new, parity = rand(rng, S, K, L), rand(rng, S, K, L), rand(rng, S, MP, L)
    after = M.updated_parity(parity, old, new, masks)
    delta = np.ascontiguousarray(np.where(M.changed(masks, K)[:, :, None], old ^ new, np.uint8(0)))
    assert np.array_equal(after ^ parity, corc.encode_stripes(delta))
    # shards outside U take no part, whatever they hold
    noise_old = np.where(M.changed(masks, K)[:, :, None], old, rand(rng, S, K, L))
    noise_new = np.where(M.changed(masks, K)[:, :, None], new, rand(rng, S, K, L))
    assert np.array_equal(M.updated_parity(parity, noise_old, noise_new, masks), after)


def splits(rng):
    yield [0x007, 0x0F8, 0x300]
    yield [1 << c for c in range(K)]
    yield [0x3FF]
    yield [0x155, 0x2AA]
    for _ in range(40):  # random partitions of 0..9 into 1 to 10 parts, in random order
        parts = rng.integers(1, K + 1)
        owner = rng.integers(0, parts, K)
        words = [int(sum(1 << c for c in range(K) if owner[c] == p)) for p in range(parts)]
        rng.shuffle(words)
        yield words


def test_progressive_accumulation_over_any_split_is_the_encode():
    rng = np.random.default_rng(0x0DD3)
    S = 16
    data = rand(rng, S, K, L)
    want = corc.encode_stripes(data)
    for words in splits(rng):
        assert sum(words) == 0x3FF and all(a & b == 0 for i, a in enumerate(words) for b in words[:i])
        parity = np.zeros((S, MP, L), np.uint8)
        for w in words:
            parity = M.updated_parity(parity, None, data, np.full(S, w, np.uint32))
        assert np.array_equal(parity, want), [hex(w) for w in words]


def test_other_codecs():
    rng = np.random.default_rng(0x0DD4)
    for k, m in ((5, 5), (3, 2)):
        S = 1 << k
        masks = np.arange(S, dtype=np.uint32)
        old, new = rand(rng, S, k, L), rand(rng, S, k, L)
        rs = corc.CReedSolomon(k, m)

        def encode(data):
            out = np.zeros((S, m, L), np.uint8)
            for s in range(S):
                bufs = [data[s, i].copy() for i in range(k)] + [np.zeros(L, np.uint8) for _ in range(m)]
                rs.encode(bufs)
                out[s] = bufs[k:]
            return out

        after = M.updated_parity(encode(old), old, new, masks, k, m)
        assert np.array_equal(after, encode(M.merged(old, new, masks, k)))
