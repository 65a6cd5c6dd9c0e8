"""tests/update_ragged_model.py without a GPU: the per-stripe wrapper over
update_model pinned against the C oracle's encode on a mixed-length batch, its
write footprint, and the in-place descriptor helper against hec_stripe_desc's
addressing."""
import numpy as np

import update_model
import update_ragged_model as R
from oracle import corc

LENS = [1, 15, 16, 17, 33, 1000, 4096, 4099]


def rand(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8)


def mixed(rng, with_old=True):
    """Three separate arenas with different strides; the parity is the old data's codeword."""
    S = len(LENS)
    masks = [int(m) for m in rng.integers(1, 1 << 10, S)]
    masks[2] = 0                 # a stripe nobody changed
    masks[5] |= 0xFFFF0000       # bits from ten up mean nothing
    par = R.arena_layout(LENS, 4, [16 * (1 + s % 3) for s in range(S)], gap=32, lead=16)
    new = R.arena_layout(LENS, 10, [16 * (s % 4) for s in range(S)], order=list(reversed(range(S))))
    old = R.arena_layout(LENS, 10, [48] * S, gap=16)
    d_par, d_new, d_old = rand(rng, par[2]), rand(rng, new[2]), rand(rng, old[2])
    descs = R.desc_rows(LENS, masks, par[:2], new[:2], old[:2] if with_old else None)
    for s, ln in enumerate(LENS):  # the stored parity: the codeword of the old data (zero without an old arena)
        data = R.shard_rows(d_old, old[0][s], old[1][s], ln, 10) if with_old else np.zeros((10, ln), np.uint8)
        code = corc.encode_stripes(np.ascontiguousarray(data[None]))[0]
        for j in range(4):
            d_par[par[0][s] + j * par[1][s]: par[0][s] + j * par[1][s] + ln] = code[j]
    return d_par, d_old if with_old else None, d_new, descs, masks


def test_mixed_lengths_over_codewords_give_the_encode_of_the_merged_data():
    rng = np.random.default_rng(0x4A66)
    d_par, d_old, d_new, descs, masks = mixed(rng)
    after = R.updated(d_par, d_old, d_new, descs)
    for s, d in enumerate(descs):
        po, ps, no, ns, oo, os_, ln, mask = d
        old, new = R.shard_rows(d_old, oo, os_, ln, 10), R.shard_rows(d_new, no, ns, ln, 10)
        want = corc.encode_stripes(np.ascontiguousarray(update_model.merged(old[None], new[None], [mask])))[0]
        assert np.array_equal(R.shard_rows(after, po, ps, ln, 4), want), s
    # nothing but [0, len) of the four parity shards of the stripes with U non-empty moves
    touched = np.zeros(d_par.size, bool)
    for po, ps, _no, _ns, _oo, _os, ln, mask in descs:
        if mask & 0x3FF:
            for j in range(4):
                touched[po + j * ps: po + j * ps + ln] = True
    assert np.array_equal(after[~touched], d_par[~touched])
    assert (after != d_par).any()


def test_accumulation_without_old_over_a_partition_is_the_encode():
    rng = np.random.default_rng(0x4A67)
    d_par, _none, d_new, descs, _masks = mixed(rng, with_old=False)
    for parts in ([0x007, 0x0F8, 0x300], [0x3FF], [0x2AA, 0x155]):
        acc = d_par.copy()  # zero parity inside the shards (the codeword of zero data)
        for w in parts:
            acc = R.updated(acc, None, d_new, [d[:7] + (w,) for d in descs])
        for s, d in enumerate(descs):
            po, ps, no, ns, _oo, _os, ln, _m = d
            want = corc.encode_stripes(np.ascontiguousarray(R.shard_rows(d_new, no, ns, ln, 10)[None]))[0]
            assert np.array_equal(R.shard_rows(acc, po, ps, ln, 4), want), (s, parts)


def test_in_place_descriptors_address_the_ragged_arena():
    """update_descs_in_place against hec_stripe_desc's addressing (shard i of a
    stripe at offset + i * shard_stride): the old shards are shards 0..9, the
    parity shards are shards 10..13."""
    import helyim_amd.batch as B
    rng = np.random.default_rng(0x4A68)
    S = len(LENS)
    arena = R.arena_layout(LENS, 14, [16 * (1 + s % 5) for s in range(S)], gap=48)
    new = R.arena_layout(LENS, 10, [32] * S, lead=64)
    descs = np.array([(arena[0][s], arena[1][s], LENS[s], 0x3FFF) for s in range(S)], dtype=B.desc_dtype())
    new_descs = [(new[0][s], new[1][s], LENS[s], 0) for s in range(S)]
    masks = rng.integers(0, 1 << 10, S).astype(np.uint32)
    got = B.update_descs_in_place(descs, new_descs, masks)
    assert got.dtype == B.update_desc_dtype() and got.dtype.itemsize == 56 and got.dtype.names == R.FIELDS
    assert [tuple(int(x) for x in r) for r in got] == R.in_place_descs(descs, new_descs, masks)
    for s in range(S):
        off, stride = arena[0][s], arena[1][s]
        for c in range(10):
            assert int(got["old_offset"][s]) + c * int(got["old_stride"][s]) == off + c * stride
            assert int(got["new_offset"][s]) + c * int(got["new_stride"][s]) == new[0][s] + c * new[1][s]
        for j in range(4):
            assert int(got["parity_offset"][s]) + j * int(got["parity_stride"][s]) == off + (10 + j) * stride
    # the model over an in-place arena: encode's parity of the merged data, the data shards untouched
    base, d_new = rand(rng, arena[2]), rand(rng, new[2])
    for s, ln in enumerate(LENS):
        code = corc.encode_stripes(np.ascontiguousarray(R.shard_rows(base, arena[0][s], arena[1][s], ln, 10)[None]))[0]
        for j in range(4):
            at = arena[0][s] + (10 + j) * arena[1][s]
            base[at: at + ln] = code[j]
    after = R.updated(base, base, d_new, got)
    for s, ln in enumerate(LENS):
        rows = R.shard_rows(after, arena[0][s], arena[1][s], ln, 14)
        old = R.shard_rows(base, arena[0][s], arena[1][s], ln, 10)
        assert np.array_equal(rows[:10], old), s
        merged = update_model.merged(old[None], R.shard_rows(d_new, new[0][s], new[1][s], ln, 10)[None], [masks[s]])
        assert np.array_equal(rows[10:], corc.encode_stripes(np.ascontiguousarray(merged))[0]), s
    with np.testing.assert_raises(ValueError):
        B.update_descs_in_place(descs, new_descs[:-1], masks)
    with np.testing.assert_raises(ValueError):
        B.update_descs_in_place(descs, [(o, st, ln + 1, 0) for o, st, ln, _ in new_descs], masks)
