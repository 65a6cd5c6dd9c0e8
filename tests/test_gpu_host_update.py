"""hec_host_update_batch on the GPU against tests/update_model.py, down the three
staging paths of the host driver: pinned memory in place, pageable memory
through the pinned slots, and H2D / D2H copies with zero copy off. The delta
and parity arenas hold seeded random bytes in every pad and gap; the delta
arena must come back unchanged and the parity arena different only in [0, L) of
the parity shards of the stripes whose mask names a shard."""
import numpy as np
import pytest

import update_model as M

pytestmark = pytest.mark.gpu

K, MP = 10, 4
S, L = 41, 1000                  # under the small-chunk build: 13 chunks of 3 stripes and one of 2
DELTA_PITCH, PARITY_PITCH = 1008, 1024
HIGH = 0xFFFFFC00


def masks_of(n, seed):
    """n >= 13 update masks: empty stripes at both ends and in the middle,
    single shards, all ten, and bits that mean nothing on some words."""
    rng = np.random.default_rng(seed)
    m = rng.integers(1, 1 << K, n).astype(np.uint32)
    m[2:2 + K] = 1 << np.arange(K, dtype=np.uint32)
    m[2 + K] = 0x3FF
    m[[0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1]] = 0
    m[[2, n // 2, n - 2]] |= np.uint32(HIGH)  # n // 2 stays empty: the high bits alone name nothing
    return m


def arenas(n, length, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 256, (n, K, DELTA_PITCH), dtype=np.uint8),
            rng.integers(0, 256, (n, MP, PARITY_PITCH), dtype=np.uint8))


def expected(delta, parity, masks, length):
    want = parity.copy()
    after = M.updated_parity(np.ascontiguousarray(parity[:, :, :length]), None,
                             np.ascontiguousarray(delta[:, :, :length]), masks)
    live = (np.asarray(masks) & 0x3FF) != 0
    want[live, :, :length] = after[live]
    assert np.array_equal(want[~live], parity[~live])
    return want


def host_update(rs, delta, parity, masks, length):
    """batch.host_update_batch on the [n, shards, pitch] arrays' first `length` bytes a shard, in place."""
    import torch

    import helyim_amd.batch as B
    B.host_update_batch(rs, torch.from_numpy(delta)[:, :, :length], torch.from_numpy(parity)[:, :, :length], masks)


def run_three_paths(n, length, seed):
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(K, MP)
    masks = masks_of(n, seed)
    delta, parity = arenas(n, length, seed + 1)
    want = expected(delta, parity, masks, length)
    got = {}
    # pinned, GPU-addressable memory: coded in place
    pd, pp = H.HostBuffer(delta.nbytes), H.HostBuffer(parity.nbytes)
    hd, hp = pd.array.reshape(delta.shape), pp.array.reshape(parity.shape)
    hd[:], hp[:] = delta, parity
    assert B.host_zero_copy(pd.tensor(delta.shape)) and B.host_zero_copy(pp.tensor(parity.shape))
    host_update(rs, hd, hp, masks, length)
    got["pinned"] = hp.copy()
    assert np.array_equal(hd, delta)
    del hd, hp, pd, pp
    # pageable memory through the pinned slots
    d, p = delta.copy(), parity.copy()
    host_update(rs, d, p, masks, length)
    got["pageable"] = p
    assert np.array_equal(d, delta)
    # the copy pipeline
    assert H.lib.hec_set_host_zero_copy(0) == 0
    try:
        d, p = delta.copy(), parity.copy()
        host_update(rs, d, p, masks, length)
        got["copies"] = p
        assert np.array_equal(d, delta)
    finally:
        assert H.lib.hec_set_host_zero_copy(1) == 0
    for path, p in got.items():
        diff = np.argwhere(p != want)
        assert not len(diff), (path, "stripe, parity shard, byte", diff[0].tolist(), hex(int(masks[diff[0][0]])))


def test_three_paths_give_the_models_parity(gpu):
    run_three_paths(S, L, 0x40570)


@pytest.mark.parametrize("length", [1, 999, 1008])
def test_other_lengths(gpu, length):
    run_three_paths(13, length, 0x40580 + length)


def test_progressive_encode_on_host_memory(gpu):
    """The delta is the new shard itself where the parity has not seen it: over
    zeroed parity three calls on a partition of the data shards give the encode."""
    import helyim_amd as H
    from oracle import corc
    rs = H.ReedSolomon(K, MP)
    data, parity = arenas(S, L, 0x40590)
    parity[:, :, :L] = 0
    start = parity.copy()
    for word in (0x007, 0x0F8, 0x300):
        host_update(rs, data, parity, np.full(S, word, np.uint32), L)
    assert np.array_equal(parity[:, :, :L], corc.encode_stripes(np.ascontiguousarray(data[:, :, :L])))
    assert np.array_equal(parity[:, :, L:], start[:, :, L:])
