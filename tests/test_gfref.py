"""The batched plain reference of tests/gfref.py and its every-mask image,
pinned against the C oracle and the numpy oracle on the CPU."""
import numpy as np
import pytest

import gfref
from oracle import corc
from oracle import rs_oracle as O

CODECS = [(3, 2), (6, 3), (10, 2), (10, 4), (10, 6), (8, 8), (1, 15), (15, 1)]


@pytest.mark.parametrize("k,m", CODECS)
def test_ref_encode_equals_the_c_oracle(k, m):
    rng = np.random.default_rng(100 * k + m)
    crs = corc.CReedSolomon(k, m)
    for S, L in ((1, 1), (5, 17), (3, 4096 + 3)):
        data = rng.integers(0, 256, (S, k, L), dtype=np.uint8)
        par = gfref.ref_encode(k, m, data)
        assert par.shape == (S, m, L) and par.dtype == np.uint8
        for s in range(S):
            bufs = [data[s, i].copy() for i in range(k)] + [np.zeros(L, np.uint8) for _ in range(m)]
            crs.encode(bufs)
            for j in range(m):
                assert np.array_equal(par[s, j], bufs[k + j]), (k, m, S, L, s, j)


@pytest.mark.parametrize("k,m", CODECS)
def test_torch_encode_equals_ref_encode(k, m):
    import torch
    rng = np.random.default_rng(200 * k + m)
    for S, L in ((1, 1), (7, 17), (5, 1000)):
        data = rng.integers(0, 256, (S, k, L), dtype=np.uint8)
        want = gfref.ref_encode(k, m, data)
        t = torch.from_numpy(data)
        assert np.array_equal(gfref.torch_encode(k, m, t).numpy(), want)
        # several chunks of stripes (an index tensor of at most two stripes), a strided input and output
        wide = torch.zeros((S, k + m, L + 5), dtype=torch.uint8)
        wide[:, :k, :L] = t
        out = gfref.torch_encode(k, m, wide[:, :k, :L], out=wide[:, k:, :L], max_index_bytes=2 * 8 * L)
        assert out.data_ptr() == wide[:, k:, :L].data_ptr()
        assert np.array_equal(wide[:, k:, :L].numpy(), want)
        assert not wide[:, :, L:].any()


def _check_stripe_with(reconstruct, case, k, m, L, s):
    """reconstruct(bufs, present) on stripe s of the start image must give
    exactly the expected image's stripe."""
    n = k + m
    present = [bool(p) for p in case.tables.present[s]]
    bufs = [case.start[s, i, :L].copy() for i in range(n)]
    reconstruct(bufs, present)
    for i in range(n):
        assert np.array_equal(bufs[i], case.expected[s, i, :L]), (k, m, s, i)


@pytest.mark.parametrize("k,m,stride", [(3, 2, 1), (6, 3, 1), (10, 2, 1), (8, 8, 31), (10, 6, 31), (4, 12, 31)])
def test_all_masks_case_is_what_the_oracles_reconstruct(k, m, stride):
    """Every decodable mask (the small codecs) or every 31st mask (about 2000
    of the 16-shard codecs): the C oracle turns the poisoned-and-garbaged
    stripe into exactly the expected stripe; on the small codecs the numpy
    oracle too."""
    n, L, pitch = k + m, 17, 19
    case = gfref.all_masks_case(k, m, L, pitch, seed=7 * k + m)
    tb = case.tables
    S = 1 << n
    assert case.start.shape == case.expected.shape == (S, n, pitch)
    assert tb.n_bad == sum(1 for s in range(S) if bin(s).count("1") < k)
    # pitch bytes, skipped and complete stripes: the same in both images; codeword stripes where nothing is garbage
    assert np.array_equal(case.start[:, :, L:], case.expected[:, :, L:])
    assert np.array_equal(case.start[~tb.decodable], case.expected[~tb.decodable])
    full = case.expected[S - 1]
    assert np.array_equal(gfref.ref_encode(k, m, full[None, :k, :L])[0], full[k:, :L])
    crs = corc.CReedSolomon(k, m)
    ors = O.ReedSolomon(k, m)

    def c_reconstruct(bufs, present):
        assert crs.reconstruct(bufs, present) == 0

    def numpy_reconstruct(bufs, present):
        sh = [b if p else None for b, p in zip(bufs, present)]
        ors.reconstruct(sh)
        for i, p in enumerate(present):
            if not p:
                bufs[i][:] = sh[i]

    checked = 0
    for s in range(0, S, stride):
        if not tb.decodable[s]:
            continue
        erased = [i for i in range(n) if not (s >> i) & 1]
        assert (case.start[s, erased, :L] == gfref.POISON).all()
        _check_stripe_with(c_reconstruct, case, k, m, L, s)
        if stride == 1:
            _check_stripe_with(numpy_reconstruct, case, k, m, L, s)
        checked += 1
    assert checked == int(tb.decodable[::stride].sum()) and checked >= 15
    # the garbage is there: some stripe has a surplus survivor that is not its codeword parity
    assert tb.surplus.any() == (m > 1)


def test_all_masks_case_torch_equals_numpy():
    import torch
    k, m, L, pitch = 6, 3, 17, 32
    case = gfref.all_masks_case(k, m, L, pitch, seed=3)
    twin = gfref.all_masks_case_torch(k, m, L, pitch, seed=3, device="cpu", image=torch.from_numpy(case.raw))
    assert np.array_equal(twin.start.numpy(), case.start)
    assert np.array_equal(twin.expected.numpy(), case.expected)
    own = gfref.all_masks_case_torch(k, m, L, pitch, seed=3, device="cpu")
    assert tuple(own.start.shape) == case.start.shape
    back = gfref.all_masks_case(k, m, L, pitch, seed=0, image=own.raw.numpy())
    assert np.array_equal(own.start.numpy(), back.start) and np.array_equal(own.expected.numpy(), back.expected)


def test_describe_first_difference_names_the_role():
    k, m, L = 3, 2, 17
    case = gfref.all_masks_case(k, m, L, 19, seed=1)
    got = case.expected.copy()
    assert gfref.describe_first_difference(got, case.expected, case.tables, L) == "no difference"
    got[0b01011, 2, 5] ^= 1  # shard 2 erased in mask 0b01011
    text = gfref.describe_first_difference(got, case.expected, case.tables, L)
    assert text.startswith("stripe 11 (present mask 0xb) shard 2 byte 5: erased slot"), text
    # the torch form walks the images in chunks of stripes and names the same byte
    import torch
    assert gfref.describe_first_difference(torch.from_numpy(got), torch.from_numpy(case.expected), case.tables,
                                           L) == text
    got[0b11100, 4, 18] ^= 1  # a later stripe, past the shard's 17 bytes: still the first difference counts
    assert gfref.describe_first_difference(got, case.expected, case.tables, L) == text
    plain = gfref.describe_first_difference(got[12:], case.expected[12:], None, L, first=12)
    assert plain.startswith("stripe 28 shard 4 byte 18: pitch byte past the shard"), plain
