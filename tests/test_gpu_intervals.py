"""Batched degraded-read reconstruct: many independent
stripes of arbitrary lengths and erasure patterns in one GPU round trip,
bit-exact against the oracle."""
import numpy as np
import pytest

from oracle import corc
from oracle import rs_oracle as O

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["zero_copy", "copies"])
def staging_path(request, gpu):
    """The compact staging is decoded in place by the kernel over PCIe (zero
    copy, default) or copied H2D / D2H around the kernel."""
    import helyim_amd as H
    H.lib.hec_set_host_zero_copy(1 if request.param == "zero_copy" else 0)
    yield request.param
    H.lib.hec_set_host_zero_copy(1)


def _stripe(rng, L):
    data = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(10)]
    full = data + [np.zeros(L, np.uint8) for _ in range(4)]
    corc.CReedSolomon(10, 4).encode(full)
    return full


@pytest.mark.parametrize("data_only", [False, True])
def test_reconstruct_batch_ragged(gpu, data_only):
    import helyim_amd as H
    rng = np.random.default_rng(11 + data_only)
    rs = H.ReedSolomon(10, 4)
    lens = [1, 7, 15, 16, 17, 4095, 4096, 4097, 12000, 65536 + 3] + \
        [int(x) for x in np.exp(rng.uniform(np.log(64), np.log(300000), 300))]
    fulls, stripes, erased = [], [], []
    for L in lens:
        full = _stripe(rng, L)
        e = set(rng.choice(14, int(rng.integers(0, 5)), replace=False).tolist())
        fulls.append(full)
        erased.append(e)
        stripes.append([None if i in e else full[i].copy() for i in range(14)])
    rs.reconstruct_batch(stripes, data_only=data_only)
    for full, st, e in zip(fulls, stripes, erased):
        for i in range(14):
            if data_only and i >= 10 and i in e:
                assert st[i] is None
            else:
                assert np.array_equal(st[i], full[i])


def test_reconstruct_batch_generic_geometry(gpu):
    import helyim_amd as H
    rng = np.random.default_rng(5)
    rs, ors = H.ReedSolomon(6, 3), O.ReedSolomon(6, 3)
    stripes, fulls = [], []
    for L in (3, 100, 5000):
        full = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(6)] + [np.zeros(L, np.uint8)] * 3
        full = [f.copy() for f in full]
        ors.encode(full)
        fulls.append(full)
        stripes.append([None if i in (1, 7) else full[i].copy() for i in range(9)])
    rs.reconstruct_batch(stripes)
    for full, st in zip(fulls, stripes):
        for a, b in zip(full, st):
            assert np.array_equal(a, b)


def _every_mask_stripes_63():
    """RS(6,3): one stripe per decodable mask (129) plus 3 complete ones,
    lengths cycling through (3, 100, 4097); survivors after the first 6 present
    hold garbage (gfref.all_masks_case). -> [(mask, start shards, expected shards)]"""
    import gfref
    k, m, n = 6, 3, 9
    lens = (3, 100, 4097)
    cases = {L: gfref.all_masks_case(k, m, L, L, seed=63 + L) for L in lens}
    tb = cases[3].tables
    chosen = [int(s) for s in np.flatnonzero(tb.decodable)]
    assert len(chosen) == 129
    chosen[40:40] = [(1 << n) - 1]  # complete stripes between the others and at both ends
    chosen = [(1 << n) - 1] + chosen + [(1 << n) - 1]
    out = []
    for j, s in enumerate(chosen):
        c = cases[lens[j % 3]]
        out.append((s, [c.start[s, i].copy() for i in range(n)], [c.expected[s, i].copy() for i in range(n)]))
    return out


@pytest.mark.parametrize("data_only", [False, True])
def test_reconstruct_batch_generic_every_mask(gpu, data_only):
    """The generic branch of hec_rs_reconstruct_batch on every decodable mask
    of RS(6,3) in one call."""
    import helyim_amd as H
    k, n = 6, 9
    rs = H.ReedSolomon(6, 3)
    table = _every_mask_stripes_63()
    assert len(table) == 132
    stripes = [[sh[i] if (s >> i) & 1 else None for i in range(n)] for s, sh, _ in table]
    rs.reconstruct_batch(stripes, data_only=data_only)
    for j, ((s, _, want), st) in enumerate(zip(table, stripes)):
        for i in range(n):
            if data_only and i >= k and not (s >> i) & 1:
                assert st[i] is None, (j, hex(s), i)
            else:
                assert st[i] is not None and np.array_equal(st[i], want[i]), (j, hex(s), data_only, i)


def test_reconstruct_batch_generic_error_writes_nothing(gpu):
    """One stripe with 5 of RS(6,3)'s shards present in the middle of the
    every-mask batch: TooFewShardsPresent naming that stripe, and no byte of
    any buffer of any stripe is written (hec.h: "on error nothing is written")."""
    import ctypes
    import helyim_amd as H
    from helyim_amd.rs import _len_array, _ptr_array
    k, n = 6, 9
    rs = H.ReedSolomon(6, 3)
    table = _every_mask_stripes_63()
    bad_at = 70
    few = 0b000011111
    table.insert(bad_at, (few, [b.copy() for b in table[5][1]], None))
    # through the Python mirror: absent slots are None
    stripes = [[sh[i].copy() if (s >> i) & 1 else None for i in range(n)] for s, sh, _ in table]
    with pytest.raises(H.TooFewShardsPresent) as ei:
        rs.reconstruct_batch(stripes)
    assert ei.value.stripe == bad_at
    for (s, sh, _), st in zip(table, stripes):
        for i in range(n):
            assert (st[i] is None) if not (s >> i) & 1 else np.array_equal(st[i], sh[i])
    # the C ABI: every slot has a buffer (absent ones hold poison), all must come back as they were
    flat = [b.copy() for _, sh, _ in table for b in sh]
    before = [b.copy() for b in flat]
    present = (ctypes.c_uint8 * len(flat))(*[(s >> i) & 1 for s, _, _ in table for i in range(n)])
    bad = ctypes.c_size_t(12345)
    for data_only in (0, 1):
        rc = H.lib.hec_rs_reconstruct_batch(rs.handle, _ptr_array(flat), _len_array(flat), present, len(table),
                                            data_only, ctypes.byref(bad))
        assert rc == H.TooFewShardsPresent.code and bad.value == bad_at
        for j, (a, b) in enumerate(zip(flat, before)):
            assert np.array_equal(a, b), (data_only, "stripe", j // n, "shard", j % n)
