"""Parity of the HIP path against the oracle (GPU). Every comparison is
bit-exact: this is GF(2^8) byte arithmetic."""
import itertools

import numpy as np
import pytest

from oracle import corc
from oracle import rs_oracle as O

pytestmark = pytest.mark.gpu


def _rand(rng, L):
    return rng.integers(0, 256, L, dtype=np.uint8)


def test_encode_host_api_golden(gpu, golden):
    import helyim_amd as H
    g = golden("encode_vectors.json")
    rs = H.ReedSolomon(10, 4)
    for L, ent in g["vectors"].items():
        L = int(L)
        data = corc.splitmix64_bytes(g["seed"], 10 * L).reshape(10, L)
        shards = [data[i].copy() for i in range(10)] + [np.zeros(L, np.uint8) for _ in range(4)]
        rs.encode(shards)
        assert [O.sha256(s) for s in shards[10:]] == ent["parity_sha256"], L
        assert rs.verify(shards)
        shards[12][L // 2] ^= 1
        assert not rs.verify(shards)


def test_rs_5_5_kat_through_product(gpu, golden):
    import helyim_amd as H
    kat = golden("upstream_kat.json")["rs_5_5_one_encode"]
    shards = [np.array(d, np.uint8) for d in kat["data"]] + [np.zeros(2, np.uint8) for _ in range(5)]
    H.ReedSolomon(5, 5).encode(shards)
    assert [s.tolist() for s in shards[5:]] == kat["parity"]


@pytest.mark.parametrize("k,m", [(10, 4), (3, 2), (17, 3), (4, 6), (1, 1), (12, 9), (30, 2)])
def test_generic_geometry_encode_reconstruct(gpu, k, m):
    import helyim_amd as H
    rng = np.random.default_rng(1000 * k + m)
    rs, ors = H.ReedSolomon(k, m), O.ReedSolomon(k, m)
    for L in (1, 17, 1000, 4096 + 3):
        data = [_rand(rng, L) for _ in range(k)]
        sh = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(m)]
        ref = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(m)]
        rs.encode(sh)
        ors.encode(ref)
        for a, b in zip(sh, ref):
            assert np.array_equal(a, b)
        for _ in range(4):
            e = int(rng.integers(1, m + 1))
            erased = set(rng.choice(k + m, e, replace=False).tolist())
            got = [None if i in erased else ref[i].copy() for i in range(k + m)]
            rs.reconstruct(got)
            for i in range(k + m):
                assert np.array_equal(got[i], ref[i]), (k, m, L, sorted(erased), i)


def test_random_geometries_property_sweep(gpu):
    """Seeded hypothesis sweep through the product's per-call API: random
    geometries (k + m <= 256), shard lengths 1 B .. 40 KiB (both sides of the
    16-byte alignment and of the table kernels' 4 KiB column range), random
    erasure sets of 1..m shards and reconstruct_data, against the C oracle."""
    from hypothesis import given, settings, HealthCheck, strategies as st
    import helyim_amd as H
    from oracle import corc

    @settings(max_examples=60, deadline=None, derandomize=True,
              suppress_health_check=[HealthCheck.too_slow])
    @given(st.integers(1, 200), st.integers(1, 56), st.integers(1, 40 << 10), st.integers(0, 2**32 - 1),
           st.booleans())
    def check(k, m, L, seed, data_only):
        rng = np.random.default_rng(seed)
        n = k + m
        rs, crs = H.ReedSolomon(k, m), corc.CReedSolomon(k, m)
        data = [_rand(rng, L) for _ in range(k)]
        sh = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(m)]
        ref = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(m)]
        rs.encode(sh)
        crs.encode(ref)
        for i in range(n):
            assert np.array_equal(sh[i], ref[i]), (k, m, L, i)
        e = int(rng.integers(1, m + 1))
        erased = set(rng.choice(n, e, replace=False).tolist())
        got = [None if i in erased else ref[i].copy() for i in range(n)]
        if data_only:
            rs.reconstruct_data(got)
            for i in range(n):
                if i < k or i not in erased:
                    assert np.array_equal(got[i], ref[i]), (k, m, L, sorted(erased), i)
                else:
                    assert got[i] is None, (k, m, i)  # missing parity stays missing (upstream)
        else:
            rs.reconstruct(got)
            for i in range(n):
                assert np.array_equal(got[i], ref[i]), (k, m, L, sorted(erased), i)

    check()


@pytest.mark.parametrize("k,m", [(255, 1), (1, 255), (128, 128), (200, 56)])
def test_widest_geometries_encode_reconstruct(gpu, k, m):
    """The widest codecs upstream accepts (data + parity = 256, the GF(2^8)
    limit; ReedSolomon::new refuses 257) through the per-call API: encode,
    verify, and reconstruct / reconstruct_data with the most erasures the code
    can take (m), the first m data shards erased, and every parity shard
    erased, against the numpy oracle."""
    import helyim_amd as H
    rng = np.random.default_rng(4000 + 7 * k + m)
    n = k + m
    rs, ors = H.ReedSolomon(k, m), O.ReedSolomon(k, m)
    with pytest.raises(H.TooManyShards):
        H.ReedSolomon(k, m + 1)
    for L in (1, 4096 + 3):
        data = [_rand(rng, L) for _ in range(k)]
        sh = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(m)]
        ref = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(m)]
        rs.encode(sh)
        ors.encode(ref)
        for i in range(n):
            assert np.array_equal(sh[i], ref[i]), (k, m, L, i)
        assert rs.verify(sh)
        patterns = [set(rng.choice(n, m, replace=False).tolist()), set(range(min(k, m))), set(range(k, n))]
        for erased in patterns:
            got = [None if i in erased else ref[i].copy() for i in range(n)]
            rs.reconstruct(got)
            for i in range(n):
                assert np.array_equal(got[i], ref[i]), (k, m, L, i)
            got = [None if i in erased else ref[i].copy() for i in range(n)]
            rs.reconstruct_data(got)
            for i in range(n):
                if i in erased and i >= k:
                    assert got[i] is None
                else:
                    assert np.array_equal(got[i], ref[i]), (k, m, L, i)
        # the batched degraded-read entry point, one stripe per pattern
        stripes = [[None if i in erased else ref[i].copy() for i in range(n)] for erased in patterns]
        rs.reconstruct_batch(stripes)
        for st in stripes:
            for i in range(n):
                assert np.array_equal(st[i], ref[i]), (k, m, L, i)


@pytest.mark.parametrize("k,m", [(255, 1), (128, 128), (1, 255)])
def test_widest_geometries_batch_encode(gpu, k, m):
    """Batch encodes of the widest codecs (the plan kernel with up to 255
    inputs or outputs): a device batch and a pinned and a pageable host batch
    (zero copy and the copy pipeline), against the C oracle. (Batch
    reconstructs take per-stripe masks and stop at 16 shards.)"""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rng = np.random.default_rng(5000 + k)
    n, S, L = k + m, 3, 4096 + 5
    rs, ors = H.ReedSolomon(k, m), corc.CReedSolomon(k, m)
    host = np.zeros((S, n, L), np.uint8)
    host[:, :k] = rng.integers(0, 256, (S, k, L), dtype=np.uint8)
    for s in range(S):
        ors.encode([host[s, i] for i in range(n)])
    t = torch.zeros((S, n, L), dtype=torch.uint8, device="cuda")
    t[:, :k] = torch.from_numpy(host[:, :k]).cuda()
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), host)
    for pin in (True, False):
        for zc in (1, 0):
            assert H.lib.hec_set_host_zero_copy(zc) == 0
            try:
                h = torch.zeros((S, n, L), dtype=torch.uint8)
                if pin:
                    h = h.pin_memory()
                h.numpy()[:, :k] = host[:, :k]
                B.host_encode_batch(rs, h)
                assert np.array_equal(h.numpy(), host), (pin, zc)
            finally:
                H.lib.hec_set_host_zero_copy(1)


def test_reconstruct_host_api_patterns(gpu):
    import helyim_amd as H
    rng = np.random.default_rng(7)
    rs = H.ReedSolomon(10, 4)
    L = 65536 + 7
    full = [_rand(rng, L) for _ in range(10)] + [np.zeros(L, np.uint8) for _ in range(4)]
    O.ReedSolomon(10, 4).encode(full)
    pats = [c for e in range(1, 5) for c in itertools.combinations(range(14), e)]
    for idx in rng.choice(len(pats), 60, replace=False):
        erased = set(pats[idx])
        got = [None if i in erased else full[i].copy() for i in range(14)]
        rs.reconstruct(got)
        for i in range(14):
            assert np.array_equal(got[i], full[i])
        got = [None if i in erased else full[i].copy() for i in range(14)]
        rs.reconstruct_data(got)
        for i in range(14):
            if i in erased and i >= 10:
                assert got[i] is None
            else:
                assert np.array_equal(got[i], full[i])
    with pytest.raises(H.TooFewShardsPresent):
        rs.reconstruct([None] * 5 + full[5:])


@pytest.mark.parametrize("zero_copy", [1, 0])
@pytest.mark.parametrize("staging", ["off", "on", "edge"])
@pytest.mark.parametrize("k,m", [(10, 4), (3, 2)])
def test_host_calls_staged_and_direct(gpu, staging, k, m, zero_copy):
    """hec_set_host_staging picks pinned staging (the kernel coding the staging
    in place over PCIe, or one H2D + one D2H with zero copy off) or one
    pageable copy per shard; all give the oracle's bytes, including the
    reconstruct_data contract."""
    import helyim_amd as H
    rng = np.random.default_rng(11 * k + m)
    rs, ors = H.ReedSolomon(k, m), O.ReedSolomon(k, m)
    H.lib.hec_set_host_zero_copy(zero_copy)
    try:
        for L in (1, 17, 4096 + 3, 65536 + 7, (128 << 10) + 1, 256 << 10, (1 << 20) + 5):
            lim = {"off": 0, "on": 1 << 40, "edge": k * L}[staging]
            H.lib.hec_set_host_staging(lim)
            data = [_rand(rng, L) for _ in range(k)]
            sh = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(m)]
            ref = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(m)]
            rs.encode(sh)
            ors.encode(ref)
            for a, b in zip(sh, ref):
                assert np.array_equal(a, b), (staging, L)
            assert rs.verify(sh)
            sh[k][L - 1] ^= 0x80
            assert not rs.verify(sh)
            for _ in range(3):
                erased = set(rng.choice(k + m, int(rng.integers(1, m + 1)), replace=False).tolist())
                got = [None if i in erased else ref[i].copy() for i in range(k + m)]
                rs.reconstruct(got)
                for i in range(k + m):
                    assert np.array_equal(got[i], ref[i]), (staging, L, sorted(erased), i)
                got = [None if i in erased else ref[i].copy() for i in range(k + m)]
                rs.reconstruct_data(got)
                for i in range(k + m):
                    if i in erased and i >= k:
                        assert got[i] is None
                    else:
                        assert np.array_equal(got[i], ref[i])
            with pytest.raises(H.TooFewShardsPresent):
                rs.reconstruct([None] * (m + 1) + ref[m + 1:])
            with pytest.raises(H.IncorrectShardSize):
                rs.reconstruct([None, np.zeros(L + 1, np.uint8)] + ref[2:])
    finally:
        H.lib.hec_set_host_staging(16 << 20)
        H.lib.hec_set_host_zero_copy(1)


@pytest.mark.parametrize("signal", [1 << 20, 0])
def test_host_calls_completion_signal(gpu, signal):
    """Small zero-copy host calls finish on the kernel's own completion flag
    (hec_set_completion_signal; 0 = hipStreamSynchronize). 400 back-to-back
    per-call encodes and reconstructs of mixed sizes (one workgroup up to 64
    workgroups per launch, (10,4) through the fast and ragged kernels, (3,2)
    through the generic one), each result against the oracle, so a flag seen
    before the bytes landed, or a counter left non-zero, would show."""
    import helyim_amd as H
    rng = np.random.default_rng(4242)
    H.lib.hec_set_completion_signal(signal)
    try:
        for k, m in ((10, 4), (3, 2)):
            rs, ors = H.ReedSolomon(k, m), O.ReedSolomon(k, m)
            for it in range(200):
                L = int(rng.choice([1, 16, 1000, 4096, 4096 + 16, 65536 + 7, 100 * 1024]))
                ref = [_rand(rng, L) for _ in range(k)] + [np.zeros(L, np.uint8) for _ in range(m)]
                sh = [x.copy() for x in ref]
                ors.encode(ref)
                rs.encode(sh)
                for a, b in zip(sh, ref):
                    assert np.array_equal(a, b), (k, m, it, L)
                erased = set(rng.choice(k + m, int(rng.integers(1, m + 1)), replace=False).tolist())
                got = [None if i in erased else ref[i].copy() for i in range(k + m)]
                rs.reconstruct(got)
                for i in range(k + m):
                    assert np.array_equal(got[i], ref[i]), (k, m, it, L, sorted(erased), i)
    finally:
        H.lib.hec_set_completion_signal(1 << 20)


def test_completion_signal_spin_fallback(gpu):
    """Calls long enough to outlast the 200 us spin (4 MiB shards, 40 MiB
    coded zero-copy over PCIe) with the completion signal forced on: the wait
    falls back to hipStreamSynchronize and must still find the flag set and
    the bytes right."""
    import helyim_amd as H
    rng = np.random.default_rng(99)
    rs, ors = H.ReedSolomon(10, 4), corc.CReedSolomon(10, 4)
    L = 4 << 20
    H.lib.hec_set_completion_signal(1 << 40)
    H.lib.hec_set_host_staging(1 << 40)  # 40 MiB of input through pinned staging (zero copy)
    try:
        for _ in range(3):
            ref = [_rand(rng, L) for _ in range(10)] + [np.zeros(L, np.uint8) for _ in range(4)]
            sh = [x.copy() for x in ref]
            ors.encode(ref)
            rs.encode(sh)
            assert all(np.array_equal(a, b) for a, b in zip(sh, ref))
            got = [None if i in (1, 6, 10, 13) else ref[i].copy() for i in range(14)]
            rs.reconstruct(got)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref))
    finally:
        H.lib.hec_set_completion_signal(1 << 20)
        H.lib.hec_set_host_staging(16 << 20)


def _stripes(S, L, seed_base=O.STRIPE_SEED_BASE):
    import torch
    import helyim_amd.batch as B
    t = torch.empty((S, 14, L), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(t, 10 * L, seed_base)
    return t


def test_fill_splitmix_matches_oracle(gpu):
    S, L = 3, 4097
    t = _stripes(S, L).cpu().numpy()
    for s in range(S):
        ref = corc.splitmix64_bytes(O.STRIPE_SEED_BASE + s, 10 * L).reshape(10, L)
        assert np.array_equal(t[s, :10], ref)


@pytest.mark.parametrize("L", [1, 15, 16, 17, 255, 4096, 4097, 8192 + 16, 65536, 1 << 20])
def test_batch_encode_vs_oracle(gpu, L):
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    S = 6
    rs = H.ReedSolomon(10, 4)
    t = _stripes(S, L)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    host = t.cpu().numpy()
    ref = corc.encode_stripes(np.ascontiguousarray(host[:, :10]))
    assert np.array_equal(host[:, 10:], ref)


def test_bitslice_encode_matches_oracle(gpu):
    """The encode kernels against the C oracle: lengths that are a multiple of
    8 KiB take the bit-sliced kernel, other 16-byte multiples the table
    kernel; in-place [S][14][L] and separate data/parity buffers."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    for S, L in ((5, 8192), (3, 3 * 8192), (2, 1 << 20), (4, 8192 + 16), (3, 4096), (700, 16384)):
        assert H.lib.hec_encode_kernel_name(L).decode().startswith(
            "rs104_bs_encode_kernel" if L % 8192 == 0 else "rs104_kernel<DEC=false>")
        t = _stripes(S, L)
        B.encode_batch(rs, t)
        torch.cuda.synchronize()
        host = t.cpu().numpy()
        ref = corc.encode_stripes(np.ascontiguousarray(host[:, :10]))
        assert np.array_equal(host[:, 10:], ref), (S, L)
        data = t[:, :10].contiguous()
        par = torch.zeros((S, 4, L), dtype=torch.uint8, device="cuda")
        B.encode_batch_sep(rs, data, par)
        torch.cuda.synchronize()
        assert np.array_equal(par.cpu().numpy(), ref), (S, L)
    # every byte value in every shard position (all 256 x 10 inputs)
    S, L = 10, 8192
    t = torch.zeros((S, 14, L), dtype=torch.uint8, device="cuda")
    for s in range(S):
        t[s, s] = torch.arange(L, device="cuda").to(torch.uint8)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    host = t.cpu().numpy()
    assert np.array_equal(host[:, 10:], corc.encode_stripes(np.ascontiguousarray(host[:, :10])))


def test_batch_encode_separate_and_unaligned(gpu):
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    S, L = 4, 5000
    raw = torch.randint(0, 256, (S * 10 * L + 3,), dtype=torch.uint8, device="cuda")
    data = raw[3:].view(S, 10, L)  # 3-byte offset: unaligned path
    par = torch.zeros((S, 4, L), dtype=torch.uint8, device="cuda")
    B.encode_batch_sep(rs, data, par)
    torch.cuda.synchronize()
    ref = corc.encode_stripes(data.cpu().numpy().copy())
    assert np.array_equal(par.cpu().numpy(), ref)


def test_batch_reconstruct_every_pattern(gpu):
    """All 1470 erasure patterns with 1..4 erasures, one per stripe, one launch."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    pats = [c for e in range(1, 5) for c in itertools.combinations(range(14), e)]
    assert len(pats) == 1470
    S, L = len(pats) + 1, 1024 + 48 + 5
    t = _stripes(S, L)
    B.encode_batch(rs, t)
    good = t.clone()
    masks = np.full(S, (1 << 14) - 1, dtype=np.int32)  # last stripe: nothing erased
    for s, p in enumerate(pats):
        for i in p:
            t[s, i] = 0xA5
            masks[s] &= ~(1 << i)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_batch(rs, t, torch.from_numpy(masks).cuda(), bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    assert torch.equal(t, good)


@pytest.mark.parametrize("L", [8192, 3 * 8192, 8 * 8192 + 16, 2048 * 5, 4096 + 48])
def test_decode_kernels_every_pattern(gpu, L):
    """The RS(10,4) decode kernels -- 8 bytes per lane over 2 KiB column
    ranges where the shard length is a multiple of 2 KiB, 16 bytes per lane
    over 4 KiB otherwise -- with all ten loads issued before the math: all
    1470 patterns (erased slots poisoned), plus an all-present stripe (no-op)
    and two with too few present (skipped, counted), vs the originals; the
    kernel-name report follows the length."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    pats = [c for e in range(1, 5) for c in itertools.combinations(range(14), e)]
    S = len(pats) + 3
    t = _stripes(S, L)
    B.encode_batch(rs, t)
    good = t.clone()
    masks = np.full(S, (1 << 14) - 1, dtype=np.int32)
    for s, p in enumerate(pats):
        for i in p:
            t[s, i] = 0xA5
            masks[s] &= ~(1 << i)
    masks[-2] = (1 << 14) - 1 - 0b11111           # 9 present
    masks[-1] = (1 << 14) - 1 - (0b1111 << 10) - 1  # 9 present, all parity gone
    name = H.lib.hec_decode_kernel_name(L).decode()
    assert ("8 B per lane" in name) == (L % 2048 == 0), name
    assert name.startswith("rs104_narrow_kernel<DEC=true" if L % 2048 == 0 else "rs104_kernel<DEC=true>"), name
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_batch(rs, t, torch.from_numpy(masks).cuda(), bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 2
    assert torch.equal(t, good)


def test_batch_reconstruct_too_few_present(gpu):
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    S, L = 3, 4096
    t = _stripes(S, L)
    B.encode_batch(rs, t)
    before = t.clone()
    masks = torch.tensor([(1 << 14) - 1 - 1, (1 << 14) - 1 - 0b11111, (1 << 14) - 1], dtype=torch.int32,
                         device="cuda")
    t[0, 0] = 0
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_batch(rs, t, masks, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 1
    assert torch.equal(t[1], before[1])          # skipped, untouched
    assert torch.equal(t[0], before[0])           # shard 0 rebuilt
    ref = corc.encode_stripes(before[0:1, :10].cpu().numpy().copy())
    assert np.array_equal(t[0, 10:].cpu().numpy(), ref[0])


@pytest.mark.parametrize("pad", [0, 64 << 10])
def test_full_config_roundtrip(gpu, pad):
    """BASELINE config 2/3 sizes (4096 x 1 MiB), packed and in the bench's
    padded layout (a 64 KiB gap after every shard): encode -> erase 4 random
    shards per stripe -> reconstruct == original. EVERY stripe is checked
    against the C oracle (VERDICT r03 "next" 2), copied back in 64-stripe
    chunks and checked on 16 threads: after the encode, all 4096 stripes are
    the oracle's codeword of their seeded data; after the reconstruct, again,
    and all 16,384 rebuilt shards equal the oracle's reconstruct from the same
    survivors. The parity checksum survives the round trip."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    S, L = 4096, 1 << 20
    torch.cuda.empty_cache()
    if pad:
        t = B.empty_stripes(S, 14, L, shard_pad=pad)
        B.fill_stripes_splitmix(t, 10, O.STRIPE_SEED_BASE)
    else:
        t = _stripes(S, L)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    rng = np.random.default_rng(3)
    seeds = O.STRIPE_SEED_BASE + np.arange(S, dtype=np.uint64)
    assert corc.check_device_batch(t, data_seeds=seeds) == []
    parity_sum = t[:, 10:].view(torch.int64).sum(dtype=torch.int64).item()
    masks = np.zeros(S, dtype=np.int32)
    erased = np.zeros((S, 14), dtype=bool)
    for s in range(S):
        e = rng.choice(14, 4, replace=False)
        erased[s, e] = True
        masks[s] = ((1 << 14) - 1) & ~int(sum(1 << int(i) for i in e))
    er = torch.from_numpy(erased).cuda()
    snap = t[er].clone()  # [S*4, L]
    t[er] = 0
    B.reconstruct_batch(rs, t, torch.from_numpy(masks).cuda())
    torch.cuda.synchronize()
    assert torch.equal(t[er], snap)
    assert t[:, 10:].view(torch.int64).sum(dtype=torch.int64).item() == parity_sum
    assert corc.check_device_batch(t, masks, data_seeds=seeds) == []
    del t, snap, er
    torch.cuda.empty_cache()


@pytest.mark.parametrize("lengths", ["odd", "multiple_of_8k"])
def test_ragged_device_batch(gpu, lengths):
    """Mixed-length stripes (config 5 shape plus odd lengths) in one launch each
    for encode and reconstruct, against the C oracle. All lengths multiples of
    8 KiB: the encode takes the bit-sliced ragged kernel."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(21)
    lens = [int(64 << 10) << int(rng.integers(0, 7)) for _ in range(20)]
    if lengths == "odd":
        lens = [1, 17, 1000, 4096, 4097, 65536, 100003, 1 << 20, 3 << 20] + lens
    else:
        lens = [8192, 24576, 1 << 20] + lens
    descs, off = [], 0
    for L in lens:
        stride = (L + 255) // 256 * 256
        descs.append([off, stride, L, 0])
        off += 14 * stride
    buf = torch.zeros(off, dtype=torch.uint8, device="cuda")
    host = np.zeros(off, dtype=np.uint8)
    for j, (o, st, L, _) in enumerate(descs):
        for i in range(10):
            host[o + i * st: o + i * st + L] = rng.integers(0, 256, L, dtype=np.uint8)
    buf.copy_(torch.from_numpy(host))
    B.encode_ragged(rs, buf, descs)
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    for o, st, L, _ in descs:
        data = np.stack([host[o + i * st: o + i * st + L] for i in range(10)])
        ref = corc.encode_stripes(data[None].copy())[0]
        for j in range(4):
            assert np.array_equal(got[o + (10 + j) * st: o + (10 + j) * st + L], ref[j])
    good = buf.clone()
    full = (1 << 14) - 1
    for d in descs:
        e = rng.choice(14, int(rng.integers(0, 5)), replace=False)
        d[3] = full & ~int(sum(1 << int(i) for i in e))
        for i in e:
            buf[d[0] + int(i) * d[1]: d[0] + int(i) * d[1] + d[2]] = 0x33
    descs[0][3] = full & ~0b11111  # too few present: skipped + counted
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_ragged(rs, buf, descs, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 1
    for j, (o, st, L, m) in enumerate(descs):
        if j == 0:
            continue
        assert torch.equal(buf[o: o + 14 * st], good[o: o + 14 * st]), j
    # every stripe complete: upstream's no-op, and the call launches no
    # workgroup at all (all-present stripes get none); poisoned parity stays
    for d in descs:
        d[3] = full
    buf[descs[1][0] + 12 * descs[1][1]] ^= 0xFF
    snap = buf.clone()
    bad.zero_()
    B.reconstruct_ragged(rs, buf, descs, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0 and torch.equal(buf, snap)


def test_concurrent_host_calls(gpu):
    """Reentrancy (SURVEY §8b Threading): host-API calls from 8 threads at once,
    mixed encode / reconstruct / batch reconstruct and different lengths."""
    import threading
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    errors = []

    def worker(t):
        try:
            rng = np.random.default_rng(1000 + t)
            for it in range(6):
                L = int(rng.integers(1, 200000))
                data = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(10)]
                sh = data + [np.zeros(L, np.uint8) for _ in range(4)]
                rs.encode(sh)
                ref = [d.copy() for d in data] + [np.zeros(L, np.uint8) for _ in range(4)]
                corc.CReedSolomon(10, 4).encode(ref)
                assert all(np.array_equal(a, b) for a, b in zip(sh, ref))
                e = set(rng.choice(14, 4, replace=False).tolist())
                got = [None if i in e else ref[i].copy() for i in range(14)]
                if it % 2:
                    rs.reconstruct(got)
                else:
                    st = [got]
                    rs.reconstruct_batch(st)
                    got = st[0]
                assert all(np.array_equal(got[i], ref[i]) for i in range(14))
        except Exception as ex:  # pragma: no cover - reported below
            errors.append(repr(ex))

    ths = [threading.Thread(target=worker, args=(t,)) for t in range(8)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    assert not errors, errors


def test_masks_with_stray_high_bits(gpu):
    """Present masks with bits above the shard count set are clipped, never
    index past the decode LUT (generic geometry and RS(10,4) fast path)."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    for k, m in ((10, 4), (6, 3)):
        rs = H.ReedSolomon(k, m)
        n = k + m
        S, L = 4, 4096
        t = torch.randint(0, 256, (S, n, L), dtype=torch.uint8, device="cuda")
        B.encode_batch(rs, t)
        good = t.clone()
        masks = torch.tensor([((1 << n) - 1) & ~1 | (0x7FFF0000)] * S, dtype=torch.int32, device="cuda")
        t[:, 0] = 0
        B.reconstruct_batch(rs, t, masks)
        torch.cuda.synchronize()
        assert torch.equal(t, good)


def test_full_config_every_4_erasure_pattern_and_linearity(gpu):
    """At the BASELINE shard length (1 MiB): every one of the 1001 4-erasure
    patterns, 4 stripes each (4004 stripes), rebuilt == original; and the
    encode is GF(2)-linear: parity(A ^ B) == parity(A) ^ parity(B) over the
    whole batch (a size-independent property of the bit-sliced program)."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    pats = list(itertools.combinations(range(14), 4))
    assert len(pats) == 1001
    S, L = 4 * len(pats), 1 << 20
    t = _stripes(S, L)
    B.encode_batch(rs, t)
    good_par = t[:, 10:].clone()
    masks = np.array([((1 << 14) - 1) & ~sum(1 << i for i in pats[s % len(pats)]) for s in range(S)], np.int32)
    er = torch.from_numpy(((masks[:, None] >> np.arange(14)[None, :]) & 1) == 0).cuda()
    snap = t[er].clone()
    t[er] = 0x6B
    B.reconstruct_batch(rs, t, torch.from_numpy(masks).cuda())
    torch.cuda.synchronize()
    assert torch.equal(t[er], snap)
    # linearity: a second batch, then the XOR of the two
    u = _stripes(S, L, seed_base=O.STRIPE_SEED_BASE + 77777)
    B.encode_batch(rs, u)
    par_u = u[:, 10:].clone()
    u[:, :10] ^= t[:, :10]
    B.encode_batch(rs, u)
    torch.cuda.synchronize()
    assert torch.equal(u[:, 10:], good_par ^ par_u)


def test_batch_argument_checks_before_launch(gpu):
    """The Python mirror rejects shapes the kernels would run past (the C ABI
    only sees pointers), before anything is launched."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    t = torch.zeros((2, 14, 4096), dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        B.encode_batch(rs, t[:, :13])                       # 13 shards
    with pytest.raises(ValueError):
        B.encode_batch_sep(rs, t[:, :10], torch.zeros((2, 4, 1024), dtype=torch.uint8, device="cuda"))
    with pytest.raises(ValueError):
        B.reconstruct_batch(rs, t, torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        B.reconstruct_batch(rs, t, torch.zeros(2, dtype=torch.int64, device="cuda"))
    base = torch.zeros(14 * 4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        B.encode_ragged(rs, base, [[1, 4096, 4096, 0]])        # last shard runs 1 byte past base
    with pytest.raises(ValueError):
        B.reconstruct_ragged(rs, base, [[0, 1024, 4096, 0x3FF]])  # shards overlap
    with pytest.raises(ValueError):
        B.fill_splitmix(t, 14 * 4096 + 1, 1)
    B.encode_ragged(rs, base, [[0, 4096, 4096, 0]])            # exact fit is fine
    torch.cuda.synchronize()


def test_batch_over_launch_limit_is_split(gpu):
    """2^24 + 5 stripes of 16 B: more workgroups than one launch can carry
    (a 256-thread grid of 2^24 workgroups is 2^32 work-items), so the batch
    runs in stripe ranges of kMaxLaunchBlocks; stripes on both sides of every
    range edge are checked against the oracle."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    S, L = (1 << 24) + 5, 16
    t = torch.empty((S, 14, L), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(t, 10 * L, 0x5EED1000)
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    idx = torch.tensor([0, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24, S - 1], device="cuda")
    host = t[idx].cpu().numpy()
    assert np.array_equal(host[:, 10:], corc.encode_stripes(np.ascontiguousarray(host[:, :10])))
    masks = torch.full((S,), 0x3FFF & ~0b10000000100101, dtype=torch.int32, device="cuda")  # shards 0, 2, 5, 13
    want = t[idx].clone()
    for i in (0, 2, 5, 13):
        t[:, i] = 0
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_batch(rs, t, masks, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    assert torch.equal(t[idx], want)
    assert int(t[:, 13].sum(dtype=torch.int64).item()) > 0  # last range rebuilt too


def test_ragged_over_launch_limit_is_split(gpu):
    """2^24 + 5 ragged stripes of 16 B (one workgroup each): the ragged
    launchers split the workgroup map into launches of kMaxLaunchBlocks.
    Descriptors go straight to the C ABI (numpy), not the per-row helper."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    S, L = (1 << 24) + 5, 16
    t = torch.empty((S, 14, L), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(t, 10 * L, 0x5EED2000)
    dt = np.dtype([("offset", "<u8"), ("shard_stride", "<u8"), ("shard_len", "<u4"), ("present_mask", "<u4")])
    d = np.zeros(S, dtype=dt)
    d["offset"] = np.arange(S, dtype=np.uint64) * (14 * L)
    d["shard_stride"] = L
    d["shard_len"] = L
    st = torch.cuda.current_stream().cuda_stream
    assert H.lib.hec_gpu_encode_ragged(rs.handle, t.data_ptr(), d.ctypes.data, S, st) == 0
    torch.cuda.synchronize()
    idx = torch.tensor([0, (1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24, S - 1], device="cuda")
    host = t[idx].cpu().numpy()
    assert np.array_equal(host[:, 10:], corc.encode_stripes(np.ascontiguousarray(host[:, :10])))
    want = t[idx].clone()
    d["present_mask"] = 0x3FFF & ~0b01000000010011  # shards 0, 1, 4, 12 erased
    for i in (0, 1, 4, 12):
        t[:, i] = 0
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert H.lib.hec_gpu_reconstruct_ragged(rs.handle, t.data_ptr(), d.ctypes.data, S, bad.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    assert torch.equal(t[idx], want)


def test_ragged_shard_len_near_4gib(gpu):
    """One ragged stripe with shard_len = 2^32 - 16 (56 GiB in HBM): the
    workgroup count is computed in 64 bits (it once wrapped to 0 chunks and
    left the stripe uncoded without an error). Parity and a 4-erasure rebuild
    are checked against the C oracle on the first and last 64 KiB of every
    shard (the columns a wrapped count would have skipped)."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    L, W = (1 << 32) - 16, 1 << 16
    t = torch.empty(14 * L, dtype=torch.uint8, device="cuda")
    B.fill_splitmix(t[:10 * L].view(1, -1), 10 * L, 0x5EED4000)
    t[10 * L:].zero_()
    B.encode_ragged(rs, t, [(0, L, L, 0)])
    torch.cuda.synchronize()

    def cols(lo):
        return np.stack([t[i * L + lo:i * L + lo + W].cpu().numpy() for i in range(14)])

    heads, tails = cols(0), cols(L - W)
    for c in (heads, tails):
        assert np.array_equal(c[10:], corc.encode_stripes(np.ascontiguousarray(c[None, :10]))[0])
    drop = (0, 3, 11, 13)
    for i in drop:
        t[i * L:(i + 1) * L].zero_()
    mask = 0x3FFF & ~sum(1 << i for i in drop)
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_ragged(rs, t, [(0, L, L, mask)], bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    assert np.array_equal(cols(0), heads) and np.array_equal(cols(L - W), tails)
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("L", [(1 << 32) - 8192, (1 << 32) - 4096, (1 << 32) + 8192])
def test_strided_batch_shard_len_near_4gib(gpu, L):
    """Two-stripe strided device batches (112 GiB in HBM) at the edge of the
    fast kernels' 32-bit lane offsets (fast_map_ok: shards below 4 GiB):
    2^32 - 8 KiB runs the bit-sliced encode with SGPR shard bases + 32-bit
    offsets, 2^32 - 4 KiB the table encode on the same fast map, 2^32 + 8 KiB
    the 64-bit-offset kernels. Both stripes' parity and a per-stripe
    4-erasure rebuild are checked against the C oracle on the first and last
    64 KiB of every shard, where a wrapped offset would land."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    S, W = 2, 1 << 16
    torch.cuda.empty_cache()
    t = torch.empty((S, 14, L), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(t, 10 * L, 0x5EED5000)
    t[:, 10:].zero_()
    B.encode_batch(rs, t)
    torch.cuda.synchronize()

    def cols(s, lo):
        return t[s, :, lo:lo + W].cpu().numpy()

    ref = {}
    for s in range(S):
        for lo in (0, L - W):
            c = cols(s, lo)
            assert np.array_equal(c[10:], corc.encode_stripes(np.ascontiguousarray(c[None, :10]))[0]), (L, s, lo)
            ref[s, lo] = c
    drops = ((0, 3, 11, 13), (2, 5, 9, 10))
    masks = torch.tensor([0x3FFF & ~sum(1 << i for i in d) for d in drops], dtype=torch.int32, device="cuda")
    for s, d in enumerate(drops):
        for i in d:
            t[s, i].zero_()
    B.reconstruct_batch(rs, t, masks)
    torch.cuda.synchronize()
    for s in range(S):
        for lo in (0, L - W):
            assert np.array_equal(cols(s, lo), ref[s, lo]), (L, s, lo)
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k,m", [(3, 2), (6, 3), (12, 4), (8, 8), (1, 1)])
def test_device_batches_generic_geometry(gpu, k, m):
    """hec_gpu_encode_batch / hec_gpu_reconstruct_batch on geometries other
    than RS(10,4) (the generic plan kernel; total shards <= 16 for device
    masks), per-stripe random erasure patterns, against the C oracle."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rng = np.random.default_rng(77 * k + m)
    n = k + m
    rs, ors = H.ReedSolomon(k, m), corc.CReedSolomon(k, m)
    for S, L in ((5, 1), (7, 4099), (3, 65536)):
        host = np.zeros((S, n, L), np.uint8)
        host[:, :k] = rng.integers(0, 256, (S, k, L), dtype=np.uint8)
        for s in range(S):
            ors.encode([host[s, i] for i in range(n)])
        t = torch.zeros((S, n, L), dtype=torch.uint8, device="cuda")
        t[:, :k] = torch.from_numpy(host[:, :k]).cuda()
        B.encode_batch(rs, t)
        torch.cuda.synchronize()
        assert np.array_equal(t.cpu().numpy(), host), (k, m, S, L)
        masks = np.full(S, (1 << n) - 1, np.int64)
        for s in range(S):
            for i in rng.choice(n, int(rng.integers(0, m + 1)), replace=False):
                masks[s] &= ~(1 << int(i))
                t[s, int(i)] = 0x5A
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        B.reconstruct_batch(rs, t, torch.from_numpy(masks.astype(np.int32)).cuda(), bad)
        torch.cuda.synchronize()
        assert int(bad.item()) == 0
        assert np.array_equal(t.cpu().numpy(), host), (k, m, S, L)


def test_randomised_device_batches_vs_oracle(gpu):
    """Seeded sweep over the device batch API: shard lengths (tiny, odd,
    16-byte and 8 KiB multiples), shard pitches (tight, padded, unaligned),
    in-place and separate parity buffers and per-stripe erasure patterns, all
    against the C oracle."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rng = np.random.default_rng(20261016)
    rs = H.ReedSolomon(10, 4)
    lens = [1, 15, 16, 17, 100, 4080, 4096, 4112, 8192, 12288, 16384, 24576, 65536, 65536 + 48, 100003]
    for case in range(120):
        L = int(rng.choice(lens))
        S = int(rng.integers(1, 9))
        pad = int(rng.choice([0, 16, 48, 4096, 3]))
        sep = bool(rng.integers(0, 2))
        P = L + pad
        raw = torch.zeros(S * 14 * P + 16, dtype=torch.uint8, device="cuda")
        t = raw[:S * 14 * P].view(S, 14, P)[:, :, :L]
        host = np.zeros((S, 14, L), np.uint8)
        host[:, :10] = rng.integers(0, 256, (S, 10, L), dtype=np.uint8)
        host[:, 10:] = corc.encode_stripes(np.ascontiguousarray(host[:, :10]))
        t[:, :10] = torch.from_numpy(host[:, :10]).cuda()
        if sep:
            par_raw = torch.zeros(S * 4 * P + 16, dtype=torch.uint8, device="cuda")
            par = par_raw[:S * 4 * P].view(S, 4, P)[:, :, :L]
            B.encode_batch_sep(rs, t[:, :10], par)
            torch.cuda.synchronize()
            assert np.array_equal(par.cpu().numpy(), host[:, 10:]), (case, L, S, pad)
            t[:, 10:] = par
        else:
            B.encode_batch(rs, t)
            torch.cuda.synchronize()
            assert np.array_equal(t.cpu().numpy(), host), (case, L, S, pad)
        masks = np.full(S, 0x3FFF, np.int64)
        for s in range(S):
            for i in rng.choice(14, int(rng.integers(0, 5)), replace=False):
                masks[s] &= ~(1 << int(i))
                t[s, int(i)] = 0xEE
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        B.reconstruct_batch(rs, t, torch.from_numpy(masks.astype(np.int32)).cuda(), bad)
        torch.cuda.synchronize()
        assert int(bad.item()) == 0
        assert np.array_equal(t.cpu().numpy(), host), (case, L, S, pad, "decode")


def test_randomised_ragged_batches_vs_oracle(gpu):
    """Seeded sweep over ragged device batches: per-stripe lengths (all 8 KiB
    multiples -> bit-sliced ragged encode, or mixed -> table kernel), padded
    strides and gaps, 0..5 erasures per stripe (5 = skipped and counted)."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rng = np.random.default_rng(1016)
    rs = H.ReedSolomon(10, 4)
    _ragged_sweep(H, B, torch, rng, rs)


def _ragged_sweep(H, B, torch, rng, rs):
    for case in range(40):
        n = int(rng.integers(1, 25))
        if case % 2:
            lens = [8192 * int(rng.integers(1, 9)) for _ in range(n)]
        else:
            lens = [int(rng.choice([1, 17, 4096, 5000, 8192, 65536 + 16, 70001])) for _ in range(n)]
        descs, off = [], 0
        for L in lens:
            stride = (L + 15) // 16 * 16 + 16 * int(rng.integers(0, 3))
            off += 16 * int(rng.integers(0, 4))
            descs.append([off, stride, L, 0x3FFF])
            off += 14 * stride
        host = np.zeros(off, np.uint8)
        want = []
        for o, st, L, _ in descs:
            data = rng.integers(0, 256, (10, L), dtype=np.uint8)
            par = corc.encode_stripes(data[None].copy())[0]
            for i in range(10):
                host[o + i * st: o + i * st + L] = data[i]
            want.append(np.concatenate([data, par]))
        buf = torch.from_numpy(host).cuda()
        B.encode_ragged(rs, buf, descs)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        for j, (o, st, L, _) in enumerate(descs):
            for i in range(14):
                assert np.array_equal(got[o + i * st: o + i * st + L], want[j][i]), (case, j, i)
        n_bad = 0
        for d in descs:
            e = int(rng.integers(0, 6))
            n_bad += e == 5
            for i in rng.choice(14, e, replace=False):
                d[3] &= ~(1 << int(i))
                buf[d[0] + int(i) * d[1]: d[0] + int(i) * d[1] + d[2]] = 0x77
        bad = torch.zeros(1, dtype=torch.int32, device="cuda")
        before = buf.cpu().numpy()
        B.reconstruct_ragged(rs, buf, descs, bad)
        torch.cuda.synchronize()
        assert int(bad.item()) == n_bad, case
        got = buf.cpu().numpy()
        for j, (o, st, L, m) in enumerate(descs):
            if bin(m).count("1") < 10:  # skipped: all 14 shard ranges hold what they held before the call
                for i in range(14):
                    assert np.array_equal(got[o + i * st: o + i * st + L],
                                          before[o + i * st: o + i * st + L]), (case, j, i, "skipped")
                continue
            for i in range(14):
                assert np.array_equal(got[o + i * st: o + i * st + L], want[j][i]), (case, j, i, "decode")


@pytest.mark.parametrize("L,pad", [(4096, 65536), (65536, 8), (1 << 20, 64 << 10)])
def test_padded_batch_layout(gpu, L, pad):
    """The bench's HBM layout (batch.empty_stripes: shard stride L + pad):
    fill_stripes_splitmix writes the same data bytes as the packed fill, and
    encode + a per-stripe 4-erasure rebuild on the padded batch match the C
    oracle; the pad bytes between shards are never written."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    S = 5
    rs = H.ReedSolomon(10, 4)
    t = B.empty_stripes(S, 14, L, shard_pad=pad)
    assert t.stride() == (14 * (L + pad), L + pad, 1)
    raw = t.as_strided((t.untyped_storage().nbytes(),), (1,), 0)
    raw.fill_(0xA5)
    B.fill_stripes_splitmix(t, 10, O.STRIPE_SEED_BASE)
    packed = _stripes(S, L)
    assert torch.equal(t[:, :10], packed[:, :10])
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    host = t.cpu().numpy()
    assert np.array_equal(host[:, 10:], corc.encode_stripes(np.ascontiguousarray(host[:, :10])))
    full = host.copy()
    drops = [(s % 14, (s + 3) % 14, (s + 7) % 14, (s + 11) % 14) for s in range(S)]
    masks = torch.tensor([0x3FFF & ~sum(1 << i for i in d) for d in drops], dtype=torch.int32, device="cuda")
    for s, d in enumerate(drops):
        for i in d:
            t[s, i] = 0
    B.reconstruct_batch(rs, t, masks)
    torch.cuda.synchronize()
    assert np.array_equal(t.cpu().numpy(), full)
    gaps = raw.view(S * 14, L + pad)[:, L:]
    assert bool((gaps == 0xA5).all())


def test_ragged_and_batched_reconstruct_every_pattern(gpu):
    """All 1470 erasure patterns with 1..4 erasures, one per stripe, through
    the two ragged decode paths the degraded reads and config 5 use: one
    device-resident ragged launch (hec_gpu_reconstruct_ragged, stripes of 4
    lengths cycling, packed back to back) and one compact host batch
    (hec_rs_reconstruct_batch); every rebuilt shard against the C oracle's
    encode of the original stripe."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    rng = np.random.default_rng(1470)
    pats = [c for e in range(1, 5) for c in itertools.combinations(range(14), e)]
    assert len(pats) == 1470
    lens = [16, 1000, 4096, 8192 + 16]
    full = []
    for j in range(len(pats)):
        L = lens[j % 4]
        data = rng.integers(0, 256, (1, 10, L), dtype=np.uint8)
        full.append(np.concatenate([data[0], corc.encode_stripes(data)[0]]))
    # device-resident ragged launch
    descs, off = [], 0
    for j, p in enumerate(pats):
        L = full[j].shape[1]
        st = (L + 15) // 16 * 16  # ragged strides and offsets are 16-byte aligned
        descs.append((off, st, L, ((1 << 14) - 1) & ~sum(1 << i for i in p)))
        off += 14 * st
    host = np.zeros(off, np.uint8)
    for (o, st, L, _), f in zip(descs, full):
        for i in range(14):
            host[o + i * st: o + i * st + L] = f[i]
    poisoned = host.copy()
    for (o, st, L, m), p in zip(descs, pats):
        for i in p:
            poisoned[o + i * st: o + i * st + L] = 0xD7
    buf = torch.from_numpy(poisoned).cuda()
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_ragged(rs, buf, descs, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    assert np.array_equal(buf.cpu().numpy(), host)
    # compact host batch: every stripe's erased slots absent, rebuilt in one call
    stripes = [[None if i in p else full[j][i].copy() for i in range(14)] for j, p in enumerate(pats)]
    rs.reconstruct_batch(stripes)
    for j, s in enumerate(stripes):
        for i in range(14):
            assert np.array_equal(s[i], full[j][i]), (pats[j], i)


def _check_ragged_all(dev, descs, seeds, masks=None, group=32):
    """Every stripe of a packed ragged device batch against the C oracle
    (corc.check_stripes), stripes of one length copied back `group` at a time.
    -> indices of the stripes that differ."""
    by_len = {}
    for s, (_, _, L, _) in enumerate(descs):
        by_len.setdefault(L, []).append(s)
    bad = []
    for L, idx in by_len.items():
        for g in range(0, len(idx), group):
            sel = idx[g:g + group]
            host = np.stack([dev[descs[s][0]:descs[s][0] + 14 * L].view(14, L).cpu().numpy() for s in sel])
            m = None if masks is None else np.array([masks[s] for s in sel], dtype=np.int64)
            sd = np.array([seeds[s] for s in sel], dtype=np.uint64)
            bad += [sel[j] for j in corc.check_stripes(host, m, 16, sd)]
    return sorted(bad)


def test_config5_whole_batch_vs_oracle(gpu):
    """BASELINE config 5 exactly as the bench runs it (bench.mixed_workload:
    2048 stripes, 64 KiB..4 MiB, 0..4 erasures, 32 GiB in HBM), EVERY stripe
    against the C oracle: after one ragged encode launch, data and parity of
    all 2048 stripes; then every erased shard overwritten, one ragged
    reconstruct launch, and all stripes again (rebuilt shards = the oracle's
    reconstruct from the same survivors). The bench's own mixed leg
    (bench.mixed_verify) checks all 2048 stripes after its timed launches,
    after the reconstruct only."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    import bench
    rs = H.ReedSolomon(10, 4)
    Ls, es, masks, descs, off = bench.mixed_workload(0, 2048)
    seeds = [bench.rank_seed_base(0) + s for s in range(len(descs))]
    torch.cuda.empty_cache()
    dev = torch.empty(off, dtype=torch.uint8, device="cuda")
    for s, (o, _, L, _) in enumerate(descs):
        B.fill_splitmix(dev[o:o + 10 * L].view(1, 1, -1), 10 * L, seeds[s])
    darr = np.array(descs, dtype=B.desc_dtype())
    B.encode_ragged(rs, dev, darr)
    torch.cuda.synchronize()
    assert _check_ragged_all(dev, descs, seeds) == []
    erased = 0
    for (o, _, L, m) in descs:
        for i in range(14):
            if not (m >> i) & 1:
                dev[o + i * L:o + (i + 1) * L].fill_(0xA5)
                erased += 1
    assert erased == int(sum(es))
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    B.reconstruct_ragged(rs, dev, darr, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == 0
    assert _check_ragged_all(dev, descs, seeds, masks) == []
    del dev
    torch.cuda.empty_cache()
