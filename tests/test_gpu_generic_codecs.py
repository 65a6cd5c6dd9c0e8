"""The generic kernels (rs_apply_kernel, rs_verify_kernel), the dense decode
LUT and the per-call plans, on codecs other than RS(10,4) and on batches past
one grid, against the plain reference of tests/gfref.py (GPU). Every
comparison is bit-exact.

* every present mask of a codec in one device reconstruct (gfref.all_masks_case:
  surplus survivors hold garbage, so a plan that reads any shard but the first
  k present ones fails), whole buffer compared, pitch bytes and slack included;
* k = 10 codecs that are not RS(10,4): rs_apply_kernel<10> / rs_verify_kernel<10>
  with 2 and 6 table rows;
* batches of 2^23 + 5 items: the grid-stride loops' second pass, checked whole
  on the device with gfref.torch_encode;
* the per-call API over every decodable mask of three small codecs.
"""
import time

import numpy as np
import pytest

import gfref
from oracle import corc

pytestmark = pytest.mark.gpu

PRESET_BAD = 7
STRAY = 0x7FFF0000


def _r16(x):
    return (x + 15) // 16 * 16


# ---- every present mask through the device batch ---------------------------------
SWEEP_CODECS = [(3, 2), (6, 3), (10, 2), (10, 6), (12, 4), (8, 8), (4, 12), (1, 15), (15, 1), (10, 4)]
SWEEP = [(k, m, 17, pitch) for k, m in SWEEP_CODECS for pitch in (32, 19)] + \
        [(10, 4, 2048, 2048), (10, 4, 4096 + 16, 4096 + 16), (10, 6, 4096 + 3, 4096 + 16), (8, 8, 4096 + 3, 4096 + 16)]


def run_every_mask(k, m, L, pitch, stray=0):
    """One hec_gpu_reconstruct_batch launch over the every-mask image (masks
    arange(2^n) | stray), inside SLACK bytes of garbage on both sides: the
    whole buffer must equal the expected image, bad_stripes must go up by the
    number of masks with fewer than k shards present."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    n = k + m
    S = 1 << n
    seed = 100000 * k + 1000 * m + L + pitch
    if S * n * pitch <= (64 << 20):
        case = gfref.all_masks_case(k, m, L, pitch, seed)
        start, expected = torch.from_numpy(case.start).cuda(), torch.from_numpy(case.expected).cuda()
    else:  # hundreds of MB and more: composed on the device
        case = gfref.all_masks_case_torch(k, m, L, pitch, seed, "cuda")
        start, expected = case.start, case.expected
    tb = case.tables
    N, slack = S * n * pitch, gfref.SLACK
    g = torch.Generator(device="cuda").manual_seed(seed + 1)
    buf = torch.randint(0, 256, (N + 2 * slack,), dtype=torch.uint8, device="cuda", generator=g)
    lo, hi = buf[:slack].clone(), buf[slack + N:].clone()
    image = buf[slack:slack + N].view(S, n, pitch)
    image.copy_(start)
    del start
    t = image[:, :, :L]
    assert t.data_ptr() % 16 == 0
    rs = H.ReedSolomon(k, m)
    masks = torch.from_numpy(tb.masks | np.int32(stray)).cuda()
    bad = torch.full((1,), PRESET_BAD, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    B.reconstruct_batch(rs, t, masks, bad)
    torch.cuda.synchronize()
    print(f"every mask RS({k},{m}) L={L} pitch={pitch}: reconstruct call {time.perf_counter() - t0:.3f} s "
          f"(the first of a geometry builds its decode LUT)")
    assert int(bad.item()) == PRESET_BAD + tb.n_bad
    assert torch.equal(buf[:slack], lo), "bytes before the first stripe were written"
    assert torch.equal(buf[slack + N:], hi), "bytes after the last stripe were written"
    if not torch.equal(image, expected):
        pytest.fail(gfref.describe_first_difference(image, expected, tb, L))


@pytest.mark.parametrize("k,m,L,pitch", SWEEP)
def test_device_reconstruct_every_mask(gpu, k, m, L, pitch):
    import torch
    import helyim_amd as H
    if (k, m) == (10, 4) and L > 17:
        name = H.lib.hec_decode_kernel_name(L).decode()
        assert name.startswith("rs104_narrow_kernel<DEC=true" if L % 2048 == 0 else "rs104_kernel<DEC=true>"), name
    run_every_mask(k, m, L, pitch)
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k,m", [(6, 3), (10, 4)])
def test_device_reconstruct_every_mask_with_stray_high_bits(gpu, k, m):
    """Bits above the shard count in every mask: the same result."""
    run_every_mask(k, m, 17, 32, stray=STRAY)


# ---- k = 10 codecs that are not RS(10,4) ------------------------------------------
@pytest.mark.parametrize("k,m", [(10, 2), (10, 6)])
@pytest.mark.parametrize("L", [1, 17, 4096 + 3, 65536])
def test_device_encode_k10_codecs(gpu, k, m, L):
    """hec_gpu_encode_batch of RS(10,2) and RS(10,6): in place and with the
    parity in a buffer of its own, on a 16-byte-aligned and on an odd pitch,
    against ref_encode; every other byte of the buffers unchanged."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(k, m)
    n, S = k + m, 5
    rng = np.random.default_rng(10000 * m + L)
    for pitch in (_r16(L) + 16, L + 3):
        raw = rng.integers(0, 256, (S, n, pitch), dtype=np.uint8)
        want = raw.copy()
        want[:, k:, :L] = gfref.ref_encode(k, m, raw[:, :k, :L])
        dev = torch.from_numpy(raw).cuda()
        B.encode_batch(rs, dev[:, :, :L])
        torch.cuda.synchronize()
        got = dev.cpu().numpy()
        assert np.array_equal(got, want), (pitch, gfref.describe_first_difference(got, want, None, L))
        # separate parity: the data batch packed, the parity on this pitch
        data = torch.from_numpy(np.ascontiguousarray(raw[:, :k, :L])).cuda()
        praw = rng.integers(0, 256, (S, m, pitch), dtype=np.uint8)
        pwant = praw.copy()
        pwant[:, :, :L] = want[:, k:, :L]
        par = torch.from_numpy(praw).cuda()
        B.encode_batch_sep(rs, data, par[:, :, :L])
        torch.cuda.synchronize()
        pgot = par.cpu().numpy()
        assert np.array_equal(pgot, pwant), (pitch, gfref.describe_first_difference(pgot, pwant, None, L))
        assert np.array_equal(data.cpu().numpy(), raw[:, :k, :L])


def _staging(limit):
    import helyim_amd as H
    assert H.lib.hec_set_host_staging(limit) == 0


@pytest.mark.parametrize("k,m", [(3, 2), (6, 3), (10, 2)])
@pytest.mark.parametrize("L", [1, 17, 4096 + 3])
def test_per_call_api_every_decodable_mask(gpu, k, m, L):
    """encode, verify, and reconstruct / reconstruct_data for every decodable
    mask, with pinned staging off and on: the survivors after the first k
    present hold garbage, the erased slots must come back as the codeword,
    and reconstruct_data leaves an erased parity slot None."""
    import helyim_amd as H
    n = k + m
    case = gfref.all_masks_case(k, m, L, L, seed=31 * k + m + L)
    tb = case.tables
    rs = H.ReedSolomon(k, m)
    full = [case.expected[(1 << n) - 1, i].copy() for i in range(n)]  # the all-present stripe: a codeword
    try:
        for limit in (0, 1 << 40):
            _staging(limit)
            sh = [f.copy() for f in full[:k]] + [np.full(L, 0x3C, np.uint8) for _ in range(m)]
            rs.encode(sh)
            for i in range(n):
                assert np.array_equal(sh[i], full[i]), (limit, "encode", i)
            assert rs.verify(sh)
            for j in range(m):
                sh[k + j][(5 * j) % L] ^= 0x10
                assert not rs.verify(sh), (limit, "verify", j)
                sh[k + j][(5 * j) % L] ^= 0x10
            for s in np.flatnonzero(tb.decodable):
                s = int(s)
                for data_only in (False, True):
                    got = [case.start[s, i].copy() if tb.present[s, i] else None for i in range(n)]
                    (rs.reconstruct_data if data_only else rs.reconstruct)(got)
                    for i in range(n):
                        if data_only and i >= k and not tb.present[s, i]:
                            assert got[i] is None, (limit, hex(s), i)
                        else:
                            assert got[i] is not None and np.array_equal(got[i], case.expected[s, i]), \
                                (limit, hex(s), data_only, i)
    finally:
        _staging(16 << 20)


# ---- grid-stride past one grid ------------------------------------------------------
OVER = (1 << 23) + 5  # stripes of one 4 KiB chunk each: more items than kMaxLaunchBlocks
EDGES = (0, (1 << 23) - 1, 1 << 23, OVER - 1)


def _first_bad_stripe(got, want):
    """Index of the first stripe of two [S, ...] device tensors that differs."""
    import torch
    S = got.shape[0]
    for s0 in range(0, S, 1 << 20):
        ne = (got[s0:s0 + (1 << 20)] != want[s0:s0 + (1 << 20)]).flatten(1).any(dim=1)
        if bool(ne.any()):
            return s0 + int(torch.nonzero(ne)[0].item())
    return None


def _over_limit_batch(k, m, L, base_offset, seed):
    """[OVER, n, L] uint8 view with seeded random data shards and zeroed
    parity, starting base_offset bytes into its allocation."""
    import torch
    n = k + m
    g = torch.Generator(device="cuda").manual_seed(seed)
    raw = torch.empty(OVER * n * L + 16, dtype=torch.uint8, device="cuda")
    t = raw.as_strided((OVER, n, L), (n * L, L, 1), base_offset)
    t[:, :k] = torch.randint(0, 256, (OVER, k, L), dtype=torch.uint8, device="cuda", generator=g)
    t[:, k:] = 0
    return raw, t


def _encode_then_reconstruct_over_limit(k, m, L, base_offset, erase, seed):
    """Encode, whole parity against torch_encode; then one fixed erasure
    pattern everywhere except the EDGES stripes, which have too few present
    (counted, untouched); the whole buffer against the expected image."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    n = k + m
    rs = H.ReedSolomon(k, m)
    raw, t = _over_limit_batch(k, m, L, base_offset, seed)
    assert (t.data_ptr() % 16 == 0) == (base_offset == 0)
    ref = gfref.torch_encode(k, m, t[:, :k])
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    if not torch.equal(t[:, k:], ref):
        pytest.fail(f"encode: first wrong stripe {_first_bad_stripe(t[:, k:], ref)}")
    del ref
    want = t.clone()
    assert len(erase) == m
    full = (1 << n) - 1
    mask = full & ~sum(1 << i for i in erase)
    few = mask & ~(1 << [i for i in range(n) if i not in erase][0])  # one more gone: k - 1 present
    masks = torch.full((OVER,), mask, dtype=torch.int32, device="cuda")
    edges = torch.tensor(EDGES, device="cuda")
    masks[edges] = few
    for i in erase:
        t[:, i] = gfref.POISON
    want[edges] = t[edges]  # skipped stripes keep their poison
    bad = torch.full((1,), PRESET_BAD, dtype=torch.int32, device="cuda")
    B.reconstruct_batch(rs, t, masks, bad)
    torch.cuda.synchronize()
    assert int(bad.item()) == PRESET_BAD + len(EDGES)
    if not torch.equal(t, want):
        pytest.fail(f"reconstruct: first wrong stripe {_first_bad_stripe(t, want)}")
    del raw, t, want
    torch.cuda.empty_cache()


@pytest.mark.parametrize("L", [16, 1])
def test_generic_batch_past_one_grid(gpu, L):
    """RS(3,2), 2^23 + 5 stripes: 16-byte shards on a 16-byte pitch (aligned)
    and 1-byte shards (unaligned). The last 5 items are reached only by the
    second pass of rs_apply_kernel's grid-stride loop."""
    _encode_then_reconstruct_over_limit(3, 2, L, 0, erase=(1, 3), seed=23 + L)


def test_rs104_odd_base_batch_past_one_grid(gpu):
    """RS(10,4), 2^23 + 5 stripes of 16 bytes on an odd base: no fast kernel
    takes an unaligned batch, rs_apply_kernel<10, false> codes all of it.
    (launch_apply cuts an RS(10,4) batch past the limit into stripe ranges
    whatever its alignment, so here the kernel runs once per range and its
    loop makes one pass; the RS(10,2) test below is the k = 10 batch that one
    launch loops over.)"""
    _encode_then_reconstruct_over_limit(10, 4, 16, 3, erase=(0, 2, 5, 13), seed=104)


def test_k10_odd_base_batch_past_one_grid(gpu):
    """RS(10,2), 2^23 + 5 stripes of 16 bytes on an odd base: one launch of
    rs_apply_kernel<10, false> with two table rows, the last 5 items in the
    second pass of its loop."""
    _encode_then_reconstruct_over_limit(10, 2, 16, 3, erase=(4, 11), seed=102)


@pytest.mark.parametrize("k,m,L", [(10, 4, 16), (3, 2, 1)])
def test_verify_past_one_grid(gpu, k, m, L):
    """hec_gpu_verify_batch over 2^23 + 5 stripes (rs_verify_kernel: 16 is no
    multiple of 8 KiB), stored parity from torch_encode. Clean: every word 0.
    Then one flipped byte in a parity shard of the stripes around the grid
    edge and of one mid-batch stripe, and one in a data shard: exactly those
    words are non-zero, with the expected bits."""
    import torch
    import helyim_amd as H
    n = k + m
    rs = H.ReedSolomon(k, m)
    if (k, m) == (10, 4):
        assert H.verify_kernel_name(L).startswith("rs_verify_kernel<10>")
    raw, t = _over_limit_batch(k, m, L, 0, seed=500 + k)
    gfref.torch_encode(k, m, t[:, :k], out=t[:, k:])
    words = torch.full((OVER,), -1, dtype=torch.int32, device="cuda")
    bad = torch.full((1,), PRESET_BAD, dtype=torch.int32, device="cuda")
    H.verify_batch(rs, t, mismatch=words, bad_stripes=bad)
    torch.cuda.synchronize()
    assert int(torch.count_nonzero(words).item()) == 0
    assert int(bad.item()) == PRESET_BAD
    # stripe -> parity shard flipped
    flips = {0: 1 % m, (1 << 23) - 1: 2 % m, 1 << 23: 3 % m, (1 << 23) + 4: 0, 3_000_001: m - 1}
    for s, j in flips.items():
        t[s, k + j, (7 * j) % L] ^= 0x21
    ds = 5_000_003  # a data-shard flip: the oracle says which parity shards then differ
    t[ds, k - 1, L - 1] ^= 0x80
    host = t[ds].cpu().numpy()
    bufs = [host[i].copy() for i in range(k)] + [np.zeros(L, np.uint8) for _ in range(m)]
    corc.CReedSolomon(k, m).encode(bufs)
    want = {s: 1 << j for s, j in flips.items()}
    want[ds] = sum(1 << j for j in range(m) if (bufs[k + j] != host[k + j]).any())
    assert want[ds] != 0
    words.fill_(-1)
    H.verify_batch(rs, t, mismatch=words, bad_stripes=bad)
    torch.cuda.synchronize()
    hit = torch.nonzero(words).flatten().cpu().tolist()
    assert hit == sorted(want), (hit[:10], len(hit))
    assert [int(words[s].item()) for s in sorted(want)] == [want[s] for s in sorted(want)]
    assert int(bad.item()) == PRESET_BAD + len(want)
    del raw, t, words
    torch.cuda.empty_cache()
