"""Batched parity verify (scrub) on the GPU: hec_gpu_verify_batch,
hec_host_verify_batch and hec_verify_ec_files against the C oracle.

The expected word of a stripe always comes from the oracle: CReedSolomon(k,
m).encode on a copy of the stripe's current data shards, bit j =
any(oracle_parity[j] != stored_parity[j]) -- which also covers data-shard
corruption without assuming which coefficients are non-zero. Shards live in
tests/footprint.py arenas of seeded random bytes, so gaps, slack and the pads
past a shard's end are garbage: a verify that compares a byte at or past
shard_len reports a false mismatch here. Every device call is also a footprint
check: the arenas must come back byte for byte, the result word at index S
untouched."""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

import footprint as F
import scrub_harness as SH
from oracle import corc
from scrub_harness import SENTINEL, clean_case, copies, flip_positions, oracle_words, shard_of

pytestmark = pytest.mark.gpu

INVALID_ARGUMENT, EC_SHARD_SIZE, SHARD_NOT_FOUND = 66, 34, 49
LENGTHS = (8192, 16384, 8192 + 2048, 4096 + 16, 1000, 17, 1)


def device_verify(rs, arenas, stripes, data, par, preset_bad=7):
    """Run hec_gpu_verify_batch on the arenas -> (words [S], bad_stripes).
    Asserts the footprint: arenas unchanged, word S untouched."""
    (words,), (bad,) = SH.device_words("hec_gpu_verify_batch", rs, arenas, stripes, data, par, 1, [preset_bad])
    return words, bad


# ---- device batches --------------------------------------------------------------
@pytest.mark.parametrize("L", LENGTHS)
def test_clean_batch_every_layout(gpu, L):
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for which in range(4):
        name, data, par, stripes, arenas = clean_case(10, 4, L, 5, which)
        words, bad = device_verify(rs, copies(arenas), stripes, data, par)
        assert words == [0] * 5, (name, [hex(w) for w in words])
        assert bad == 7, name


@pytest.mark.parametrize("L", LENGTHS)
def test_single_byte_flips(gpu, L):
    """One flipped byte per stripe, one stripe of each launch left clean: every
    position of interest in every parity shard (word exactly 1 << j) and in
    data shards 0, 4 and 9 (the oracle's word), on the aligned stripe-major
    layout and on the odd base (the generic kernel's unaligned path)."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 5
    combos = [(shard, pos) for shard in (10, 11, 12, 13, 0, 4, 9) for pos in flip_positions(L)]
    for which in (0, 3):
        name, data, par, stripes, arenas = clean_case(10, 4, L, S, which)
        for b0 in range(0, len(combos), S - 1):
            batch = combos[b0:b0 + S - 1]
            clean_stripe = (b0 // (S - 1)) % S
            targets = [s for s in range(S) if s != clean_stripe][:len(batch)]
            work = copies(arenas)
            for s, (shard, pos) in zip(targets, batch):
                shard_of(work, stripes, s, shard)[pos] ^= 0x40
            want = oracle_words(work, stripes, 10, 4)
            for s, (shard, pos) in zip(targets, batch):
                if shard >= 10:
                    assert want[s] == 1 << (shard - 10)
                else:
                    assert want[s] != 0
            assert [want[s] for s in range(S) if s not in targets] == [0] * (S - len(targets))
            words, bad = device_verify(rs, work, stripes, data, par)
            assert words == want, (name, batch, [hex(w) for w in words], [hex(w) for w in want])
            assert bad == 7 + len(batch), (name, batch)


def test_single_bit_flips_reach_every_bit_plane(gpu):
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S = 9
    name, data, par, stripes, arenas = clean_case(10, 4, 8192, S, 0)
    assert H.lib.hec_verify_kernel_name(8192).decode().startswith("rs104_bs_verify_kernel")
    work = copies(arenas)
    for bit in range(8):
        shard_of(work, stripes, bit, 12)[4097 + 16 * bit] ^= 1 << bit
    want = oracle_words(work, stripes, 10, 4)
    assert want == [1 << 2] * 8 + [0]
    words, bad = device_verify(rs, work, stripes, data, par)
    assert words == want and bad == 7 + 8


@pytest.mark.parametrize("which", [0, 3])
def test_bad_stripes_counts_a_stripe_exactly_once(gpu, which):
    """Stripe 0 is corrupted in three different 8 KiB chunks and two parity
    shards, stripe 2 once: bad_stripes goes 7 -> 9."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    L = 4 * 8192
    name, data, par, stripes, arenas = clean_case(10, 4, L, 3, which)
    work = copies(arenas)
    for shard, pos in ((11, 5), (11, 8192 + 4100), (13, 3 * 8192 + 8191), (13, 77)):
        shard_of(work, stripes, 0, shard)[pos] ^= 0xFF
    shard_of(work, stripes, 2, 10)[L - 1] ^= 1
    want = oracle_words(work, stripes, 10, 4)
    assert want == [0b1010, 0, 0b0001]
    words, bad = device_verify(rs, work, stripes, data, par)
    assert words == want and bad == 9, (name, words, bad)


def test_bitsliced_batch_of_three_chunk_stripes(gpu):
    """70 stripes of 3 x 8 KiB: 210 bit-sliced workgroups, a chunk count per
    stripe that is no power of two and a grid that is no multiple of 8. Flips
    in chunks 0, 1 and 2 of the first and last stripe and of stripes 32, 33, 65
    and 66: with the launch limit of the small-grid build
    (tests/test_gpu_small_grid.py) a launch takes 33 such stripes, so those are
    the two sides of its stripe ranges and the words of a range land at its
    first stripe."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    S, L = 70, 3 * 8192
    assert H.lib.hec_verify_kernel_name(L).decode().startswith("rs104_bs_verify_kernel")
    name, data, par, stripes, arenas = clean_case(10, 4, L, S, 0)
    work = copies(arenas)
    want = [0] * S
    for n, s in enumerate((0, 32, 33, 65, 66, S - 1)):
        j = n % 4
        shard_of(work, stripes, s, 10 + j)[(n % 3) * 8192 + 4095 + n] ^= 0x01 << n
        want[s] = 1 << j
    shard_of(work, stripes, 34, 3)[L - 1] ^= 0x80  # a data shard: every parity shard differs
    want[34] = 0b1111
    assert oracle_words(work, stripes, 10, 4) == want
    words, bad = device_verify(rs, work, stripes, data, par)
    assert words == want, ([hex(w) for w in words], [hex(w) for w in want])
    assert bad == 7 + 7


@pytest.mark.parametrize("k,m", [(5, 5), (3, 2), (17, 3), (4, 32), (10, 2), (10, 6)])
@pytest.mark.parametrize("L", [4096, 100])
def test_other_codecs_take_the_generic_kernel(gpu, k, m, L):
    """Clean, then one flip per parity shard (stripe j: parity shard j; the
    last stripe stays clean). RS(10,2) and RS(10,6) run rs_verify_kernel<10>
    with 2 and 6 table rows; for RS(10,6) also parity shards 4 and 5 of one
    stripe, the bits of the second row group."""
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    S = m + 1
    for which in (0, 3):
        name, data, par, stripes, arenas = clean_case(k, m, L, S, which)
        words, bad = device_verify(rs, copies(arenas), stripes, data, par)
        assert words == [0] * S and bad == 7, name
        work = copies(arenas)
        for j in range(m):
            shard_of(work, stripes, j, k + j)[(37 * j + L - 1) % L] ^= 0x81
        want = oracle_words(work, stripes, k, m)
        assert want == [1 << j for j in range(m)] + [0]
        words, bad = device_verify(rs, work, stripes, data, par)
        assert words == want and bad == 7 + m, (name, [hex(w) for w in words])
        if (k, m) == (10, 6):
            work = copies(arenas)
            shard_of(work, stripes, 2, k + 4)[L - 1] ^= 0x04
            shard_of(work, stripes, 2, k + 5)[0] ^= 0x40
            want = oracle_words(work, stripes, k, m)
            assert want == [0, 0, 0b110000] + [0] * (S - 3)
            words, bad = device_verify(rs, work, stripes, data, par)
            assert words == want and bad == 7 + 1, (name, [hex(w) for w in words])


@pytest.mark.parametrize("L", [(1 << 32) - 8192, (1 << 32) + 8192, (1 << 32) + 4096 + 16])
def test_verify_shard_len_near_4gib(gpu, L):
    """Two-stripe verifies (112 GiB in HBM) at the edge of the 32-bit lane
    offsets: 2^32 - 8 KiB runs the bit-sliced verify with 32-bit offsets up to
    its last chunk, 2^32 + 8 KiB rs104_bs_verify_kernel<uint64_t>, 2^32 + 4 KiB
    + 16 rs_verify_kernel<10, true> with chunk offsets above 2^32 and a
    16-byte last chunk. The stored parity is encode_batch's, checked against
    the C oracle on the first and last 64 KiB of every shard; every flipped
    bit lies in one of those windows. A wrapped offset would compare other
    bytes: a clean word, or the wrong bit."""
    import torch
    import helyim_amd as H
    import helyim_amd.batch as B
    rs = H.ReedSolomon(10, 4)
    S, W = 2, 1 << 16
    name = H.lib.hec_verify_kernel_name(L).decode()
    assert name.startswith("rs104_bs_verify_kernel" if L % 8192 == 0 else "rs_verify_kernel<10>"), name
    torch.cuda.empty_cache()
    t = torch.empty((S, 14, L), dtype=torch.uint8, device="cuda")
    B.fill_splitmix(t, 10 * L, 0x5EED6000)
    t[:, 10:].zero_()
    B.encode_batch(rs, t)
    torch.cuda.synchronize()
    for s in range(S):
        for lo in (0, L - W):
            c = t[s, :, lo:lo + W].cpu().numpy()
            assert np.array_equal(c[10:], corc.encode_stripes(np.ascontiguousarray(c[None, :10]))[0]), (L, s, lo)
    words = torch.full((S,), -1, dtype=torch.int32, device="cuda")
    bad = torch.full((1,), 7, dtype=torch.int32, device="cuda")

    def verify():
        words.fill_(-1)
        H.verify_batch(rs, t, mismatch=words, bad_stripes=bad)
        torch.cuda.synchronize()
        return words.cpu().tolist(), int(bad.item())

    assert verify() == ([0, 0], 7)
    flips = [(0, 11, 0), (1, 13, L - 1)] + [(1, 10, o) for o in ((1 << 32) - 1, (1 << 32) + 5) if o < L]
    assert all(o < W or o >= L - W for _, _, o in flips)
    for s, i, o in flips:
        t[s, i, o] ^= 0x08
    assert verify() == ([0b0010, 0b1001 if len(flips) > 2 else 0b1000], 9)
    for s, i, o in flips:
        t[s, i, o] ^= 0x08
    t[0, 9, L - 1] ^= 0x01
    c = t[0, :, L - W:].cpu().numpy()
    ref = corc.encode_stripes(np.ascontiguousarray(c[None, :10]))[0]
    want = sum(1 << j for j in range(4) if (ref[j] != c[10 + j]).any())
    assert want != 0
    assert verify() == ([want, 0], 10)
    del t
    torch.cuda.empty_cache()


def test_more_than_32_parity_shards_is_refused(gpu):
    import torch
    import helyim_amd as H
    rs = H.ReedSolomon(4, 33)
    t = torch.zeros(37 * 64, dtype=torch.uint8, device="cuda")
    res = torch.zeros(2, dtype=torch.int32, device="cuda")
    assert H.lib.hec_gpu_verify_batch(rs.handle, t.data_ptr(), 37 * 64, 64, t.data_ptr() + 4 * 64, 37 * 64, 64, 64, 1,
                                      res.data_ptr(), None, None) == INVALID_ARGUMENT


def test_encode_then_verify_in_stream_order(gpu):
    """encode_batch then verify_batch on one non-default stream, no synchronise between."""
    import torch
    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    g = torch.Generator(device="cuda").manual_seed(11)
    t = torch.randint(0, 256, (6, 14, 16384), dtype=torch.uint8, device="cuda", generator=g)
    res = torch.full((6,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    batch.encode_batch(rs, t, stream=s)
    out = H.verify_batch(rs, t, mismatch=res, stream=s)
    s.synchronize()
    assert out is res and res.cpu().tolist() == [0] * 6
    # and the Python mirror's other shapes: allocated result, separate buffers
    t[3, 11, 9000] ^= 0x10
    torch.cuda.synchronize()
    assert H.verify_batch(rs, t).cpu().tolist() == [0, 0, 0, 2, 0, 0]
    data, par = t[:, :10].contiguous(), t[:, 10:].contiguous()
    bad = torch.zeros(1, dtype=torch.int32, device="cuda")
    assert H.verify_batch_sep(rs, data, par, bad_stripes=bad).cpu().tolist() == [0, 0, 0, 2, 0, 0]
    assert int(bad.item()) == 1
    with pytest.raises(ValueError):
        H.verify_batch(rs, t, mismatch=torch.zeros(5, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        H.verify_batch(rs, t, mismatch=torch.zeros(6, dtype=torch.int64, device="cuda"))


def test_kernel_names(gpu):
    import helyim_amd as H
    assert H.verify_kernel_name(1 << 20) == "rs104_bs_verify_kernel (bit-sliced)"
    assert H.verify_kernel_name(1000).startswith("rs_verify_kernel")
    assert H.verify_kernel_name(0).startswith("none")


# ---- host batches ----------------------------------------------------------------
def host_words(rs, base_ptr, L, S, pitch):
    import helyim_amd as H
    words = (ctypes.c_uint32 * (S + 1))(*([0xFFFFFFFF] * S + [SENTINEL]))
    n_bad = ctypes.c_uint32(1234)  # set, not accumulated
    rc = H.lib.hec_host_verify_batch(rs.handle, base_ptr, 14 * pitch, pitch, base_ptr + 10 * pitch, 14 * pitch, pitch,
                                     L, S, words, ctypes.byref(n_bad))
    assert rc == 0, (rc, H._lib.last_detail())
    assert words[S] == SENTINEL
    return [int(w) for w in words[:S]], int(n_bad.value)


@pytest.mark.parametrize("L", [8192, 1000])
def test_host_batch_three_paths_agree(gpu, L):
    import torch
    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    S, pitch = 3, F.r16(L) + 48
    rng = np.random.default_rng(L)
    image = rng.integers(0, 256, S * 14 * pitch, dtype=np.uint8)  # garbage in the shard gaps too
    view = image.reshape(S, 14, pitch)
    for s in range(S):
        bufs = [view[s, i, :L].copy() for i in range(10)] + [np.zeros(L, np.uint8) for _ in range(4)]
        corc.CReedSolomon(10, 4).encode(bufs)
        for j in range(4):
            view[s, 10 + j, :L] = bufs[10 + j]
    dirty = image.copy()
    dv = dirty.reshape(S, 14, pitch)
    dv[0, 12, L - 1] ^= 0x01
    dv[2, 4, 0] ^= 0x80
    stripes = F.stripes_of(F.stripe_major(14, L, S, pitch, 0, base=0))
    want = oracle_words([dirty], stripes, 10, 4)
    assert want[0] == 1 << 2 and want[1] == 0 and want[2] != 0

    pinned = H.HostBuffer(image.nbytes)
    results = {}
    try:
        for label, img in (("clean", image), ("dirty", dirty)):
            expect = [0] * S if label == "clean" else want
            # pinned, GPU-addressable memory: read in place
            pinned.array[:] = img
            assert batch.host_zero_copy(pinned.tensor((S, 14, pitch)))
            results[label, "pinned"] = host_words(rs, pinned.ptr, L, S, pitch)
            assert (pinned.array == img).all()
            # pageable memory through the pinned slots; for the short length a
            # full-size batch of random stripes goes first, so the reused slots
            # hold garbage where this call's pads fall
            page = img.copy()
            if L == 1000:
                big = rng.integers(0, 256, S * 14 * 8192, dtype=np.uint8)
                w, nb = host_words(rs, big.ctypes.data, 8192, S, 8192)
                assert all(w) and nb == S
            results[label, "pageable"] = host_words(rs, page.ctypes.data, L, S, pitch)
            assert (page == img).all()
            assert H.lib.hec_set_host_zero_copy(0) == 0
            try:
                if L == 1000:  # the same for the device slots of the copy pipeline
                    assert all(host_words(rs, big.ctypes.data, 8192, S, 8192)[0])
                results[label, "copies"] = host_words(rs, page.ctypes.data, L, S, pitch)
            finally:
                assert H.lib.hec_set_host_zero_copy(1) == 0
            for path in ("pinned", "pageable", "copies"):
                assert results[label, path] == (expect, sum(1 for w in expect if w)), (label, path, results)
        t = torch.from_numpy(dirty).view(S, 14, pitch)[:, :, :L]
        assert batch.host_verify_batch(rs, t).tolist() == want
    finally:
        H.lib.hec_set_host_zero_copy(1)
        pinned.close()


# ---- host batches past one chunk ---------------------------------------------------
CHUNK_BYTES = 96 << 20  # kChunkBytes of host_pipeline.cpp: a constant with no knob
# (k, m, L, shard pitch of the caller's image, stripes of a chunk, stripes): the
# smallest batches of four chunks with a short last one
CHUNKED = [(10, 4, 17, 64, 28086, 3 * 28086 + 13),
           (10, 4, 65541, F.r16(65541) + 48, 109, 3 * 109 + 13),
           (4, 32, 17, 32, 10922, 3 * 10922 + 7)]


def oracle_parity(k, m, data):
    """data [S, k, L] (any strides) -> the oracle's parity [m, S, L]. RS parity
    is bytewise, so the batch is one stripe of S * L columns: one encode call."""
    S, _, L = data.shape
    bufs = [np.ascontiguousarray(data[:, i]).reshape(S * L) for i in range(k)] + \
           [np.zeros(S * L, np.uint8) for _ in range(m)]
    corc.CReedSolomon(k, m).encode(bufs)
    return np.stack(bufs[k:]).reshape(m, S, L)


def batch_words(k, m, data, stored):
    """The expected words [S] (uint32) of data [S, k, L] with the stored parity
    [S, m, L]: bit j = the oracle's parity shard j differs somewhere."""
    par = oracle_parity(k, m, data)
    words = np.zeros(data.shape[0], np.uint32)
    for j in range(m):
        words |= (par[j] != stored[:, j]).any(axis=1).astype(np.uint32) << np.uint32(j)
    return words


@functools.lru_cache(maxsize=1)
def chunked_image(k, m, L, pitch, S, seed=0):
    """[S, k + m, pitch] of seeded random bytes, the shard gaps too, with the
    oracle's parity in place (never modified: tests damage copies). Only the
    last one is kept: the largest is 312 MB."""
    rng = np.random.default_rng([k, m, L, S, seed])
    image = np.frombuffer(bytearray(rng.bytes(S * (k + m) * pitch)), np.uint8).reshape(S, k + m, pitch)
    image[:, k:, :L] = oracle_parity(k, m, image[:, :k, :L]).transpose(1, 0, 2)
    image.setflags(write=False)
    return image


def random_image(nbytes):
    return np.frombuffer(np.random.default_rng(nbytes).bytes(nbytes), np.uint8)


def chunk_damage(image, k, m, L, C, seed=None):
    """A damaged copy of a clean image and its reference words. Dirty are the
    stripes on both sides of every chunk edge, the first, the last and one in
    the middle of each chunk (seeded: a random one); all others stay clean.
    Of the twelve dirty stripes (in a seeded order) four get one flip in a
    data shard, whose word is read from the reference, and the i-th of the
    other eight gets the parity rows j = i mod 8 (and row i mod m): every
    parity row is flipped in a stripe whose word is also asserted by
    construction -- one row per stripe at m = 4, rows 7, 15, 23 and 31 in
    one stripe at m = 32. The flips alternate between byte 0 and byte L - 1,
    in data and in parity."""
    S = image.shape[0]
    rng = np.random.default_rng(seed)
    last = S - 3 * C
    mids = [C // 2, C + C // 3, 2 * C + C // 5, 3 * C + last // 2] if seed is None else \
        [c * C + int(rng.integers(1, (C if c < 3 else last) - 1)) for c in range(4)]
    stripes = [0, C - 1, C, 2 * C - 1, 2 * C, 3 * C - 1, 3 * C, S - 1] + mids
    assert len(set(stripes)) == 12 and max(stripes) == S - 1
    order = list(range(12)) if seed is None else [int(t) for t in rng.permutation(12)]
    dirty = image.copy()
    alone = {}
    for s, t in zip(stripes, order):
        if t % 3 == 2:
            dirty[s, (7 * t) % k, L - 1 if t % 2 else 0] ^= 0x80 >> (t % 8)
            continue
        i = t - t // 3  # 0..7 over the stripes without a data flip
        rows = {j for j in range(m) if j % 8 == i} | {i % m}
        for j in rows:
            dirty[s, k + j, 0 if (i + j // 8) % 2 == 0 else L - 1] ^= 0x01 << (j % 8)
        alone[s] = sum(1 << j for j in rows)
    want = batch_words(k, m, dirty[:, :k, :L], dirty[:, k:, :L])
    assert sorted(np.flatnonzero(want).tolist()) == sorted(stripes)  # the reference calls every other stripe clean
    assert all(int(want[s]) == w for s, w in alone.items())          # parity flips alone: exactly their bits
    return dirty, want, stripes


def host_verify(rs, data, par, L, S):
    """hec_host_verify_batch on data / par = (address, stripe stride, shard
    stride) -> (words [S] uint32, n_bad_stripes). Words are prefilled with
    0xFFFFFFFF (a chunk that is never handed back shows), word S is a sentinel,
    and n_bad_stripes is preset: it is set, not accumulated."""
    import helyim_amd as H
    words = np.full(S + 1, 0xFFFFFFFF, np.uint32)
    words[S] = SENTINEL
    n_bad = ctypes.c_uint32(1234)
    rc = H.lib.hec_host_verify_batch(rs.handle, *data, *par, L, S, words.ctypes.data, ctypes.byref(n_bad))
    assert rc == 0, (rc, H._lib.last_detail())
    assert int(words[S]) == SENTINEL
    return words[:S].copy(), int(n_bad.value)


def in_place(ptr, k, n, pitch):
    return (ptr, n * pitch, pitch), (ptr + k * pitch, n * pitch, pitch)


def check_words(got, want, note):
    words, n_bad = got
    differ = np.flatnonzero(words != want)
    assert differ.size == 0, (note, differ[:8].tolist(), [hex(w) for w in words[differ[:8]]],
                              [hex(w) for w in want[differ[:8]]])
    assert n_bad == int(np.count_nonzero(want)), (note, n_bad)


def chunk_bytes_of_slot(n, L, C):
    return C * n * (-(-L // 256) * 256)


PAGEABLE = ("pageable", "copies")


@contextlib.contextmanager
def host_path(path):
    """Pageable batches go through the two pinned slots ("pageable": zero copy
    on, the default) or through the three device slots ("copies": zero copy
    off, restored on the way out)."""
    import helyim_amd as H
    assert path in PAGEABLE
    assert H.lib.hec_set_host_zero_copy(int(path == "pageable")) == 0
    try:
        yield path
    finally:
        assert H.lib.hec_set_host_zero_copy(1) == 0


@pytest.mark.parametrize("k,m,L,pitch,C,S", CHUNKED)
def test_host_verify_across_chunks(gpu, k, m, L, pitch, C, S):
    """Four chunks, the last one short, through every host path: pinned memory
    read in place, pageable memory through the two recycled pinned slots, and
    through the three recycled device slots with zero copy off. Every path must
    return exactly the reference words of a batch whose dirty stripes sit on
    both sides of every chunk edge, and all-zero words for the clean batch; the
    caller's bytes stay as they were. RS(4,32) uses all 32 bits of a word.

    At RS(10,4), L = 17 each pageable path first sizes its slots with the dirty
    batch, then verifies 340 random stripes of 65541 bytes -- every one
    mismatches -- so that the recycled slots hold garbage in bytes 17..255 of
    every 256-byte shard pitch when the clean batch follows: a launch that
    compares a byte past shard_len reports a clean stripe as bad."""
    import time
    import torch
    import helyim_amd as H
    from helyim_amd import batch
    n = k + m
    # else kChunkBytes changed; a small-chunk build (tests/test_gpu_small_chunk.py) takes the same batch, dirty
    # stripes and reference words in thousands of chunks, whose edges then fall elsewhere
    if not hasattr(H.lib, "hec_test_host_chunk_limits"):
        assert C == max(1, CHUNK_BYTES // (n * -(-L // 256) * 256)) and 3 * C < S < 4 * C
    rs = H.ReedSolomon(k, m)
    image = chunked_image(k, m, L, pitch, S)
    dirty, want, _ = chunk_damage(image, k, m, L, C)
    zeros = np.zeros(S, np.uint32)
    stale_pads = (k, m, L) == (10, 4, 17)
    if stale_pads:
        bS, bL, bpitch = CHUNKED[1][5], CHUNKED[1][2], CHUNKED[1][3]
        big = random_image(bS * 14 * bpitch)
        assert chunk_bytes_of_slot(14, bL, CHUNKED[1][4]) <= chunk_bytes_of_slot(n, L, C)  # no slot grows after `big`
    pinned = H.HostBuffer(image.nbytes)
    page = np.empty_like(image)
    try:
        for label, img, expect in (("dirty", dirty, want), ("clean", image, zeros)):
            pinned.array[:] = img.reshape(-1)
            assert batch.host_zero_copy(pinned.tensor((S, n, pitch)))
            t0 = time.perf_counter()
            got = host_verify(rs, *in_place(pinned.ptr, k, n, pitch), L, S)
            print(f"host verify RS({k},{m}) L={L} S={S} {label} pinned: {time.perf_counter() - t0:.3f} s")
            check_words(got, expect, (label, "pinned"))
            assert np.array_equal(pinned.array, img.reshape(-1)), label
        # with zero copy off a batch goes up in two 2-D copies per stripe: 1.7 s a
        # call at 84271 stripes, so of the two L = 17 codecs RS(10,4) alone takes that path
        for path in PAGEABLE if (m, L) != (32, 17) else PAGEABLE[:1]:
            for label, img, expect in (("dirty", dirty, want), ("clean", image, zeros)):
                page[...] = img
                with host_path(path):
                    if stale_pads and label == "clean":
                        words, n_bad = host_verify(rs, *in_place(big.ctypes.data, 10, 14, bpitch), bL, bS)
                        assert words.all() and n_bad == bS, path
                    t0 = time.perf_counter()
                    got = host_verify(rs, *in_place(page.ctypes.data, k, n, pitch), L, S)
                print(f"host verify RS({k},{m}) L={L} S={S} {label} {path}: {time.perf_counter() - t0:.3f} s")
                check_words(got, expect, (label, path))
                assert np.array_equal(page, img), (label, path)
        if L == 65541:  # the Python mirror on the same batch
            t = torch.from_numpy(dirty)[:, :, :L]
            assert np.array_equal(batch.host_verify_batch(rs, t), want)
    finally:
        H.lib.hec_set_host_zero_copy(1)
        pinned.close()


@pytest.mark.parametrize("path", PAGEABLE)
def test_host_verify_across_chunks_shard_major(gpu, path):
    """The four chunks of the RS(10,4), L = 17 batch with data and parity in
    arrays of their own, shard-major: [10][S][64] and [4][S][64], so a stripe
    is 64 bytes from the next and a shard S * 64."""
    import time
    import helyim_amd as H
    k, m, L, pitch, C, S = CHUNKED[0]
    rs = H.ReedSolomon(k, m)
    dirty, want, _ = chunk_damage(chunked_image(k, m, L, pitch, S), k, m, L, C)
    data = np.ascontiguousarray(dirty[:, :k].transpose(1, 0, 2))
    par = np.ascontiguousarray(dirty[:, k:].transpose(1, 0, 2))
    d0, p0 = data.copy(), par.copy()
    with host_path(path):
        t0 = time.perf_counter()
        got = host_verify(rs, (data.ctypes.data, pitch, S * pitch), (par.ctypes.data, pitch, S * pitch), L, S)
    print(f"host verify RS({k},{m}) L={L} S={S} dirty shard-major {path}: {time.perf_counter() - t0:.3f} s")
    check_words(got, want, (path, "shard-major"))
    assert np.array_equal(data, d0) and np.array_equal(par, p0), path


PINNED_COPIES = (10, 1000)  # stripes, shard length: chunks of 3, 3, 3 and 1 stripes in the small-chunk build


def test_host_verify_pinned_memory_on_the_copy_pipeline(gpu):
    """Pinned memory with zero copy off: the copy pipeline's two 2-D copies a
    stripe read the caller's pinned arena (the tests above give that path
    pageable memory only). Ten RS(10,4) stripes of 1000 bytes -- a multiple of
    neither 16 nor 256 -- after ten random stripes of 1024 bytes went through
    the same device slots, so the pads of the 1024-byte staging pitch hold
    garbage. Dirty are both sides of the first chunk edge of the small-chunk
    build (stripes 2 and 3), stripe 5 in its last data byte and the short last
    chunk's only stripe; words and count against the oracle, clean batch all
    zero, the caller's bytes as they were."""
    import helyim_amd as H
    S, L = PINNED_COPIES
    k, m, n, pitch = 10, 4, 14, F.r16(L) + 48
    rs = H.ReedSolomon(k, m)
    image = np.random.default_rng(L).integers(0, 256, (S, n, pitch), dtype=np.uint8)  # the shard gaps too
    image[:, k:, :L] = oracle_parity(k, m, image[:, :k, :L]).transpose(1, 0, 2)
    dirty = image.copy()
    dirty[2, 11, 0] ^= 0x01
    dirty[3, 0, 17] ^= 0x80
    dirty[5, 9, L - 1] ^= 0x10
    dirty[9, 13, L - 1] ^= 0x04
    want = batch_words(k, m, dirty[:, :k, :L], dirty[:, k:, :L])
    assert np.flatnonzero(want).tolist() == [2, 3, 5, 9] and int(want[2]) == 1 << 1 and int(want[9]) == 1 << 3
    big = random_image(S * n * 1024)
    pinned = H.HostBuffer(image.nbytes)
    try:
        with host_path("copies"):
            words, n_bad = host_verify(rs, *in_place(big.ctypes.data, k, n, 1024), 1024, S)
            assert words.all() and n_bad == S
            for label, img, expect in (("dirty", dirty, want), ("clean", image, np.zeros(S, np.uint32))):
                pinned.array[:] = img.reshape(-1)
                got = host_verify(rs, *in_place(pinned.ptr, k, n, pitch), L, S)
                check_words(got, expect, (label, "pinned copies"))
                assert np.array_equal(pinned.array, img.reshape(-1)), label
    finally:
        H.lib.hec_set_host_zero_copy(1)
        pinned.close()


@pytest.fixture(scope="module")
def thread_batches():
    """Four batches (dirty, its copy, reference words), each built by a thread
    of its own: the clean RS(10,4), L = 17 image with its stripes in a seeded
    order (which keeps every stripe's parity right) and a seeded dirty set."""
    import threading
    T = 4
    k, m, L, pitch, C, S = CHUNKED[0]
    image = chunked_image(k, m, L, pitch, S)
    batches = [None] * T

    def prepare(t):
        own = image[np.random.default_rng(100 + t).permutation(S)]
        dirty, want, _ = chunk_damage(own, k, m, L, C, seed=200 + t)
        batches[t] = (dirty, dirty.copy(), want)

    workers = [threading.Thread(target=prepare, args=(t,)) for t in range(T)]
    for th in workers:
        th.start()
    for th in workers:
        th.join()
    assert all(batches), "a thread failed to build its batch"
    assert len({tuple(np.flatnonzero(b[2]).tolist()) for b in batches}) == T  # T different dirty sets
    return batches


@pytest.mark.parametrize("path", PAGEABLE)
def test_host_verify_four_threads(gpu, thread_batches, path):
    """Four threads, each with its own four-chunk RS(10,4) batch of 17-byte
    shards and its own dirty stripes, the chunk edges among them. Each calls
    hec_host_verify_batch twice while the others do: a pipeline and its result
    words are leased per call, so every result is the thread's own reference."""
    import threading
    import time
    import helyim_amd as H
    k, m, L, pitch, C, S = CHUNKED[0]
    rs = H.ReedSolomon(k, m)
    batches = thread_batches
    T = len(batches)
    gate = threading.Barrier(T)
    results, errors = [None] * T, []

    def run(t):
        try:
            gate.wait(timeout=60)
            results[t] = [host_verify(rs, *in_place(batches[t][0].ctypes.data, k, 14, pitch), L, S) for _ in range(2)]
        except BaseException as e:  # an assertion in a thread fails the test, not the thread alone
            errors.append((t, repr(e)))
            gate.abort()

    threads = [threading.Thread(target=run, args=(t,)) for t in range(T)]
    with host_path(path):
        t0 = time.perf_counter()
        for th in threads:
            th.start()
        for th in threads:
            th.join()
    print(f"host verify four threads x two calls, {path}: {time.perf_counter() - t0:.3f} s")
    assert not errors, (path, errors)
    for t, (dirty, before, want) in enumerate(batches):
        for call in range(2):
            check_words(results[t][call], want, (path, "thread", t, "call", call))
        assert np.array_equal(dirty, before), (path, t)


# ---- shard files -----------------------------------------------------------------
BLOCK = 4096


@pytest.fixture(scope="module")
def shard_files(tmp_path_factory):
    """Oracle-written shard files of a seeded .dat: small geometry, each shard
    a few hundred KiB and not a multiple of the 4096-byte scrub block."""
    d = tmp_path_factory.mktemp("scrub")
    base = str(d / "7")
    large, small = 64 * 1001, 1001  # three large rows, then 58 small ones: 250250 bytes per shard
    open(base + ".dat", "wb").write(corc.splitmix64_bytes(99, 10 * large * 3 + 10 * small * 57 + 123).tobytes())
    assert corc.write_ec_files(base, small, large, small) == 0
    files = [open(base + ".ec%02d" % i, "rb").read() for i in range(14)]
    size = len(files[0])
    assert all(len(f) == size for f in files) and 200_000 < size < 500_000
    assert size % BLOCK > 1 and (size % BLOCK) % 16 != 0  # a short last block with a ragged tail
    return base, files, size


def scrub_copy(shard_files, tmp_path):
    base, files, size = shard_files
    new = str(tmp_path / "v")
    for i, f in enumerate(files):
        open(new + ".ec%02d" % i, "wb").write(f)
    return new, [bytearray(f) for f in files], size


def flip(base, shard, offset):
    with open(base + ".ec%02d" % shard, "r+b") as f:
        f.seek(offset)
        b = f.read(1)
        f.seek(offset)
        f.write(bytes([b[0] ^ 0x5A]))


def file_oracle_mask(files, lo, hi):
    rs = corc.CReedSolomon(10, 4)
    bufs = [np.frombuffer(bytes(files[i][lo:hi]), np.uint8).copy() for i in range(10)] + \
           [np.zeros(hi - lo, np.uint8) for _ in range(4)]
    rs.encode(bufs)
    return sum(1 << j for j in range(4)
               if (bufs[10 + j] != np.frombuffer(bytes(files[10 + j][lo:hi]), np.uint8)).any())


def test_files_clean_and_read_only(gpu, shard_files, tmp_path):
    import helyim_amd as H
    base, files, size = scrub_copy(shard_files, tmp_path)
    for i in range(14):
        os.utime(base + ".ec%02d" % i, ns=(10**18, 10**18 + i))
    before = [os.stat(base + ".ec%02d" % i).st_mtime_ns for i in range(14)]
    n_blocks, n_bad, bad = H.verify_ec_files(base, BLOCK)
    assert (n_blocks, n_bad, bad) == (-(-size // BLOCK), 0, [])
    # the default 1 MiB block: one short block
    assert H.verify_ec_files(base) == (1, 0, [])
    assert [os.stat(base + ".ec%02d" % i).st_mtime_ns for i in range(14)] == before
    assert [open(base + ".ec%02d" % i, "rb").read() for i in range(14)] == [bytes(f) for f in files]


def test_files_flips_are_located(gpu, shard_files, tmp_path):
    import helyim_amd as H
    base, files, size = scrub_copy(shard_files, tmp_path)
    x = 5 * BLOCK + 1234
    flip(base, 3, x)
    files[3][x] ^= 0x5A
    lo = x // BLOCK * BLOCK
    mask = file_oracle_mask(files, lo, lo + BLOCK)
    assert mask != 0
    assert H.verify_ec_files(base, BLOCK) == (-(-size // BLOCK), 1, [(lo, BLOCK, mask)])
    # the short last block
    last = size // BLOCK * BLOCK
    flip(base, 12, size - 1)
    files[12][size - 1] ^= 0x5A
    assert H.verify_ec_files(base, BLOCK) == (-(-size // BLOCK), 2, [(lo, BLOCK, mask), (last, size - last, 1 << 2)])
    # a third bad block, cap 2: the total and the first two in ascending offset
    flip(base, 10, 0)
    n_blocks, n_bad, bad = H.verify_ec_files(base, BLOCK, cap=2)
    assert (n_bad, bad) == (3, [(0, BLOCK, 1), (lo, BLOCK, mask)])
    assert H.verify_ec_files(base, BLOCK, cap=0) == (n_blocks, 3, [])
    # 8 KiB blocks take the bit-sliced kernel for the whole blocks
    got = H.verify_ec_files(base, 2 * BLOCK)
    l2 = x // (2 * BLOCK) * (2 * BLOCK)
    last2 = size // (2 * BLOCK) * (2 * BLOCK)
    assert got == (-(-size // (2 * BLOCK)), 3, [(0, 2 * BLOCK, 1), (l2, 2 * BLOCK, mask),
                                                (last2, size - last2, 1 << 2)])


def test_files_longer_than_the_two_slots(gpu, tmp_path):
    """Shards of 8 MiB and a ragged rest: three chunks of the scrub's 4 MiB
    column range, so both pinned slots are reused and the results of a chunk
    are collected while later ones are in flight. Parity is bytewise, so the
    files are the oracle's encode of ten random streams, no block geometry."""
    import helyim_amd as H
    block, size = 65536, (8 << 20) + 300_000 + 7
    rng = np.random.default_rng(2024)
    bufs = [rng.integers(0, 256, size, dtype=np.uint8) for _ in range(10)] + [np.zeros(size, np.uint8) for _ in range(4)]
    corc.CReedSolomon(10, 4).encode(bufs)
    hits = [(11, 5), (2, (4 << 20) - 1), (13, (4 << 20)), (10, (8 << 20) + 12345), (12, size - 1)]
    for shard, off in hits:
        bufs[shard][off] ^= 0x33
    base = str(tmp_path / "big")
    for i in range(14):
        bufs[i].tofile(base + ".ec%02d" % i)
    # 5 MiB blocks are larger than a chunk's 4 MiB: one block per chunk, and the
    # last chunk is a short block alone, whose word is the slot's first
    for block in (65536, 5 << 20):
        want = {}
        for shard, off in hits:
            lo = off // block * block
            want[lo] = (lo, min(block, size - lo), file_oracle_mask(bufs, lo, min(lo + block, size)))
        assert want[0][2] & 1 << 1 and want[size // block * block][:2] == (size // block * block, size % block)
        if block == 65536:
            assert want[0][2] == 1 << 1 and want[size // block * block][2] == 1 << 2
        assert H.verify_ec_files(base, block) == (-(-size // block), len(want), [want[k] for k in sorted(want)]), block
    # 1 MiB blocks: four blocks per chunk; the same bytes, coarser
    n_blocks, n_bad, bad = H.verify_ec_files(base)
    assert (n_blocks, n_bad) == (9, 4) and [b[0] >> 20 for b in bad] == [0, 3, 4, 8]
    assert bad[3] == (8 << 20, size - (8 << 20), file_oracle_mask(bufs, 8 << 20, size))


def test_files_errors(gpu, shard_files, tmp_path):
    import helyim_amd as H
    base, files, size = scrub_copy(shard_files, tmp_path)
    lib = H.lib
    nb, nbl = ctypes.c_size_t(9), ctypes.c_uint64(9)
    assert lib.hec_verify_ec_files(base.encode(), 1000, None, 0, ctypes.byref(nb), ctypes.byref(nbl)) == INVALID_ARGUMENT
    os.truncate(base + ".ec05", size - 1)
    assert lib.hec_verify_ec_files(base.encode(), BLOCK, None, 0, ctypes.byref(nb), ctypes.byref(nbl)) == EC_SHARD_SIZE
    assert H._lib.last_values()[:2] == (size, size - 1)
    with pytest.raises(H.UnexpectedEcShardSize):
        H.verify_ec_files(base, BLOCK)
    os.remove(base + ".ec13")
    assert lib.hec_verify_ec_files(base.encode(), BLOCK, None, 0, ctypes.byref(nb), ctypes.byref(nbl)) == SHARD_NOT_FOUND
    assert ".ec13" in H._lib.last_detail()
    empty = str(tmp_path / "e")
    for i in range(14):
        open(empty + ".ec%02d" % i, "wb").close()
    assert H.verify_ec_files(empty, BLOCK) == (0, 0, [])
