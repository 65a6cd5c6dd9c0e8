"""The update entry points without a GPU: the symbols, and every argument and
codec check that precedes device work, in the order include/hec.h states (fake
non-null pointers are never touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_util import L, P, c_parameters, codes, has_gpu
from conftest import ROOT

C = codes()
INVALID_ARGUMENT, EMPTY_SHARD, NO_DEVICE = C["HEC_ERR_INVALID_ARGUMENT"], C["HEC_ERR_EMPTY_SHARD"], C["HEC_ERR_NO_DEVICE"]
NEW = ("hec_gpu_update_batch", "hec_host_update_batch", "hec_rs_update", "hec_update_kernel_name")
Q = P + (1 << 30)  # a second fake arena


def gpu_update(rs, **change):
    """hec_gpu_update_batch on fake pointers: the old arena in place with the parity, the new data apart."""
    import helyim_amd as H
    a = dict(old=P, ost=14 * L, osh=L, new=Q, nst=10 * L, nsh=L, par=P + 10 * L, pst=14 * L, psh=L, length=L, n=2,
             masks=P)
    assert set(change) <= set(a), change
    a.update(change)
    return H.lib.hec_gpu_update_batch(rs, *a.values(), None)


def host_update(rs, **change):
    import helyim_amd as H
    a = dict(new=Q, nst=10 * L, nsh=L, par=P, pst=4 * L, psh=L, length=L, n=2, masks=P)
    assert set(change) <= set(a), change
    a.update(change)
    return H.lib.hec_host_update_batch(rs, *a.values())


BATCHED = (gpu_update, host_update)


def test_symbols_and_signatures():
    import helyim_amd as H
    from helyim_amd import _lib, batch
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hec.h")).read(), flags=re.S)
    rust = open(os.path.join(ROOT, "rust", "hec-sys", "src", "lib.rs")).read()
    for name in NEW:
        assert hasattr(H.lib, name), name
        assert name in _lib.SIGNATURES, name
        assert len(_lib.SIGNATURES[name][1]) == len(c_parameters(header, name)), name
        assert "pub fn %s(" % name in rust, name
    # the device call is the encode's with an old arena in front and the mask words before the stream
    enc = c_parameters(header, "hec_gpu_encode_batch")
    got = c_parameters(header, NEW[0])
    assert len(got) == len(enc) + 4 and got[0] == enc[0] and got[-4:-2] == enc[-3:-1] and got[-1] == enc[-1]
    assert got[1:4] == ["const uint8_t* d_old", "uint64_t old_stripe_stride", "uint64_t old_shard_stride"]
    assert got[-2] == "const uint32_t* d_update_masks"
    host = c_parameters(header, NEW[1])
    assert len(host) == len(c_parameters(header, "hec_host_encode_batch")) + 1 and host[-1] == "const uint32_t* h_update_masks"
    assert c_parameters(header, NEW[2])[3] == "const uint8_t* const* new_data"
    for name in ("update_batch", "update_batch_sep", "host_update_batch", "update_kernel_name"):
        assert callable(getattr(batch, name)), name
    assert callable(H.ReedSolomon.update)


@pytest.mark.parametrize("call", BATCHED, ids=lambda f: f.__name__)
def test_batch_arguments_checked_before_device_in_order(call):
    import helyim_amd as H
    codec = H.ReedSolomon(10, 4)  # kept alive: the handle dies with it
    rs = codec.handle
    assert call(rs, n=0) == 0
    assert call(None) == INVALID_ARGUMENT
    for pointer in ("new", "par", "masks"):
        assert call(rs, **{pointer: None}) == INVALID_ARGUMENT, pointer
        assert "null" in H._lib.last_detail()
        assert call(rs, n=0, **{pointer: None}) == INVALID_ARGUMENT, pointer
        assert call(rs, length=0, **{pointer: None}) == INVALID_ARGUMENT, pointer  # the nulls come first
    assert call(rs, length=0) == EMPTY_SHARD
    assert call(rs, length=0, nsh=0, psh=0) == EMPTY_SHARD  # the empty shard before the layout
    for st, sh in (("nst", "nsh"), ("pst", "psh")):
        assert call(rs, **{sh: L - 1}) == INVALID_ARGUMENT, sh              # shards overlap
        assert call(rs, **{sh: L - 16}) == INVALID_ARGUMENT, sh
        assert call(rs, **{st: L - 1, sh: 2 * L}) == INVALID_ARGUMENT, st   # stripes overlap
        assert call(rs, **{st: 1 << 62}, n=8) == INVALID_ARGUMENT, st       # extent wraps 64 bits
        assert "overflows" in H._lib.last_detail()
    assert call(rs, n=0, nsh=L, psh=L) == 0


def test_old_arena_is_checked_only_when_given():
    import helyim_amd as H
    codec = H.ReedSolomon(10, 4)  # kept alive: the handle dies with it
    rs = codec.handle
    assert gpu_update(rs, osh=L - 1) == INVALID_ARGUMENT
    assert "old" in H._lib.last_detail()
    assert gpu_update(rs, ost=L - 1, osh=2 * L) == INVALID_ARGUMENT
    assert gpu_update(rs, ost=1 << 62, n=8) == INVALID_ARGUMENT
    assert "overflows" in H._lib.last_detail()
    # a null old arena is valid (old is zero) and its strides mean nothing
    assert gpu_update(rs, old=None, n=0) == 0
    assert gpu_update(rs, old=None, ost=0, osh=0, n=0) == 0
    assert gpu_update(rs, old=None, osh=L - 1, nsh=L - 1) == INVALID_ARGUMENT
    assert "new data" in H._lib.last_detail()
    assert gpu_update(rs, old=None, length=0) == EMPTY_SHARD


@pytest.mark.parametrize("k,m", [(5, 5), (10, 2), (10, 6)])
def test_other_codecs_are_refused_by_the_batched_calls(k, m):
    import helyim_amd as H
    codec = H.ReedSolomon(k, m)
    rs = codec.handle
    for call in BATCHED:
        assert call(rs) == INVALID_ARGUMENT
        assert "RS(10,4) only" in H._lib.last_detail()
        assert call(rs, n=0) == INVALID_ARGUMENT
        assert call(rs, nsh=L - 1) == INVALID_ARGUMENT and "RS(10,4) only" in H._lib.last_detail()  # before the layout
        assert call(rs, length=0) == EMPTY_SHARD   # after the empty shard
        assert call(rs, masks=None) == INVALID_ARGUMENT and "null" in H._lib.last_detail()  # after the nulls


def per_call(rs, k, m, n_bytes=64, changed=(1,), lens=None, null=(), no_new=False, n=None, fill=None):
    """hec_rs_update on real host buffers -> (status, buffers). changed: the
    data shards with a new_data entry; null: shard slots passed as NULL."""
    import helyim_amd as H
    total = k + m
    bufs = [np.full(n_bytes, 0x11 * (i + 1) & 0xFF if fill is None else fill, dtype=np.uint8) for i in range(total)]
    news = [np.full(n_bytes, 0xC3, dtype=np.uint8) for _ in range(k)]
    ptrs = (ctypes.c_void_p * total)(*[None if i in null else b.ctypes.data for i, b in enumerate(bufs)])
    ln = (ctypes.c_size_t * total)(*(lens or [n_bytes] * total))
    nw = None if no_new else (ctypes.c_void_p * k)(*[news[c].ctypes.data if c in changed else None for c in range(k)])
    return H.lib.hec_rs_update(rs.handle, ptrs, ln, nw, total if n is None else n), (bufs, news)


@pytest.mark.parametrize("k,m", [(10, 4), (5, 3)])
def test_per_call_validation_in_order(k, m):
    import helyim_amd as H
    rs, n = H.ReedSolomon(k, m), k + m
    assert H.lib.hec_rs_update(None, None, None, None, n) == INVALID_ARGUMENT
    bufs = (ctypes.c_void_p * n)()
    ln = (ctypes.c_size_t * n)()
    nw = (ctypes.c_void_p * k)()
    assert H.lib.hec_rs_update(None, bufs, ln, nw, n) == INVALID_ARGUMENT
    assert H.lib.hec_rs_update(rs.handle, None, ln, nw, n) == INVALID_ARGUMENT
    assert H.lib.hec_rs_update(rs.handle, bufs, None, nw, n) == INVALID_ARGUMENT
    assert per_call(rs, k, m, no_new=True)[0] == INVALID_ARGUMENT
    # the count before the pointers and the lengths
    assert per_call(rs, k, m, n=n - 1, null=(1, k), lens=[0] * n)[0] == C["HEC_ERR_TOO_FEW_SHARDS"]
    assert per_call(rs, k, m, n=n + 1, null=(1, k), lens=[0] * n)[0] == C["HEC_ERR_TOO_MANY_SHARDS"]
    # a changed shard without its old buffer, a null parity pointer: before the lengths
    assert per_call(rs, k, m, changed=(1,), null=(1,), lens=[0] * n)[0] == INVALID_ARGUMENT
    assert "old buffer" in H._lib.last_detail()
    assert per_call(rs, k, m, changed=(1,), null=(n - 1,), lens=[0] * n)[0] == INVALID_ARGUMENT
    assert "parity" in H._lib.last_detail()
    assert per_call(rs, k, m, changed=(), null=(k,))[0] == INVALID_ARGUMENT  # the parity is required even for a no-op
    # the lengths in use: the changed shards' old slots and the parity
    lens = [64] * n
    lens[1] = 0
    assert per_call(rs, k, m, changed=(1,), lens=lens)[0] == EMPTY_SHARD
    lens[1], lens[k] = 64, 0
    assert per_call(rs, k, m, changed=(1,), lens=lens)[0] == EMPTY_SHARD
    lens[k] = 65
    assert per_call(rs, k, m, changed=(1,), lens=lens)[0] == C["HEC_ERR_INCORRECT_SHARD_SIZE"]
    lens[k], lens[n - 1] = 64, 63
    assert per_call(rs, k, m, changed=(), lens=lens)[0] == C["HEC_ERR_INCORRECT_SHARD_SIZE"]


@pytest.mark.parametrize("k,m", [(10, 4), (5, 3)])
def test_per_call_without_a_changed_shard_touches_nothing(k, m):
    import helyim_amd as H
    rs, n = H.ReedSolomon(k, m), k + m
    # lengths and pointers of unused old slots are ignored
    lens = [0, 7, 9] + [5] * (k - 3) + [64] * m
    rc, (bufs, _news) = per_call(rs, k, m, changed=(), lens=lens, null=(0, 2))
    assert rc == 0
    for i, b in enumerate(bufs):
        assert (b == (0x11 * (i + 1) & 0xFF)).all(), i


def test_kernel_names():
    import helyim_amd as H
    from helyim_amd import batch
    for length in (1, 15, 16, 1000, 4096, 4097, 1 << 20, (1 << 32) + 16):
        assert batch.update_kernel_name(length).startswith("rs104_update_kernel"), length
    assert H.lib.hec_update_kernel_name(0).decode().startswith("none")


def test_python_mirror_checks_its_arguments():
    import torch

    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    host = torch.zeros((2, 10, 64), dtype=torch.uint8)
    with pytest.raises(TypeError):
        batch.update_batch_sep(rs, None, host, torch.zeros((2, 4, 64), dtype=torch.uint8), [1, 1])
    with pytest.raises(ValueError):
        batch.host_update_batch(rs, host, torch.zeros((2, 4, 32), dtype=torch.uint8), [1, 1])
    with pytest.raises(ValueError):
        batch.host_update_batch(rs, host, torch.zeros((2, 4, 64), dtype=torch.uint8), [1, 1, 1])
    with pytest.raises(ValueError):
        batch.host_update_batch(rs, torch.zeros((2, 14, 64), dtype=torch.uint8), torch.zeros((2, 4, 64), dtype=torch.uint8),
                                [1, 1])
    with pytest.raises(ValueError):
        rs.update([np.zeros(8, np.uint8)] * 14, [None] * 9)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_no_device_is_an_error_not_a_fallback():
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for call in BATCHED:
        assert call(rs.handle) == NO_DEVICE, call.__name__
    assert gpu_update(rs.handle, old=None) == NO_DEVICE
    for k, m in ((10, 4), (5, 3)):
        rc, (bufs, _news) = per_call(H.ReedSolomon(k, m), k, m, changed=(0, k - 1))
        assert rc == NO_DEVICE
        for i, b in enumerate(bufs):
            assert (b == (0x11 * (i + 1) & 0xFF)).all(), i
