"""The reconstruct-some entry points without a GPU: the symbols, and every
argument and codec check that precedes device work (fake non-null pointers are
never touched)."""
import ctypes
import os
import re

import numpy as np
import pytest

from abi_util import L, P, c_parameters, call, codes, has_gpu
from conftest import ROOT

C = codes()
INVALID_ARGUMENT, EMPTY_SHARD, NO_DEVICE = C["HEC_ERR_INVALID_ARGUMENT"], C["HEC_ERR_EMPTY_SHARD"], C["HEC_ERR_NO_DEVICE"]
NEW = ("hec_gpu_reconstruct_some_batch", "hec_gpu_reconstruct_some_ragged", "hec_host_reconstruct_some_batch",
       "hec_rs_reconstruct_some", "hec_rs_reconstruct_some_batch", "hec_reconstruct_some_kernel_name",
       "hec_reconstruct_some_batch_kernel_name")


def gpu_some(lib, rs, **args):
    return call("hec_gpu_reconstruct_some_batch", rs, **args)


def host_some(lib, rs, **args):
    return call("hec_host_reconstruct_some_batch", rs, **args)


STRIDED = (gpu_some, host_some)


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
    # each call is the one it extends with the want words (or flags) after the masks (or presence flags)
    full = c_parameters(header, "hec_gpu_reconstruct_batch")
    assert c_parameters(header, NEW[0]) == full[:7] + ["const uint32_t* d_want_masks"] + full[7:]
    full = c_parameters(header, "hec_gpu_reconstruct_ragged")
    assert c_parameters(header, NEW[1]) == full[:3] + ["const uint32_t* h_want_masks"] + full[3:]
    full = c_parameters(header, "hec_host_reconstruct_batch")
    assert c_parameters(header, NEW[2]) == full[:7] + ["const uint32_t* h_want_masks"] + full[7:]
    full = c_parameters(header, "hec_rs_reconstruct")
    assert c_parameters(header, NEW[3]) == full[:4] + ["const uint8_t* required"] + full[4:]
    full = c_parameters(header, "hec_rs_reconstruct_batch")
    assert c_parameters(header, NEW[4]) == full[:4] + ["const uint8_t* required", "size_t n_stripes", "size_t* bad_index"]
    for name in ("reconstruct_some_batch", "reconstruct_some_ragged", "host_reconstruct_some_batch"):
        assert callable(getattr(batch, name)), name
    assert callable(H.ReedSolomon.reconstruct_some)


@pytest.mark.parametrize("call", STRIDED, ids=lambda f: f.__name__)
def test_strided_arguments_checked_before_device(call):
    import helyim_amd as H
    lib, rs = H.lib, H.ReedSolomon(10, 4)
    assert call(lib, rs.handle, n=0) == 0
    assert call(lib, None) == INVALID_ARGUMENT
    for pointer in ("shards", "masks", "wants"):
        assert call(lib, rs.handle, **{pointer: None}) == INVALID_ARGUMENT, pointer
        assert "null" in H._lib.last_detail()
        assert call(lib, rs.handle, n=0, **{pointer: None}) == INVALID_ARGUMENT, pointer
        # the nulls come first, as in the call each extends
        assert call(lib, rs.handle, length=0, **{pointer: None}) == INVALID_ARGUMENT, pointer
    assert call(lib, rs.handle, length=0) == EMPTY_SHARD
    assert call(lib, rs.handle, length=0, sh=0) == EMPTY_SHARD             # the empty shard before the layout
    assert call(lib, rs.handle, sh=L - 1) == INVALID_ARGUMENT              # shards overlap
    assert call(lib, rs.handle, sh=L - 16) == INVALID_ARGUMENT
    assert call(lib, rs.handle, st=L - 1, sh=2 * L) == INVALID_ARGUMENT    # stripes overlap
    assert call(lib, rs.handle, st=1 << 62, n=8) == INVALID_ARGUMENT       # extent wraps 64 bits
    assert "overflows" in H._lib.last_detail()


def test_ragged_arguments_checked_before_device():
    import helyim_amd as H
    from helyim_amd import batch
    lib, rs = H.lib, H.ReedSolomon(10, 4)
    descs = np.zeros(2, dtype=batch.desc_dtype())
    descs["offset"], descs["shard_stride"], descs["shard_len"], descs["present_mask"] = (0, 16 * L), L, L, 0x3FFE
    wants = np.array([1, 1], dtype=np.uint32)

    def call(rs_=rs.handle, base=P, d=descs.ctypes.data, w=wants.ctypes.data, n=2):
        return lib.hec_gpu_reconstruct_some_ragged(rs_, base, d, w, n, None, None)

    assert call(n=0) == 0 and call(n=0, d=None, w=None) == 0
    for kw in ({"rs_": None}, {"base": None}, {"d": None}, {"w": None}):
        assert call(**kw) == INVALID_ARGUMENT, kw
        assert "null" in H._lib.last_detail()
    bad = descs.copy()
    bad["shard_len"][1] = 0
    assert call(d=bad.ctypes.data) == EMPTY_SHARD
    bad = descs.copy()
    bad["offset"][1] += 8
    assert call(d=bad.ctypes.data) == INVALID_ARGUMENT
    bad = descs.copy()
    bad["shard_stride"][0] = L - 16
    assert call(d=bad.ctypes.data) == INVALID_ARGUMENT
    assert call(base=P + 4) == INVALID_ARGUMENT


@pytest.mark.parametrize("k,m", [(5, 5), (10, 2), (10, 6)])
def test_other_codecs_are_refused_by_the_batched_calls(k, m):
    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(k, m)
    for call in STRIDED:
        assert call(H.lib, rs.handle, st=(k + m) * L) == INVALID_ARGUMENT
        assert "RS(10,4) only" in H._lib.last_detail()
        assert call(H.lib, rs.handle, st=(k + m) * L, n=0) == INVALID_ARGUMENT
        assert call(H.lib, rs.handle, st=(k + m) * L, length=0) == EMPTY_SHARD  # as the scrub calls: after the empty shard
    descs = np.zeros(1, dtype=batch.desc_dtype())
    descs["shard_stride"], descs["shard_len"], descs["present_mask"] = L, L, 1
    wants = np.ones(1, dtype=np.uint32)
    assert H.lib.hec_gpu_reconstruct_some_ragged(rs.handle, P, descs.ctypes.data, wants.ctypes.data, 1, None,
                                                 None) == INVALID_ARGUMENT
    assert "RS(10,4) only" in H._lib.last_detail()


def _per_call(rs, n, L_, present, required, lens=None, null=()):
    import helyim_amd as H
    bufs = [np.zeros(L_, dtype=np.uint8) for _ in range(n)]
    ptrs = (ctypes.c_void_p * n)(*[None if i in null else b.ctypes.data for i, b in enumerate(bufs)])
    ln = (ctypes.c_size_t * n)(*(lens or [L_] * n))
    pr = (ctypes.c_uint8 * n)(*present)
    rq = None if required is None else (ctypes.c_uint8 * n)(*required)
    return H.lib.hec_rs_reconstruct_some(rs.handle, ptrs, ln, pr, rq, n), (ptrs, ln, pr, rq, bufs)


@pytest.mark.parametrize("k,m", [(10, 4), (5, 3)])
def test_per_call_validation_is_reconstructs_in_its_order(k, m):
    import helyim_amd as H
    rs, n = H.ReedSolomon(k, m), k + m
    ones = [1] * n
    erased = [0] + [1] * (n - 1)
    assert H.lib.hec_rs_reconstruct_some(None, None, None, None, None, n) == INVALID_ARGUMENT
    assert _per_call(rs, n, 64, ones, None)[0] == INVALID_ARGUMENT
    rc, (ptrs, ln, pr, rq, _) = _per_call(rs, n, 64, erased, ones)
    assert H.lib.hec_rs_reconstruct_some(rs.handle, ptrs, ln, pr, rq, n - 1) == C["HEC_ERR_TOO_FEW_SHARDS"]
    assert H.lib.hec_rs_reconstruct_some(rs.handle, ptrs, ln, pr, rq, n + 1) == C["HEC_ERR_TOO_MANY_SHARDS"]
    assert _per_call(rs, n, 64, erased, ones, lens=[64, 0] + [64] * (n - 2))[0] == C["HEC_ERR_EMPTY_SHARD"]
    assert _per_call(rs, n, 64, erased, ones, lens=[64, 64, 65] + [64] * (n - 3))[0] == C["HEC_ERR_INCORRECT_SHARD_SIZE"]
    few = [0] * (m + 1) + [1] * (k - 1)
    assert _per_call(rs, n, 64, few, ones)[0] == C["HEC_ERR_TOO_FEW_SHARDS_PRESENT"]
    assert _per_call(rs, n, 64, few, [0] * n)[0] == C["HEC_ERR_TOO_FEW_SHARDS_PRESENT"]  # whatever is required
    # all present: a no-op whatever the flags say, without a device
    assert _per_call(rs, n, 64, ones, ones)[0] == 0
    # an absent required slot that is NULL is refused before device work
    assert _per_call(rs, n, 64, erased, ones, null=(0,))[0] == INVALID_ARGUMENT
    assert "without a buffer" in H._lib.last_detail()
    two = [0, 0] + [1] * (n - 2)
    assert _per_call(rs, n, 64, two, [0, 1] + [0] * (n - 2), null=(1,))[0] == INVALID_ARGUMENT


def test_batch_validation_names_the_stripe():
    import helyim_amd as H
    rs, n = H.ReedSolomon(10, 4), 14
    bufs = [np.zeros(32, dtype=np.uint8) for _ in range(2 * n)]
    ptrs = (ctypes.c_void_p * (2 * n))(*[b.ctypes.data for b in bufs])
    lens = (ctypes.c_size_t * (2 * n))(*[32] * (2 * n))
    present = (ctypes.c_uint8 * (2 * n))(*([1] * n + [0] * 6 + [1] * 8))
    required = (ctypes.c_uint8 * (2 * n))(*[1] * (2 * n))
    bad = ctypes.c_size_t(99)
    call = H.lib.hec_rs_reconstruct_some_batch
    assert call(rs.handle, ptrs, lens, present, required, 2, ctypes.byref(bad)) == C["HEC_ERR_TOO_FEW_SHARDS_PRESENT"]
    assert bad.value == 1
    assert call(rs.handle, ptrs, lens, present, None, 2, ctypes.byref(bad)) == INVALID_ARGUMENT
    assert call(rs.handle, ptrs, lens, present, None, 0, ctypes.byref(bad)) == 0
    assert call(None, ptrs, lens, present, required, 2, None) == INVALID_ARGUMENT


def test_kernel_names():
    import helyim_amd as H
    name = H.lib.hec_reconstruct_some_kernel_name
    assert name(2048).decode().startswith("rs104_narrow_some_kernel")
    assert name(1040).decode().startswith("rs104_some_kernel") and name(1000).decode().startswith("rs104_some_kernel")
    assert name(0).decode().startswith("none")
    batch = H.lib.hec_reconstruct_some_batch_kernel_name
    assert batch(P, 14 * 2048, 2048, 2048, 8).decode() == name(2048).decode()
    for base, st, sh in ((P + 3, 14 * 320, 320), (P, 14 * 304 + 5, 304), (P, 14 * 304, 304 + 3)):
        assert batch(base, st, sh, 301, 8).decode().startswith("rs_some_kernel"), (base, st, sh)


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_no_device_is_an_error_not_a_fallback():
    import helyim_amd as H
    from helyim_amd import batch
    rs = H.ReedSolomon(10, 4)
    for call in STRIDED:
        assert call(H.lib, rs.handle) == NO_DEVICE, call.__name__
    descs = np.zeros(1, dtype=batch.desc_dtype())
    descs["shard_stride"], descs["shard_len"], descs["present_mask"] = L, L, 0x3FFE
    wants = np.ones(1, dtype=np.uint32)
    assert H.lib.hec_gpu_reconstruct_some_ragged(rs.handle, P, descs.ctypes.data, wants.ctypes.data, 1, None,
                                                 None) == NO_DEVICE
    for k, m in ((10, 4), (5, 3)):
        rs2, n = H.ReedSolomon(k, m), k + m
        assert _per_call(rs2, n, 64, [0] + [1] * (n - 1), [1] * n)[0] == NO_DEVICE
