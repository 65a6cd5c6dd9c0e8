"""The locate and repair entry points without a GPU: the symbols, and every
argument and file check that precedes device work (fake non-null pointers are
never touched)."""
import ctypes
import os

import pytest

from abi_util import (EC_SHARD_SIZE, EMPTY_SHARD, INVALID_ARGUMENT, L, P, SHARD_NOT_FOUND, c_parameters, call,  # noqa: F401
                      volume)
from conftest import ROOT

NAMES = ("hec_gpu_locate_corrupt_batch", "hec_gpu_repair_batch", "hec_locate_corrupt_ec_files")


def gpu_locate(lib, rs, **args):
    return call("hec_gpu_locate_corrupt_batch", rs, **args)


def gpu_repair(lib, rs, **args):
    return call("hec_gpu_repair_batch", rs, **args)


def test_symbols_and_signatures():
    import helyim_amd as H
    from helyim_amd import _lib
    for name in NAMES:
        assert hasattr(H.lib, name), name
        assert name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "hec.h")).read()
    assert "#define HEC_SUSPECT_UNEXPLAINED 0x80000000u" in header
    assert H.SUSPECT_UNEXPLAINED == 0x80000000
    for name in ("locate_corrupt_ec_files", "locate_corrupt_batch", "locate_corrupt_batch_sep", "repair_batch"):
        assert callable(getattr(H, name)), name


def test_locate_arguments_checked_before_device():
    import helyim_amd as H
    lib, rs = H.lib, H.ReedSolomon(10, 4)
    assert gpu_locate(lib, None) == INVALID_ARGUMENT
    assert gpu_locate(lib, rs.handle, data=None) == INVALID_ARGUMENT
    assert gpu_locate(lib, rs.handle, par=None) == INVALID_ARGUMENT
    assert gpu_locate(lib, rs.handle, res=None) == INVALID_ARGUMENT
    assert gpu_locate(lib, rs.handle, sus=None) == INVALID_ARGUMENT
    assert gpu_locate(lib, rs.handle, length=0) == EMPTY_SHARD
    assert gpu_locate(lib, rs.handle, dsh=L - 16) == INVALID_ARGUMENT      # data shards overlap
    assert gpu_locate(lib, rs.handle, psh=L - 1) == INVALID_ARGUMENT       # parity shards overlap
    assert gpu_locate(lib, rs.handle, ds=L - 1, dsh=10 * L) == INVALID_ARGUMENT  # data stripes overlap
    assert gpu_locate(lib, rs.handle, ps=L - 1, psh=4 * L) == INVALID_ARGUMENT   # parity stripes overlap
    assert gpu_locate(lib, rs.handle, ds=1 << 62, n=8) == INVALID_ARGUMENT  # extent wraps 64 bits
    assert "overflows" in H._lib.last_detail()
    assert gpu_locate(lib, rs.handle, n=0) == 0


def test_repair_arguments_checked_before_device():
    import helyim_amd as H
    lib, rs = H.lib, H.ReedSolomon(10, 4)
    assert gpu_repair(lib, None) == INVALID_ARGUMENT
    assert gpu_repair(lib, rs.handle, shards=None) == INVALID_ARGUMENT
    assert gpu_repair(lib, rs.handle, res=None) == INVALID_ARGUMENT
    assert gpu_repair(lib, rs.handle, sus=None) == INVALID_ARGUMENT
    assert gpu_repair(lib, rs.handle, masks=None) == INVALID_ARGUMENT
    assert gpu_repair(lib, rs.handle, length=0) == EMPTY_SHARD
    assert gpu_repair(lib, rs.handle, sh=L - 1) == INVALID_ARGUMENT        # shards overlap
    assert gpu_repair(lib, rs.handle, st=L - 1, sh=2 * L) == INVALID_ARGUMENT  # stripes overlap
    assert gpu_repair(lib, rs.handle, st=1 << 62, n=8) == INVALID_ARGUMENT  # extent wraps 64 bits
    assert "overflows" in H._lib.last_detail()
    assert gpu_repair(lib, rs.handle, n=0) == 0


@pytest.mark.parametrize("k,m", [(5, 5), (10, 2), (10, 6)])
def test_other_codecs_are_refused_with_the_reason(k, m):
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    n = k + m
    assert gpu_locate(H.lib, rs.handle, ds=n * L, par=P + k * L, ps=n * L) == INVALID_ARGUMENT
    assert "RS(10,4) only" in H._lib.last_detail()
    assert gpu_repair(H.lib, rs.handle, st=n * L) == INVALID_ARGUMENT
    assert "RS(10,4) only" in H._lib.last_detail()
    assert gpu_locate(H.lib, rs.handle, ds=n * L, par=P + k * L, ps=n * L, n=0) == INVALID_ARGUMENT


def test_file_locate_checks_need_no_device(tmp_path):
    import helyim_amd as H
    lib = H.lib
    n_bad, n_blocks = ctypes.c_size_t(5), ctypes.c_uint64(5)

    def locate(base, block):
        return lib.hec_locate_corrupt_ec_files(str(base).encode(), block, None, 0, ctypes.byref(n_bad),
                                               ctypes.byref(n_blocks))

    assert locate(tmp_path / "missing", 4096) == SHARD_NOT_FOUND
    assert ".ec00" in H._lib.last_detail()
    with pytest.raises(H.ShardNotFound):
        H.locate_corrupt_ec_files(str(tmp_path / "missing"))
    base = tmp_path / "v"
    volume(base, odd=(6, 650))
    for block in (1000, 4095, 4096 + 512):
        assert locate(base, block) == INVALID_ARGUMENT, block
    assert locate(base, 4096) == EC_SHARD_SIZE
    assert H._lib.last_values()[:2] == (700, 650)
    assert (n_bad.value, n_blocks.value) == (0, 0)
    with pytest.raises(H.UnexpectedEcShardSize):
        H.locate_corrupt_ec_files(str(base), 4096)
    assert lib.hec_locate_corrupt_ec_files(None, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert lib.hec_locate_corrupt_ec_files(str(base).encode(), 0, None, 3, None, None) == INVALID_ARGUMENT  # cap, no bad
    with pytest.raises(ValueError):
        H.locate_corrupt_ec_files(str(base), 4096, cap=-1)
    empty = tmp_path / "e"
    volume(empty, size=0)
    assert H.locate_corrupt_ec_files(str(empty), 4096) == (0, 0, [])


def test_scrub_suspect_struct_layout():
    from helyim_amd import ec
    assert ctypes.sizeof(ec._ScrubSuspect) == 24
    assert [f[0] for f in ec._ScrubSuspect._fields_] == ["offset", "length", "parity_mask", "suspects", "reserved"]
    assert ec._ScrubSuspect.suspects.offset == 16
