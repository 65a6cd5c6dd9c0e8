"""The degraded-scrub entry points without a GPU: the symbols, and every
argument and file check that precedes device work (fake non-null pointers are
never touched)."""
import ctypes
import os

import pytest

from abi_util import EC_SHARD_SIZE, EMPTY_SHARD, INVALID_ARGUMENT, L, SHARD_NOT_FOUND, TOO_FEW_PRESENT, call, volume
from conftest import ROOT

NAMES = ("hec_gpu_verify_present_batch", "hec_gpu_locate_corrupt_present_batch",
         "hec_gpu_reconstruct_checked_batch", "hec_check_kernel_name", "hec_locate_corrupt_ec_files_present")


def gpu_check(lib, rs, **args):
    return call("hec_gpu_verify_present_batch", rs, **args)


def gpu_locate(lib, rs, **args):
    return call("hec_gpu_locate_corrupt_present_batch", rs, **args)


def gpu_checked(lib, rs, **args):
    return call("hec_gpu_reconstruct_checked_batch", rs, **args)


CALLS = {gpu_check: ("shards", "masks", "res"), gpu_locate: ("shards", "masks", "res", "sus"),
         gpu_checked: ("shards", "masks", "res", "sus", "use")}


def test_symbols_signatures_and_python_names():
    import helyim_amd as H
    from helyim_amd import _lib
    header = open(os.path.join(ROOT, "include", "hec.h")).read()
    for name in NAMES:
        assert hasattr(H.lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
        assert not name.startswith("hec_set_")
    for name in ("verify_present_batch", "locate_corrupt_present_batch", "reconstruct_checked_batch",
                 "check_kernel_name", "locate_corrupt_ec_files_present"):
        assert callable(getattr(H, name)), name
    assert len(_lib.SIGNATURES["hec_gpu_verify_present_batch"][1]) == 11
    assert len(_lib.SIGNATURES["hec_gpu_locate_corrupt_present_batch"][1]) == 12
    assert len(_lib.SIGNATURES["hec_gpu_reconstruct_checked_batch"][1]) == 13
    assert len(_lib.SIGNATURES["hec_locate_corrupt_ec_files_present"][1]) == 7


def test_check_kernel_name_reports_the_choice():
    import helyim_amd as H
    name = lambda n: H.lib.hec_check_kernel_name(n).decode()  # noqa: E731
    fast, generic = name(2048), name(1000)
    assert fast != generic and "rs104_check_kernel" in fast and "stride" in generic
    assert name(8192 + 2048) == fast and name(1 << 20) == fast
    assert name(4096 + 16) == generic and name(1) == generic
    assert name(1 << 32) == generic          # 4 GiB: past the 32-bit lane offsets
    assert name((1 << 32) - 2048) == fast
    assert name(0).startswith("none")


@pytest.mark.parametrize("call", list(CALLS), ids=lambda f: f.__name__)
def test_arguments_checked_before_device(call):
    import helyim_amd as H
    lib, rs = H.lib, H.ReedSolomon(10, 4)
    assert call(lib, rs.handle, n=0) == 0
    assert call(lib, None) == INVALID_ARGUMENT
    for pointer in CALLS[call]:
        assert call(lib, rs.handle, **{pointer: None}) == INVALID_ARGUMENT, pointer
        assert "null" in H._lib.last_detail()
        assert call(lib, rs.handle, n=0, **{pointer: None}) == INVALID_ARGUMENT, pointer
    assert call(lib, rs.handle, length=0) == EMPTY_SHARD
    assert call(lib, rs.handle, sh=L - 1) == INVALID_ARGUMENT              # shards overlap
    assert call(lib, rs.handle, sh=L - 16) == INVALID_ARGUMENT
    assert call(lib, rs.handle, st=L - 1, sh=2 * L) == INVALID_ARGUMENT    # stripes overlap
    assert call(lib, rs.handle, st=1 << 62, n=8) == INVALID_ARGUMENT       # extent wraps 64 bits
    assert "overflows" in H._lib.last_detail()
    assert call(lib, rs.handle, n=0) == 0


@pytest.mark.parametrize("k,m", [(5, 5), (10, 2), (10, 6)])
def test_other_codecs_are_refused_with_the_reason(k, m):
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    for call in CALLS:
        assert call(H.lib, rs.handle, st=(k + m) * L) == INVALID_ARGUMENT
        assert "RS(10,4) only" in H._lib.last_detail()
        assert call(H.lib, rs.handle, st=(k + m) * L, n=0) == INVALID_ARGUMENT


def test_file_checks_need_no_device(tmp_path):
    import helyim_amd as H
    lib = H.lib
    n_bad, n_blocks, present = ctypes.c_size_t(5), ctypes.c_uint64(5), ctypes.c_uint32(5)

    def locate(base, block=4096):
        return lib.hec_locate_corrupt_ec_files_present(str(base).encode(), block, None, 0, ctypes.byref(n_bad),
                                                       ctypes.byref(n_blocks), ctypes.byref(present))

    # no file at all
    assert locate(tmp_path / "missing") == SHARD_NOT_FOUND
    assert (n_bad.value, n_blocks.value, present.value) == (0, 0, 0)
    with pytest.raises(H.ShardNotFound):
        H.locate_corrupt_ec_files_present(str(tmp_path / "missing"))
    # 7 and 10 present: too few, the detail gives the count
    for count, ids in ((7, (0, 2, 3, 5, 8, 11, 13)), (10, range(2, 12))):
        base = tmp_path / ("few%d" % count)
        volume(base, present=ids)
        assert locate(base) == TOO_FEW_PRESENT, count
        assert ("%d of 14" % count) in H._lib.last_detail()
        assert present.value == sum(1 << i for i in ids)
        with pytest.raises(H.ErasureCoding) as e:  # file-level calls wrap RS errors, as helyim does
            H.locate_corrupt_ec_files_present(str(base), 4096)
        assert isinstance(e.value.inner, H.TooFewShardsPresent)
    # unequal sizes among the present files (the absent ones say nothing)
    base = tmp_path / "v"
    volume(base, present=[i for i in range(14) if i not in (0, 9)], sizes={6: 650})
    for block in (1000, 4095, 4096 + 512):
        assert locate(base, block) == INVALID_ARGUMENT, block
    assert locate(base) == EC_SHARD_SIZE
    assert H._lib.last_values()[:2] == (700, 650)
    assert (n_bad.value, n_blocks.value, present.value) == (0, 0, 0x3FFF & ~(1 | 1 << 9))
    with pytest.raises(H.UnexpectedEcShardSize):
        H.locate_corrupt_ec_files_present(str(base), 4096)
    enc = str(base).encode()
    assert lib.hec_locate_corrupt_ec_files_present(None, 0, None, 0, None, None, None) == INVALID_ARGUMENT
    assert lib.hec_locate_corrupt_ec_files_present(enc, 0, None, 3, None, None, None) == INVALID_ARGUMENT  # cap, no bad
    with pytest.raises(ValueError):
        H.locate_corrupt_ec_files_present(str(base), 4096, cap=-1)
    # all-empty files: nothing to check, with 14 and with 11 present
    for name, ids in (("e14", range(14)), ("e11", (0, 1, 2, 4, 5, 6, 7, 9, 10, 12, 13))):
        empty = tmp_path / name
        volume(empty, size=0, present=ids)
        assert H.locate_corrupt_ec_files_present(str(empty), 4096) == (0, 0, [], sum(1 << i for i in ids))
    # the full-volume entry point still refuses a missing file
    assert lib.hec_locate_corrupt_ec_files(str(tmp_path / "e11").encode(), 4096, None, 0, None, None) == SHARD_NOT_FOUND
