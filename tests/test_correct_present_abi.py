"""The masked correct entry points without a GPU: the symbols, and every
argument, codec and file check that precedes device work (fake non-null
pointers are never touched). hec_gpu_correct_present_batch,
hec_gpu_reconstruct_corrected_batch and hec_correct_ec_files_present."""
import ctypes
import errno
import os
import re
import stat

import pytest

from abi_util import (EC_SHARD_SIZE, EMPTY_SHARD, INVALID_ARGUMENT, IO, NO_DEVICE, SHARD_NOT_FOUND, TOO_FEW_PRESENT, L,
                      c_parameters, call, has_gpu, volume)
from conftest import ROOT

BATCH = ("hec_gpu_correct_present_batch", "hec_gpu_reconstruct_corrected_batch")
FILES = "hec_correct_ec_files_present"


def gpu_correct(lib, rs, **args):
    return call("hec_gpu_correct_present_batch", rs, **args)


def gpu_corrected(lib, rs, **args):
    return call("hec_gpu_reconstruct_corrected_batch", rs, **args)


CALLS = {gpu_correct: ("shards", "masks", "res", "sus"), gpu_corrected: ("shards", "masks", "res", "sus", "use")}


def test_symbols_and_signatures():
    import helyim_amd as H
    from helyim_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hec.h")).read(), flags=re.S)
    for name in BATCH + (FILES,):
        assert hasattr(H.lib, name), name
        assert name in _lib.SIGNATURES, name
    # the masked locate's list with writable shards, min_spares after the masks, the two counters before the stream
    locate = c_parameters(header, "hec_gpu_locate_corrupt_present_batch")
    got = c_parameters(header, BATCH[0])
    assert got == ([locate[1].replace("const uint8_t*", "uint8_t*") if i == 1 else a for i, a in enumerate(locate[:7])]
                   + ["uint32_t min_spares"] + locate[7:-1]
                   + ["uint32_t* d_uncorrected", "unsigned long long* d_corrected_bytes", "void* stream"])
    checked = c_parameters(header, "hec_gpu_reconstruct_checked_batch")
    assert c_parameters(header, BATCH[1]) == (checked[:7] + ["uint32_t min_spares"] + checked[7:-1]
                                              + ["unsigned long long* d_corrected_bytes", "void* stream"])
    files = c_parameters(header, "hec_locate_corrupt_ec_files_present")
    assert c_parameters(header, FILES) == files[:2] + ["uint32_t min_spares"] + files[2:]
    assert len(_lib.SIGNATURES[BATCH[0]][1]) == 15 and len(_lib.SIGNATURES[BATCH[1]][1]) == 15
    present = _lib.SIGNATURES["hec_locate_corrupt_ec_files_present"]
    assert _lib.SIGNATURES[FILES] == (present[0], present[1][:2] + [ctypes.c_uint32] + present[1][2:])
    for name in ("correct_present_batch", "reconstruct_corrected_batch", "correct_ec_files_present"):
        assert callable(getattr(H, name)), name
    rust = open(os.path.join(ROOT, "rust", "hec-sys", "src", "lib.rs")).read()
    for name in BATCH + (FILES,):
        assert "pub fn %s(" % name in rust, name
    wrapper = open(os.path.join(ROOT, "rust", "helyim-ec-hip", "src", "lib.rs")).read()
    assert "pub fn correct_ec_files_present(" in wrapper and "sys::%s(" % FILES in wrapper


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
    for spares in (0, 1, 5, 1 << 31):
        assert call(lib, rs.handle, spares=spares) == INVALID_ARGUMENT, spares
        assert "min_spares" in H._lib.last_detail()
        assert call(lib, rs.handle, spares=spares, n=0) == INVALID_ARGUMENT, spares
    for spares in (2, 3, 4):
        assert call(lib, rs.handle, spares=spares, n=0) == 0
    assert call(lib, rs.handle, length=0) == EMPTY_SHARD
    assert call(lib, rs.handle, sh=L - 1) == INVALID_ARGUMENT              # shards overlap
    assert call(lib, rs.handle, sh=L - 16) == INVALID_ARGUMENT
    assert call(lib, rs.handle, st=L - 1, sh=2 * L) == INVALID_ARGUMENT    # stripes overlap
    assert call(lib, rs.handle, st=1 << 62, n=8) == INVALID_ARGUMENT       # extent wraps 64 bits
    assert "overflows" in H._lib.last_detail()


@pytest.mark.parametrize("k,m", [(5, 5), (10, 2), (10, 6)])
def test_other_codecs_are_refused_with_the_reason(k, m):
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    for call in CALLS:
        assert call(H.lib, rs.handle, st=(k + m) * L) == INVALID_ARGUMENT
        assert "RS(10,4) only" in H._lib.last_detail()
        assert call(H.lib, rs.handle, st=(k + m) * L, n=0) == INVALID_ARGUMENT


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_no_device_is_an_error_not_a_fallback():
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for call in CALLS:
        assert call(H.lib, rs.handle) == NO_DEVICE, call.__name__


def test_file_checks_need_no_device(tmp_path):
    import helyim_amd as H
    lib = H.lib
    n_bad, n_blocks, present = ctypes.c_size_t(5), ctypes.c_uint64(5), ctypes.c_uint32(5)

    def correct(base, block=4096, spares=2):
        return lib.hec_correct_ec_files_present(str(base).encode(), block, spares, None, 0, ctypes.byref(n_bad),
                                                ctypes.byref(n_blocks), ctypes.byref(present))

    assert correct(tmp_path / "missing") == SHARD_NOT_FOUND
    assert (n_bad.value, n_blocks.value, present.value) == (0, 0, 0)
    with pytest.raises(H.ShardNotFound):
        H.correct_ec_files_present(str(tmp_path / "missing"))
    for count, ids in ((1, (6,)), (7, (0, 2, 3, 5, 8, 11, 13)), (10, range(2, 12))):
        base = tmp_path / ("few%d" % count)
        volume(base, present=ids)
        assert correct(base) == TOO_FEW_PRESENT, count
        assert ("%d of 14" % count) in H._lib.last_detail()
        assert present.value == sum(1 << i for i in ids)
        with pytest.raises(H.ErasureCoding) as e:
            H.correct_ec_files_present(str(base), 4096)
        assert isinstance(e.value.inner, H.TooFewShardsPresent)
    base = tmp_path / "v"
    volume(base, present=[i for i in range(14) if i not in (0, 9)], sizes={6: 650})
    for block in (1000, 4095, 4096 + 512):
        assert correct(base, block) == INVALID_ARGUMENT, block
    for spares in (0, 1, 5):
        assert correct(base, 4096, spares) == INVALID_ARGUMENT, spares
        assert "min_spares" in H._lib.last_detail()
    assert correct(base) == EC_SHARD_SIZE
    assert H._lib.last_values()[:2] == (700, 650)
    assert (n_bad.value, n_blocks.value, present.value) == (0, 0, 0x3FFF & ~(1 | 1 << 9))
    with pytest.raises(H.UnexpectedEcShardSize):
        H.correct_ec_files_present(str(base), 4096)
    enc = str(base).encode()
    assert lib.hec_correct_ec_files_present(None, 0, 2, None, 0, None, None, None) == INVALID_ARGUMENT
    assert lib.hec_correct_ec_files_present(enc, 0, 2, None, 3, None, None, None) == INVALID_ARGUMENT  # cap, no bad
    with pytest.raises(ValueError):
        H.correct_ec_files_present(str(base), 4096, cap=-1)
    for name, ids in (("e14", range(14)), ("e11", (0, 1, 2, 4, 5, 6, 7, 9, 10, 12, 13))):
        empty = tmp_path / name
        volume(empty, size=0, present=ids)
        assert H.correct_ec_files_present(str(empty), 4096) == (0, 0, [], sum(1 << i for i in ids))


def test_a_present_file_that_cannot_be_opened_for_writing_is_an_io_error(tmp_path):
    """A directory in a shard file's place cannot be opened for writing by
    anybody (EISDIR); a read-only file cannot by an ordinary user (EACCES).
    Both give HEC_ERR_IO with the errno before any device work; a missing file
    (ENOENT) is an erased shard."""
    import helyim_amd as H
    io = IO
    call = H.lib.hec_correct_ec_files_present
    base = tmp_path / "d"
    volume(base, present=[i for i in range(14) if i != 2])
    os.remove(str(base) + ".ec05")
    os.mkdir(str(base) + ".ec05")
    assert call(str(base).encode(), 4096, 2, None, 0, None, None, None) == io
    assert H._lib.last_values()[2] == errno.EISDIR and ".ec05" in H._lib.last_detail()
    with pytest.raises(H.Io):
        H.correct_ec_files_present(str(base), 4096)
    base = tmp_path / "r"
    volume(base, present=[i for i in range(14) if i != 2])
    os.chmod(str(base) + ".ec09", stat.S_IRUSR)
    if os.access(str(base) + ".ec09", os.W_OK):
        return  # a user whom file modes do not bind (root)
    assert call(str(base).encode(), 4096, 2, None, 0, None, None, None) == io
    assert H._lib.last_values()[2] == errno.EACCES and ".ec09" in H._lib.last_detail()
    assert open(str(base) + ".ec09", "rb").read() == b"\0" * 700
