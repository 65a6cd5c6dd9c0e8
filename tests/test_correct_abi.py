"""The correct entry points without a GPU: the symbols, and every argument,
codec and file check that precedes device work (fake non-null pointers are
never touched). hec_gpu_correct_batch, hec_gpu_correct_pairs_batch,
hec_correct_ec_files and hec_correct_pairs_ec_files."""
import ctypes
import os
import re
import stat

import pytest

from abi_util import (EC_SHARD_SIZE, EMPTY_SHARD, INVALID_ARGUMENT, IO, NO_DEVICE, SHARD_NOT_FOUND, L, P, c_parameters, call,
                      has_gpu, volume)
from conftest import ROOT

BATCH = ("hec_gpu_correct_batch", "hec_gpu_correct_pairs_batch")
FILES = ("hec_correct_ec_files", "hec_correct_pairs_ec_files")


def gpu_correct(lib, name, rs, **args):
    return call(name, rs, **args)


def test_symbols_and_signatures():
    import helyim_amd as H
    from helyim_amd import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hec.h")).read(), flags=re.S)
    for name in BATCH + FILES:
        assert hasattr(H.lib, name), name
        assert name in _lib.SIGNATURES, name
    # the locate's list with writable shards and the two counters before the stream
    locate = c_parameters(header, "hec_gpu_locate_corrupt_batch")
    for name in BATCH:
        got = c_parameters(header, name)
        assert got[:-3] == [a.replace("const uint8_t*", "uint8_t*") for a in locate[:-1]], name
        assert got[-3:] == ["uint32_t* d_uncorrected", "unsigned long long* d_corrected_bytes", "void* stream"], name
        assert len(_lib.SIGNATURES[name][1]) == 15
    for name in FILES:
        assert c_parameters(header, name) == c_parameters(header, "hec_locate_corrupt_ec_files"), name
        assert _lib.SIGNATURES[name] == _lib.SIGNATURES["hec_locate_corrupt_ec_files"], name
    for name in ("correct_batch", "correct_batch_sep", "correct_ec_files"):
        assert callable(getattr(H, name)), name
    rust = open(os.path.join(ROOT, "rust", "hec-sys", "src", "lib.rs")).read()
    for name in BATCH + FILES:
        assert "pub fn %s(" % name in rust, name
    wrapper = open(os.path.join(ROOT, "rust", "helyim-ec-hip", "src", "lib.rs")).read()
    assert "pub fn correct_ec_files(" in wrapper
    for name in FILES:
        assert "sys::%s(" % name in wrapper, name


@pytest.mark.parametrize("name", BATCH)
def test_batch_arguments_checked_before_device(name):
    import helyim_amd as H
    lib, rs = H.lib, H.ReedSolomon(10, 4)
    assert gpu_correct(lib, name, None) == INVALID_ARGUMENT
    assert gpu_correct(lib, name, rs.handle, data=None) == INVALID_ARGUMENT
    assert gpu_correct(lib, name, rs.handle, par=None) == INVALID_ARGUMENT
    assert gpu_correct(lib, name, rs.handle, res=None) == INVALID_ARGUMENT
    assert gpu_correct(lib, name, rs.handle, sus=None) == INVALID_ARGUMENT
    assert gpu_correct(lib, name, rs.handle, length=0) == EMPTY_SHARD
    assert gpu_correct(lib, name, rs.handle, dsh=L - 16) == INVALID_ARGUMENT      # data shards overlap
    assert gpu_correct(lib, name, rs.handle, psh=L - 1) == INVALID_ARGUMENT       # parity shards overlap
    assert gpu_correct(lib, name, rs.handle, ds=L - 1, dsh=10 * L) == INVALID_ARGUMENT  # data stripes overlap
    assert gpu_correct(lib, name, rs.handle, ps=L - 1, psh=4 * L) == INVALID_ARGUMENT   # parity stripes overlap
    assert gpu_correct(lib, name, rs.handle, ds=1 << 62, n=8) == INVALID_ARGUMENT  # extent wraps 64 bits
    assert "overflows" in H._lib.last_detail()
    assert gpu_correct(lib, name, rs.handle, n=0) == 0  # nothing to do, nothing touched


@pytest.mark.parametrize("k,m", [(5, 5), (10, 2), (10, 6)])
def test_other_codecs_are_refused_with_the_reason(k, m):
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    n = k + m
    for name in BATCH:
        assert gpu_correct(H.lib, name, rs.handle, ds=n * L, par=P + k * L, ps=n * L) == INVALID_ARGUMENT
        assert "RS(10,4) only" in H._lib.last_detail()
        assert gpu_correct(H.lib, name, rs.handle, ds=n * L, par=P + k * L, ps=n * L, n=0) == INVALID_ARGUMENT


@pytest.mark.skipif(has_gpu(), reason="checks the no-GPU error path")
def test_no_device_is_an_error_not_a_fallback():
    """Without a GPU a well-formed call ends in HEC_ERR_NO_DEVICE (the
    geometry's upload is the first device work), also for the files."""
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    for name in BATCH:
        assert gpu_correct(H.lib, name, rs.handle) == NO_DEVICE, name


@pytest.mark.parametrize("pairs", [False, True])
def test_file_checks_need_no_device(tmp_path, pairs):
    import helyim_amd as H
    lib = H.lib
    call = lib.hec_correct_pairs_ec_files if pairs else lib.hec_correct_ec_files
    n_bad, n_blocks = ctypes.c_size_t(5), ctypes.c_uint64(5)

    def correct(base, block):
        return call(str(base).encode(), block, None, 0, ctypes.byref(n_bad), ctypes.byref(n_blocks))

    assert correct(tmp_path / "missing", 4096) == SHARD_NOT_FOUND
    assert ".ec00" in H._lib.last_detail()
    with pytest.raises(H.ShardNotFound):
        H.correct_ec_files(str(tmp_path / "missing"), pairs=pairs)
    base = tmp_path / "v"
    volume(base, odd=(6, 650))
    for block in (1000, 4095, 4096 + 512):
        assert correct(base, block) == INVALID_ARGUMENT, block
    assert correct(base, 4096) == EC_SHARD_SIZE
    assert H._lib.last_values()[:2] == (700, 650)
    assert (n_bad.value, n_blocks.value) == (0, 0)
    with pytest.raises(H.UnexpectedEcShardSize):
        H.correct_ec_files(str(base), 4096, pairs=pairs)
    assert call(None, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert call(str(base).encode(), 0, None, 3, None, None) == INVALID_ARGUMENT
    with pytest.raises(ValueError):
        H.correct_ec_files(str(base), 4096, cap=-1, pairs=pairs)
    empty = tmp_path / "e"
    volume(empty, size=0)
    assert H.correct_ec_files(str(empty), 4096, pairs=pairs) == (0, 0, [])
    os.remove(str(empty) + ".ec03")  # the degraded form is out of scope: a missing file is an error
    with pytest.raises(H.ShardNotFound):
        H.correct_ec_files(str(empty), 4096, pairs=pairs)


@pytest.mark.parametrize("pairs", [False, True])
def test_a_shard_that_cannot_be_opened_for_writing_is_an_io_error(tmp_path, pairs):
    """A directory in a shard file's place cannot be opened for writing by
    anybody (EISDIR); a read-only file cannot by an ordinary user (EACCES).
    Both give HEC_ERR_IO with the errno before any device work, and nothing
    is changed."""
    import errno
    import helyim_amd as H
    io = IO
    call = H.lib.hec_correct_pairs_ec_files if pairs else H.lib.hec_correct_ec_files
    base = tmp_path / "d"
    volume(base)
    os.remove(str(base) + ".ec05")
    os.mkdir(str(base) + ".ec05")
    assert call(str(base).encode(), 4096, None, 0, None, None) == io
    assert H._lib.last_values()[2] == errno.EISDIR and ".ec05" in H._lib.last_detail()
    base = tmp_path / "r"
    volume(base)
    os.chmod(str(base) + ".ec09", stat.S_IRUSR)
    if os.access(str(base) + ".ec09", os.W_OK):
        return  # a user whom file modes do not bind (root)
    assert call(str(base).encode(), 4096, None, 0, None, None) == io
    assert H._lib.last_values()[2] == errno.EACCES and ".ec09" in H._lib.last_detail()
    assert open(str(base) + ".ec09", "rb").read() == b"\0" * 700
