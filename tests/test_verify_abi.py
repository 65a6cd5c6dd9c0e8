"""The verify (scrub) entry points without a GPU: every argument and file
check that precedes device work (fake non-null pointers are never touched)."""
import ctypes

import pytest

from abi_util import EC_SHARD_SIZE, EMPTY_SHARD, INVALID_ARGUMENT, L, P, SHARD_NOT_FOUND, call, volume  # noqa: F401


def gpu_verify(lib, rs, **args):
    return call("hec_gpu_verify_batch", rs, **args)


def host_verify(lib, rs, **args):
    return call("hec_host_verify_batch", rs, **args)


@pytest.mark.parametrize("call", [gpu_verify, host_verify])
def test_batch_arguments_checked_before_device(call):
    import helyim_amd as H
    lib, rs = H.lib, H.ReedSolomon(10, 4)
    assert call(lib, None) == INVALID_ARGUMENT
    assert call(lib, rs.handle, data=None) == INVALID_ARGUMENT
    assert call(lib, rs.handle, par=None) == INVALID_ARGUMENT
    assert call(lib, rs.handle, res=None) == INVALID_ARGUMENT
    assert call(lib, rs.handle, length=0) == EMPTY_SHARD
    assert call(lib, rs.handle, dsh=L - 16) == INVALID_ARGUMENT      # data shards overlap
    assert call(lib, rs.handle, psh=L - 1) == INVALID_ARGUMENT       # parity shards overlap
    assert call(lib, rs.handle, ds=L - 1, dsh=10 * L) == INVALID_ARGUMENT  # data stripes overlap
    assert call(lib, rs.handle, ds=1 << 62, n=8) == INVALID_ARGUMENT  # extent wraps 64 bits
    assert "overflows" in H._lib.last_detail()


@pytest.mark.parametrize("call", [gpu_verify, host_verify])
def test_more_than_32_parity_shards_refused(call):
    import helyim_amd as H
    rs = H.ReedSolomon(4, 33)
    assert call(H.lib, rs.handle, ds=37 * L, par=P + 4 * L, ps=37 * L) == INVALID_ARGUMENT
    assert "32 parity" in H._lib.last_detail()


def test_empty_device_batch_is_ok_without_a_device():
    import helyim_amd as H
    assert gpu_verify(H.lib, H.ReedSolomon(10, 4).handle, n=0) == 0


def test_file_scrub_checks_need_no_device(tmp_path):
    import helyim_amd as H
    lib = H.lib
    n_bad, n_blocks = ctypes.c_size_t(5), ctypes.c_uint64(5)

    def scrub(base, block):
        return lib.hec_verify_ec_files(str(base).encode(), block, None, 0, ctypes.byref(n_bad), ctypes.byref(n_blocks))

    assert scrub(tmp_path / "missing", 4096) == SHARD_NOT_FOUND
    assert ".ec00" in H._lib.last_detail()
    with pytest.raises(H.ShardNotFound):
        H.verify_ec_files(str(tmp_path / "missing"))
    base = tmp_path / "v"
    volume(base, odd=(6, 650))
    for block in (1000, 4095, 4096 + 512):
        assert scrub(base, block) == INVALID_ARGUMENT, block
    assert scrub(base, 4096) == EC_SHARD_SIZE
    assert H._lib.last_values()[:2] == (700, 650)
    assert (n_bad.value, n_blocks.value) == (0, 0)
    assert lib.hec_verify_ec_files(None, 0, None, 0, None, None) == INVALID_ARGUMENT
    assert lib.hec_verify_ec_files(str(base).encode(), 0, None, 3, None, None) == INVALID_ARGUMENT  # cap without bad


def test_names_and_version():
    import helyim_amd as H
    assert H.lib.hec_verify_kernel_name(0).decode().startswith("none")
    assert H.lib.hec_verify_kernel_name(1 << 20).decode() == "rs104_bs_verify_kernel (bit-sliced)"
    assert H.lib.hec_verify_kernel_name(1000).decode().startswith("rs_verify_kernel")
    assert "0.2.0" in H.version() and "gfx950" in H.version()
