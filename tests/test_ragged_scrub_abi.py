"""The ragged scrub entry points without a GPU: the symbols, the kernel pick,
and every argument and descriptor check that precedes device work (fake
non-null pointers are never touched)."""
import os

import pytest

from abi_util import EMPTY_SHARD, FULL, INVALID_ARGUMENT, P, call_ragged, descs_of, two  # noqa: F401
from conftest import ROOT

NAMES = ("hec_gpu_verify_ragged", "hec_gpu_locate_corrupt_ragged", "hec_ragged_scrub_kernel_name")


def verify(lib, rs, **args):
    return call_ragged("hec_gpu_verify_ragged", rs, **args)


def locate(lib, rs, **args):
    return call_ragged("hec_gpu_locate_corrupt_ragged", rs, **args)


CALLS = {verify: ("base", "res"), locate: ("base", "res", "sus")}


def test_symbols_signatures_and_python_names():
    import helyim_amd as H
    from helyim_amd import _lib
    header = open(os.path.join(ROOT, "include", "hec.h")).read()
    for name in NAMES:
        assert hasattr(H.lib, name), name
        assert name in _lib.SIGNATURES, name
        assert name + "(" in header, name
    assert len(_lib.SIGNATURES["hec_gpu_verify_ragged"][1]) == 8
    assert len(_lib.SIGNATURES["hec_gpu_locate_corrupt_ragged"][1]) == 9
    assert len(_lib.SIGNATURES["hec_ragged_scrub_kernel_name"][1]) == 2
    for name in ("verify_ragged", "locate_corrupt_ragged", "ragged_scrub_kernel_name"):
        assert callable(getattr(H, name)), name


@pytest.mark.parametrize("call", list(CALLS), ids=lambda f: f.__name__)
def test_arguments_checked_before_device(call):
    import helyim_amd as H
    lib, rs = H.lib, H.ReedSolomon(10, 4)
    assert call(lib, rs.handle, n=0) == 0
    assert call(lib, rs.handle, descs=None, n=0) == 0
    assert call(lib, None) == INVALID_ARGUMENT
    assert "null" in H._lib.last_detail()
    for pointer in CALLS[call]:
        assert call(lib, rs.handle, **{pointer: None}) == INVALID_ARGUMENT, pointer
        assert "null" in H._lib.last_detail()
        assert call(lib, rs.handle, n=0, **{pointer: None}) == INVALID_ARGUMENT, pointer
    assert call(lib, rs.handle, descs=None, n=2) == INVALID_ARGUMENT
    assert "null" in H._lib.last_detail()
    # alignment and overlap, as hec_gpu_encode_ragged
    assert call(lib, rs.handle, base=P + 8) == INVALID_ARGUMENT
    assert call(lib, rs.handle, descs=two(offset=14 * 4096 + 8)) == INVALID_ARGUMENT
    assert "stripe 1" in H._lib.last_detail()
    assert call(lib, rs.handle, descs=two(shard_stride=1000)) == INVALID_ARGUMENT     # 1000 % 16 != 0
    assert "stripe 1" in H._lib.last_detail()
    assert call(lib, rs.handle, descs=two(shard_stride=992)) == INVALID_ARGUMENT      # stride < len
    assert call(lib, rs.handle, descs=two(shard_len=0)) == EMPTY_SHARD
    assert "stripe 1" in H._lib.last_detail()
    # a stripe that will not be read (nine shards present) is still checked
    assert call(lib, rs.handle, descs=two(shard_len=0, present_mask=0x1FF)) == EMPTY_SHARD
    assert call(lib, rs.handle, n=0) == 0


@pytest.mark.parametrize("k,m", [(5, 5), (10, 2), (10, 6)])
def test_other_codecs_are_refused_with_the_reason(k, m):
    import helyim_amd as H
    rs = H.ReedSolomon(k, m)
    for call in CALLS:
        assert call(H.lib, rs.handle) == INVALID_ARGUMENT
        assert "RS(10,4) only" in H._lib.last_detail()


def test_above_2_32_map_entries_is_refused():
    import helyim_amd as H
    rs = H.ReedSolomon(10, 4)
    big = (1 << 32) - 16  # 2^20 entries of 4 KiB each; 4097 such stripes pass 2^32
    d = descs_of([(0, 1 << 32, big, FULL & ~1)] * 4097)
    for call in CALLS:
        assert call(H.lib, rs.handle, descs=d) == INVALID_ARGUMENT
        assert "2^32" in H._lib.last_detail()


def test_kernel_name_reports_the_pick():
    import helyim_amd as H
    name = H.ragged_scrub_kernel_name
    row = lambda L, mask=FULL: (0, 32768, L, mask)  # noqa: E731
    bs = name([row(8192), row(24576)])
    table = name([row(8192), row(1000)])
    assert bs != table and "bit-sliced" in bs and "rs104_bs_ragged_verify_kernel" in bs
    assert "rs104_ragged_check_kernel" in table
    assert name([row(8192), row(8192, FULL & ~(1 << 12))]) == table
    assert name([row(8192), row(8192, 0x1FF)]) == table          # a stripe that is not read decides too
    assert name([row(8192, FULL | 0xFFFF0000)]) == bs            # bits past 13 are ignored
    assert name([row(4096)]) == table
    assert name([]) in (bs, table)                                # a name, not a crash
    assert H.lib.hec_ragged_scrub_kernel_name(None, 3) == b"invalid argument"
