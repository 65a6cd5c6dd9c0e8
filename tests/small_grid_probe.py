"""Proof that the library a process loaded is the Makefile's smallgrid variant
(build/variants/libhec_smallgrid.so: kMaxLaunchBlocks = 100, kLocateMaxBlocks
= 4) -- TEST INFRASTRUCTURE ONLY.

A pytest plugin (`-p small_grid_probe`, tests/test_gpu_small_grid.py): probe()
runs at session start, before anything is collected, and a child whose limits
are not live ends there with return code 3. Run as a script it prints the
names it saw. The name functions need no device."""
import ctypes
import os

MAX_LAUNCH_BLOCKS, LOCATE_MAX_BLOCKS = 100, 4
QUERY = "hec_test_launch_limits"  # exported by builds with HEC_MAX_LAUNCH_BLOCKS only

# (name function, shard length, prefix of the name): the longest shard a
# one-chunk-per-workgroup kernel takes at 100 workgroups, and the next one
NAMES = [
    ("hec_encode_kernel_name", 100 * 4096, "rs104_bs_encode_kernel"),        # 50 chunks of 8 KiB
    ("hec_encode_kernel_name", 99 * 4096 + 16, "rs104_kernel<DEC=false>"),   # 100 chunks of 4 KiB
    ("hec_encode_kernel_name", 100 * 4096 + 16, "rs_apply_kernel<10>"),      # 101: the grid-stride kernel
    ("hec_encode_kernel_name", 102 * 4096, "rs_apply_kernel<10>"),           # 8 KiB multiple, 102 chunks of 4 KiB
    ("hec_decode_kernel_name", 100 * 2048, "rs104_narrow_kernel<DEC=true"),  # 100 chunks of 2 KiB
    ("hec_decode_kernel_name", 101 * 2048, "rs104_kernel<DEC=true>"),        # 101: 16 bytes per lane, 51 chunks
    ("hec_decode_kernel_name", 100 * 4096 + 16, "rs_apply_kernel<10>"),
    ("hec_verify_kernel_name", 100 * 8192, "rs104_bs_verify_kernel"),
    ("hec_verify_kernel_name", 101 * 8192, "rs_verify_kernel<10>"),
    ("hec_check_kernel_name", 100 * 2048, "rs104_check_kernel"),
    ("hec_check_kernel_name", 101 * 2048, "rs104_check_stride_kernel"),
]


def limits(lib):
    """(kMaxLaunchBlocks, kLocateMaxBlocks) of a variant build; None for the product."""
    try:
        fn = getattr(lib, QUERY)
    except AttributeError:
        return None
    fn.restype, fn.argtypes = None, [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint32)]
    a, b = ctypes.c_uint64(), ctypes.c_uint32()
    fn(ctypes.byref(a), ctypes.byref(b))
    return a.value, b.value


def probe():
    from helyim_amd import _lib
    want = os.environ.get("HEC_LIB_PATH")
    assert want and os.path.samefile(_lib.LIB_PATH, want), (_lib.LIB_PATH, want)
    got = limits(_lib.lib)
    assert got == (MAX_LAUNCH_BLOCKS, LOCATE_MAX_BLOCKS), f"limits of {_lib.LIB_PATH}: {got}"
    seen = []
    for fn, length, prefix in NAMES:
        name = getattr(_lib.lib, fn)(length).decode()
        assert name.startswith(prefix), (fn, length, name, prefix)
        seen.append((fn, length, name))
    return seen


def pytest_sessionstart(session):
    import pytest
    try:
        probe()
    except Exception as e:  # the child must not run one test against another library
        pytest.exit(f"small-grid probe failed: {e!r}", returncode=3)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    for row in probe():
        print(*row)
    print("small-grid probe ok")
