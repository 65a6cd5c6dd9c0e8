"""Proof that the library a process loaded is the Makefile's smallchunk variant
(build/variants/libhec_smallchunk.so: 48 KiB host chunks, 12 KiB of columns a
scrub chunk, 5000-byte reads) -- TEST INFRASTRUCTURE ONLY.

A pytest plugin (`-p small_chunk_probe`, tests/test_gpu_small_chunk.py):
probe() runs at session start, before anything is collected, and a child whose
chunk sizes are not live ends there with return code 3. At the end the plugin
names every test the child's --deselect options left out. Run as a script it
prints the sizes it saw. The query needs no device.

chunk_stripes() and per_chunk() restate the two chunk rules of
host_pipeline.cpp and verify_files.cpp for the tests that pin which shapes
cross a chunk edge."""
import ctypes
import os

CHUNK_BYTES, CHUNK_COLS, READ_PIECE = 48 << 10, 12 << 10, 5000
PRODUCT = (96 << 20, 4 << 20, 1 << 20)  # the shipped library's three sizes
QUERY = "hec_test_host_chunk_limits"  # exported by builds with one of the three size macros only


def limits(lib):
    """(kChunkBytes, kChunkCols, kReadPiece) of a variant build; None for the product."""
    try:
        fn = getattr(lib, QUERY)
    except AttributeError:
        return None
    fn.restype, fn.argtypes = None, [ctypes.POINTER(ctypes.c_uint64)] * 3
    a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    fn(ctypes.byref(a), ctypes.byref(b), ctypes.byref(c))
    return a.value, b.value, c.value


def chunk_stripes(L, n, S, chunk_bytes=CHUNK_BYTES):
    """Stripes per chunk of a pageable host batch: host_pipeline.cpp's
    chunk_stripes on the staging pitch round_up(L, 256)."""
    return min(S, max(1, chunk_bytes // (n * (-(-L // 256) * 256))))


def host_chunks(L, n, S, chunk_bytes=CHUNK_BYTES):
    """-> (stripes per chunk, chunks, stripes of the last chunk)"""
    c = chunk_stripes(L, n, S, chunk_bytes)
    return c, -(-S // c), S - (-(-S // c) - 1) * c


def per_chunk(block, chunk_cols=CHUNK_COLS):
    """Blocks per chunk of a file scrub (verify_files.cpp)."""
    return max(1, chunk_cols // block)


def probe():
    from helyim_amd import _lib
    want = os.environ.get("HEC_LIB_PATH")
    assert want and os.path.samefile(_lib.LIB_PATH, want), (_lib.LIB_PATH, want)
    got = limits(_lib.lib)
    assert got == (CHUNK_BYTES, CHUNK_COLS, READ_PIECE), f"chunk sizes of {_lib.LIB_PATH}: {got}"
    return got


def pytest_sessionstart(session):
    import pytest
    try:
        probe()
    except Exception as e:  # the child must not run one test against another library
        pytest.exit(f"small-chunk probe failed: {e!r}", returncode=3)


_left_out = []


def pytest_deselected(items):
    ids = tuple(items[0].config.getoption("deselect") or ()) if items else ()
    _left_out.extend(it.nodeid for it in items if it.nodeid.startswith(ids))


def pytest_terminal_summary(terminalreporter):
    from variant_children import DESELECTED_LINE
    for nodeid in _left_out:
        terminalreporter.write_line(DESELECTED_LINE + nodeid)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    print(*probe())
    print("small-chunk probe ok")
