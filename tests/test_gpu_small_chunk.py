"""The host and file suites again, against build/variants/libhec_smallchunk.so:
host_pipeline.cpp and verify_files.cpp rebuilt with 48 KiB host chunks,
12 KiB of columns a scrub chunk and 5000-byte reads (Makefile,
VFLAGS_smallchunk), linked with the product's other objects, kernels included.
The product's sizes (96 MiB, 4 MiB, 1 MiB) keep almost every host batch and
volume of the suite inside chunk 0, slot 0. Every selected test compares the
library with the C oracle, tests/footprint.py, some_model or the scrub models,
never with itself, so under the variant their batches of a few hundred KiB
become chunk-boundary tests: both pinned slots and all three streams and
device slots of run_host_op reused, s0 > 0 in every pack, launch and unpack, short
last chunks, the file scrubs' collect(c - 2) while later chunks are in flight,
and rows read in several pieces with a ragged last one.

The mechanism is tests/test_gpu_small_grid.py's (tests/variant_children.py):
one child `python -m pytest <file> -m gpu -k <selection>` per file with
HEC_LIB_PATH set, tests/small_chunk_probe.py first in the child, a time limit
per child, and no further child after one died of a signal or ran out of
time. tests/test_ec_read.py is no child: it does not reach the two rebuilt
files."""
import ctypes
import os
import subprocess
import sys

import pytest

import small_chunk_probe as probe
import variant_children as C
from variant_children import ROOT, TESTS, tail

VARIANT = C.variant_path("smallchunk")

# file -> (-k selection or None for the whole file, wall seconds of the selection's process with the product
# library on one MI355X, the same under the variant; profiles/small_chunk/mutations.md). The time limit of a child
# is LIMIT_FACTOR times the product's time, at least LIMIT_FLOOR: the small-grid module's margin (300 s for files
# of 5 to 45 s, 420 s for its one-minute file), so 348 s for the verify selection and 300 s for the others.
CHILDREN = {
    "test_gpu_host_batch.py": (None, 22.7, 16.1),
    "test_gpu_footprint.py": ("host", 7.4, 4.7),
    "test_gpu_reconstruct_some.py": ("host", 6.0, 3.9),
    "test_gpu_verify.py": ("host or files", 49.7, 54.6),  # the 84271-stripe host verifies: 6483 chunks a call here
    "test_gpu_locate.py": ("files", 5.6, 4.6),
    "test_gpu_locate_pairs.py": ("files", 5.2, 4.9),
    "test_gpu_check.py": ("files", 6.2, 6.8),
    "test_gpu_correct.py": ("files", 6.5, 6.9),
    "test_gpu_correct_present.py": ("files", 5.7, 5.7),
}
LIMIT_FACTOR, LIMIT_FLOOR = 7, 300

# Deselected under the variant, by node id (without parameters: every case).
# Only two kinds: shapes of tens of GiB ("size"), and expectations that are
# themselves a chunk index or a staging byte count the constants legitimately
# change ("chunk"). The -k selections above already leave the near-4-GiB and
# past-one-launch device shapes out; none of them is a host or a file test.
DESELECT = {
    "test_gpu_host_batch.py": [
        ("test_error_return_leaves_nothing_in_flight", "chunk: expects the failure hook's chunk 2 to begin at stripe "
                                                       "12 (six 14 MiB stripes a chunk); here it is stripe 2"),
    ],
    "test_gpu_footprint.py": [],
    "test_gpu_reconstruct_some.py": [],
    "test_gpu_verify.py": [],
    "test_gpu_locate.py": [],
    "test_gpu_locate_pairs.py": [],
    "test_gpu_check.py": [],
    "test_gpu_correct.py": [],
    "test_gpu_correct_present.py": [],
}


def test_variant_is_built_and_the_product_exports_no_query():
    """build() leaves the variant beside the product; a process that loads it
    reports the three sizes, and the product library exports no such query."""
    assert os.path.exists(VARIANT), VARIANT + " is missing: `make all` builds it"
    product = ctypes.CDLL(os.path.join(ROOT, "helyim_amd", "libhec.so"))
    assert probe.limits(product) is None
    assert probe.limits(ctypes.CDLL(VARIANT)) == (probe.CHUNK_BYTES, probe.CHUNK_COLS, probe.READ_PIECE)
    r = subprocess.run([sys.executable, os.path.join(TESTS, "small_chunk_probe.py")], env=C.child_env(VARIANT),
                       cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("small-chunk probe ok"), tail(r.stdout + r.stderr)


def test_selected_host_shapes_cross_chunk_edges_under_the_variant():
    """From the selected tests' own shape constants: under the variant there
    are batches of several stripes a chunk in four or more chunks -- slot 0 of
    both loops and stream 0 of the copy pipeline reused -- with a short last chunk,
    batches of one stripe a chunk, and batches that stay in one chunk; the
    product takes the reconstruct-some, footprint and generic-codec batches
    in one chunk each."""
    import test_gpu_footprint as TF
    import test_gpu_host_batch as TH
    import test_gpu_reconstruct_some as TS
    import test_gpu_verify as TV
    product = probe.PRODUCT[0]
    # reconstruct some: 64 stripes of 1000 bytes in 21 chunks of 3 and one of 1; 2048 bytes one stripe a chunk
    assert (TS.EDGE_S, TS.EDGE_L) == (TS.HOST_S, TS.HOST_LENGTHS[0]) == (64, 1000)
    assert probe.host_chunks(TS.EDGE_L, 14, TS.EDGE_S) == (3, 22, 1)
    assert probe.host_chunks(TS.HOST_LENGTHS[1], 14, TS.HOST_S) == (1, 64, 1)
    assert probe.host_chunks(3000, 14, TS.HOST_S)[0] == 1  # the longer stripes that go through the slots first
    assert probe.host_chunks(TS.EDGE_L, 14, TS.EDGE_S, product)[1] == 1
    # pinned memory on the copy pipeline, reconstruct some and verify: ten stripes in chunks of 3, 3, 3 and 1
    for L, S in ((TS.PINNED_COPY_L, TS.PINNED_COPY_S), TV.PINNED_COPIES[::-1]):
        assert probe.host_chunks(L, 14, S) == (3, 4, 1) and probe.host_chunks(L, 14, S, product)[1] == 1
    assert (TS.PINNED_COPY_LOST[2], TS.PINNED_COPY_LOST[3], TS.PINNED_COPY_LOST[9]) == (5, 0, 5)
    # footprint: the mixed-mask batch in chunks of 3, 3, 3 and 2 with the edges the test names; the layout
    # families one stripe a chunk from 2048 bytes up, and nine stripes of 17 bytes in one chunk of up to 13
    L, lost = TF.MIXED
    c, chunks, last = probe.host_chunks(L, 14, len(lost))
    assert (c, chunks, last) == (3, 4, 2)
    assert [(lost[e - 1], lost[e]) for e in range(c, len(lost), c)] == [(4, 5), (5, 4), (1, 0)]
    assert {0, 1, 4, 5} == set(lost)
    for L in TF.HOST_LENGTHS:
        assert probe.host_chunks(L, 14, max(TF.SIZES)) == ((1, 9, 1) if L >= 2048 else (9, 1, 9))
    assert probe.chunk_stripes(17, 14, 1 << 20) == 13
    # host batches: the generic codec in eight chunks of 5 and one of 1; the three ranges of the 41-stripe
    # _multi case in chunks of 3 with a last one of 1 or 2, so range edges and chunk edges fall at
    # different stripes; 1 MiB and 65541-byte stripes one a chunk
    k, m, S, L = TH.GENERIC_CHUNKED
    assert probe.host_chunks(L, k + m, S) == (5, 9, 1) and probe.host_chunks(L, k + m, S, product)[1] == 1
    ranges = [41 * (r + 1) // 3 - 41 * r // 3 for r in range(3)]
    assert ranges == [13, 14, 14] and [probe.host_chunks(1000, 14, r) for r in ranges] == [(3, 5, 1), (3, 5, 2), (3, 5, 2)]
    assert 13 % 3  # the second range's chunks begin at 13, 16, ...: not where one call's would
    assert probe.host_chunks(1 << 20, 14, 40) == (1, 40, 1) and probe.host_chunks(65541, 14, 340) == (1, 340, 1)
    # verify: the four-chunk batches of the product go in thousands of chunks with a short last one
    for k, m, L, _pitch, c_product, S in TV.CHUNKED:
        assert probe.host_chunks(L, k + m, S, product) == (c_product, 4, S - 3 * c_product)
        c, chunks, last = probe.host_chunks(L, k + m, S)
        assert chunks >= 4 and (c == 1 or 0 < last < c), (k, m, L, c, chunks, last)
    assert probe.host_chunks(*[(L, k + m, S) for k, m, L, _, _, S in TV.CHUNKED][0]) == (13, 6483, 5)


def test_selected_volumes_cross_scrub_chunks_under_the_variant():
    """The file tests' 4096-byte blocks go three to a chunk -- two or more, no
    power of two -- so their volumes of a few hundred KiB take tens of chunks
    with a short last one, and a chunk's row is read in three pieces, the last
    one ragged; the product reads each of them as one chunk in one piece."""
    import scrub_harness as SH
    import test_gpu_correct as TC
    import test_gpu_verify as TV
    assert SH.BLOCK == TV.BLOCK == TC.BLOCK == 4096
    per = probe.per_chunk(SH.BLOCK)
    assert per == 3 and per >= 2 and per & (per - 1)
    cols = per * SH.BLOCK
    assert probe.READ_PIECE < cols and probe.READ_PIECE % 256 and cols % probe.READ_PIECE
    assert -(-cols // probe.READ_PIECE) == 3
    for size in (200_001, 250250, 499_999):  # test_gpu_verify.py's shard_files: 250250 bytes, asserted within these
        assert -(-size // cols) >= 17 and probe.per_chunk(SH.BLOCK, probe.PRODUCT[1]) * SH.BLOCK > size
    # the long volumes: 64 KiB and 5 MiB blocks go one block a chunk, the 5 MiB ones in 1049 pieces
    assert probe.per_chunk(65536) == probe.per_chunk(5 << 20) == probe.per_chunk(1 << 20) == 1
    assert SH.BIG_SIZE > 2 * probe.PRODUCT[1]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CHILDREN))
def test_suite_against_small_chunk(gpu, name):
    select, product_seconds, _variant_seconds = CHILDREN[name]
    C.run_child("small chunk", VARIANT, "small_chunk_probe", name, DESELECT[name],
                max(LIMIT_FLOOR, LIMIT_FACTOR * product_seconds), select=select, named=True)
