"""The update suites again, against the Makefile's two test variants
(tests/variant_children.py: one child per file with HEC_LIB_PATH set, the
variant's probe plugin first in the child, a time limit per child, and no
further child after one died of a signal or ran out of time).

tests/test_gpu_update.py against build/variants/libhec_smallgrid.so: with 100
workgroups a launch every aligned batch of more than 50 two-range stripes goes
in stripe ranges, where the mask words and all three arenas have to advance
with the range, and the generic kernel runs second and later iterations of its
grid-stride loop. tests/test_gpu_host_update.py against libhec_smallchunk.so:
with 48 KiB host chunks the 41-stripe batch goes in 14 chunks, through both
pinned slots and all three streams and device slots of the host driver many
times over. Nothing is deselected."""
import pytest

import small_chunk_probe as chunk_probe
import small_grid_probe as grid_probe
import variant_children as C

CHILD_TIMEOUT = 300  # seconds; each file takes well under a minute with the product library


def test_update_batches_pass_one_launch_and_one_round_of_slots():
    """From the two files' own shapes: the every-mask batch needs about 21
    launches of the small-grid build, and the host batch more chunks than the
    host driver has slots and streams; the product takes either in one."""
    import test_gpu_host_update as TH
    import test_gpu_update as TU
    per_stripe = -(-TU.EVERY_L // 4096)
    assert per_stripe == 2 and TU.EVERY_L % 4096  # two column ranges a stripe, the second partial
    assert TU.EVERY_S * per_stripe > grid_probe.MAX_LAUNCH_BLOCKS
    stripes_a_launch = grid_probe.MAX_LAUNCH_BLOCKS // per_stripe
    assert -(-TU.EVERY_S // stripes_a_launch) == 21
    assert TU.EVERY_S * per_stripe <= 1 << 23  # the product: one launch
    # the generic kernel's batch: more items than the small grid has workgroups, so its loop goes round
    assert TU.GENERIC_S * per_stripe > grid_probe.MAX_LAUNCH_BLOCKS
    c, chunks, last = chunk_probe.host_chunks(TH.L, 14, TH.S)
    assert (c, chunks, last) == (3, 14, 2)
    assert chunks > 3 * 3 and chunks > 2 * 2  # every device slot and stream, and both pinned slots, several times
    assert chunk_probe.host_chunks(TH.L, 14, TH.S, chunk_probe.PRODUCT[0])[1] == 1


@pytest.mark.gpu
def test_update_suite_against_small_grid(gpu):
    C.run_child("small grid", C.variant_path("smallgrid"), "small_grid_probe", "test_gpu_update.py", [], CHILD_TIMEOUT)


@pytest.mark.gpu
def test_host_update_suite_against_small_chunk(gpu):
    C.run_child("small chunk", C.variant_path("smallchunk"), "small_chunk_probe", "test_gpu_host_update.py", [],
                CHILD_TIMEOUT, select=None, named=True)
