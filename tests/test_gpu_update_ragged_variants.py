"""The ragged update suite again, against the Makefile's small-grid variant
(tests/variant_children.py: one child with HEC_LIB_PATH set, the variant's
probe plugin first in the child, a time limit, and no further child after one
died of a signal or ran out of time).

tests/test_gpu_update_ragged.py against build/variants/libhec_smallgrid.so:
with 100 workgroups a launch, launch_ragged splits every batch of more than 100
map entries, so later launches run with a non-zero block_base and their own XCD
eighths; the every-mask batch goes in 16 launches. Nothing is deselected."""
import pytest

import small_grid_probe as grid_probe
import variant_children as C

CHILD_TIMEOUT = 300  # seconds; the file takes well under a minute with the product library


def test_every_mask_batch_passes_one_launch():
    """From the file's own shapes: the every-mask batch owns more map entries
    than the small-grid build launches at once; the product takes it in one."""
    import test_gpu_update_ragged as TU
    lens, masks = TU.every_mask_batch()
    assert len(lens) == 1024 and sorted(masks) == list(range(1024))
    per_stripe = [-(-ln // 4096) for ln in TU.EVERY_LENS]
    assert per_stripe == [2, 1] and all(ln % 4096 for ln in TU.EVERY_LENS)  # every last range partial
    empty = masks.index(0)
    entries = TU.map_entries(lens, masks)
    assert entries == 512 * 2 + 512 * 1 - per_stripe[empty % 2] == 1534
    assert entries > grid_probe.MAX_LAUNCH_BLOCKS
    assert -(-entries // grid_probe.MAX_LAUNCH_BLOCKS) == 16  # block_base is non-zero in fifteen of them
    assert entries % grid_probe.MAX_LAUNCH_BLOCKS % 8        # the last launch's eighths are uneven
    assert entries <= 1 << 23                                 # the product: one launch
    # the empty stripe sits inside the batch, between stripes that own entries
    assert 0 < empty < len(lens) - 1 and masks[empty - 1] & 0x3FF and masks[empty + 1] & 0x3FF
    # the mixed-length batch stays below the limit: the child covers the unsplit path as well
    assert TU.map_entries(list(TU.LENGTHS), [1] * len(TU.LENGTHS)) < grid_probe.MAX_LAUNCH_BLOCKS


@pytest.mark.gpu
def test_update_ragged_suite_against_small_grid(gpu):
    C.run_child("small grid", C.variant_path("smallgrid"), "small_grid_probe", "test_gpu_update_ragged.py", [],
                CHILD_TIMEOUT)
