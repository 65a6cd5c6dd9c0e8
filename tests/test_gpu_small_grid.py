"""The model-based GPU suites again, against build/variants/libhec_smallgrid.so:
the product's sources with kMaxLaunchBlocks = 100 and kLocateMaxBlocks = 4
(Makefile, VFLAGS_smallgrid). Every test of the files below compares the
library with check_model, locate_model, gfref or the C oracle, never with
itself, so under the variant their batches of a few hundred stripes become
split tests: stripe ranges in launch_apply, launch_verify, launch_check and
launch_ragged, second and later iterations of every grid-stride loop, and
several rounds of the two mask kernels -- paths that need 2^23 workgroups (up
to 960 GB of shards) at the product's limits.

One child process per file (`python -m pytest <file> -m gpu` with HEC_LIB_PATH
set); tests/small_grid_probe.py runs first in the child and ends it unless the
limits are live. Every child has a time limit of its own. A child that dies of
a signal or runs out of time fails every remaining file without starting
another process on the device: all children start from run_child of
tests/variant_children.py, so the rule holds by construction."""
import os
import subprocess
import sys

import pytest

import small_grid_probe as probe
import variant_children as C
from variant_children import ROOT, TESTS, tail

VARIANT = C.variant_path("smallgrid")
CHILD_TIMEOUT = 300  # seconds; a child takes about what its file takes with the product library

FILES = ["test_gpu_check.py", "test_gpu_locate.py", "test_gpu_verify.py", "test_gpu_generic_codecs.py",
         "test_gpu_footprint.py", "test_gpu_intervals.py", "test_gpu_parity.py",
         # With four workgroups every batch of the file runs second and later iterations of the correct
         # kernel's grid-stride loop, stores included, and the verify launches ahead of it go in several
         # ranges. Largest device batch 2053 stripes of 4 KiB; largest file scrub fourteen shard files of
         # 8 MiB + 300007 bytes in blocks of up to 5 MiB (one stripe per block, about 120 MB in all).
         "test_gpu_correct.py",
         # The same for the masked correct kernel; the check launches ahead of it go in several ranges and
         # the use-mask kernel goes round after 1024 stripes. Largest batch 2053 stripes of 4 KiB.
         "test_gpu_correct_present.py",
         # Second and later iterations of the pair kernel's grid-stride loop on every batch; the verify,
         # mask and reconstruct launches around it go in several ranges and rounds. Sizes as test_gpu_correct.py.
         "test_gpu_locate_pairs.py",
         # The clean batch and the batch of single flips have more than 100 map entries each
         # (test_ragged_scrub_batches_pass_one_launch_of_the_variant), so pass 1 goes in several launches
         # (launch_ragged's block_base and XCD eighths per launch), and with four workgroups pass 2 runs
         # second and later rounds over the map on every batch with more than four 4 KiB ranges.
         "test_gpu_ragged_scrub.py",
         # The same for the correct pass (test_ragged_correct_batches_pass_one_launch_of_the_variant); the
         # decode of the corrected reconstruct goes through launch_ragged's launches from its own map.
         "test_gpu_ragged_correct.py",
         # Every strided batch goes in stripe ranges of at most 100 workgroups, where the want words have to
         # advance with the masks; the generic kernel runs second and later iterations of its grid-stride
         # loop, and the ragged batches are split into several launches.
         "test_gpu_reconstruct_some.py"]
TIMEOUTS = {"test_gpu_reconstruct_some.py": 420}  # about a minute with the product library; the others CHILD_TIMEOUT

# Deselected under the variant, by node id. Only two kinds: shapes of more than
# 2 GiB of device memory or more than 2^20 stripes ("size"), and expectations
# that are a kernel name or a path choice the limit legitimately changes
# ("name"). No verify, locate, repair, check or checked-reconstruct test at
# shards of 16 KiB or less is here.
DESELECT = {
    "test_gpu_check.py": [
        ("test_shard_len_near_4gib[4294965248]", "size: 112 GiB in HBM"),
        ("test_shard_len_near_4gib[4294971408]", "size: 112 GiB in HBM"),
        ("test_masked_scrub_past_one_launch", "size: 2^23 + 5 stripes, 1.9 GB and a clone"),
    ],
    "test_gpu_locate.py": [
        ("test_locate_and_repair_past_one_launch", "size: 2^23 + 5 stripes, 1.9 GB and a clone"),
    ],
    "test_gpu_verify.py": [
        ("test_verify_shard_len_near_4gib[4294959104]", "size: 56 GiB in HBM"),
        ("test_verify_shard_len_near_4gib[4294975488]", "size: 56 GiB in HBM"),
        ("test_verify_shard_len_near_4gib[4294971408]", "size: 56 GiB in HBM"),
        ("test_kernel_names", "name: 1 MiB shards are 128 chunks of 8 KiB, more than 100: the generic verify"),
    ],
    "test_gpu_generic_codecs.py": [
        ("test_generic_batch_past_one_grid[16]", "size: 2^23 + 5 stripes"),
        ("test_generic_batch_past_one_grid[1]", "size: 2^23 + 5 stripes"),
        ("test_rs104_odd_base_batch_past_one_grid", "size: 2^23 + 5 stripes"),
        ("test_k10_odd_base_batch_past_one_grid", "size: 2^23 + 5 stripes"),
        ("test_verify_past_one_grid[10-4-16]", "size: 2^23 + 5 stripes"),
        ("test_verify_past_one_grid[3-2-1]", "size: 2^23 + 5 stripes"),
    ],
    "test_gpu_footprint.py": [],
    "test_gpu_intervals.py": [],
    "test_gpu_parity.py": [
        ("test_bitslice_encode_matches_oracle", "name: asserts the bit-sliced encode at 1 MiB shards (256 chunks > 100)"),
        ("test_full_config_roundtrip[0]", "size: 4096 stripes of 14 x 1 MiB, 56 GiB"),
        ("test_full_config_roundtrip[65536]", "size: 4096 stripes of 14 x 1 MiB, 56 GiB"),
        ("test_full_config_every_4_erasure_pattern_and_linearity", "size: 4004 stripes of 14 x 1 MiB, 55 GiB"),
        ("test_batch_over_launch_limit_is_split", "size: 2^24 + 5 stripes"),
        ("test_ragged_over_launch_limit_is_split", "size: 2^24 + 5 stripes"),
        ("test_ragged_shard_len_near_4gib", "size: 56 GiB in HBM"),
        ("test_strided_batch_shard_len_near_4gib[4294959104]", "size: 56 GiB in HBM"),
        ("test_strided_batch_shard_len_near_4gib[4294963200]", "size: 56 GiB in HBM"),
        ("test_strided_batch_shard_len_near_4gib[4294975488]", "size: 56 GiB in HBM"),
        ("test_config5_whole_batch_vs_oracle", "size: 32 GiB in HBM, and 17 of this child's 26 s"),
    ],
    "test_gpu_correct.py": [],
    "test_gpu_correct_present.py": [],
    "test_gpu_locate_pairs.py": [],
    "test_gpu_ragged_scrub.py": [],
    "test_gpu_ragged_correct.py": [],
    "test_gpu_reconstruct_some.py": [],
}


def child_env():
    return C.child_env(VARIANT)


def test_variant_is_built_and_its_limits_are_live():
    """build() leaves the variant beside the product; a process that loads it
    reports the limits and the kernel names that flip with them, and the
    product library exports no such query."""
    import helyim_amd as H
    assert os.path.exists(VARIANT), VARIANT + " is missing: `make all` builds it"
    assert probe.limits(H.lib) is None or os.environ.get("HEC_LIB_PATH")
    r = subprocess.run([sys.executable, os.path.join(TESTS, "small_grid_probe.py")], env=child_env(), cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("small-grid probe ok"), tail(r.stdout + r.stderr)
    # the same shard lengths name the one-chunk-per-workgroup kernels in the product
    product = {(fn, length): getattr(H.lib, fn)(length).decode() for fn, length, _ in probe.NAMES}
    if not os.environ.get("HEC_LIB_PATH"):
        assert product["hec_encode_kernel_name", 102 * 4096].startswith("rs104_bs_encode_kernel")
        assert product["hec_verify_kernel_name", 101 * 8192].startswith("rs104_bs_verify_kernel")
        assert product["hec_check_kernel_name", 101 * 2048].startswith("rs104_check_kernel")
        assert product["hec_decode_kernel_name", 101 * 2048].startswith("rs104_narrow_kernel<DEC=true")


def test_ragged_scrub_batches_pass_one_launch_of_the_variant():
    """The entry counts FILES' comment on test_gpu_ragged_scrub.py relies on, from the file's own shapes."""
    import test_gpu_ragged_scrub as T
    clean = T.Ragged([(L, m) for L in T.LENGTHS for m in T.MASKS] + [(24576, m) for m in (T.R3, T.R2, T.R1) * 3])
    flips = T.Ragged([(L, m) for L, m, _, _ in T.flip_cases(T.LENGTHS, (T.R4, T.R3, T.R2, T.R1))])
    assert clean.entries() > probe.MAX_LAUNCH_BLOCKS and flips.entries() > 2 * probe.MAX_LAUNCH_BLOCKS
    assert clean.entries() > probe.LOCATE_MAX_BLOCKS


def test_ragged_correct_batches_pass_one_launch_of_the_variant():
    """The same for test_gpu_ragged_correct.py."""
    import test_gpu_ragged_correct as T
    clean = T.Ragged(T.clean_shapes())
    flips = T.Ragged([(L, m) for L, m, _, _ in T.single_flip_cases("table")])
    assert clean.entries() > probe.MAX_LAUNCH_BLOCKS and flips.entries() > 2 * probe.MAX_LAUNCH_BLOCKS
    assert clean.entries() > probe.LOCATE_MAX_BLOCKS and flips.entries() > probe.LOCATE_MAX_BLOCKS


def run_child(name, deselect, timeout):
    """tests/<name> in a child process against the variant (variant_children.run_child)."""
    C.run_child("small grid", VARIANT, "small_grid_probe", name, deselect, timeout)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FILES)
def test_suite_against_small_grid(gpu, name):
    run_child(name, DESELECT[name], TIMEOUTS.get(name, CHILD_TIMEOUT))
