"""The kernel launch layer of helyim_amd/csrc/rs_kernels.hip, pinned on a CPU:
which kernel every launch_* function launches, how often, on what grid and with
which launcher-computed arguments. tests/c/launch_record.cpp defines the few
HIP entry points the compiled object needs (registration, call configuration,
hipLaunchKernel), is linked with g++ against the object without the HIP
runtime, calls the launchers with fixed fake pointers and prints one line per
launch. No device is opened. Its output must equal the recorded files
tests/golden/launch_record_{product,smallgrid}.txt byte for byte, for

  * build/obj/rs_kernels.hip.o, the product's object (2^23 workgroups a
    launch, 2048 in the locate grid), and
  * build/variants/smallgrid/rs_kernels.o, the Makefile's smallgrid variant
    (100 and 4), where batches of a few hundred stripes reach every split.

Both are made by `make all`; a missing one fails the test. A launch line reads
`tag: kernel g=grid` and then, for the strided kernels, n_stripes (ns), the
stripe offsets of in_base / out_base / masks (in, out, m; `-` = null) from the
values put in, chunks_per_stripe (cps), n_items (ni), map_q8 / map_r8 (q, r),
cps_mul / cps_shift (mul, sh), the stripe offset of the struct's own advancing
pointer (wants, old, mis, chk) and whether done_flag is still set (every batch
is given one: only its last launch may keep it); for the ragged kernels
n_blocks (nb), block_base, map_q8 / map_r8, half_shift where there is one and
done_flag; for the mask kernels the grid and n_stripes.

Shapes (P = kMaxLaunchBlocks + 5: 105 stripes, or 2^23 + 5):
  * the seven ranged paths -- encode, encode over_pcie, decode (launch_apply),
    launch_some, launch_update with an old arena, launch_verify (fast104) and
    launch_check, all aligned RS(10,4) -- over (len, stripes) =
    {1, 2048, 4096, 4096 + 16, 8192} x {1, 130}; 101 x 2048 x {1, 3} (51 4 KiB
    chunks: a stripe a launch at 100); (kMaxLaunchBlocks + 2) x 4096 x {1, 3}
    (102 x 4096 at 100: one stripe's chunks pass a launch, the grid-stride
    kernel); 4 GiB + 8192 x {1, 9} and
    4 GiB + 8208 x 1 (the 64-bit offset kernels; 9 stripes pass 2^23 chunks);
    {4096, 4096 + 16} x {50, 51, 100, 101}; 8192 x 101; 2048 x 101;
    {2048, 8192} x P; the empty batches 4096 x 0 and 0 x 130; and 4096 x 1000
    for the encode and the decode (ten ranges). Together: one launch, equal
    ranges, a short last range, a last range that picks another kernel
    (4096 x 130 decode at 100: rs104_kernel<true> on 100 workgroups, then
    rs104_narrow_kernel<true> on 60), one stripe past the limit.
  * every other layout -- decode over_pcie, encode / decode / some unaligned,
    nin = 6 aligned and not, nin = 10 without fast104, update without an old
    arena aligned and not and with one unaligned, verify unaligned / without
    fast104 / nin = 6 aligned and not, check unaligned -- over (1, 1),
    (4096 + 16, 130), ((kMaxLaunchBlocks + 2) x 4096, 3), (4 GiB + 8192, 1), (2048, P) and the
    two empty batches.
  * launch_locate / launch_correct and launch_locate_present /
    launch_correct_present, aligned: 4096 x {1, 3, 4, 5, 2047, 2049},
    (4096 + 16) x 2, 1 x 130, 4 GiB + 8192 x 1 and the empty batches (item
    counts below, at and above either kLocateMaxBlocks); unaligned and pairs
    on the first three of those.
  * the ragged launchers with 0, 1, 99, 100, 101, 257 and P map entries:
    encode, bit-sliced encode, and check / locate / correct on a 4 KiB and on a
    bit-sliced map; decode and some, compact and not, with 0 and 101.
  * the four mask launchers with 0, 1, 1024, 1025 and 5000 stripes.

The test also checks that every kernel the object registers is launched at
least once in each file, fill_splitmix_kernel and add_word_kernel aside. In the
small-grid build the 64-bit offset kernels (shards of 4 GiB and more, one
workgroup per chunk of at most 8 KiB) cannot be launched at all: such a stripe
has more than 100 chunks, so its batch takes the grid-stride kernel. The test
expects exactly them to be missing there; the product record has them.

The golden files were recorded from objects built from the commit before the
launch layer was folded (`launch_record > tests/golden/launch_record_<build>.txt`
with the program linked against that commit's objects); a change
to rs_kernels.hip that alters them alters a launch."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
NOT_RECORDED = {"fill_splitmix_kernel", "add_word_kernel"}


def variant_flags(name):
    """The -D flags the Makefile compiles a variant's sources with."""
    text = open(os.path.join(ROOT, "Makefile")).read()
    return re.search(r"^VFLAGS_%s := (.*)$" % name, text, re.M).group(1).split()


@pytest.mark.parametrize("name,obj,flags", [
    ("product", "build/obj/rs_kernels.hip.o", lambda: []),
    ("smallgrid", "build/variants/smallgrid/rs_kernels.o", lambda: variant_flags("smallgrid")),
])
def test_launches_match_the_record(tmp_path, name, obj, flags):
    obj = os.path.join(ROOT, obj)
    assert os.path.exists(obj), obj + " is missing: run `make all`"
    exe = str(tmp_path / "launch_record")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__", *flags(),
                    "-I" + os.path.join(ROCM, "include"), "-I" + os.path.join(ROOT, "helyim_amd", "csrc"),
                    os.path.join(ROOT, "tests", "c", "launch_record.cpp"), obj, "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    assert "!" not in r.stdout and "?" not in r.stdout  # the recorder's marks of something it could not decode
    golden = open(os.path.join(ROOT, "tests", "golden", "launch_record_%s.txt" % name)).read()
    if r.stdout != golden:
        got, want = r.stdout.splitlines(), golden.splitlines()
        at = next((i for i, (g, w) in enumerate(zip(got, want)) if g != w), min(len(got), len(want)))
        pytest.fail("launches differ from the record at line %d (%d lines against %d):\n got  %s\n want %s" % (
            at + 1, len(got), len(want), "\n".join(got[at:at + 3]), "\n".join(want[at:at + 3])))
    # every registered kernel is launched somewhere in the record
    names = subprocess.run([exe, "--registered"], capture_output=True, text=True, check=True).stdout.splitlines()
    registered = {n.split("(")[0] for n in names}
    assert len(registered) == len(names) > 50
    launched = set(re.findall(r"^ [^:]+: (.+?) g=\d+", golden, re.M))
    assert launched <= registered
    unreachable = {n for n in registered if "unsigned long" in n} if name == "smallgrid" else set()
    assert len(unreachable) in (0, 7)
    assert registered - launched == NOT_RECORDED | unreachable
