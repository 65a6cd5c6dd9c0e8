"""The launch splitter (helyim_amd/csrc/launch_split.hpp): block launches of
the ragged kernels and stripe ranges of the strided RS(10,4) fast paths, for a
batch of more workgroups than one launch takes. A real split needs more than
2^23 workgroups (the launchers around it run on the GPU at the small-grid
build's limit of 100, tests/test_gpu_small_grid.py); the arithmetic takes the
limit as a parameter and tests/c/launch_split_check.cpp, compiled with g++
(the header is plain C++), checks it at small limits piece by piece and at the
production limit and at 100 by counting. A wrong piece would skip or code twice a range of stripes,
or signal completion before the last launch."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_launch_split_covers_every_item_once(tmp_path):
    exe = str(tmp_path / "launch_split_check")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "c", "launch_split_check.cpp"),
                    "-I" + os.path.join(ROOT, "helyim_amd", "csrc"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.startswith("ok ")
