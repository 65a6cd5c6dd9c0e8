"""tests/test_gpu_reconstruct_some.py again, against
build/variants/libhec_smallgrid.so (kMaxLaunchBlocks = 100;
tests/test_gpu_small_grid.py has the reasons): every strided batch of the file
goes in stripe ranges of at most 100 workgroups, where the want words have to
advance with the masks, the generic kernel runs second and later iterations of
its grid-stride loop, and the ragged batches are split into several launches.

One child process (`python -m pytest tests/test_gpu_reconstruct_some.py -m gpu`
with HEC_LIB_PATH set); tests/small_grid_probe.py runs first in the child and
ends it unless the limits are live. Nothing is deselected. The child has a time
limit of its own, and is not started when an earlier small-grid child died of
a signal or ran out of time."""
import os
import subprocess
import sys

import pytest

import test_gpu_small_grid as G
from test_gpu_small_grid import ROOT, VARIANT, child_env, tail

NAME = "test_gpu_reconstruct_some.py"
CHILD_TIMEOUT = 420  # seconds; the file takes about a minute with the product library


@pytest.mark.gpu
def test_reconstruct_some_suite_against_small_grid(gpu):
    assert not G._stopped, "not started: " + G._stopped[0]
    assert os.path.exists(VARIANT), VARIANT + " is missing: `make all` builds it"
    cmd = [sys.executable, "-m", "pytest", "-p", "small_grid_probe", os.path.join("tests", NAME), "-m", "gpu", "-q",
           "--maxfail=5", "-p", "no:cacheprovider"]
    try:
        r = subprocess.run(cmd, env=child_env(), cwd=ROOT, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        G._stopped.append(f"the child of {NAME} was killed after {CHILD_TIMEOUT} s")
        out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
        pytest.fail(G._stopped[0] + "\n" + tail(out))
    out = r.stdout + r.stderr
    if r.returncode < 0:
        G._stopped.append(f"the child of {NAME} died of signal {-r.returncode}")
        pytest.fail(G._stopped[0] + "\n" + tail(out))
    assert r.returncode == 0, f"{NAME} under the small-grid variant (return code {r.returncode}):\n{tail(out)}"
    assert G.count("passed", r.stdout) > 0 and G.count("deselected", r.stdout) == 0, tail(out)
