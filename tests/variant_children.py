"""GPU test files run again in child processes against a variant library of
build/variants (Makefile, VARIANTS) -- TEST INFRASTRUCTURE ONLY.

One child per file: `python -m pytest -p <probe plugin> <file> -m gpu` with
HEC_LIB_PATH set to the variant; the probe plugin runs at session start in the
child and ends it unless the variant's constants are live. Every child has a
time limit of its own. A child that dies of a signal or runs out of time fails
every later child without starting another process on the device: all children
of tests/test_gpu_small_grid.py and tests/test_gpu_small_chunk.py start from
run_child below and share one stop list, so the rule holds by construction."""
import os
import re
import subprocess
import sys
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.join(ROOT, "tests")
DESELECTED_LINE = "deselected node: "  # written by a probe plugin that reports what the child left out

_stopped = []  # why no further child may start (a child died of a signal or ran out of time)


def variant_path(name):
    return os.path.join(ROOT, "build", "variants", f"libhec_{name}.so")


def child_env(variant):
    env = dict(os.environ)
    env["HEC_LIB_PATH"] = variant
    env["PYTHONPATH"] = os.pathsep.join([TESTS] + [p for p in env.get("PYTHONPATH", "").split(os.pathsep) if p])
    return env


def tail(text, n=60):
    return "\n".join(text.splitlines()[-n:])


def count(word, text):
    m = re.search(r"(\d+) " + word, text.splitlines()[-1] if text.strip() else "")
    return int(m.group(1)) if m else 0


def run_child(label, variant, plugin, name, deselect, timeout, select=None, named=False):
    """tests/<name> in a child process against `variant`; none starts after one
    died of a signal or ran out of time. deselect: (node id, reason) pairs,
    every one of which must match a test. select: a -k expression. named: the
    child's probe plugin names what the ids left out (DESELECTED_LINE) -- the
    summary's count also holds what -k dropped and counts an id without its
    parameters once per case."""
    assert not _stopped, "not started: " + _stopped[0]
    assert os.path.exists(variant), variant + " is missing: `make all` builds it"
    cmd = [sys.executable, "-m", "pytest", "-p", plugin, os.path.join("tests", name), "-m", "gpu", "-q",
           "--maxfail=5", "-p", "no:cacheprovider"]
    if select:
        cmd += ["-k", select]
    for node, _reason in deselect:
        cmd += ["--deselect", f"tests/{name}::{node}"]
    t0 = time.monotonic()
    try:
        r = subprocess.run(cmd, env=child_env(variant), cwd=ROOT, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        _stopped.append(f"the child of {name} ({label}) was killed after {timeout} s")
        out = e.stdout if isinstance(e.stdout, str) else (e.stdout or b"").decode(errors="replace")
        pytest.fail(_stopped[0] + "\n" + tail(out))
    wall = time.monotonic() - t0
    out = r.stdout + r.stderr
    if r.returncode < 0:
        _stopped.append(f"the child of {name} ({label}) died of signal {-r.returncode}")
        pytest.fail(_stopped[0] + "\n" + tail(out))
    passed, deselected = count("passed", r.stdout), count("deselected", r.stdout)
    print(f"{label} {name}: {passed + deselected + count('failed', r.stdout)} collected, {deselected} deselected, "
          f"{passed} passed, {wall:.1f} s")
    assert r.returncode == 0, f"{name} under the {label} variant (return code {r.returncode}):\n{tail(out)}"
    assert passed > 0, tail(out)
    if not named:
        assert select is None
        assert deselected == len(deselect), f"a deselected node id of {name} matches no test:\n{tail(out)}"
        return
    left_out = {line[len(DESELECTED_LINE):].strip() for line in r.stdout.splitlines()
                if line.startswith(DESELECTED_LINE)}
    for node, _reason in deselect:  # an id without its parameters stands for every case of the test
        assert any(got.startswith(f"tests/{name}::{node}") for got in left_out), \
            f"the deselected node id {node} of {name} matches no test:\n{tail(out)}"
