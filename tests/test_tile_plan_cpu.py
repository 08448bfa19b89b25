"""The host-side tile planner of the tiled ConvNet kernels (csrc/tile_plan.hpp) on synthetic families, without a GPU.

tests/tile_plan_check.cpp is a stand-alone program (its own main, no HIP header): tables and cost functions written there, the
search held to a brute-force minimum, the pins to their precedence, the head + tail split to its invariants.  It is built with
the host compiler that ships next to hipcc, as plain C++17, and run once; each case prints one line, the first failure ends
the process with a non-zero status."""
import os
import shutil
import subprocess

import pytest

from riser_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tile_plan_check.cpp")


def _host_cxx():
    """the clang++ beside hipcc (riser_amd/build.py: _hipcc): <rocm>/bin/hipcc -> <rocm>/lib/llvm/bin/clang++"""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(B._hipcc())))
    for c in (os.path.join(rocm, "lib", "llvm", "bin", "clang++"), os.path.join(rocm, "llvm", "bin", "clang++"),
              os.path.join(rocm, "bin", "amdclang++"), shutil.which("clang++"), shutil.which("g++")):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("no host C++ compiler found next to hipcc")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tile_plan") / "tile_plan_check")
    r = subprocess.run([_host_cxx(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + B.CSRC, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_planner_headers_are_host_only():
    """tile_plan.hpp includes no HIP header and has no compiler-dependent part; tile_walk.hpp keeps its device half behind one"""
    with open(os.path.join(B.CSRC, "tile_plan.hpp")) as f:
        text = f.read()
    assert "hip/" not in text and "__HIPCC__" not in text and "__device__" not in text
    assert "std::function" not in text and "std::vector" not in text and "<vector>" not in text and "<functional>" not in text
    with open(os.path.join(B.CSRC, "tile_walk.hpp")) as f:
        walk = f.read()
    assert "hip/" not in walk and walk.count("#ifdef __HIPCC__") == 1


def test_tile_plan_check_passes(check_output):
    lines = [ln for ln in check_output if ln.strip()]
    assert not [ln for ln in lines if ln.startswith("FAIL")]
    cases = [ln for ln in lines if ln.startswith("ok ")]
    assert len(cases) >= 16 and lines[-1] == f"all {len(cases)} cases passed"
    # every family of checks the planner's description promises is there
    for word in ("brute-force", "tie", "no shape", "two passes", "force string", "tuned list", "any pin", "split", "margin"):
        assert any(word in ln for ln in cases), word
