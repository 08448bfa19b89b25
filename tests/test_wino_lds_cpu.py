"""The LDS rows of the tiled F(4,3) kernel (csrc/conv_wino4.hip) without a GPU: pitch kc + 2, and for the one tile that does
not fit the LDS that way (512 x 80 at chunks of 20) unpadded rows with the k index swizzled by bit 3 of the row
(csrc/conv_wino_device.hpp: wino_unpadded, wino_pitch, wino_swizzle, wino_word).

tests/wino_lds_check.cpp is a stand-alone program (its own main, no HIP header) that includes the host half of that header and
walks every read and write pattern of the kernel through it: each 32-lane group of every fragment read on 32 distinct banks,
every stored word read back where the reader looks for it, no word shared by two (row, channel) pairs, and the two sides of
the 160 KB budget.  Built with the host compiler next to hipcc as plain C++17, like tests/tile_plan_check.cpp, and run once."""
import os
import subprocess

import pytest

from riser_amd import build as B
from tests.test_tile_plan_cpu import _host_cxx

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "wino_lds_check.cpp")


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wino_lds") / "wino_lds_check")
    r = subprocess.run([_host_cxx(), "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + B.CSRC, SRC, "-o", exe],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.splitlines()


def test_the_pitch_helpers_are_host_usable():
    """the header keeps everything that needs the HIP compiler behind one #ifdef, the pitch functions in front of it"""
    with open(os.path.join(B.CSRC, "conv_wino_device.hpp")) as f:
        text = f.read()
    head = text.split("#ifdef __HIPCC__")
    assert len(head) == 2
    assert head[0].count("#include") == 1 and '#include "tile_plan.hpp"' in head[0] and "__device__" not in head[0]
    for name in ("bool wino_unpadded", "int wino_pitch", "int wino_swizzle", "int wino_word", "int wino_stage_rows", "int wino_stage_cols",
                 "int wino_buf_floats"):
        assert f"constexpr {name}(" in head[0], name


def test_wino_lds_check_passes(check_output):
    lines = [ln for ln in check_output if ln.strip()]
    assert not [ln for ln in lines if ln.startswith("FAIL")]
    cases = [ln for ln in lines if ln.startswith("ok ")]
    assert len(cases) == 10 and lines[-1] == f"all {len(cases)} cases passed"
    for kc, form in ((16, "padded"), (20, "padded"), (20, "unpadded")):
        for word in ("A fragment", "B fragment", "stores and reads meet"):
            assert any(word in ln and f"kc {kc}: {form}," in ln for ln in cases), (kc, form, word)
    assert any("LDS budget" in ln for ln in cases)


def test_the_check_mirrors_the_kernels_lines():
    """the address lines the check writes out again are the kernel's own (a kernel edit that moves them must move the check)"""
    with open(os.path.join(B.CSRC, "conv_wino4.hip")) as f:
        kernel = f.read()
    for line in ("const int a_st = (a_row & 3) * PL + (a_row >> 2) * S + 4 * a_c4;",
                 "const int b_st = A_ELEMS + ((b_rem / KQ) * BN + b_n) * S + 4 * (b_rem % KQ);",
                 "const int a_rd = (wm * 16 * MT + r) * S + (kq ^ T::swz(r));",
                 "const int a_rd1 = (wm * 16 * MT + r) * S + (kq ^ T::swz(r + 1));",
                 "const int b_rd = A_ELEMS + (wn * 16 * NT + r) * S + (kq ^ T::swz(r));",
                 "const int a_h0 = (a_row >> 5) & 1, b_h0 = (b_n >> 3) & 1;",
                 "int h = (((a_row >> 2) + u * (RPT / 4)) >> 3) & 1;",
                 "if constexpr (RPT % 32 == 0) h = a_h0 ^ ((u * (RPT / 32)) & 1);",
                 "int h = ((b_n + v * NPP) >> 3) & 1;",
                 "if constexpr (NPP % 16 == 0) h = b_h0;",
                 "(k < 4 ? Ab : Ab1)[(k & 3) * PL + (i * 16 + (k >> 2)) * S + c0]"):
        assert line in kernel, line
