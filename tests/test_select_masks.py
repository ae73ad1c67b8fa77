"""The bit logic of the mask-based descent (stochastic-muzero_amd/csrc/smz_select_masks.hpp, SMZ_SELECT_MASKS) on the CPU.

The header holds plain-integer functions that the search kernel and this test share.  tests/select_masks_check.cpp -- a
stand-alone program with its own main, built here with AddressSanitizer and UBSan -- emulates a wavefront's 64 lanes with two
trees of up to 64 two-child blocks, hands block lineages from lane to lane as the kernel's expansion does, and checks on some
thousands of random trees (random picks, random "evaluated" flags) that the mask rule yields exactly the path, the length, the
leaf location, the leaf's action and the parent node of a plain pointer chase from the root, and reports the fallback exactly
when the chase meets an unevaluated block.  Degenerate shapes: a 51-deep and a 64-deep chain (paths that cross from blocks
below 32 into blocks from 32 on), a single root, a switched-off tree slot, both tree slots interleaved in one ballot.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stochastic-muzero_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_mask_rule_equals_a_pointer_chase_from_the_root(tmp_path):
    exe = os.path.join(tmp_path, "select_masks_check")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "select_masks_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.startswith("ok: ")
