"""csrc/smz_othello.hpp -- the rule core the device env and the host entry points share -- compiled by a plain host compiler
into a stand-alone program (tests/othello_rules_check.cpp) with AddressSanitizer and UndefinedBehaviorSanitizer: random legal
games with the rules' invariants checked at every move (disjoint colours, flips inside the opponent's discs, one disc more
per placement, the move mask inside the empty squares).  A shift by a bad count or a read past a row shows here.  Nothing is
loaded into Python under a sanitizer.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "stochastic-muzero_amd", "csrc")
CXX = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("g++")


@pytest.mark.skipif(CXX is None, reason="needs a host C++ compiler")
def test_random_legal_games_keep_the_invariants(tmp_path):
    exe = os.path.join(tmp_path, "othello_rules_check")
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-sanitize-recover=all", "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "othello_rules_check.cpp")],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.startswith("ok: ")
