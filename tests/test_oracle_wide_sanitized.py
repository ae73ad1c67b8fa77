"""oracle/smz_oracle.c at the widths its stack arrays were enlarged for (ORC_MAX_A = 1024), compiled by a plain host compiler
into a stand-alone program (tests/oracle_wide_check.c) with AddressSanitizer and UndefinedBehaviorSanitizer: root init, six
rounds of select / expand_backup and act at T = 0, 0.5 and 1 at (A, K) = (1024, 1024) and (1000, 5).  An A-wide stack array
that is still 128 entries long, or a node index past the tree's capacity, shows here.  Nothing is loaded into Python under a
sanitizer.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CC = shutil.which(os.environ.get("CC", "gcc")) or shutil.which("gcc")


@pytest.mark.skipif(CC is None, reason="needs a host C compiler")
def test_wide_searches_stay_inside_the_oracles_arrays(tmp_path):
    exe = os.path.join(tmp_path, "oracle_wide_check")
    r = subprocess.run([CC, "-std=c11", "-O1", "-g", "-ffp-contract=off", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Werror",
                        "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "oracle"), "-o", exe,
                        os.path.join(ROOT, "tests", "oracle_wide_check.c"), "-lm", "-lpthread"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.startswith("ok: ")
