#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.  No GPU needed.

    hipcc $(HIPFLAGS) -S --cuda-device-only -o before/smz_search.s smz_search.hip      (one .s per translation unit)
    tools/kernel_diff.py before/ after/

For every .s file present in both directories and every kernel (.amdhsa_kernel name) in it, the text from the kernel's label
to its .Lfunc_end -- instructions and the .amdhsa_kernel block with the register, scratch and LDS figures -- must be the same
after normalisation: __hip_cuid_ lines (they depend on the file name) are dropped, the per-function index is stripped from
.LBB<n>_<m>, .Lfunc_begin<n>, .Lfunc_end<n>, jump-table labels and the loop comments (the assembler numbers functions by
their position in the unit), the unit-wide counter from .Lpost_getpc<n> (long branches), and runs of blanks count as one.
Kernels present on one side only are listed.  For a kernel that differs, one line says how far apart the two sides are --
whether the .amdhsa_kernel block is identical, the number of instruction lines on each side, and the size of the symmetric
difference of the two sides as multisets of normalised lines (0: a reordering only; 2: one line changed) -- before the first
40 lines of the diff.  Exit status 1 if a common kernel differs or a file is missing.
"""
import difflib
import os
from collections import Counter
import re
import sys

_INDEXED = re.compile(r"(\.LBB|\.Lfunc_begin|\.Lfunc_end|\.LJTI|\.LCPI|\.Lpost_getpc|\bBB)\d+")      # (BB<n>_<m>: the loop comments)
_SPACES = re.compile(r"[ \t]+")          # (the comment column moves with the width of the stripped index)
_KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
_LABEL = re.compile(r"^([^\s:]+):")


def kernels(path):
    """{kernel name: normalised lines from its label to its .Lfunc_end}"""
    with open(path) as f:
        lines = [_SPACES.sub(" ", _INDEXED.sub(r"\1", l.rstrip("\n"))) for l in f if "__hip_cuid_" not in l]
    names = {m.group(1) for m in map(_KERNEL.match, lines) if m}
    out, name, start = {}, None, 0
    for i, l in enumerate(lines):
        if name is None:
            m = _LABEL.match(l)
            if m and m.group(1) in names:
                name, start = m.group(1), i
        elif l.startswith(".Lfunc_end"):
            out[name] = lines[start:i + 1]
            name = None
    return out


def resource_block(lines):
    """the lines from .amdhsa_kernel to .end_amdhsa_kernel: registers, scratch, LDS and the other launch figures"""
    start = next((i for i, l in enumerate(lines) if _KERNEL.match(l)), len(lines))
    end = next((i for i in range(start, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel"), len(lines) - 1)
    return lines[start:end + 1]


def instruction_lines(lines):
    """what is neither blank, a label, a directive nor a comment, without its trailing comment"""
    out = []
    for l in lines:
        l = l.split(";")[0].strip()
        if l and not l.startswith(".") and not l.endswith(":"):
            out.append(l)
    return out


def difference_summary(a, b):
    """How far apart two differing kernels are.  The multiset difference counts lines without regard to their order: a
    reordering alone gives 0, one changed line (say, the operands of a commutative instruction swapped) gives 2."""
    same = "identical" if resource_block(a) == resource_block(b) else "DIFFERENT"
    ca, cb = Counter(a), Counter(b)
    moved = sum(((ca - cb) + (cb - ca)).values())
    return (f".amdhsa_kernel block {same}; instructions {len(instruction_lines(a))} | {len(instruction_lines(b))}; "
            f"multiset difference {moved} lines")


def main(argv):
    if len(argv) != 3:
        print(__doc__)
        return 2
    a_dir, b_dir = argv[1], argv[2]
    a_files = {f for f in os.listdir(a_dir) if f.endswith(".s")}
    b_files = {f for f in os.listdir(b_dir) if f.endswith(".s")}
    bad = False
    for f in sorted(a_files ^ b_files):
        print(f"{f}: only in {a_dir if f in a_files else b_dir}")
        bad = True
    for f in sorted(a_files & b_files):
        a, b = kernels(os.path.join(a_dir, f)), kernels(os.path.join(b_dir, f))
        differ = [k for k in sorted(a.keys() & b.keys()) if a[k] != b[k]]
        print(f"{f}: {len(a)} | {len(b)} kernels, {len(a.keys() & b.keys())} in both, {len(differ)} differ")
        for k in sorted(a.keys() - b.keys()):
            print(f"  only in {a_dir}: {k}")
        for k in sorted(b.keys() - a.keys()):
            print(f"  only in {b_dir}: {k}")
        for k in differ:
            bad = True
            print(f"  DIFFERS: {k}")
            print("    " + difference_summary(a[k], b[k]))
            for l in list(difflib.unified_diff(a[k], b[k], "a", "b", n=1, lineterm=""))[:40]:
                print("    " + l)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
