#!/usr/bin/env python3
"""sha256 over csrc/solve/*.hpp, the files window_solve.hip includes, and the same over csrc/fsel/*.hpp, which fsel.hip includes: every
file's name and contents, sorted by name.  bench.py's kernel_source_sha256() does not see them; scripts/gpu_profile.sh stores these
hashes beside it and tests/test_bench_launch.py compares.  Prints the solve parts' hash, or with the argument `fsel` the selector parts'."""
import hashlib
import os
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anticipated-vins-mono_amd", "csrc")


def _parts_sha256(folder):
    h = hashlib.sha256()
    for f in sorted(f for f in os.listdir(os.path.join(CSRC, folder)) if f.endswith(".hpp")):
        h.update(f.encode() + b"\0")
        h.update(open(os.path.join(CSRC, folder, f), "rb").read())
    return h.hexdigest()


def solve_parts_sha256():
    return _parts_sha256("solve")


def fsel_parts_sha256():
    return _parts_sha256("fsel")


if __name__ == "__main__":
    print(fsel_parts_sha256() if sys.argv[1:] == ["fsel"] else solve_parts_sha256())
