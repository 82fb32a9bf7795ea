#!/usr/bin/env python3
"""sha256 over csrc/solve/*.hpp, the files window_solve.hip includes: every file's name and contents, sorted by name.  bench.py's
kernel_source_sha256() does not see them; scripts/gpu_profile.sh stores this hash beside it and tests/test_bench_launch.py compares."""
import hashlib
import os

SOLVE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anticipated-vins-mono_amd", "csrc", "solve")


def solve_parts_sha256():
    h = hashlib.sha256()
    for f in sorted(f for f in os.listdir(SOLVE) if f.endswith(".hpp")):
        h.update(f.encode() + b"\0")
        h.update(open(os.path.join(SOLVE, f), "rb").read())
    return h.hexdigest()


if __name__ == "__main__":
    print(solve_parts_sha256())
