#!/usr/bin/env python3
"""Is the device code of every device translation unit the same as at another revision?  (cross-compiles, no GPU needed; needs
the git history)

    scripts/isa_same.py REV          (e.g. HEAD, HEAD~1, main)

Builds window_solve.hip three ways (latency, -DAVM_X=1, -DAVM_TP=1), each once more over a window list (-DAVM_WIN_LIST=1), and fsel.hip, prior_eig.hip, preint.hip, triangulate.hip and
visual_align.hip (the Makefile's plain FLAGS) with
scripts/isa_mix.py's build_co() (csrc/Makefile's flags for that build plus --cuda-device-only) from `git archive REV` of csrc/ and include/ in a temporary directory and from the working tree, dumps the
gfx950 code objects' .text, .rodata and .note sections (.note: every kernel's registers, spills, LDS and scratch) and prints one line
per build and section with both sha256 hashes.  Exit status 1 on any difference.  (.dynstr / .strtab carry a string derived from the
source file's name and are not compared.)  A build whose macro REV's sources do not know yet is reported as "new" and not compared.

The check of every refactor of the kernels and of the helpers they share (devmath.hpp): the compiler is deterministic and blind to how the source is cut into files, so a
change that moves no instruction gives the same bytes.
"""
import concurrent.futures
import hashlib
import io
import os
import shutil
import subprocess
import sys
import tarfile
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import CSRC, LLVM, ROOT, build_co  # noqa: E402

BUILDS = [("latency", "window_solve.hip", []), ("extended", "window_solve.hip", ["-DAVM_X=1"]), ("throughput", "window_solve.hip", ["-DAVM_TP=1"]),
          ("latency_list", "window_solve.hip", ["-DAVM_WIN_LIST=1"]), ("extended_list", "window_solve.hip", ["-DAVM_X=1", "-DAVM_WIN_LIST=1"]),
          ("throughput_list", "window_solve.hip", ["-DAVM_TP=1", "-DAVM_WIN_LIST=1"]),
          ("selector", "fsel.hip", []), ("prior_eig", "prior_eig.hip", []), ("preint", "preint.hip", []), ("triangulate", "triangulate.hip", []),
          ("visual_align", "visual_align.hip", [])]
SECTIONS = [".text", ".rodata", ".note"]


def section_hashes(csrc, src, defs):
    co = build_co(src, defs, csrc)
    out = {}
    for sec in SECTIONS:
        dump = co + sec
        subprocess.check_call([LLVM + "/llvm-objcopy", "--dump-section", "%s=%s" % (sec, dump), co])
        with open(dump, "rb") as f:
            out[sec] = hashlib.sha256(f.read()).hexdigest()
    shutil.rmtree(os.path.dirname(co))  # build_co()'s temporary directory, the dumps with it
    return out


def main():
    if len(sys.argv) != 2 or sys.argv[1].startswith("-"):
        sys.exit(__doc__)
    rev = sys.argv[1]
    rel = os.path.relpath(CSRC, ROOT)
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.check_output(["git", "archive", rev, rel, "include"], cwd=ROOT)
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
        sides = [os.path.join(tmp, rel), CSRC]
        # the -D macros REV's sources test: a build with another one would only repeat its parent build there
        old_src = "".join(open(os.path.join(d, f), errors="replace").read() for d, _, fs in os.walk(sides[0]) for f in fs)
        old_known = {d for _, _, defs in BUILDS for d in defs if d[2:].split("=")[0] in old_src}
        with concurrent.futures.ThreadPoolExecutor(8) as ex:
            jobs = {(b, i): ex.submit(section_hashes, side, src, defs) for b, src, defs in BUILDS for i, side in enumerate(sides)}
            res = {k: j.result() for k, j in jobs.items()}
    differ = 0
    for b, _, defs in BUILDS:
        if any(d not in old_known for d in defs):
            print("%-15s new: %s does not know %s" % (b, rev, " ".join(d for d in defs if d not in old_known)))
            continue
        for sec in SECTIONS:
            old, new = res[(b, 0)][sec], res[(b, 1)][sec]
            differ += old != new
            print("%-15s %-7s %s %s %s" % (b, sec, old[:16], new[:16], "same" if old == new else "DIFFERENT"))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
