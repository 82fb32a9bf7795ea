#!/usr/bin/env python3
"""Is the device code of every device translation unit the same as at another revision?  (cross-compiles, no GPU needed; needs
the git history)

    scripts/isa_same.py REV          (e.g. HEAD, HEAD~1, main)
    scripts/isa_same.py REV --functions [REGEX]
                                     (the six solve builds function by function, for a change that is meant to touch some functions only:
                                      one line per build with the functions that differ; exit status 1 if one differs whose symbol does not
                                      match REGEX.  See function_texts() for what is normalised.)

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
import re
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


GETPC_ADD = re.compile(r"^(s_add_u32|s_addc_u32)\b")


def function_texts(csrc, src, defs):
    """{symbol: sha256 of the function's instructions} of one build.  Addresses are dropped, branch targets are the disassembler's
    labels renumbered per function, and the literals of the s_add_u32 / s_addc_u32 pair behind an s_getpc_b64 (the distance to a callee or a table,
    which moves with every function laid out in between) are masked: a function whose own instructions did not change hashes the same
    wherever it ends up in .text."""
    co = build_co(src, defs, csrc)
    txt = subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--symbolize-operands", co], text=True)
    shutil.rmtree(os.path.dirname(co))
    out, cur, after_getpc = {}, None, 0
    for l in txt.split("\n"):
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", l)
        if m:
            if re.match(r"^(L\d+|.*\+0x[0-9a-f]+)$", m.group(1)):
                cur.append("<%s>:" % m.group(1)) if cur is not None else None
            else:
                cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not l.strip():
            continue
        insn = l.split("//")[0].strip()
        if insn.startswith("s_getpc_b64"):
            after_getpc = 2
        elif after_getpc and GETPC_ADD.match(insn):
            insn, after_getpc = ",".join(insn.split(",")[:2]) + ", <pc-relative>", after_getpc - 1
        cur.append(insn)
    def renumbered(lines):  # the disassembler numbers its labels through the whole section: here in the order the function mentions them
        # (a label no instruction of the function refers to is some other instruction's literal read as a target: dropped)
        used = set(re.findall(r"\bL\d+\b", "\n".join(l for l in lines if not l.startswith("<"))))
        lines = [l for l in lines if not l.startswith("<") or l[1:-2] in used]
        while lines and lines[-1] in ("s_nop 0", "s_code_end"):  # padding up to the next aligned symbol: as long as the layout leaves it
            lines.pop()
        order = {}
        return re.sub(r"\bL\d+\b", lambda m: "L#%d" % order.setdefault(m.group(0), len(order)), "\n".join(lines))

    return {f: hashlib.sha256(renumbered(t).encode()).hexdigest() for f, t in out.items()}


def compare_functions(sides, allow):
    """per build: the functions whose instructions differ between the two sides, apart from those whose symbol matches `allow`"""
    builds = [b for b in BUILDS if b[1] == "window_solve.hip"]
    with concurrent.futures.ThreadPoolExecutor(8) as ex:
        jobs = {(b, i): ex.submit(function_texts, side, src, defs) for b, src, defs in builds for i, side in enumerate(sides)}
        res = {k: j.result() for k, j in jobs.items()}
    bad = 0
    for b, _, _ in builds:
        old, new = res[(b, 0)], res[(b, 1)]
        changed = sorted(f for f in set(old) | set(new) if old.get(f) != new.get(f))
        expected = [f for f in changed if allow and re.search(allow, f)]
        other = [f for f in changed if f not in expected]
        bad += len(other)
        print("%-15s %d functions, %d the same, changed as allowed: %s%s" % (
            b, len(set(old) | set(new)), len(set(old) & set(new)) - len([f for f in changed if f in old and f in new]),
            ", ".join(expected) or "none", "; CHANGED: " + ", ".join(other) if other else ""))
    return bad


def main():
    args = sys.argv[1:]
    allow = None
    if "--functions" in args:  # scripts/isa_same.py REV --functions [REGEX]: per function of the solve builds; REGEX: the symbols that may differ
        i = args.index("--functions")
        allow = args[i + 1] if len(args) > i + 1 else ""
        del args[i:i + 2]
    if len(args) != 1 or args[0].startswith("-"):
        sys.exit(__doc__)
    rev = args[0]
    rel = os.path.relpath(CSRC, ROOT)
    if allow is not None:
        with tempfile.TemporaryDirectory() as tmp:
            tar = subprocess.check_output(["git", "archive", rev, rel, "include"], cwd=ROOT)
            tarfile.open(fileobj=io.BytesIO(tar)).extractall(tmp)
            sys.exit(1 if compare_functions([os.path.join(tmp, rel), CSRC], allow) else 0)
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
