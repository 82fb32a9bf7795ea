#!/usr/bin/env python3
"""Serial trips to spill memory in a kernel body (cross-compiles, no GPU needed):

    scripts/isa_spill_trips.py window_solve.hip window_solve_tp_kernel -DAVM_TP=1
    scripts/isa_spill_trips.py window_solve.hip marginalize_tp_kernel -DAVM_TP=1 --lines      (per source line, 20-line buckets)
    scripts/isa_spill_trips.py window_solve.hip window_solve_tp_kernel -DAVM_TP=1 --range solve_kernel.hpp:466:748
                                                                                              (only what the line table puts in that range of
                                                                                               that file, e.g. the trust-region loop; implies the
                                                                                               line-table build of --lines)

Per kernel (the function whose symbol contains the name; outlined callees are functions of their own and are not counted):
    scratch loads   scratch_load_* instructions
    reload trips    an `s_waitcnt` with a vmcnt field that has a scratch load outstanding in front of it in the same basic block: the
                    wavefront stands still for one round trip to memory there, however many reloads that wait retires
    fed cross-lane  lane-exchange instructions (ds_bpermute / ds_permute / ds_swizzle, any *_dpp, v_permlane*) one of whose VGPR
                    operands was last written, in the same basic block, by a scratch load: the exchange starts with a trip to memory.
                    (v_readlane / v_writelane are how SGPR spills travel: scripts/isa_sgpr_reloads.py counts those.)
"""
import collections
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_mix import LLVM, build_co  # noqa: E402

FUNC = re.compile(r"^[0-9a-f]+ <([^>]+)>:")
LABEL = re.compile(r"^[0-9a-f]+ <(L\d+|[^>]+\+0x[0-9a-f]+)>:")
SRCLINE = re.compile(r"^; (\S+):(\d+)")
INSN = re.compile(r"^\s+([a-z][a-z0-9_]+)\b([^/]*)")
VREG = re.compile(r"^v(\d+)$|^v\[(\d+):(\d+)\]$")
BLOCK_END = ("s_branch", "s_cbranch_", "s_setpc", "s_swappc", "s_endpgm")


def vgprs(operand):
    m = VREG.match(operand.strip())
    if not m:
        return set()
    if m.group(1) is not None:
        return {int(m.group(1))}
    return set(range(int(m.group(2)), int(m.group(3)) + 1))


def operands(rest):
    return [o.strip().split(" ")[0] for o in rest.strip().split(",")] if rest.strip() else []


def is_lane_exchange(op):
    return op.endswith("_dpp") or op.startswith("v_permlane") or op.startswith(("ds_bpermute", "ds_permute", "ds_swizzle"))


def writes_vgprs(op, ops):
    """the VGPRs an instruction writes: the first operand of VALU instructions and of loads (DS / scratch / global / flat / buffer)"""
    if not ops:
        return set()
    if op.startswith("v_") and not op.startswith(("v_cmp", "v_readlane", "v_readfirstlane")):
        w = vgprs(ops[0])
        if op.startswith("v_permlane") and op.endswith("_swap_b32") and len(ops) > 1:
            w |= vgprs(ops[1])
        return w
    if op.startswith(("ds_read", "ds_bpermute", "ds_permute", "ds_swizzle", "ds_consume", "ds_append")) or "_load_" in op or "_atomic_" in op:
        return vgprs(ops[0])
    return set()


def scan(disasm, kernel, src_range=None):
    """{function: dict(instructions, scratch_loads, trips, fed=[(source line, instruction, reload)], trip_lines=Counter, load_lines=Counter)}
    for every function of the disassembly (llvm-objdump -d [-l] --symbolize-operands) whose symbol contains `kernel`.
    src_range = (file name, first line, last line): count only the instructions the line table (-l) attributes to that range - a trip where
    its wait stands, a fed exchange where the exchange stands; what is outstanding or reloaded is still followed through the whole function."""
    def inside(ln):
        return src_range is None or (ln is not None and ln[0] == src_range[0] and src_range[1] <= ln[1] <= src_range[2])

    res = {}
    cur = st = None
    line = None
    reloaded, outstanding = {}, 0  # per basic block: VGPR -> text of the scratch load that wrote it last; scratch loads not yet waited for
    for l in disasm.split("\n"):
        m = FUNC.match(l)
        if m:
            if not LABEL.match(l):
                cur = m.group(1)
                st = res.setdefault(cur, dict(instructions=0, scratch_loads=0, trips=0, fed=[], trip_lines=collections.Counter(),
                                              load_lines=collections.Counter())) if kernel in cur else None
            reloaded, outstanding = {}, 0
            continue
        m = SRCLINE.match(l)
        if m:
            line = (m.group(1).split("/")[-1], int(m.group(2)))
            continue
        m = INSN.match(l)
        if not m or st is None:
            continue
        op, ops = m.group(1), operands(m.group(2))
        counted = inside(line)
        st["instructions"] += counted
        bucket = (line[0], line[1] // 20 * 20) if line else None
        if is_lane_exchange(op):
            for o in ops[1:]:
                hit = [reloaded[r] for r in vgprs(o) if r in reloaded]
                if hit:
                    if counted:
                        st["fed"].append((line, l.strip(), hit[0]))
                    break
        if op == "s_waitcnt" and "vmcnt" in m.group(2) and outstanding:
            st["trips"] += counted
            st["trip_lines"][bucket] += counted
            outstanding = 0
        for r in writes_vgprs(op, ops):
            reloaded.pop(r, None)
        if op.startswith("scratch_load"):
            st["scratch_loads"] += counted
            st["load_lines"][bucket] += counted
            outstanding += 1
            for r in vgprs(ops[0]):
                reloaded[r] = l.strip()
        if op.startswith(BLOCK_END):
            reloaded, outstanding = {}, 0
    return res


def disassemble(co, lines=False):
    return subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", "--symbolize-operands"] + (["-l"] if lines else []) + [co], text=True)


def parse_range(text):
    """'solve_kernel.hpp:466:748' -> ('solve_kernel.hpp', 466, 748)"""
    f, lo, hi = text.rsplit(":", 2)
    return os.path.basename(f), int(lo), int(hi)


def disassemble_with_lines(src, defs):
    """the line-table build of scripts/isa_lines.py (the Makefile's flags plus -gline-tables-only), disassembled with source lines"""
    from isa_lines import build
    return disassemble(build(src, defs), True)


def main():
    argv, src_range = sys.argv[1:], None
    if "--range" in argv:
        i = argv.index("--range")
        src_range = parse_range(argv[i + 1])
        del argv[i:i + 2]
    args = [a for a in argv if a != "--lines"]
    lines = "--lines" in argv or src_range is not None
    src, kernel, defs = args[0], args[1], args[2:]
    disasm = disassemble_with_lines(src, defs) if lines else disassemble(build_co(src, defs))
    if src_range:
        print("only %s:%d..%d" % src_range)
    for f, st in scan(disasm, kernel, src_range).items():
        print("%s: instructions %d, scratch loads %d, reload trips %d, lane exchanges fed by a reload %d" % (
            f, st["instructions"], st["scratch_loads"], st["trips"], len(st["fed"])))
        for ln, insn, rel in st["fed"][:20]:
            print("  fed: %s  <-  %s%s" % (insn, rel, "   (%s:%d)" % ln if ln else ""))
        if lines:
            for k in sorted(set(st["trip_lines"]) | set(st["load_lines"]), key=lambda k: (k is None, k)):
                print("  %s:%d.. loads %d trips %d" % (k[0], k[1], st["load_lines"][k], st["trip_lines"][k]) if k else
                      "  (no line) loads %d trips %d" % (st["load_lines"][k], st["trip_lines"][k]))


if __name__ == "__main__":
    main()
