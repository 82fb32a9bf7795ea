"""The DPP wait states of the selector's code object (CPU tier: cross-compiles csrc/fsel.hip, i.e. the parts under csrc/fsel/, for gfx950, no GPU needed).

A DPP instruction reads its DPP source - its first source operand - correctly only if no VALU instruction has written that VGPR within the
two wait states before it.  The compiler's hazard recognizer does not look inside inline assembly, and the selector's elimination issues
its v_fmac_f64_dpp runs from inline assembly (fs_fmac_bcast, fsel/dpp.hpp) with separate `s_nop 1` statements (fs_dpp_fence) for the wait
states: the scheduler may move other instructions between such a fence and its run, so only the compiled code can show that the rule holds.
The scan is per basic block: `s_nop N` counts as N + 1 wait states, any other instruction as one.
(window_solve.hip's back substitution carries its `s_nop 1` inside the same asm statement as each v_fmac_f64_dpp: safe by construction.)
"""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "anticipated-vins-mono_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"
OBJDUMP = "/opt/rocm/llvm/bin/llvm-objdump"

HEADER = re.compile(r"^[0-9a-f]+ <([^>]+)>:")  # a function or a label (--symbolize-operands): the start of a basic block
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
    # (the DPP controls follow the operands after a space: "v_mov_b32_dpp v1, v2 quad_perm:[1,0,3,2] row_mask:0xf ...")
    return [o.strip().split(" ")[0] for o in rest.strip().split(",")] if rest.strip() else []


def dpp_source(ops):
    """the VGPRs of the first source operand: the first VGPR operand after the destination (VOPC / carry forms name vcc in between)"""
    for o in ops[1:]:
        r = vgprs(o)
        if r:
            return r
    return set()


def wait_states(op, ops):
    return int(ops[0], 0) + 1 if op == "s_nop" else 1


def scan(disasm):
    """[(block, dpp instruction, writer)] for every DPP instruction whose DPP source a VALU instruction of the same basic block wrote
    within the two wait states before it; and the number of DPP instructions checked per opcode"""
    hazards, seen = [], {}
    block, insns = None, []
    for line in disasm.split("\n"):
        h = HEADER.match(line)
        if h:
            block, insns = h.group(1), []
            continue
        m = INSN.match(line)
        if not m or block is None:
            continue
        op, ops = m.group(1), operands(m.group(2))
        if op.endswith("_dpp"):
            seen[op] = seen.get(op, 0) + 1
            src, ws = dpp_source(ops), 0
            for pop, pops, ptext in reversed(insns):
                if ws >= 2:
                    break
                if pop.startswith("v_") and pops and vgprs(pops[0]) & src:
                    hazards.append((block, line.strip(), ptext))
                ws += wait_states(pop, pops)
        insns.append((op, ops, line.strip()))
        if op.startswith(BLOCK_END):
            block, insns = block + "'", []
    return hazards, seen


def test_the_scanner_reports_a_planted_hazard():
    disasm = """
0000000000001000 <kernel>:
	v_mov_b32_e32 v3, v4
	v_mov_b32_dpp v5, v3 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf
	v_fma_f64 v[12:13], v[0:1], v[2:3], v[12:13]
	s_nop 0
	v_fmac_f64_dpp v[20:21], v[12:13], v[6:7] row_newbcast:1 row_mask:0xf bank_mask:0xf
	v_add_f64 v[30:31], v[0:1], v[2:3]
	s_nop 1
	v_fmac_f64_dpp v[22:23], v[30:31], v[6:7] row_newbcast:2 row_mask:0xf bank_mask:0xf
	v_mul_f64 v[40:41], v[0:1], v[2:3]
	s_cbranch_scc1 L0
	v_fmac_f64_dpp v[24:25], v[40:41], v[6:7] row_newbcast:3 row_mask:0xf bank_mask:0xf
	v_mov_b32_e32 v8, 0
	v_fmac_f64_dpp v[8:9], v[40:41], v[6:7] row_newbcast:4 row_mask:0xf bank_mask:0xf
0000000000001100 <L0>:
	v_fmac_f64_dpp v[26:27], v[40:41], v[6:7] row_newbcast:5 row_mask:0xf bank_mask:0xf
"""
    hazards, seen = scan(disasm)
    # planted: a write right behind (v3), and a 64-bit source one wait state behind its write (v[12:13]); not hazards: two wait states
    # (s_nop 1), a write in another basic block, a write of the accumulator rather than the DPP source
    assert [(h[0], h[1].split(" ")[0], h[2]) for h in hazards] == [
        ("kernel", "v_mov_b32_dpp", "v_mov_b32_e32 v3, v4"), ("kernel", "v_fmac_f64_dpp", "v_fma_f64 v[12:13], v[0:1], v[2:3], v[12:13]")]
    assert seen == {"v_mov_b32_dpp": 1, "v_fmac_f64_dpp": 5}


def test_the_selector_code_object_keeps_the_dpp_wait_states(tmp_path):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    mk = open(os.path.join(CSRC, "Makefile")).read()
    flags = re.search(r"^FLAGS \?= (.*)$", mk, re.M).group(1).replace("$(ARCH)", "gfx950").split()
    co = str(tmp_path / "fsel.co")
    subprocess.check_call([HIPCC] + flags + ["--offload-device-only", "--no-gpu-bundle-output", "-c", "fsel.hip", "-o", co], cwd=CSRC)
    disasm = subprocess.check_output([OBJDUMP, "-d", "--no-show-raw-insn", "--symbolize-operands", co], text=True)
    hazards, seen = scan(disasm)
    assert seen.get("v_fmac_f64_dpp", 0) > 0, seen  # (the elimination's runs are there, so the check covers them)
    assert not hazards, "%d DPP reads within two wait states of a VALU write of their source, e.g. %s" % (len(hazards), hazards[:5])
