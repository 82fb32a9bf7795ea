"""Serial trips to spill memory in the bodies of the solve and marginalization kernels (CPU tier: cross-compiles csrc/window_solve.hip
for gfx950 in its three builds with csrc/Makefile's flags, no GPU needed).

A wavefront reduction written with __shfl_xor is a ladder of ds_bpermute_b32 whose per-lane address registers the compiler hoists out of
the kernel's loops; in these kernels, which use the whole register file, it spilled them, and every step of every reduction of the
trust-region loop then began with a `scratch_load_dword ... s_waitcnt vmcnt(0)` in front of the permute - a dependent round trip to
memory per step, in no source line.  devmath.hpp's lane_xor / lane_swap carry the lane pattern as an immediate instead; the address of
the reductions' LDS counter is recomputed at every reduction (red_counter) and the loop's own FP64 scalars live in scalar registers (uni).  The scan
(scripts/isa_spill_trips.py) asserts per kernel body that
  - no lane-exchange instruction takes a VGPR operand that a scratch load wrote last in front of it (same basic block), and
  - the number of reload trips (an s_waitcnt vmcnt with a scratch load outstanding) stays at or below the count reached with
    those three changes.  Before that: 135 / 183 / 85 trips in the throughput / latency / extended solve bodies, 130 / 130 / 0
    permutes fed by a reload; 92 / 19 trips in the two marginalization bodies.
The caps belong to ROCm 7.2 with every option csrc/Makefile probes for; a toolchain that allocates registers differently may need new ones.
"""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"

# build -> {kernel: cap on the reload trips of its body}
CAPS = {
    "-DAVM_TP=1": {"window_solve_tp_kernel": 53, "marginalize_tp_kernel": 92},
    "": {"window_solve_kernel": 85, "marginalize_kernel": 19},
    "-DAVM_X=1": {"window_solve_x_kernel": 53},
}


def _scanner():
    spec = importlib.util.spec_from_file_location("isa_spill_trips", os.path.join(ROOT, "scripts", "isa_spill_trips.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_the_scanner_reports_planted_trips_and_a_planted_fed_permute():
    T = _scanner()
    disasm = """
0000000000001000 <_ZN3avm6kernelE>:
	scratch_load_dword v3, off, off offset:16
	scratch_load_dword v4, off, off offset:20
	s_waitcnt vmcnt(0)
	ds_bpermute_b32 v5, v3, v6
	v_mov_b32_e32 v4, v7
	v_mov_b32_dpp v8, v4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf
	s_waitcnt lgkmcnt(0)
	scratch_load_dwordx2 v[10:11], off, off offset:24
	s_cbranch_scc1 L0
	s_waitcnt vmcnt(0)
	v_permlane32_swap_b32_e32 v10, v12
0000000000001100 <L0>:
	scratch_load_dword v20, off, off offset:32
	s_waitcnt vmcnt(0) lgkmcnt(0)
	v_add_f64_dpp v[22:23], v[20:21], v[24:25] row_newbcast:1 row_mask:0xf bank_mask:0xf
0000000000002000 <_ZN3avm5otherE>:
	scratch_load_dword v3, off, off offset:16
	s_waitcnt vmcnt(0)
"""
    st = T.scan(disasm, "kernel")
    assert list(st) == ["_ZN3avm6kernelE"]
    st = st["_ZN3avm6kernelE"]
    # trips: the first wait (two loads, one trip) and the one in L0; the wait behind the branch has nothing outstanding in its own block
    assert (st["instructions"], st["scratch_loads"], st["trips"]) == (14, 4, 2)
    # fed: the permute's address (v3) and the DPP source in L0 (v20); not fed: v4 (overwritten since), v10 (reloaded in another block)
    assert [f[1].split(" ")[0] for f in st["fed"]] == ["ds_bpermute_b32", "v_add_f64_dpp"]


@pytest.mark.parametrize("defs", list(CAPS))
def test_no_lane_exchange_waits_for_a_spill_reload_and_the_trips_stay_capped(defs):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    T = _scanner()
    co = T.build_co("window_solve.hip", [defs] if defs else [])
    disasm = T.disassemble(co)
    for kernel, cap in CAPS[defs].items():
        found = T.scan(disasm, kernel)
        assert len(found) == 1, (kernel, list(found))
        (st,) = found.values()
        print("%s: instructions %d, scratch loads %d, reload trips %d (cap %d), lane exchanges fed by a reload %d" % (
            kernel, st["instructions"], st["scratch_loads"], st["trips"], cap, len(st["fed"])))
        assert not st["fed"], "%s: %d lane exchanges start with a trip to scratch memory, e.g. %s" % (kernel, len(st["fed"]), st["fed"][:3])
        assert st["trips"] <= cap, "%s: %d reload trips in the kernel body, were %d" % (kernel, st["trips"], cap)
