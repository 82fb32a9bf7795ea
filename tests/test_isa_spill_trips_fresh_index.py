"""Serial trips to spill memory in the bodies of the three solve kernels after the bodies stopped keeping thread-derived values (CPU
tier: cross-compiles csrc/window_solve.hip for gfx950 in its three builds with csrc/Makefile's flags, like tests/test_isa_spill_trips.py;
no GPU needed).

What the bodies do now (second part; csrc/solve/lds.hpp, csrc/solve/solve_kernel.hpp):
  - every segment takes a fresh, opaque thread index (fresh_tid / fresh_lane / fresh_wave): nothing derived from threadIdx.x is hoisted
    out of the trust-region loop or the window loop, kept live across the outlined phases, spilled and reloaded at its use;
  - the speculation's parking address comes from the LDS context at every use;
  - the loop's branches are decided in scalar registers (the options from the kernel arguments, uni() on what an outlined phase returns)
    and its FP64 scalars are carried as two 32-bit halves (unid), so that they are merged in scalar registers too.
Caps, per kernel body: the counts reached with that (ROCm 7.2, every option csrc/Makefile probes for), each at or below what laundering
the index at six points of the loop alone reached (37 / 33 / 28 trips, 55 / 48 / 43 scratch loads).  The instruction counts are capped
by the bodies' counts BEFORE the change: a fresh index costs a few VALU instructions where it is taken and must not cost more than the
reloads it removes.  Inside the source range of the trust-region loop (its lambdas, the first evaluation, the loop) no trip is left:
what remains is once per window - the context's hand-over to LDS (lds_store_ctx) and R2q's run-time indexed v[3] of the gauge fix,
which is a private array, not a spill.
"""
import importlib.util
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SOLVE_KERNEL = os.path.join(ROOT, "anticipated-vins-mono_amd", "csrc", "solve", "solve_kernel.hpp")

# build -> (kernel, cap on reload trips, cap on scratch loads, instructions of the body before the change)
CAPS = {
    "-DAVM_TP=1": ("window_solve_tp_kernel", 13, 24, 7868),
    "": ("window_solve_kernel", 13, 21, 7970),
    "-DAVM_X=1": ("window_solve_x_kernel", 10, 18, 11496),
}
LOOP_TRIPS_CAP = 0  # reload trips the line table puts between the two markers below, every build


def _scanner():
    spec = importlib.util.spec_from_file_location("isa_spill_trips", os.path.join(ROOT, "scripts", "isa_spill_trips.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _loop_range():
    """solve_kernel.hpp from the head of the TrustRegionMinimizer section (the lambdas the loop calls are defined there) to the line in
    front of the gauge fix"""
    lines = open(SOLVE_KERNEL).read().split("\n")
    first = [i for i, l in enumerate(lines, 1) if re.search(r"// -+ TrustRegionMinimizer -+", l)]
    last = [i for i, l in enumerate(lines, 1) if re.search(r"// -+ double2vector \+ vector2double", l)]
    assert len(first) == 1 and len(last) == 1 and first[0] < last[0], (first, last)
    assert any("while (true) {" in l for l in lines[first[0]:last[0]])
    return "solve_kernel.hpp", first[0], last[0] - 1


def test_the_range_option_counts_only_what_the_line_table_puts_in_the_range():
    T = _scanner()
    disasm = """
0000000000001000 <_ZN3avm6kernelE>:
; /src/csrc/./solve/solve_kernel.hpp:10
	scratch_load_dword v3, off, off offset:16
	s_waitcnt vmcnt(0)
; /src/csrc/./solve/solve_kernel.hpp:20
	scratch_load_dword v4, off, off offset:20
; /src/csrc/./solve/lds.hpp:25
	s_waitcnt vmcnt(0)
; /src/csrc/./solve/solve_kernel.hpp:30
	scratch_load_dword v5, off, off offset:24
	s_waitcnt vmcnt(0)
	ds_bpermute_b32 v6, v5, v7
"""
    assert T.parse_range("solve/solve_kernel.hpp:20:30") == ("solve_kernel.hpp", 20, 30)
    (st,) = T.scan(disasm, "kernel").values()
    assert (st["instructions"], st["scratch_loads"], st["trips"], len(st["fed"])) == (7, 3, 3, 1)
    # lines 20..30: the load of line 20 (its wait stands in another file: not a trip of the range) and the load, trip and fed permute of line 30
    (st,) = T.scan(disasm, "kernel", ("solve_kernel.hpp", 20, 30)).values()
    assert (st["instructions"], st["scratch_loads"], st["trips"], len(st["fed"])) == (4, 2, 1, 1)
    (st,) = T.scan(disasm, "kernel", ("solve_kernel.hpp", 1, 10)).values()
    assert (st["instructions"], st["scratch_loads"], st["trips"], len(st["fed"])) == (2, 1, 1, 0)
    (st,) = T.scan(disasm, "kernel", ("lds.hpp", 1, 100)).values()
    assert (st["instructions"], st["scratch_loads"], st["trips"], len(st["fed"])) == (1, 0, 1, 0)


@pytest.mark.parametrize("defs", list(CAPS))
def test_the_solve_bodies_keep_no_thread_derived_value_in_spill_memory(defs):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    T = _scanner()
    kernel, trips, loads, instructions_before = CAPS[defs]
    found = T.scan(T.disassemble(T.build_co("window_solve.hip", [defs] if defs else [])), kernel)
    assert len(found) == 1, (kernel, list(found))
    (st,) = found.values()
    print("%s: instructions %d (were %d), scratch loads %d (cap %d), reload trips %d (cap %d), lane exchanges fed by a reload %d" % (
        kernel, st["instructions"], instructions_before, st["scratch_loads"], loads, st["trips"], trips, len(st["fed"])))
    assert not st["fed"], "%s: %d lane exchanges start with a trip to scratch memory, e.g. %s" % (kernel, len(st["fed"]), st["fed"][:3])
    assert st["trips"] <= trips, "%s: %d reload trips in the kernel body, were %d" % (kernel, st["trips"], trips)
    assert st["scratch_loads"] <= loads, "%s: %d scratch loads in the kernel body, were %d" % (kernel, st["scratch_loads"], loads)
    assert st["instructions"] <= instructions_before, "%s: %d instructions in the kernel body, %d before the fresh indices" % (
        kernel, st["instructions"], instructions_before)


@pytest.mark.parametrize("defs", list(CAPS))
def test_no_reload_trip_inside_the_trust_region_loop(defs):
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc on this machine")
    T = _scanner()
    kernel = CAPS[defs][0]
    rng = _loop_range()
    found = T.scan(T.disassemble_with_lines("window_solve.hip", [defs] if defs else []), kernel, rng)
    assert len(found) == 1, (kernel, list(found))
    (st,) = found.values()
    print("%s, %s:%d..%d: instructions %d, scratch loads %d, reload trips %d (cap %d)" % ((kernel,) + rng + (
        st["instructions"], st["scratch_loads"], st["trips"], LOOP_TRIPS_CAP)))
    assert st["instructions"] > 1000, "the line table no longer attributes the loop to %s:%d..%d" % rng
    assert not st["fed"]
    assert st["trips"] <= LOOP_TRIPS_CAP, "%s: %d reload trips inside the trust-region loop's source range" % (kernel, st["trips"])
