"""Every exit of the trust-region minimizer and every option the solve kernels read, against the binary128 solve.

The solve kernels (csrc/solve/solve_kernel.hpp in its three builds) restate Ceres' trust-region minimizer and read almost every
field of avm_options; the other GPU tests run them at avm_default_options(), where only FUNCTION_TOL, NO_CONVERGENCE and (NaN inputs)
FAILURE ever occur and no IMU factor is ever dropped.  tests/solve_option_cases.py is a table of cases that reach the other exits
(GRADIENT_TOL, PARAMETER_TOL with its spec_restore(), MIN_RADIUS after an attempt and before the first), rejected steps under two
acceptance thresholds, both clamps of the Levenberg-Marquardt diagonal, jacobi_scaling = 0, another loss width and focal length, one
and sixteen iterations (the cost-only last iteration; the last slot of the traces and bit 15 of accept_mask), and IMU factors
that max_sum_dt drops next to factors that sit exactly at equality and stay.

CPU tier: each case is well-posed - the FP64 oracle takes the binary128 solve's decisions, a tolerance-driven exit does not move when
the tolerance moves by 1e-3 (it is not decided by rounding), and each case exercises what its table entry says.
GPU tier: case x build (latency, throughput; the extended kernel for the x_ cases): the device takes the binary128 decisions, its states
are within the 1e-6 contract of the binary128 states and within ten times the FP64 oracle's own distance (tests/test_solve_truth.py's
rule, per key and per window), its traces follow the binary128 traces, and what lies past num_iterations is zero.

Measured distances, device next to oracle: DESIGN.md section 2.4.1.
"""
import importlib

import numpy as np
import pytest

import solve_option_cases as cases
from helpers import abi, buffers, rel
from solve_option_cases import CASES, TERM, decisions, reference

est_m = importlib.import_module("anticipated-vins-mono_amd.estimator")
lib_m = importlib.import_module("anticipated-vins-mono_amd.lib")

STATE_TOL = cases.STATE_TOL                        # 1e-6: the contract (the floors of the 10 x oracle rule: cases.FLOOR, cases.state_bound)
COST_TRACE_TOL, RADIUS_TRACE_TOL = 1e-7, 1e-9     # test_solve_truth.py, test_solve_tp.py / test_small_trust_region_dogleg_branches_parity

# the cases the table must hold (a case that disappears from the table must fail here, not pass by absence)
REQUIRED = ["gradient_tol", "parameter_tol", "function_tol", "max_it_1", "max_it_16", "rejected", "min_rel_decrease", "min_radius",
            "min_radius_at_once", "jacobi_off", "lm_clamp", "loss_focal", "sum_dt_skip", "sum_dt_skip_noprior", "invalid_steps",
            "x_parameter_tol", "x_function_tol", "x_jacobi_off", "x_loss_focal", "x_sum_dt_skip", "x_max_it_1"]


def _rejects(s):
    """Per window: an attempt was evaluated and turned down (not the attempt an exit by a tolerance ends in, not an invalid step)."""
    out = []
    for i in range(len(s)):
        term, n = int(s["termination"][i]), int(s["num_iterations"][i])
        if term == TERM["FAILURE"]:
            n = 0
        elif term in (TERM["PARAMETER_TOL"], TERM["FUNCTION_TOL"]):
            n -= 1
        out.append(any(not (int(s["accept_mask"][i]) >> k) & 1 for k in range(n)))
    return np.array(out, bool)


def _trace_gap(s, t, key):
    """Worst window of: the first num_iterations entries of s[key] against t[key] (max |difference| over max |t|, helpers.rel)."""
    worst = 0.0
    for i in range(len(t)):
        n = int(t["num_iterations"][i])
        if n:
            worst = max(worst, rel(s[key][i][:n], t[key][i][:n]))
    return worst


# ---------------------------------------------------------------------------------------------------------------- CPU tier
def test_the_table_holds_every_case():
    assert sorted(CASES) == sorted(REQUIRED)
    assert sorted(cases.TOLERANCE_CASES) == sorted(["gradient_tol", "parameter_tol", "function_tol", "min_radius", "x_parameter_tol", "x_function_tol"])
    assert cases.windows("gradient_tol").a["n_feat"].tolist() == [24] * 4 + [33] * 4      # both sides of the 32-feature boundary


@pytest.mark.parametrize("name", REQUIRED)
def test_case_is_well_posed_and_exercises_what_it_says(oracle, name):
    """The FP64 oracle takes the binary128 solve's decisions (termination, num_iterations, num_successful, accept_mask of every window) and
    ends within the contract of it - so a device that decides otherwise, or ends further away, is wrong and not unlucky - and the binary128
    run shows what the case is in the table for."""
    c, R = CASES[name], reference(name)
    so, st = R["so"], R["st"]
    t = st if c.truth else so
    if c.truth:
        assert decisions(so) == decisions(st)
        gaps = {k: max(rel(R["wo"].a[k][i], R["wt"].a[k][i]) for i in range(len(st))) for k in cases.state_keys(name)}
        print(f"\n[{name}] oracle - binary128: " + " ".join(f"{k} {v:.1e}" for k, v in gaps.items())
              + f" | cost_trace {_trace_gap(so, st, 'cost_trace'):.1e} radius_trace {_trace_gap(so, st, 'radius_trace'):.1e}")
        assert max(gaps.values()) < STATE_TOL, gaps
    term, nit = np.asarray(t["termination"]), np.asarray(t["num_iterations"])
    ex = c.exercises
    for n in ex.get("terminations", ()):
        assert (term == TERM[n]).any(), (n, term.tolist())
    if "all_terminate" in ex:
        assert (term == TERM[ex["all_terminate"]]).all(), term.tolist()
    if "attempts" in ex:
        assert (nit == ex["attempts"]).all(), nit.tolist()
        assert (np.asarray(t["accept_mask"]) == (1 << ex["attempts"]) - 1).all()          # (every attempt accepted: 0x1, 0xff, 0xffff)
    if "rejected" in ex:
        assert _rejects(t).any() == ex["rejected"]
    if ex.get("rejected_past_32_features"):
        assert (_rejects(t) & (R["w"].a["n_feat"] > 32)).any() and (_rejects(t) & (R["w"].a["n_feat"] <= 32)).any()
    if ex.get("after_an_attempt"):
        assert (nit >= 1).all()
    if "differs_from" in ex:
        other = reference(ex["differs_from"])["st"]
        assert (np.asarray(t["accept_mask"]) != np.asarray(other["accept_mask"])).any()
        # ... because this threshold rejects attempts the other one accepts
        assert ((np.asarray(other["accept_mask"]) & ~np.asarray(t["accept_mask"])) != 0).any()
    if name == "invalid_steps":
        assert term.tolist() == [TERM["FAILURE"]] * 5 + [TERM["NO_CONVERGENCE"]] and nit.tolist() == [2] * 5 + [8]
    if name == "min_radius":
        # the radius that decides: the first halving of a window that rejects a step starts ABOVE the threshold and ends BELOW it, sqrt 2 each way
        i, k, before, after = cases.first_halving(st, R["opt"].initial_trust_region_radius)
        assert after < R["opt"].min_trust_region_radius < before and k == int(nit[i])
        assert abs(before / R["opt"].min_trust_region_radius - np.sqrt(2.0)) < 1e-12
    if name == "max_it_16":
        assert (np.asarray(t["cost_trace"])[:, 15] > 0).all() and (np.asarray(t["radius_trace"])[:, 15] > 0).all()


@pytest.mark.parametrize("name", cases.TRUTH_CASES)
def test_the_grading_of_a_case_is_not_decided_by_rounding(oracle, name):
    """The FP64 oracle with every input moved by -1, 0 or +1 unit in the last place (four draws; twelve for the windows started far from their minimum) takes the same decisions and stays within
    HALF of what the device is allowed (the 1e-6 contract; ten times the unperturbed oracle's distance per window and key, or the floor):
    the other half is left to an implementation that orders its operations differently.  A case that fails here grades one draw of
    rounding noise against another - its input has to change, not its bound."""
    worst, where, same = cases.oracle_scatter(name)
    print(f"\n[{name}] the oracle one ulp aside uses {worst:.2f} of the bound at (seed, key, window) {where}")
    assert same and worst <= 0.5, (worst, where)


@pytest.mark.parametrize("name", cases.TOLERANCE_CASES)
def test_a_tolerance_driven_exit_is_not_decided_by_rounding(oracle, name):
    """The binary128 decisions do not change when the tolerance that drives the exit is multiplied by 1 +- 1e-3: the quantity it is compared
    with is nowhere within 1e-3 of it, which is six orders of magnitude more than any FP64 evaluation of it is off."""
    R = reference(name)
    field = CASES[name].varied
    for f in (1.0 - 1e-3, 1.0 + 1e-3):
        _, s = cases.truth(R["w"], cases.options(name, **{field: getattr(R["opt"], field) * f}))
        assert decisions(s) == decisions(R["st"]), (field, f)


def test_the_cases_cover_every_exit_and_a_rejected_step(oracle):
    seen, rejected = set(), []
    for name in REQUIRED:
        R = reference(name)
        t = R["st"] if CASES[name].truth else R["so"]
        seen |= {abi.TERM_NAMES[v] for v in np.asarray(t["termination"]).tolist()}
        if _rejects(t).any():
            rejected.append(name)
    assert seen == set(abi.TERM_NAMES), seen
    assert "rejected" in rejected and "min_rel_decrease" in rejected
    for kind in ("", "x_"):   # the extended problem reaches the three exits it is graded on
        got = {abi.TERM_NAMES[v] for n in REQUIRED if n.startswith("x_") == bool(kind) for v in np.asarray(reference(n)["so"]["termination"]).tolist()}
        assert {"PARAMETER_TOL", "FUNCTION_TOL", "NO_CONVERGENCE"} <= got, (kind, got)


@pytest.mark.parametrize("name", cases.SUM_DT_CASES)
def test_max_sum_dt_drops_the_factors_the_case_names_and_keeps_the_ones_at_equality(oracle, name):
    """From the FP64 pre-integration's sum_dt: the stretched intervals lie above max_sum_dt (their factors are dropped), every other
    interval sits EXACTLY at it and stays (estimator.cpp:705 tests `<=`)."""
    want = CASES[name].exercises["skipped"]
    per_window = cases.skipped_factors(name)
    assert len(per_window) == cases.windows(name).n_windows
    for dropped, at_equality in per_window:
        assert dropped == want and at_equality == set(range(10)) - want
    # ... and the dropped factors matter: the solve differs from the one that keeps them
    R = reference(name)
    wo = R["w"].copy()
    oracle.window_solve(cases.options(name, max_sum_dt=10.0), wo, None, buffers.summary_alloc(wo.n_windows))
    assert min(rel(wo.a["speedbias"][i], R["wo"].a["speedbias"][i]) for i in range(wo.n_windows)) > 1e-6


# ---------------------------------------------------------------------------------------------------------------- GPU tier
BUILDS = [(n, b) for n in REQUIRED if not CASES[n].x for b in ("latency", "throughput")] + [(n, "extended") for n in REQUIRED if CASES[n].x]


def _device_solve(ctx, monkeypatch, name, build, w=None, opt=None):
    """The case's windows through the given build of the solve kernel; the summaries land in a buffer that held garbage."""
    R = reference(name)
    if build == "extended":
        monkeypatch.delenv("AVM_SOLVE_TP", raising=False)
    else:
        monkeypatch.setenv("AVM_SOLVE_TP", "1" if build == "throughput" else "0")
    wg = (R["w"] if w is None else w).copy()
    out = buffers.summary_alloc(wg.n_windows)
    out.view(np.uint8)[...] = 0xFF
    sg = buffers.summary_to_numpy(est_m.Estimator(ctx=ctx, options=R["opt"] if opt is None else opt).optimization(wg, summary_out=out)).copy()
    # (the extended problem has one kernel, which last_solve_form() reports as the latency form: tests/test_solve_tp.py)
    assert ctx.last_solve_form() == ("throughput" if build == "throughput" else "latency")
    return wg, sg


@pytest.mark.gpu
@pytest.mark.parametrize("name,build", [nb for nb in BUILDS if CASES[nb[0]].truth])
def test_device_against_the_binary128_solve(ctx, oracle, monkeypatch, name, build):
    R = reference(name)
    wg, sg = _device_solve(ctx, monkeypatch, name, build)
    st, so, wt, wo = R["st"], R["so"], R["wt"], R["wo"]
    B = len(st)
    # ---- decisions: the four summary fields, per window
    assert decisions(sg) == decisions(st)
    # ---- states: per key and per window, the rule of tests/test_solve_truth.py
    failed = []
    for k in cases.state_keys(name):
        go = [rel(wo.a[k][i], wt.a[k][i]) for i in range(B)]
        gg = [rel(wg.a[k][i], wt.a[k][i]) for i in range(B)]
        print(f"\n[{name} {build}] {k}: device - binary128 worst {max(gg):.1e} | oracle - binary128 worst {max(go):.1e}")
        for i in range(B):
            if not (gg[i] < STATE_TOL and gg[i] <= cases.state_bound(name, k, i)):
                failed.append((k, i, gg[i], go[i]))
    assert not failed, failed
    # ---- zero attempts: the gauge-fixed input, as the oracle returns it
    for i in np.flatnonzero(np.asarray(st["num_iterations"]) == 0):
        for k in cases.state_keys(name):
            assert rel(wg.a[k][i], wo.a[k][i]) <= 1e-13, (k, i)
    # ---- traces: the first num_iterations entries, and zeros behind them
    for key, figure in (("cost_trace", COST_TRACE_TOL), ("radius_trace", RADIUS_TRACE_TOL)):
        bound = max(10 * _trace_gap(so, st, key), figure)
        gap = _trace_gap(sg, st, key)
        print(f"[{name} {build}] {key}: device - binary128 {gap:.1e} | oracle - binary128 {_trace_gap(so, st, key):.1e}")
        assert gap <= bound, (key, gap, bound)
        for i in range(B):
            n = int(st["num_iterations"][i])
            assert np.array_equal(sg[key][i][:n] == 0, st[key][i][:n] == 0), (key, i)     # (an exit by a tolerance leaves its attempt's entry unwritten)
            assert (sg[key][i][n:] == 0).all(), (key, i)
    for key in ("initial_cost", "final_cost"):
        assert rel(sg[key], st[key]) <= max(10 * rel(so[key], st[key]), COST_TRACE_TOL), key


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["latency", "throughput"])
def test_device_gives_up_after_the_invalid_steps_the_options_allow(ctx, oracle, monkeypatch, build):
    """max_num_consecutive_invalid_steps = 2 on NaN / Inf / singular inputs: FAILURE after two attempts, like the FP64 oracle (there is no
    binary128 answer to a NaN), and the healthy sixth window of the batch has its usual parity."""
    R = reference("invalid_steps")
    wg, sg = _device_solve(ctx, monkeypatch, "invalid_steps", build)
    so, wo = R["so"], R["wo"]
    assert sg["termination"].tolist() == so["termination"].tolist() == [TERM["FAILURE"]] * 5 + [TERM["NO_CONVERGENCE"]]
    assert sg["num_iterations"].tolist() == so["num_iterations"].tolist() == [2] * 5 + [8]
    assert sg["num_successful"].tolist() == so["num_successful"].tolist() and sg["accept_mask"].tolist() == so["accept_mask"].tolist()
    for k in ("pose", "speedbias", "inv_depth"):
        assert rel(wg.a[k][5], wo.a[k][5]) < STATE_TOL, k
    for key in ("cost_trace", "radius_trace"):
        assert (sg[key][:, 8:] == 0).all() and (sg[key][:5, 2:] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name,build", [("max_it_16", "latency"), ("max_it_16", "throughput"), ("x_max_it_1", "extended")])
def test_seventeen_iterations_are_refused_and_the_states_untouched(ctx, monkeypatch, name, build):
    """The traces hold sixteen attempts: max_num_iterations = 17 is AVM_ERR_CAPACITY (csrc/api/checks.hpp), before anything is written."""
    if build != "extended":
        monkeypatch.setenv("AVM_SOLVE_TP", "1" if build == "throughput" else "0")
    w = cases.windows(name)
    wg = w.copy()
    with pytest.raises(lib_m.AvmError, match="max_num_iterations > 16") as e:
        est_m.Estimator(ctx=ctx, options=cases.options(name, max_num_iterations=17)).optimization(wg)
    assert "status %d" % abi.AVM_ERR_CAPACITY in str(e.value)
    for k in w.a:
        assert np.array_equal(wg.a[k], w.a[k]), k
