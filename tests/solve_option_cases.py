"""The case table of tests/test_solve_options.py (test infrastructure, like sfm_cases.py / preint_cases.py): every exit of the
trust-region minimizer and every option the solve kernels read, each as (windows, option overrides, what the case must exercise).

The yardstick is the binary128 solve (oracle/avm_truth.cpp: avmt_solve, marg_sensitivity.truth_solve); the FP64 oracle shares its
source (oracle/solver.hpp) and is run next to it, so that a test can grade the device against "how far is the same algorithm in
FP64 from the exact answer".  reference(name) runs both ONCE per case and keeps the result: every build of the kernel, and every
test of a case, reads the same arrays (they are never written to - take copies).

Nothing here hard-codes what a solve decides: `exercises` names what the binary128 run of the case has to show (which exits occur,
whether a step is rejected, ...), and the CPU tier of test_solve_options.py asserts it from that run.
"""
import functools
from collections import namedtuple

import numpy as np

from helpers import abi, buffers, rel, synth
from marg_sensitivity import truth_lib, truth_solve

TERM = {n: i for i, n in enumerate(abi.TERM_NAMES)}
SUM_DT_EPS = 2.0 ** -30          # far above any rounding of a sum of twenty dt, far below anything a factor's value notices

# windows: name of a builder below; overrides: {field of avm_options: value} or a function returning that;
# exercises: terminations = exits that must occur among the windows of the binary128 run, all_terminate = every window takes that exit,
#   attempts = num_iterations of every window, rejected = some / no window rejects a step, skipped = the IMU factors max_sum_dt drops,
#   differs_from = a case on the same windows whose accept masks this one must not reproduce, after_an_attempt = no window stops before its first,
#   rejected_past_32_features = a window with more than 32 features rejects a step;
# varied: the tolerance that decides the exit (the CPU tier moves it by 1 +- 1e-3: the decisions must not change);
# x: the extended problem (ex_pose, td, a relocalization frame: the -DAVM_X kernel); truth: False = FP64 oracle only.
Case = namedtuple("Case", "windows overrides exercises varied x truth", defaults=(None, False, True))


# ------------------------------------------------------------------------------------------------------------ windows
def _concat(a, b):
    d = dict(a.dims)
    assert {k: v for k, v in d.items() if k != "n_windows"} == {k: v for k, v in b.dims.items() if k != "n_windows"}
    d["n_windows"] = a.n_windows + b.n_windows
    return buffers.WindowArrays(d, {k: np.concatenate([a.a[k], b.a[k]]) for k in a.a})


def _wild(w, seed=7, sigma_q=0.4, sigma_p=0.8):
    """The perturbation of test_gpu_parity.test_speculative_evaluation_is_exact_including_rejected_steps, at 0.4 / 0.8."""
    rng = np.random.default_rng(seed)
    q = w.a["pose"][:, 1:, 3:] + rng.normal(0, sigma_q, w.a["pose"][:, 1:, 3:].shape)
    w.a["pose"][:, 1:, 3:] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w.a["pose"][:, 1:, :3] += rng.normal(0, sigma_p, w.a["pose"][:, 1:, :3].shape)
    return w


def _pair(prior=True, first_id=4200):
    """Windows 0-3: 24 ragged tracks; windows 4-7: 33 full-length tracks (one past the 32-feature boundary of the kernels' feature loops)."""
    return _concat(*[synth.make_windows(4, first_id=first_id, tracks=t, n_feat=n, max_feat=150, with_prior=prior) for t, n in (("sparse", 24), ("dense", 33))])


# Two kinds of window amplify FP64 rounding so far that WHICH window is taken decides the grading: the ones started far from their minimum
# (they can end in minima with weakly determined depths) and the ones without a prior (four gauge directions held by the damping alone).  There
# the FP64 oracle's distance from the binary128 solve scatters over a decade when its inputs move by one unit in the last place, and "ten
# times the oracle's distance" is ten times one draw of that.  oracle_scatter() below measures it without any device - the fraction of the
# device's bound that the oracle one ulp aside uses up - and the CPU tier asserts at most one half for every case.  At first_id 4200 it is 4.2 in
# `rejected` (inverse depths of window 3: up to 4.2e-6, beyond the 1e-6 contract itself) and 0.96 in `sum_dt_skip_noprior`.  Every other case
# keeps 4200.  A 33-track window that rejects a step is rarely a quiet one (ids 4200 .. 4240 at 0.4 / 0.8: fractions of 2.7 .. 500 wherever a
# step is rejected, except 4212 and 4220 with 0.5 and 0.4 over twelve draws): the 33-track block is 4220 at 1.05 times the perturbation, where
# windows 2 and 3 reject steps (window 2 five in a row) and twelve draws stay below 0.4 of the bound.
WILD_BLOCKS = (("sparse", 24, 4212, 1.0), ("dense", 33, 4220, 1.05))
NOPRIOR_FIRST_ID = 4208


def _wild_windows():
    """The eight windows of the far-from-minimum cases: four 24-track and four 33-track ones, each block perturbed on its own (the same draws of
    default_rng(7) for both, so neither block depends on the other being there) at 0.4 / 0.8 times the block's factor.  Steps are rejected on
    both sides of the 32-feature boundary (the table entry says so, the CPU tier asserts it)."""
    return _concat(*[_wild(synth.make_windows(4, first_id=f, tracks=t, n_feat=n, max_feat=150, with_prior=True), sigma_q=0.4 * c, sigma_p=0.8 * c)
                     for t, n, f, c in WILD_BLOCKS])


def _stretch(w, intervals):
    for j in intervals:
        w.a["imu_dt"][:, j] *= 1.0 + SUM_DT_EPS
    return w


def _x_windows():
    w = synth.make_windows(2, first_id=70, tracks="sparse", n_feat=24, max_feat=150, td_true=0.012, relo=True)
    w.a["ex_pose"][:, :3] += 0.01
    return w


def _poisoned():
    from test_gpu_parity import _poisoned_windows

    return _poisoned_windows()


_BUILDERS = {
    "base": _pair,
    "wild": _wild_windows,
    "one": lambda: synth.make_windows(1, first_id=4200, tracks="sparse", n_feat=24, max_feat=150, with_prior=True),
    "sum_dt": lambda: _stretch(_pair(), (0, 4, 9)),
    "sum_dt_noprior": lambda: _stretch(_pair(prior=False, first_id=NOPRIOR_FIRST_ID), (4,)),
    "x": _x_windows,
    "x_sum_dt": lambda: _stretch(_x_windows(), (0, 4, 9)),
    "poisoned": _poisoned,
}


@functools.lru_cache(maxsize=None)
def _built(kind):
    return _BUILDERS[kind]()


def windows(name):
    """A fresh copy of the case's input windows."""
    return _built(CASES[name].windows).copy()


def truth(w, opt):
    """marg_sensitivity.truth_solve, the windows spread over four threads (one binary128 solve takes 0.2 .. 1.5 s and shares nothing with
    the next; ctypes releases the interpreter lock for the call)."""
    from concurrent.futures import ThreadPoolExecutor

    truth_lib()                                         # (loads - and on first use builds - the library before the threads start)
    with ThreadPoolExecutor(4) as pool:
        parts = list(pool.map(lambda i: truth_solve(w.slice(i, i + 1), opt), range(w.n_windows)))
    out, summ = w.copy(), buffers.summary_alloc(w.n_windows)
    for i, (wi, si) in enumerate(parts):
        for k in out.a:
            out.a[k][i] = wi.a[k][0]
        summ[i] = si[0]
    return out, summ


# ------------------------------------------------------------------------------------------------------------ options
def untouched_sum_dt(name):
    """max_sum_dt of the sum_dt cases: the FP64 sum_dt of an interval _stretch() left alone (interval 1), as the oracle's pre-integration
    accumulates it - every other untouched interval of every window has the same twenty dt and therefore exactly this sum."""
    import oracle_py

    o = abi.default_options()
    return float(oracle_py.preintegrate(o, windows(name))[3][0, 1])


def first_halving(summary, initial_radius):
    """(window, attempt k, radius before, radius after) of the first halving of the first window that rejects a step."""
    for i in range(len(summary)):
        n = int(summary["num_iterations"][i])
        if int(summary["num_successful"][i]) == n:
            continue
        r = np.concatenate([[initial_radius], summary["radius_trace"][i][:n]])
        for k in range(1, n + 1):
            if r[k] == 0.5 * r[k - 1]:
                return i, k, float(r[k - 1]), float(r[k])
    raise AssertionError("no window of the case rejects a step")


MIN_RADIUS_START = 1e6


def _min_radius():
    """min_trust_region_radius = the geometric mean of the binary128 radii before and after the first halving of the first window that
    rejects a step: a factor sqrt 2 from either decision, so whichever implementation follows the binary128 radii to anything like the
    1e-9 the traces are graded at stops exactly there (MIN_RADIUS), and not before.
    From the default initial radius (1e4) the exit cannot be reached that way: Ceres' dogleg radius only grows while steps are accepted
    (3 |step|: 3e4, 9e4, ... 8.1e5 on these windows), so the mean lies ABOVE the initial radius and the minimizer would stop before its first
    attempt (that exit is the case min_radius_at_once).  The case therefore starts at 1e6, above any 3 |step| of the first attempts, where
    the first attempt of every window ends in a halving - of a rejected step, or of an accepted one with rho < 1/4 - that starts from the
    initial radius."""
    start = dict(max_num_iterations=12, initial_trust_region_radius=MIN_RADIUS_START)
    _, st = truth(windows("min_radius"), options("rejected", **start))
    _, _, before, after = first_halving(st, MIN_RADIUS_START)
    return dict(start, min_trust_region_radius=float(np.sqrt(before * after)))


CASES = {
    "gradient_tol": Case("base", dict(gradient_tolerance=1e3), dict(all_terminate="GRADIENT_TOL"), "gradient_tolerance"),
    "parameter_tol": Case("base", dict(parameter_tolerance=1e-3), dict(terminations={"PARAMETER_TOL"}), "parameter_tolerance"),
    "function_tol": Case("base", dict(function_tolerance=1e-3), dict(terminations={"FUNCTION_TOL"}), "function_tolerance"),
    "max_it_1": Case("base", dict(max_num_iterations=1), dict(all_terminate="NO_CONVERGENCE", attempts=1, rejected=False)),
    "max_it_16": Case("base", dict(max_num_iterations=16, function_tolerance=0.0, parameter_tolerance=0.0),
                      dict(all_terminate="NO_CONVERGENCE", attempts=16, rejected=False)),
    "rejected": Case("wild", dict(max_num_iterations=12), dict(rejected=True, rejected_past_32_features=True)),
    "min_rel_decrease": Case("wild", dict(max_num_iterations=12, min_relative_decrease=0.3), dict(rejected=True, differs_from="rejected")),
    "min_radius": Case("wild", _min_radius, dict(all_terminate="MIN_RADIUS", rejected=True, after_an_attempt=True), "min_trust_region_radius"),
    "min_radius_at_once": Case("one", dict(min_trust_region_radius=1e4), dict(all_terminate="MIN_RADIUS", attempts=0)),
    "jacobi_off": Case("base", dict(jacobi_scaling=0), dict(all_terminate="NO_CONVERGENCE", attempts=8)),
    "lm_clamp": Case("base", dict(min_lm_diagonal=0.5, max_lm_diagonal=0.9), dict(all_terminate="NO_CONVERGENCE", attempts=8)),
    "loss_focal": Case("base", dict(cauchy_a=0.3, focal_length=300.0), dict(all_terminate="NO_CONVERGENCE", attempts=8)),
    "sum_dt_skip": Case("sum_dt", lambda: dict(max_sum_dt=untouched_sum_dt("sum_dt_skip")), dict(skipped={0, 4, 9})),
    "sum_dt_skip_noprior": Case("sum_dt_noprior", lambda: dict(max_sum_dt=untouched_sum_dt("sum_dt_skip_noprior")), dict(skipped={4})),
    "invalid_steps": Case("poisoned", dict(max_num_consecutive_invalid_steps=2), dict(terminations={"FAILURE"}), truth=False),
    "x_parameter_tol": Case("x", dict(parameter_tolerance=1e-3), dict(terminations={"PARAMETER_TOL"}), "parameter_tolerance", x=True),
    "x_function_tol": Case("x", dict(function_tolerance=1e-3), dict(terminations={"FUNCTION_TOL"}), "function_tolerance", x=True),
    "x_jacobi_off": Case("x", dict(jacobi_scaling=0), dict(all_terminate="NO_CONVERGENCE", attempts=8), x=True),
    "x_loss_focal": Case("x", dict(cauchy_a=0.3, focal_length=300.0), dict(all_terminate="NO_CONVERGENCE", attempts=8), x=True),
    "x_sum_dt_skip": Case("x_sum_dt", lambda: dict(max_sum_dt=untouched_sum_dt("x_sum_dt_skip")), dict(skipped={0, 4, 9}), x=True),
    "x_max_it_1": Case("x", dict(max_num_iterations=1), dict(all_terminate="NO_CONVERGENCE", attempts=1, rejected=False), x=True),
}
BASE_CASES = [n for n, c in CASES.items() if not c.x]
X_CASES = [n for n, c in CASES.items() if c.x]
TRUTH_CASES = [n for n, c in CASES.items() if c.truth]
TOLERANCE_CASES = [n for n, c in CASES.items() if c.varied and c.truth]
SUM_DT_CASES = [n for n, c in CASES.items() if "skipped" in c.exercises]


@functools.lru_cache(maxsize=None)
def _overrides(name):
    ov = CASES[name].overrides
    return dict(ov() if callable(ov) else ov)


def options(name, **more):
    """avm_options of the case: the defaults, no marginalization, the case's overrides, then `more`."""
    o = abi.default_options()
    o.marginalization_flag = abi.MARGIN_NONE
    if CASES[name].x:
        o.estimate_extrinsic = o.estimate_td = 1
    for k, v in {**_overrides(name), **more}.items():
        assert hasattr(o, k), k
        setattr(o, k, v)
    return o


def state_keys(name):
    return ["pose", "speedbias", "inv_depth", "ex_pose"] + (["td", "relo_pose"] if CASES[name].x else [])


# ------------------------------------------------------------------------------------------------------------ the references, once per case
@functools.lru_cache(maxsize=None)
def reference(name):
    """dict(w: the input, opt, wo / so: the FP64 oracle's states and summaries, wt / st: the binary128 solve's (None where the case has
    no truth)).  Computed once per process; treat every array as read-only."""
    import oracle_py

    w, opt = windows(name), options(name)
    wo, so = w.copy(), buffers.summary_alloc(w.n_windows)
    oracle_py.window_solve(opt, wo, None, so)
    wt, st = truth(w, opt) if CASES[name].truth else (None, None)
    return dict(w=w, opt=opt, wo=wo, so=so, wt=wt, st=st)


STATE_TOL = 1e-6                                  # the contract: states within 1e-6 of what the algorithm defines
FLOOR = {False: 1e-10, True: 1e-9}                # tests/test_solve_truth.py: base builds / the extended problem


def state_bound(name, key, i):
    """What the state block `key` of window i may be away from the binary128 solve (tests/test_solve_truth.py's rule, per window): less than
    the contract, and not more than ten times the FP64 oracle's own distance, or the floor."""
    R = reference(name)
    go = rel(R["wo"].a[key][i], R["wt"].a[key][i])
    return min(STATE_TOL, max(10 * go, FLOOR[CASES[name].x]))


def oracle_scatter(name, seeds=None):
    """The worst, over every window and state block, of (distance of the FP64 oracle from the binary128 solve when its inputs move by one
    unit in the last place) / state_bound(): how much of the bound the device is graded against FP64 rounding alone uses up.  Also whether
    each of these runs took the binary128 decisions.  Above 1 the case would be decided by rounding: the oracle itself, one ulp aside, would
    fail it."""
    import oracle_py
    from marg_sensitivity import ulp_perturbed

    R = reference(name)
    seeds = seeds or (12 if CASES[name].windows == "wild" else 4)       # (the far-from-minimum windows: the tail of the scatter matters there)
    worst, where, same = 0.0, None, True
    for seed in range(seeds):
        w = ulp_perturbed(R["w"], seed, keys=("pose", "speedbias", "inv_depth", "obs_xy"))
        s = buffers.summary_alloc(w.n_windows)
        oracle_py.window_solve(R["opt"], w, None, s, n_threads=4)
        same = same and decisions(s) == decisions(R["st"])
        for k in state_keys(name):
            for i in range(w.n_windows):
                q = rel(w.a[k][i], R["wt"].a[k][i]) / state_bound(name, k, i)
                if q > worst:
                    worst, where = q, (seed, k, i)
    return worst, where, same


DECISIONS = ("termination", "num_iterations", "num_successful", "accept_mask")


def decisions(s):
    return {k: np.asarray(s[k]).tolist() for k in DECISIONS}


def skipped_factors(name):
    """Per window: (the intervals whose IMU factor the solve drops (sum_dt > max_sum_dt), the intervals that sit exactly at equality and are
    kept), from the FP64 pre-integration's sum_dt."""
    import oracle_py

    opt = options(name)
    sd = oracle_py.preintegrate(opt, windows(name))[3]
    return [({j for j in range(sd.shape[1]) if sd[i, j] > opt.max_sum_dt}, {j for j in range(sd.shape[1]) if sd[i, j] == opt.max_sum_dt}) for i in range(sd.shape[0])]
