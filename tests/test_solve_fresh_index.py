"""GPU tier (-m gpu): the three builds of the solve kernel over one batch of eight windows chosen for the paths of the kernel BODY - the
per-window load, the trust-region loop's own vector passes, the speculation lambdas, the gauge fix - rather than for the bulk phases.

The body takes a fresh thread index at the head of every segment (fresh_tid(), csrc/solve/lds.hpp), derives the speculation's parking
address at every use and decides its branches in scalar registers; none of that is arithmetic, so every decision and every state has to
stay the oracle's.  What differs from window to window in the body:
  - n_feat 1 and 150, and 80 / 81: with 256 threads the loops over 176 + n_feat entries take one trip up to n_feat = 80 and two from 81;
  - with and without a prior (prior_n == 0 skips the prior's block table, its index lists and Hp = J0^T J0);
  - a window with a step that is rejected while the solve speculates (spec_restore, one more evaluation, spec_restore_gn_step);
  - windows that stop on the function tolerance (the exits that call spec_restore before they leave the loop).
The options are the default ones with function_tolerance = 1e-3, at which the oracle stops most of these windows on FUNCTION_TOL within
the eight iterations; which window takes which path is asserted on the ORACLE's summary, so the batch cannot quietly stop covering them.

Tolerances are those of tests/test_gpu_parity.py: identical iteration counts, accept masks and terminations, cost traces within 1e-6,
states within STATE_TOL = 1e-6; for the window started from wild attitudes and positions (the recipe of
test_speculative_evaluation_is_exact_including_rejected_steps, which is what produces rejected steps) that test's bounds: the speculative
and the classic order of evaluations agree within 1e-9, the states follow the oracle's within 1e-4.
"""
import importlib

import numpy as np
import pytest

from helpers import abi, buffers, rel, synth

pytestmark = pytest.mark.gpu

STATE_TOL = 1e-6
WILD = 6  # index of the window with the rejected step


def _one(first_id, n_feat, prior, tracks):
    return synth.make_windows(1, first_id=first_id, tracks=tracks, n_feat=n_feat, max_feat=150, with_prior=prior)


def _batch():
    parts = [_one(900, 1, True, "dense"), _one(901, 1, False, "dense"), _one(902, 150, True, "dense"), _one(903, 150, False, "dense"),
             _one(904, 80, True, "sparse"), _one(905, 81, False, "sparse")]
    wild = _one(1023, 150, True, "dense")
    rng = np.random.default_rng(1023)
    q = wild.a["pose"][:, 1:, 3:] + rng.normal(0, 0.5, wild.a["pose"][:, 1:, 3:].shape)
    wild.a["pose"][:, 1:, 3:] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    wild.a["pose"][:, 1:, :3] += rng.normal(0, 1.0, wild.a["pose"][:, 1:, :3].shape)
    parts.append(wild)
    far = _one(906, 60, True, "sparse")  # depths twenty times too large: six accepted steps, then FUNCTION_TOL
    far.a["inv_depth"][:, :60] *= 0.05
    parts.append(far)
    dims = dict(parts[0].dims)
    dims["n_windows"] = len(parts)
    return buffers.WindowArrays(dims, {k: np.concatenate([p.a[k] for p in parts]) for k in parts[0].a})


def _options(extended):
    o = abi.default_options()
    o.marginalization_flag = abi.MARGIN_NONE
    o.function_tolerance = 1e-3
    if extended:
        o.estimate_extrinsic = 1
    return o


@pytest.fixture(scope="module")
def reference(oracle):
    """the batch and the oracle's solve of it, once per problem (base, extended); nothing below writes to either"""
    w = _batch()
    out = {}
    for extended in (False, True):
        wo, so = w.copy(), buffers.summary_alloc(w.n_windows)
        oracle.window_solve(_options(extended), wo, None, so)
        out[extended] = (wo, so)
    return w, out


def _speculative_rejections(so, i):
    """iterations (0-based) whose step was rejected right after an accepted step that GREW the radius - only rho > 0.75 does, and that is
    the condition under which the kernel speculates on the next step"""
    m, n, rt = int(so["accept_mask"][i]), int(so["num_iterations"][i]), so["radius_trace"][i]
    first = abi.default_options().initial_trust_region_radius
    return [k for k in range(1, n) if not (m >> k) & 1 and (m >> (k - 1)) & 1 and rt[k - 1] > (rt[k - 2] if k >= 2 else first)]


def test_the_batch_covers_the_paths_it_is_for(reference):
    w, ref = reference
    assert w.n_windows == 8
    assert sorted(set(w.a["n_feat"].tolist())) == [1, 60, 80, 81, 150]
    assert (w.a["prior_n"][[0, 2, 4, 6, 7]] > 0).all() and (w.a["prior_n"][[1, 3, 5]] == 0).all()
    for extended, (wo, so) in ref.items():
        assert np.isfinite(wo.a["pose"]).all()
        assert _speculative_rejections(so, WILD), (extended, bin(int(so["accept_mask"][WILD])), so["radius_trace"][WILD])
        stopped = np.flatnonzero(so["termination"] == abi.TERM_NAMES.index("FUNCTION_TOL"))
        assert len(stopped) >= 3 and (so["num_iterations"][stopped] < 8).any(), (extended, so["termination"])
        assert (so["termination"] == abi.TERM_NAMES.index("NO_CONVERGENCE")).any()  # ... and the iteration limit is still one of the exits


@pytest.mark.parametrize("build", ["latency", "throughput", "extended"])
def test_every_build_takes_the_oracles_decisions_and_reaches_its_states(ctx, reference, monkeypatch, build):
    w, ref = reference
    extended = build == "extended"
    wo, so = ref[extended]
    monkeypatch.setenv("AVM_SOLVE_TP", "1" if build == "throughput" else "0")
    E = importlib.import_module("anticipated-vins-mono_amd.estimator").Estimator(ctx=ctx, options=_options(extended))
    monkeypatch.setenv("AVM_NO_SPECULATE", "0")
    g = w.copy()
    s = buffers.summary_to_numpy(E.optimization(g)).copy()
    assert ctx.last_solve_form() == ("throughput" if build == "throughput" else "latency")
    monkeypatch.setenv("AVM_NO_SPECULATE", "1")
    g2 = w.copy()
    s2 = buffers.summary_to_numpy(E.optimization(g2)).copy()
    for k in ("num_iterations", "num_successful", "accept_mask", "termination"):
        assert np.array_equal(s[k], so[k]), (k, s[k], so[k])
        assert np.array_equal(s2[k], so[k]), ("classic order of evaluations", k, s2[k], so[k])
    tame = [i for i in range(w.n_windows) if i != WILD]
    gaps = {k: [rel(g.a[k][i], wo.a[k][i]) for i in range(w.n_windows)] for k in ("pose", "speedbias", "inv_depth", "ex_pose")}
    print("\n[%s] cost trace %.3g, per-window gap to the oracle: %s; speculative vs classic pose %.3g" % (
        build, rel(s["cost_trace"][tame], so["cost_trace"][tame]), {k: ["%.1e" % v for v in gaps[k]] for k in gaps}, rel(g.a["pose"], g2.a["pose"])))
    assert rel(s["cost_trace"][tame], so["cost_trace"][tame]) < 1e-6
    for k in gaps:
        assert max(gaps[k][i] for i in tame) < STATE_TOL, (k, gaps[k])
        assert gaps[k][WILD] < 1e-4, (k, gaps[k][WILD])
    n = int(s["num_iterations"][WILD])
    assert rel(s["radius_trace"][WILD][:n], so["radius_trace"][WILD][:n]) < 1e-4
    for k in ("pose", "speedbias", "inv_depth"):
        assert rel(g.a[k], g2.a[k]) < 1e-9, (k, rel(g.a[k], g2.a[k]))
