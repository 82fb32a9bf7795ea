"""GPU tier (-m gpu): the HIP product path, called through the C ABI, against the CPU oracle on the
same seeded inputs, against the committed golden vectors, and through size-independent properties.

Tolerances: BASELINE.json north_star asks pose states within 1e-6 relative and selected ids bit-exact.
Per-factor quantities are checked much tighter (1e-10) because nothing iterative sits in between.
"""
import numpy as np
import pytest

from helpers import abi, blank_windows, buffers, golden, imu_window_from_golden, projection_windows_from_golden, rel, synth

pytestmark = pytest.mark.gpu


def importlib_est():
    import importlib

    return importlib.import_module("anticipated-vins-mono_amd.estimator")

STATE_TOL = 1e-6   # north_star: pose states within 1e-6 relative
FACTOR_TOL = 1e-10


def test_native_library_is_the_one_loaded(ctx):
    import ctypes as C

    assert b"gfx950" in ctx._L.avm_version()
    maps = open("/proc/self/maps").read()
    assert "libavm_hip.so" in maps


def test_preintegration_matches_oracle_and_golden(estimator, oracle):
    w = synth.make_windows(3, tracks="sparse", n_feat=10, max_feat=150)
    d, J, P, sd = estimator.preintegrate(w)
    sq = estimator.sqrt_info(3)
    od, oJ, oP, osd, osq = oracle.preintegrate(estimator.options, w)
    for a, b in ((d, od), (J, oJ), (P, oP), (sd, osd), (sq, osq)):
        assert rel(a, b) < 1e-12
    g = golden()
    wg = imu_window_from_golden(g)
    d, J, P, sd = estimator.preintegrate(wg)
    assert rel(d[0, 0, :3], g["pre_dp"]) < 1e-13 and rel(J[0, 0], g["pre_J"]) < 1e-12 and rel(P[0, 0], g["pre_P"]) < 1e-12


def test_ragged_imu_sample_counts(estimator, oracle):
    w = synth.make_windows(2, tracks="sparse", n_feat=6, max_feat=150)
    w.a["imu_n"][0, 3] = 11
    w.a["imu_n"][1, 7] = 1
    w.a["imu_n"][1, 8] = 0
    d, J, P, sd = estimator.preintegrate(w)
    sq = estimator.sqrt_info(2)
    od, oJ, oP, osd, osq = oracle.preintegrate(estimator.options, w)
    assert rel(d, od) < 1e-12 and rel(J, oJ) < 1e-12 and rel(sd, osd) < 1e-15
    ok = np.ones((2, 10), bool)
    ok[1, 8] = False  # zero samples: covariance is all zero (singular), nothing to compare
    assert rel(P[ok], oP[ok]) < 1e-12
    two = w.a["imu_n"] >= 2  # one sample: a covariance of rank 12, no sqrt_info is defined (tests/test_preint_truth.py)
    assert two.sum() == 18 and rel(sq[two], osq[two]) < 1e-12


def test_factor_evaluation_matches_oracle_and_golden(estimator, oracle):
    for tracks, nf in (("sparse", 50), ("dense", 150)):
        w = synth.make_windows(2, tracks=tracks, n_feat=nf, max_feat=150)
        for loss in (False, True):
            g, o = estimator.eval_factors(w, apply_loss=loss), oracle.eval_factors(estimator.options, w, apply_loss=loss)
            for k in g:
                assert rel(g[k], o[k]) < FACTOR_TOL, (tracks, loss, k, rel(g[k], o[k]))
    gd = golden()
    wg = projection_windows_from_golden(gd)
    ev = estimator.eval_factors(wg, apply_loss=True)
    assert rel(ev["proj_r"][:, 1], gd["proj_r_c"]) < 1e-11
    assert rel(ev["proj_J"][:, 1], gd["proj_J_c"]) < 1e-11


def _solve_both(estimator, oracle, w, opt=None):
    opt = opt or estimator.options
    old = estimator.options
    estimator.options = opt
    try:
        wg, wo = w.copy(), w.copy()
        sg = estimator.optimization(wg)
        so = buffers.summary_alloc(w.n_windows)
        oracle.window_solve(opt, wo, None, so)
    finally:
        estimator.options = old
    return wg, wo, sg, so


def _assert_state_parity(wg, wo, sg, so):
    assert np.array_equal(sg["num_iterations"], so["num_iterations"])
    assert np.array_equal(sg["accept_mask"], so["accept_mask"])
    assert np.array_equal(sg["termination"], so["termination"])
    assert rel(sg["cost_trace"], so["cost_trace"]) < 1e-6
    for k in ("pose", "speedbias", "inv_depth", "ex_pose"):
        assert rel(wg.a[k], wo.a[k]) < STATE_TOL, (k, rel(wg.a[k], wo.a[k]))


def test_newest_frame_dead_reckoning_matches_oracle(estimator, oracle):
    """Estimator::processIMU dead-reckoning on device."""
    w = synth.make_windows(5, tracks="sparse", n_feat=8, max_feat=150)
    w.a["pose"][:, 10] = w.a["pose"][:, 9]
    w.a["speedbias"][:, 10] = w.a["speedbias"][:, 9]
    w.a["imu_n"][2, 9] = 3
    w.a["imu_n"][3, 9] = 0
    wg, wo = w.copy(), w.copy()
    estimator.imu_propagate(wg)
    oracle.imu_propagate(wo, np.array(list(estimator.options.g)))
    assert rel(wg.a["pose"], wo.a["pose"]) < 1e-13 and rel(wg.a["speedbias"], wo.a["speedbias"]) < 1e-13
    assert np.array_equal(wg.a["pose"][:, :10], w.a["pose"][:, :10])
    wd = w.to_device("cuda:0")
    estimator.imu_propagate(wd)
    assert np.array_equal(wd.to_host().a["pose"], wg.a["pose"])


def test_projection_td_factor_matches_oracle(estimator, oracle):
    """A7: ProjectionTdFactor::Evaluate on device (residual + all five Jacobian blocks)."""
    rng = np.random.default_rng(5)
    n = 300
    def unit(a):
        return a / np.linalg.norm(a, axis=-1, keepdims=True)
    def pose(scale):
        return np.hstack([scale * rng.normal(size=(n, 3)), unit(np.array([0, 0, 0, 1.0]) + 0.2 * rng.normal(size=(n, 4)))])
    a = dict(pose_i=pose(0.5), pose_j=pose(0.5), ex_pose=pose(0.05), inv_depth=1.0 / rng.uniform(2, 15, n), td=0.01 * rng.normal(size=n),
             pts_i=0.4 * rng.normal(size=(n, 2)), pts_j=0.4 * rng.normal(size=(n, 2)), vel_i=0.3 * rng.normal(size=(n, 2)),
             vel_j=0.3 * rng.normal(size=(n, 2)), td_i=0.01 * rng.normal(size=n), td_j=0.01 * rng.normal(size=n),
             row_i=rng.uniform(0, 480, n), row_j=rng.uniform(0, 480, n))
    rg, Jg = estimator.projection_td_eval(a, 0.033, 480.0, 460.0)
    ro, Jo = oracle.projection_td_eval(a, 0.033, 480.0, 460.0)
    assert rel(rg, ro) < FACTOR_TOL and rel(Jg, Jo) < FACTOR_TOL
    # with no image velocity the factor is ProjectionFactor: same residuals whatever td is
    a0 = dict(a, vel_i=np.zeros((n, 2)), vel_j=np.zeros((n, 2)))
    r0, J0 = estimator.projection_td_eval(a0, 0.033, 480.0, 460.0)
    r1, _ = estimator.projection_td_eval(dict(a0, td=a0["td"] + 0.5), 0.033, 480.0, 460.0)
    assert np.array_equal(r0, r1) and np.abs(J0[:, :, 19]).max() == 0.0


def test_triangulation_matches_oracle(estimator, oracle):
    """FeatureManager::triangulate on device (the step before optimization() in solveOdometry())."""
    for tracks, nf in (("sparse", 60), ("dense", 150)):
        w = synth.make_windows(4, tracks=tracks, n_feat=nf, max_feat=150)
        keep = w.a["inv_depth"].copy()
        w.a["inv_depth"][:, ::2] = -1.0  # "no depth yet"
        w.a["inv_depth"][0, 1] = 0.0
        wg, wo = w.copy(), w.copy()
        estimator.triangulate(wg, init_depth=5.0)
        oracle.triangulate(wo, init_depth=5.0)
        assert np.array_equal(wg.a["inv_depth"][:, 3::2], keep[:, 3::2])      # features with a depth are left alone
        for b in range(4):
            n = w.a["n_feat"][b]
            assert (wg.a["inv_depth"][b, :n] > 0).all()
            assert rel(wg.a["inv_depth"][b, :n], wo.a["inv_depth"][b, :n]) < 1e-9
        # device-resident buffers give the same result
        wd = w.to_device("cuda:0")
        estimator.triangulate(wd, init_depth=5.0)
        assert np.array_equal(wd.to_host().a["inv_depth"], wg.a["inv_depth"])
    # a feature seen from (almost) one place only has no usable parallax: depth < 0.1 or NaN -> INIT_DEPTH
    w = synth.make_windows(1, tracks="dense", n_feat=8, max_feat=150)
    w.a["pose"][0, :, :3] = w.a["pose"][0, 0, :3]
    w.a["pose"][0, :, 3:] = w.a["pose"][0, 0, 3:]
    w.a["obs_xy"][0, :, :] = 0.3
    w.a["inv_depth"][:] = -1.0
    wg, wo = w.copy(), w.copy()
    estimator.triangulate(wg, init_depth=5.0)
    oracle.triangulate(wo, init_depth=5.0)
    assert rel(wg.a["inv_depth"][0, :8], wo.a["inv_depth"][0, :8]) < 1e-9


@pytest.mark.parametrize("tracks,nf", [("sparse", 60), ("dense", 150), ("sparse", 150), ("dense", 12)])
def test_window_solve_parity(estimator, oracle, tracks, nf):
    w = synth.make_windows(3, tracks=tracks, n_feat=nf, max_feat=150)
    wg, wo, sg, so = _solve_both(estimator, oracle, w)
    _assert_state_parity(wg, wo, sg, so)
    assert (sg["final_cost"] < 1e-3 * sg["initial_cost"]).all()


def test_window_solve_parity_over_many_windows(estimator, oracle):
    """A wider sweep than the fixed cases: 48 different windows (three id ranges, both track shapes, with and without
    prior): identical iteration / accept traces and termination, states within the north-star tolerance."""
    worst = 0.0
    for first_id, tracks, nf, prior in ((1000, "sparse", 90, True), (2000, "dense", 150, True), (3000, "sparse", 150, False)):
        w = synth.make_windows(16, first_id=first_id, tracks=tracks, n_feat=nf, max_feat=150, with_prior=prior)
        wg, wo, sg, so = _solve_both(estimator, oracle, w)
        _assert_state_parity(wg, wo, sg, so)
        worst = max(worst, rel(wg.a["pose"], wo.a["pose"]))
    assert worst < 1e-8, worst  # measured ~1e-10; the contract is 1e-6


def _retrack(dense, w, starts, lengths):
    """Rewrite window w of a dense batch (every feature seen in all 11 frames) to the given tracks, keeping the geometry:
    feature e keeps its observations of frames starts[e] .. starts[e] + lengths[e] - 1; sorted by start frame (list order)."""
    order = np.argsort(starts, kind="stable")
    obs = dense.a["obs_xy"][w].copy()
    ob0 = dense.a["feat_obs_begin"][w].copy()
    lam = dense.a["inv_depth"][w].copy()
    nf = len(starts)
    o = 0
    for k, e in enumerate(order):
        a, n = int(starts[e]), int(lengths[e])
        dense.a["feat_start"][w, k], dense.a["feat_nobs"][w, k], dense.a["feat_obs_begin"][w, k] = a, n, o
        dense.a["obs_xy"][w, o:o + n] = obs[ob0[e] + a: ob0[e] + a + n]
        # the inverse depth lives in the first observing frame: rescale with the ratio of the depths is not available here,
        # so keep the value (it is only the starting point of the solve; the geometry is carried by the observations)
        dense.a["inv_depth"][w, k] = lam[e]
        o += n
    dense.a["n_feat"][w] = nf


def test_window_solve_parity_over_random_track_structures(estimator, oracle):
    """Track tables the two synthetic shapes never produce: all tracks of length 2, frames nobody observes, a single
    feature, every start at the last admissible frame, full-length tracks only, and random mixtures - states, iteration
    and accept traces against the oracle."""
    rng = np.random.default_rng(11)
    structures = [
        lambda n: (np.zeros(n, int), np.full(n, 2)),                                  # frames 2..10 see nothing
        lambda n: (np.full(n, 7), np.full(n, 2)),                                     # everything starts at WINDOW_SIZE - 3
        lambda n: (rng.integers(0, 8, n), np.full(n, 2)),                             # shortest tracks everywhere
        lambda n: (np.zeros(n, int), np.full(n, 11)),                                 # full-length tracks
        lambda n: (np.array([3]), np.array([5])),                                     # one feature
        lambda n: (np.where(np.arange(n) % 2 == 0, 0, 6), np.where(np.arange(n) % 2 == 0, 3, 4)),  # two disjoint groups: frames 3-5 unseen
    ]
    for _ in range(6):
        structures.append(lambda n: (lambda a: (a, np.array([rng.integers(2, 12 - x) for x in a])))(rng.integers(0, 8, n)))
    B = len(structures)
    w = synth.make_windows(B, first_id=500, tracks="dense", n_feat=150, max_feat=150)
    for k, f in enumerate(structures):
        n = int(rng.integers(5, 151))
        a, ln = f(n)
        _retrack(w, k, np.asarray(a), np.asarray(ln))
    wg, wo, sg, so = _solve_both(estimator, oracle, w)
    _assert_state_parity(wg, wo, sg, so)
    # and through the marginalization, both flavours
    est_m = importlib_est()
    for flag in (abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW):
        o = abi.default_options()
        o.marginalization_flag = flag
        E = est_m.Estimator(ctx=estimator.ctx, options=o)
        wg2, wo2 = w.copy(), w.copy()
        E.optimization(wg2)
        po = buffers.PriorOutArrays.alloc(B)
        oracle.window_solve(o, wo2, po, buffers.summary_alloc(B))
        pg = E.last_marginalization_info
        assert np.array_equal(pg.a["n"], po.a["n"]) and np.array_equal(pg.a["nblk"], po.a["nblk"])
        for i in range(B):
            if po.a["n"][i] <= 0:
                continue
            ng, Hg, bg, _ = _prior_quadratic(pg, i)
            no, Ho, bo, _ = _prior_quadratic(po, i)
            if flag == abi.MARGIN_SECOND_NEW:
                assert rel(Hg, Ho) < 1e-9 and rel(bg, bo) < 1e-9, (flag, i, rel(Hg, Ho), rel(bg, bo))
        if flag == abi.MARGIN_OLD:
            # MARGIN_OLD goes through the eigen pseudo-inverse of an ill-conditioned Amm (two-view tracks), which FP64 only
            # determines to 1e-5: the arbiter is the binary128 statement of the reference's algorithm (oracle/avm_truth.cpp,
            # tests/test_prior_truth.py), each side against the exact result at the state it marginalized at
            from marg_sensitivity import distance_to_truth, marginalize_at, truth_marginalize
            (pg0, at_g), (po0, at_o) = marginalize_at(wo2, o, estimator=E), marginalize_at(wo2, o)
            dg_t, do_t = truth_marginalize(at_g, o)[1], truth_marginalize(at_o, o)[1]
            worst_g, worst_o = {}, {}
            for i in range(B):
                dg, do = distance_to_truth(pg0, dg_t, i), distance_to_truth(po0, do_t, i)
                for k in dg:
                    worst_g[k], worst_o[k] = max(worst_g.get(k, 0.0), dg[k]), max(worst_o.get(k, 0.0), do[k])
            print("\n[random track structures, MARGIN_OLD prior vs truth] gpu", worst_g, "oracle", worst_o)
            floor = dict(H_rel=1e-6, H_scaled=1e-5, g_scaled=1e-9, cost_rel=1e-6)
            for k in worst_g:
                assert worst_g[k] <= max(worst_o[k], floor[k]), (k, worst_g[k], worst_o[k])


def test_window_solve_without_prior_and_mixed_batch(estimator, oracle):
    a = synth.make_windows(2, tracks="sparse", n_feat=40, max_feat=150, with_prior=False)
    b = synth.make_windows(2, first_id=7, tracks="dense", n_feat=100, max_feat=150)
    dims = dict(a.dims)
    dims["n_windows"] = 4
    w = buffers.WindowArrays(dims, {k: np.concatenate([a.a[k], b.a[k]]) for k in a.a})
    wg, wo, sg, so = _solve_both(estimator, oracle, w)
    _assert_state_parity(wg, wo, sg, so)


def test_window_solve_degenerate_inputs(estimator, oracle):
    # no features at all (IMU + prior only) and a window whose IMU interval is too long (factor skipped, sum_dt > 10)
    w = synth.make_windows(2, tracks="sparse", n_feat=20, max_feat=150)
    w.a["n_feat"][0] = 0
    w.a["imu_dt"][1, 4, :] = 0.6  # 20 * 0.6 = 12 s > 10 s
    wg, wo, sg, so = _solve_both(estimator, oracle, w)
    _assert_state_parity(wg, wo, sg, so)


def test_gauge_fix_near_pitch_90_takes_the_full_rotation_branch(estimator, oracle):
    """double2vector (estimator.cpp:536-546): within one degree of pitch +-90 the yaw-only correction is replaced by the full
    rot_diff = Rs[0] * R00^T.  The whole synthetic world (poses, velocities, gravity) is turned so that frame 0 looks straight
    up / down; observations and IMU samples are body-frame quantities and stay."""
    for wid, target in ((60, 89.6), (61, -89.5), (62, 90.8)):
        w = synth.make_windows(1, first_id=wid, tracks="sparse", n_feat=60, max_feat=150, with_prior=False)
        R0 = synth.R_from_quat(w.a["pose"][0, 0, 3:])
        s_, c_ = np.sin(np.radians(target)), np.cos(np.radians(target))
        x, y = np.array([c_, 0.0, -s_]), np.array([0.0, 1.0, 0.0])       # R2ypr: pitch = atan2(-R[2,0], .) -> first column (c, 0, -s)
        Rw = np.stack([x, y, np.cross(x, y)], 1) @ R0.T
        for f in range(11):
            w.a["pose"][0, f, :3] = Rw @ w.a["pose"][0, f, :3]
            w.a["pose"][0, f, 3:] = synth.quat_from_R(Rw @ synth.R_from_quat(w.a["pose"][0, f, 3:]))
            w.a["speedbias"][0, f, :3] = Rw @ w.a["speedbias"][0, f, :3]
        o = abi.default_options()
        o.marginalization_flag = abi.MARGIN_NONE
        o.g[0], o.g[1], o.g[2] = Rw @ np.array([0, 0, 9.81007])
        Rb = synth.R_from_quat(w.a["pose"][0, 0, 3:])
        pitch = np.degrees(np.arctan2(-Rb[2, 0], Rb[0, 0] * np.cos(np.arctan2(Rb[1, 0], Rb[0, 0])) + Rb[1, 0] * np.sin(np.arctan2(Rb[1, 0], Rb[0, 0]))))
        assert abs(abs(pitch) - 90) < 1.0
        wg, wo, sg, so = _solve_both(estimator, oracle, w, o)
        _assert_state_parity(wg, wo, sg, so)
        assert (sg["final_cost"] < 1e-2 * sg["initial_cost"]).all()
        # frame 0 keeps its WHOLE attitude in this branch, not just its yaw
        assert rel(synth.R_from_quat(wg.a["pose"][0, 0, 3:]), Rb) < 1e-9


def test_small_trust_region_dogleg_branches_parity(estimator, oracle):
    o = abi.default_options()
    o.marginalization_flag = abi.MARGIN_NONE
    o.initial_trust_region_radius = 1e-2
    o.max_num_iterations = 12
    w = synth.make_windows(2, tracks="sparse", n_feat=40, max_feat=150)
    wg, wo, sg, so = _solve_both(estimator, oracle, w, o)
    assert rel(sg["radius_trace"], so["radius_trace"]) < 1e-9
    _assert_state_parity(wg, wo, sg, so)


def test_speculative_evaluation_is_exact_including_rejected_steps(estimator, oracle, monkeypatch):
    """The solve evaluates the Jacobian at the candidate directly while steps keep being accepted (one evaluation
    per iteration instead of Ceres' two); a rejected speculation restores the system at x.  Same accept/reject
    decisions and the same states as the classic order of evaluations, and as the oracle."""
    rng = np.random.default_rng(7)
    n = 64
    w = synth.make_windows(n, tracks="dense")
    q = w.a["pose"][:, 1:, 3:] + rng.normal(0, 0.5, w.a["pose"][:, 1:, 3:].shape)   # wild attitudes: many rejected steps
    w.a["pose"][:, 1:, 3:] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    w.a["pose"][:, 1:, :3] += rng.normal(0, 1.0, w.a["pose"][:, 1:, :3].shape)
    g1, g2, wo = w.copy(), w.copy(), w.copy()
    monkeypatch.setenv("AVM_NO_SPECULATE", "0")
    s1 = buffers.summary_to_numpy(estimator.optimization(g1))
    monkeypatch.setenv("AVM_NO_SPECULATE", "1")
    s2 = buffers.summary_to_numpy(estimator.optimization(g2))
    so = buffers.summary_alloc(n)
    oracle.window_solve(estimator.options, wo, None, so, n_threads=8)
    fin = np.isfinite(g1.a["pose"]).all(axis=(1, 2)) & np.isfinite(wo.a["pose"]).all(axis=(1, 2))
    rejected = (s1["num_iterations"] > s1["num_successful"]) & fin
    assert rejected.sum() >= 2, "the perturbation no longer produces rejected steps"
    # speculative == classic order of evaluations
    assert (s1["accept_mask"] == s2["accept_mask"]).all() and (s1["termination"] == s2["termination"]).all()
    assert (np.isfinite(g2.a["pose"]).all(axis=(1, 2)) == np.isfinite(g1.a["pose"]).all(axis=(1, 2))).all()
    assert rel(g1.a["pose"][fin], g2.a["pose"][fin]) < 1e-9
    # and both follow the oracle through every rejected step: same accept / reject decisions, same radii, same states
    same = fin & (s1["accept_mask"] == so["accept_mask"]) & (s1["termination"] == so["termination"])
    per_window = np.array([rel(g1.a["pose"][i], wo.a["pose"][i]) for i in np.flatnonzero(same)])
    print("\n[speculation] finite", int(fin.sum()), "same decisions", int(same.sum()), "with rejected steps", int((rejected & same).sum()),
          "worst pose gap", float(per_window.max()), "median", float(np.median(per_window)))
    assert same.sum() == fin.sum() and (rejected & same).sum() >= 10
    # (the states themselves: starting points this far off end in badly conditioned minima, where 1e-11 per iteration grows)
    assert np.median(per_window) < STATE_TOL and (per_window < 1e-4).mean() >= 0.8
    for i in np.flatnonzero(same & rejected)[:8]:
        n = int(s1["num_iterations"][i])
        assert rel(s1["radius_trace"][i][:n], so["radius_trace"][i][:n]) < 1e-4, i   # radius = 3 |step| follows the (wild) states


def test_observation_table_with_holes_solves_like_the_compact_one(estimator, monkeypatch):
    """avm_slide_window drops a feature's first observation in place, so the observation table of a rolled window has
    holes.  The slot-indexed loops of the solve (the residual-only evaluation, the Cauchy point's |J u|^2) must not see
    them - not even through what an earlier solve left in the context's slot map."""
    o = abi.default_options()
    o.marginalization_flag = abi.MARGIN_NONE
    o.initial_trust_region_radius = 1e-1          # radius-limited steps: every iteration computes the Cauchy point
    E = importlib_est().Estimator(ctx=estimator.ctx, options=o)
    w = synth.make_windows(4, tracks="sparse", n_feat=50, max_feat=150)
    holes = w.copy()
    a, b = w.a, holes.a
    for k in range(4):
        n = a["n_feat"][k]
        assert a["feat_obs_begin"][k, n - 1] + a["feat_nobs"][k, n - 1] + 2 * n <= a["obs_xy"].shape[1]
        b["obs_xy"][k] = 1e3                      # what a hole holds must never be read as an observation
        for e in range(n):
            s0, no = a["feat_obs_begin"][k, e], a["feat_nobs"][k, e]
            b["feat_obs_begin"][k, e] = s0 + 2 * e + 1
            b["obs_xy"][k, s0 + 2 * e + 1:s0 + 2 * e + 1 + no] = a["obs_xy"][k, s0:s0 + no]
    for spec in ("0", "1"):                        # "1": every candidate goes through the residual-only evaluation
        monkeypatch.setenv("AVM_NO_SPECULATE", spec)
        E.optimization(synth.make_windows(4, tracks="dense"))    # leaves a different slot map behind
        g1, g2 = w.copy(), holes.copy()
        s1 = buffers.summary_to_numpy(E.optimization(g1))
        s2 = buffers.summary_to_numpy(E.optimization(g2))
        assert (s1["num_iterations"] >= 3).all()
        for k in ("pose", "speedbias", "inv_depth"):
            assert np.array_equal(g1.a[k], g2.a[k]), (spec, k)
        # (a factor's slot decides which thread adds its cost: the sums agree to rounding, the decisions exactly)
        assert rel(s1["cost_trace"], s2["cost_trace"]) < 1e-13 and np.array_equal(s1["accept_mask"], s2["accept_mask"])


def test_solve_is_bit_reproducible_and_shard_invariant(estimator):
    w = synth.make_windows(6, tracks="sparse", n_feat=50, max_feat=150)
    a, b = w.copy(), w.copy()
    estimator.optimization(a)
    estimator.optimization(b)
    for k in ("pose", "speedbias", "inv_depth"):
        assert np.array_equal(a.a[k], b.a[k])
    # the same windows solved as two shards (what two ranks would do) give bit-identical states
    lo, hi = w.slice(0, 3).copy(), w.slice(3, 6).copy()
    estimator.optimization(lo)
    estimator.optimization(hi)
    for k in ("pose", "speedbias", "inv_depth"):
        assert np.array_equal(np.concatenate([lo.a[k], hi.a[k]]), a.a[k])


def test_full_size_batch_properties(ctx, oracle):
    """BASELINE.json configs[3] size (4096 windows x 150 features x 1500 factors, MARGIN_OLD) through size-independent
    properties: every copy of a window gives bit-identical states / priors whichever workgroup slot solved it, costs
    decrease, everything is finite, and the new prior reproduces A' = J^T J of the oracle-checked small case shape."""
    opt = abi.default_options()
    E = importlib_est().Estimator(ctx=ctx, options=opt)
    base = synth.make_windows(32, tracks="dense")
    big = synth.tile_windows(base, 4096).to_device("cuda:0")
    summ = buffers.summary_to_numpy(E.optimization(big))
    out, prior = big.to_host(), E.last_marginalization_info.to_host()
    assert np.isfinite(out.a["pose"]).all() and np.isfinite(prior.a["J"]).all()
    assert (summ["final_cost"] <= summ["initial_cost"]).all() and (summ["num_successful"] >= 1).all()
    assert (prior.a["n"] == 75).all() and (prior.a["nblk"] == 12).all()
    for k in ("pose", "speedbias", "inv_depth"):
        a = out.a[k].reshape(128, 32, *out.a[k].shape[1:])
        assert (a == a[0]).all(), k                                   # 128 copies of each of the 32 windows
    J = prior.a["J"].reshape(128, 32, 96, 96)
    assert (J == J[0]).all()
    # ... and the 32 distinct windows of the BASELINE-size batch against the oracle: same decisions, states within tolerance
    wo, so, po = base.copy(), buffers.summary_alloc(32), buffers.PriorOutArrays.alloc(32)
    oracle.window_solve(opt, wo, po, so, n_threads=8)
    assert np.array_equal(summ["accept_mask"][:32], so["accept_mask"]) and np.array_equal(summ["termination"][:32], so["termination"])
    for k in ("pose", "speedbias", "inv_depth"):
        assert rel(out.a[k][:32], wo.a[k]) < STATE_TOL, (k, rel(out.a[k][:32], wo.a[k]))
    assert np.array_equal(prior.a["n"][:32], po.a["n"]) and np.array_equal(prior.a["blk_kind"][:32], po.a["blk_kind"])
    # the prior is a square root: J^T J is symmetric positive semi-definite with the kept dimension's rank or less
    A = J[0, 0, :75, :75].T @ J[0, 0, :75, :75]
    assert np.linalg.eigvalsh(A).min() > -1e-6 * np.abs(A).max()
    # the gauge fix of double2vector (estimator.cpp:521-587): frame 0 keeps its yaw and its position in every window
    q0, q1 = synth.tile_windows(base, 4096).a["pose"][:, 0, 3:], out.a["pose"][:, 0, 3:]
    yaw = lambda q: np.arctan2(2 * (q[:, 0] * q[:, 1] + q[:, 2] * q[:, 3]), 1 - 2 * (q[:, 1] ** 2 + q[:, 2] ** 2))
    assert np.abs(yaw(q1) - yaw(q0)).max() < 1e-10
    assert np.abs(out.a["pose"][:, 0, :3] - synth.tile_windows(base, 4096).a["pose"][:, 0, :3]).max() < 1e-12
    assert np.abs(np.linalg.norm(out.a["pose"][..., 3:], axis=-1) - 1).max() < 1e-12


def test_device_resident_buffers_match_host_path(estimator):
    import torch

    w = synth.make_windows(4, tracks="dense", n_feat=60, max_feat=150)
    h = w.copy()
    host_summary = buffers.summary_to_numpy(estimator.optimization(h)).copy()
    d = w.to_device("cuda:0")
    s = estimator.optimization(d)
    torch.cuda.synchronize()
    assert np.array_equal(d.a["pose"].cpu().numpy(), h.a["pose"])
    sh = buffers.summary_to_numpy(s)
    for k in ("num_iterations", "num_successful", "accept_mask", "termination", "cost_trace", "radius_trace"):
        assert np.array_equal(sh[k], host_summary[k]), k
    assert (sh["num_iterations"] >= 1).all() and (sh["num_iterations"] <= estimator.options.max_num_iterations).all()


def test_capacity_and_unsupported_errors(ctx, abi):
    lib_m = __import__("importlib").import_module("anticipated-vins-mono_amd.lib")
    est_m = __import__("importlib").import_module("anticipated-vins-mono_amd.estimator")
    o = abi.default_options()
    o.estimate_td = 1   # ... without the per-observation velocities / cur_td / rows and para_Td: refused, nothing runs
    with pytest.raises(lib_m.AvmError, match="-1.*obs_vel_td"):
        est_m.Estimator(ctx=ctx, options=o).optimization(synth.make_windows(1, tracks="sparse", n_feat=5, max_feat=150))
    wr = synth.make_windows(1, tracks="sparse", n_feat=5, max_feat=150, relo=True)
    del wr.a["relo_xy"]
    with pytest.raises(lib_m.AvmError, match="-1.*relo"):
        est_m.Estimator(ctx=ctx, options=abi.default_options()).optimization(wr)
    # a prior_out that cannot hold the kept set (75 rows / 12 blocks here): AVM_ERR_CAPACITY, never a silently truncated prior
    E = est_m.Estimator(ctx=ctx, options=abi.default_options())
    w = synth.make_windows(2, tracks="sparse", n_feat=20, max_feat=150)
    for mp, mb in ((40, 16), (96, 8)):
        with pytest.raises(lib_m.AvmError, match="status -5.*window 0"):
            E.optimization(w.copy(), prior_out=buffers.PriorOutArrays.alloc(2, max_prior=mp, max_pblk=mb))
    E.optimization(w.copy(), prior_out=buffers.PriorOutArrays.alloc(2, max_prior=75, max_pblk=12))   # exactly enough
    # a prior_out with a missing array is refused before anything runs
    po = buffers.PriorOutArrays.alloc(2)
    del po.a["x0"]
    with pytest.raises(lib_m.AvmError, match="-1"):
        E.optimization(w.copy(), prior_out=po)


@pytest.mark.parametrize("where", ["host", "device"])
def test_malformed_tables_are_rejected_before_any_kernel_indexes_with_them(ctx, abi, selector, where):
    """Every entry point validates the caller's tables first (host tables on the host, device-resident ones by a
    one-thread-per-window kernel): AVM_ERR_INVALID naming the first bad window and the rule, states untouched."""
    lib_m = __import__("importlib").import_module("anticipated-vins-mono_amd.lib")
    est_m = __import__("importlib").import_module("anticipated-vins-mono_amd.estimator")
    E = est_m.Estimator(ctx=ctx, options=abi.default_options())
    good = synth.make_windows(3, tracks="sparse", n_feat=40, max_feat=150)
    nf = int(good.a["n_feat"][1])

    def broken(key, idx, value):
        w = good.copy()
        w.a[key][idx] = value
        return w

    cases = [
        (broken("n_feat", 1, 151), "window 1: n_feat"),
        (broken("n_feat", 2, -1), "window 2: n_feat"),
        (broken("feat_nobs", (1, 3), 12), "window 1: a feature track leaves the window"),
        (broken("feat_start", (1, nf - 1), 0) if good.a["feat_start"][1, nf - 1] > 0 else None, "window 1: feat_start must be non-decreasing"),
        (broken("feat_obs_begin", (0, 2), good.dims["max_obs"] - 1), "window 0: feat_obs_begin"),
        (broken("imu_n", (2, 4), good.dims["max_samp"] + 1), "window 2: imu_n"),
        (broken("prior_nblk", 1, 3), "window 1: prior tables"),
        (broken("prior_blk_frame", (0, 0), 11), "window 0: prior tables"),
    ]
    for w, msg in cases:
        if w is None:
            continue
        before = w.a["pose"].copy()
        x = w.to_device("cuda:0") if where == "device" else w
        with pytest.raises(lib_m.AvmError, match="status -1: " + msg):
            E.optimization(x)
        after = x.a["pose"].cpu().numpy() if where == "device" else x.a["pose"]
        assert np.array_equal(after, before)
    # the other entry points share the check
    w = broken("feat_nobs", (1, 3), 12)
    x = w.to_device("cuda:0") if where == "device" else w
    with pytest.raises(lib_m.AvmError, match="window 1: a feature track"):
        E.triangulate(x)
    with pytest.raises(lib_m.AvmError, match="window 1: a feature track"):
        E.slideWindow(x, abi.MARGIN_OLD)
    w = broken("imu_n", (0, 9), -2)
    x = w.to_device("cuda:0") if where == "device" else w
    with pytest.raises(lib_m.AvmError, match="window 0: imu_n"):
        E.imu_propagate(x)
    # selector
    pr = synth.make_fsel(2, horizon=5, n_cand=20, n_used=2, n_cloud=10, max_features=8)
    pr.a["n_cand"][1] = 21
    x = pr.to_device("cuda:0") if where == "device" else pr
    with pytest.raises(lib_m.AvmError, match="frame 1: n_cand"):
        selector.select_batch(x)
    # a single frame (all greedy rounds in one launch; the check of a device-resident frame runs ahead on the stream)
    pr1 = synth.make_fsel(1, horizon=5, n_cand=20, n_used=2, n_cloud=10, max_features=8)
    good1 = pr1.to_device("cuda:0") if where == "device" else pr1.copy()
    pr1.a["n_cand"][0] = 21
    x = pr1.to_device("cuda:0") if where == "device" else pr1
    with pytest.raises(lib_m.AvmError, match="frame 0: n_cand"):
        selector.select_batch(x)
    assert int(selector.select_batch(good1).to_host().a["n_selected"][0]) == 6
    # and a well-formed batch still runs afterwards on the same ctx
    ok = good.to_device("cuda:0") if where == "device" else good.copy()
    E.optimization(ok)


def _poisoned_windows():
    w = synth.make_windows(6, tracks="sparse", n_feat=40, max_feat=150)
    w.a["pose"][0, 3, 0] = np.nan          # a NaN state
    w.a["obs_xy"][1, 5, 0] = np.inf        # an infinite measurement
    w.a["imu_dt"][2, :, :] = 0.0           # zero-length IMU intervals: singular pre-integration covariance
    w.a["inv_depth"][3, :10] = 0.0         # points at infinity
    w.a["prior_J"][4] = np.nan             # a poisoned prior
    return w


def test_non_finite_inputs_terminate_like_the_oracle_and_do_not_leak_into_other_windows(ctx, oracle):
    """NaN / Inf / singular inputs: the solve gives up after max_num_consecutive_invalid_steps like Ceres does (FAILURE),
    the marginalization still runs, nothing hangs, and the healthy window of the same batch is solved as usual."""
    est_m = __import__("importlib").import_module("anticipated-vins-mono_amd.estimator")
    o = abi.default_options()
    E = est_m.Estimator(ctx=ctx, options=o)
    w = _poisoned_windows()
    wg, wo = w.copy(), w.copy()
    sg = E.optimization(wg)
    so, po = buffers.summary_alloc(6), buffers.PriorOutArrays.alloc(6)
    oracle.window_solve(o, wo, po, so)
    assert sg["termination"].tolist() == so["termination"].tolist() == [abi.TERM_NAMES.index("FAILURE")] * 5 + [0]
    assert sg["num_iterations"].tolist() == so["num_iterations"].tolist()
    assert rel(wg.a["pose"][5], wo.a["pose"][5]) < STATE_TOL
    assert np.array_equal(E.last_marginalization_info.a["n"], po.a["n"])
    for k in range(5):  # a failed solve leaves the states where they were (Ceres returns the initial point)
        same = (wg.a["pose"][k] == w.a["pose"][k]) | (np.isnan(wg.a["pose"][k]) & np.isnan(w.a["pose"][k]))
        assert same.all() == ((wo.a["pose"][k] == w.a["pose"][k]) | (np.isnan(wo.a["pose"][k]) & np.isnan(w.a["pose"][k]))).all()


def test_non_finite_inputs_through_the_callers_either_side(ctx, oracle):
    """triangulate / dead-reckoning / window roll on NaN states, infinite measurements, zero-length IMU intervals and zero
    quaternions: same finite-ness pattern and same finite values as the oracle, nothing hangs."""
    est_m = __import__("importlib").import_module("anticipated-vins-mono_amd.estimator")
    o = abi.default_options()
    E = est_m.Estimator(ctx=ctx, options=o)

    def poisoned(depth):
        w = synth.make_windows(5, tracks="sparse", n_feat=40, max_feat=150)
        w.a["pose"][0, 3, 0] = np.nan
        w.a["obs_xy"][1, 5, 0] = np.inf
        w.a["imu_dt"][2, :, :] = 0.0
        w.a["pose"][3, :, 3:] = 0.0
        w.a["inv_depth"][:, :] = depth
        return w

    def agree(a, b, tol):
        assert np.array_equal(np.isfinite(a), np.isfinite(b))
        m = np.isfinite(a)
        assert rel(a[m], b[m]) < tol

    wg, wo = poisoned(-1.0), poisoned(-1.0)
    E.triangulate(wg, 5.0)
    oracle.triangulate(wo, 5.0)
    agree(wg.a["inv_depth"], wo.a["inv_depth"], 1e-9)
    wg, wo = poisoned(0.3), poisoned(0.3)
    E.imu_propagate(wg)
    oracle.imu_propagate(wo, [o.g[0], o.g[1], o.g[2]])
    agree(wg.a["pose"], wo.a["pose"], 1e-9)
    agree(wg.a["speedbias"], wo.a["speedbias"], 1e-9)
    wg, wo = poisoned(0.3), poisoned(0.3)
    E.slideWindow(wg, abi.MARGIN_OLD, True, 5.0)
    oracle.slide_window(wo, abi.MARGIN_OLD, True, 5.0)
    assert np.array_equal(wg.a["n_feat"], wo.a["n_feat"])
    agree(wg.a["inv_depth"], wo.a["inv_depth"], 1e-9)


def test_two_contexts_on_two_host_threads_are_independent(ctx, abi):
    """include/avm.h: one avm_ctx per host thread, re-entrant, no statics.  Two contexts driven concurrently from two
    threads (ctypes releases the GIL) give the bits of a serial run."""
    import threading

    lib_m = __import__("importlib").import_module("anticipated-vins-mono_amd.lib")
    est_m = importlib_est()
    fs_m = __import__("importlib").import_module("anticipated-vins-mono_amd.feature_selector")
    wa = synth.make_windows(24, first_id=300, tracks="dense", n_feat=120, max_feat=150)
    wb = synth.make_windows(24, first_id=400, tracks="sparse", n_feat=90, max_feat=150)
    pr = synth.make_fsel(2, first_id=9, horizon=5, n_cand=60, n_used=3, n_cloud=30, max_features=20)
    serial = {}
    E = est_m.Estimator(ctx=ctx, options=abi.default_options())
    for k, w in (("a", wa), ("b", wb)):
        x = w.copy()
        E.optimization(x)
        serial[k] = (x.a["pose"].copy(), E.last_marginalization_info.a["J"].copy())
    serial["f"] = fs_m.FeatureSelector(ctx=ctx).select_batch(pr).to_host().a["selected_ids"].copy()
    got, errs = {}, []

    def work(key, w):
        try:
            c = lib_m.Context(0)
            Ek = est_m.Estimator(ctx=c, options=abi.default_options())
            for _ in range(3):
                x = w.copy()
                Ek.optimization(x)
                got[key] = (x.a["pose"].copy(), Ek.last_marginalization_info.a["J"].copy())
                got["f" + key] = fs_m.FeatureSelector(ctx=c).select_batch(pr).to_host().a["selected_ids"].copy()
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=work, args=("a", wa)), threading.Thread(target=work, args=("b", wb))]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not errs, errs
    for k in ("a", "b"):
        assert np.array_equal(got[k][0], serial[k][0]) and np.array_equal(got[k][1], serial[k][1]), k
        assert np.array_equal(got["f" + k], serial["f"])


def _prior_quadratic(p, i):
    n = int(p.a["n"][i])
    J, r = p.a["J"][i, :n, :n], p.a["r"][i, :n]
    return n, J.T @ J, J.T @ r, 0.5 * float(r @ r)


@pytest.mark.parametrize("flag", ["OLD", "SECOND_NEW"])
@pytest.mark.parametrize("tracks,nf", [("sparse", 60), ("dense", 150)])
def test_marginalization_parity(ctx, oracle, flag, tracks, nf):
    est_m = __import__("importlib").import_module("anticipated-vins-mono_amd.estimator")
    o = abi.default_options()
    o.marginalization_flag = abi.MARGIN_OLD if flag == "OLD" else abi.MARGIN_SECOND_NEW
    E = est_m.Estimator(ctx=ctx, options=o)
    w = synth.make_windows(2, tracks=tracks, n_feat=nf, max_feat=150)
    wg, wo = w.copy(), w.copy()
    E.optimization(wg)
    pg = E.last_marginalization_info
    po = buffers.PriorOutArrays.alloc(2)
    oracle.window_solve(o, wo, po, buffers.summary_alloc(2))
    assert np.array_equal(pg.a["n"], po.a["n"]) and np.array_equal(pg.a["nblk"], po.a["nblk"])
    for i in range(2):
        nb = int(po.a["nblk"][i])
        assert np.array_equal(pg.a["blk_kind"][i, :nb], po.a["blk_kind"][i, :nb])
        assert np.array_equal(pg.a["blk_frame"][i, :nb], po.a["blk_frame"][i, :nb])
        assert rel(pg.a["x0"][i, :nb], po.a["x0"][i, :nb]) < STATE_TOL
        # the prior only ever enters through J^T J, J^T r and |r|^2 (eigenvector signs/order are arbitrary);
        # MARGIN_OLD goes through the eigen-pseudo-inverse of an ill-conditioned Amm: conditioning-limited agreement
        n, Hg, gg, cg = _prior_quadratic(pg, i)
        _, Ho, go, co = _prior_quadratic(po, i)
        d = 1.0 / np.sqrt(np.diag(Ho))
        tol = 1e-9 if flag == "SECOND_NEW" else 2e-3
        assert rel(Hg, Ho) < (1e-11 if flag == "SECOND_NEW" else 1e-5)
        assert rel(Hg * d[:, None] * d[None, :], Ho * d[:, None] * d[None, :]) < tol
        assert rel(gg * d, go * d) < tol
        assert abs(cg - co) <= 1e-3 * co


def test_marginalization_rank_deficient_amm_takes_the_eigen_path(ctx, oracle):
    """Amm^+ of the marginalized pose0 / speed-bias0 block: the Cholesky fast path is only taken when no eigenvalue can be
    below eps (trace(Amm^-1) < 1/eps).  Without a prior and with IMU factor 0 skipped (sum_dt > 10 s) the speed-bias of
    frame 0 has no information at all: zero pivots -> eigen-decomposition with clamped eigenvalues, as in the reference."""
    est_m = __import__("importlib").import_module("anticipated-vins-mono_amd.estimator")
    o = abi.default_options()
    E = est_m.Estimator(ctx=ctx, options=o)
    w = synth.make_windows(2, tracks="dense", n_feat=60, max_feat=150, with_prior=False, max_samp=60)
    w.a["imu_n"][:, 0] = 55
    w.a["imu_dt"][:, 0, :55] = 0.2                       # 11 s: pre_integrations[1]->sum_dt > 10 -> factor skipped (estimator.cpp:705)
    w.a["imu_acc"][:, 0, 1:56] = w.a["imu_acc"][:, 0, :1]
    w.a["imu_gyr"][:, 0, 1:56] = 0.0
    wg, wo = w.copy(), w.copy()
    E.optimization(wg)
    pg, po = E.last_marginalization_info, buffers.PriorOutArrays.alloc(2)
    oracle.window_solve(o, wo, po, buffers.summary_alloc(2))
    assert np.array_equal(pg.a["n"], po.a["n"]) and np.array_equal(pg.a["nblk"], po.a["nblk"])
    for i in range(2):
        n, Hg, gg, cg = _prior_quadratic(pg, i)
        _, Ho, go, co = _prior_quadratic(po, i)
        d = 1.0 / np.sqrt(np.maximum(np.diag(Ho), 1e-300))
        assert np.isfinite(Hg).all() and rel(Hg, Ho) < 1e-5
        assert rel(Hg * d[:, None] * d[None, :], Ho * d[:, None] * d[None, :]) < 2e-3


def test_marginalization_keeps_old_prior_when_second_new_has_nothing_to_drop(ctx, oracle):
    est_m = __import__("importlib").import_module("anticipated-vins-mono_amd.estimator")
    o = abi.default_options()
    o.marginalization_flag = abi.MARGIN_SECOND_NEW
    E = est_m.Estimator(ctx=ctx, options=o)
    w = synth.make_windows(2, tracks="sparse", n_feat=30, max_feat=150, with_prior=False)
    wo = w.copy()
    E.optimization(w)
    # no prior before, none after (estimator.cpp:926-927 leaves last_marginalization_info alone); the raw ABI says n == -1
    assert (E.last_marginalization_info.a["n"] == 0).all()
    po = buffers.PriorOutArrays.alloc(2)
    oracle.window_solve(o, wo, po, buffers.summary_alloc(2))
    assert (po.a["n"] == -1).all()
    # a prior that does not contain pose[WINDOW_SIZE - 1]: the mirror hands the SAME prior back, and it chains into the next solve
    w = synth.make_windows(2, first_id=40, tracks="sparse", n_feat=30, max_feat=150)
    for b in range(2):  # drop the pose-9 block from the synthetic prior: rows / columns 54..59
        keep = [i for i in range(75) if not 54 <= i < 60]
        J = w.a["prior_J"][b][np.ix_(keep, keep)].copy()
        w.a["prior_J"][b] = 0
        w.a["prior_J"][b, :69, :69] = J
        w.a["prior_r"][b, :69] = w.a["prior_r"][b, keep]
        w.a["prior_r"][b, 69:] = 0
        kinds, frames, x0 = w.a["prior_blk_kind"][b], w.a["prior_blk_frame"][b], w.a["prior_x0"][b]
        kinds[9:11], frames[9:11], x0[9:11] = kinds[10:12].copy(), frames[10:12].copy(), x0[10:12].copy()
        w.a["prior_n"][b], w.a["prior_nblk"][b] = 69, 11
    before = w.copy()
    E.optimization(w)
    p = E.last_marginalization_info
    assert (p.a["n"] == 69).all() and (p.a["nblk"] == 11).all()
    assert np.array_equal(p.a["J"][:, :69, :69], before.a["prior_J"][:, :69, :69]) and np.array_equal(p.a["r"][:, :69], before.a["prior_r"][:, :69])
    assert np.array_equal(p.a["blk_kind"][:, :11], before.a["prior_blk_kind"][:, :11]) and np.array_equal(p.a["x0"][:, :11], before.a["prior_x0"][:, :11])
    for k, v in (("prior_n", "n"), ("prior_nblk", "nblk"), ("prior_blk_kind", "blk_kind"), ("prior_blk_frame", "blk_frame"), ("prior_J", "J"),
                 ("prior_r", "r"), ("prior_x0", "x0")):
        w.a[k][:] = p.a[v]
    E.optimization(w)   # chained SECOND_NEW solve: the tables validate (no BAD_PRIOR) and the solve runs
    assert np.isfinite(w.a["pose"]).all()


# measured on MI355X in round 6 (printed by the test: pose 3.08e-6, speed-bias 5.68e-6 for both - the literal GPU chain sits on the exact-prior chain to
# 1e-10, so its distance from the FP64 oracle's chain IS the oracle's distance from the exact one), asserted at about three times the measurement
CHAIN_LITERAL_VS_ORACLE = {"pose": 1e-5, "speedbias": 2e-5}
CHAIN_ORACLE_VS_EXACT = {"pose": 1e-5, "speedbias": 2e-5}


def test_chained_solves_through_the_new_prior(ctx, oracle):
    """optimization() twice: the prior produced by the first MARGIN_OLD solve feeds the second solve
    (window roll is host bookkeeping: here the same factors are simply re-solved with the new prior)."""
    est_m = __import__("importlib").import_module("anticipated-vins-mono_amd.estimator")
    o = abi.default_options()
    E = est_m.Estimator(ctx=ctx, options=o)
    w = synth.make_windows(2, tracks="sparse", n_feat=50, max_feat=150)
    wg, wo = w.copy(), w.copy()
    E.optimization(wg)
    pg = E.last_marginalization_info
    po = buffers.PriorOutArrays.alloc(2)
    oracle.window_solve(o, wo, po, buffers.summary_alloc(2))

    def install(win, p):
        n = p.a["n"].astype(np.int32)
        win.a["prior_n"][:] = n
        win.a["prior_nblk"][:] = p.a["nblk"]
        win.a["prior_blk_kind"][:] = p.a["blk_kind"]
        win.a["prior_blk_frame"][:] = p.a["blk_frame"]
        win.a["prior_J"][:] = p.a["J"]
        win.a["prior_r"][:] = p.a["r"]
        win.a["prior_x0"][:] = p.a["x0"]

    # the reference chain: the FP64 solver with the EXACT prior (the marginalization in binary128 at the oracle's solution,
    # oracle/avm_truth.cpp).  The FP64 oracle's own prior leads 1e-7 .. 3e-6 away from it; the GPU's chain stays within the
    # north-star 1e-6 (measured 2e-11 .. 4e-10, tests/test_prior_truth.py)
    from marg_sensitivity import truth_marginalize
    wt = wo.copy()
    install(wt, truth_marginalize(wo, o)[0])
    install(wg, pg)
    install(wo, po)
    o2 = abi.default_options()
    o2.marginalization_flag = abi.MARGIN_NONE
    E2 = est_m.Estimator(ctx=ctx, options=o2)
    sg = E2.optimization(wg)
    so, st = buffers.summary_alloc(2), buffers.summary_alloc(2)
    oracle.window_solve(o2, wo, None, so)
    oracle.window_solve(o2, wt, None, st)
    assert np.array_equal(buffers.summary_to_numpy(sg)["accept_mask"], st["accept_mask"])
    for k in ("pose", "speedbias"):
        print(f"\n[chained solve vs exact-prior chain] {k}: gpu {rel(wg.a[k], wt.a[k]):.2e}  oracle {rel(wo.a[k], wt.a[k]):.2e}")
        assert rel(wg.a[k], wt.a[k]) < 1e-6, (k, rel(wg.a[k], wt.a[k]))
    # ... and the "equal to the reference" leg: the same chain with the REFERENCE-LITERAL clamp (marg_noise_rel = 0, what the
    # FP64 oracle always runs) against the FP64 oracle's own chain, asserted at the bounds measured in round 6 (CHAIN_LITERAL_VS_ORACLE below: two FP64
    # roundings of the pseudo-inverse of a 1e12-conditioned block apart - a regression of this leg is red, not a log line), and the oracle's own
    # distance from the exact-prior chain, so that the yardstick cannot move unnoticed either
    o_lit = abi.default_options()
    o_lit.marg_noise_rel = 0.0
    wl = w.copy()
    El = est_m.Estimator(ctx=ctx, options=o_lit)
    El.optimization(wl)
    install(wl, El.last_marginalization_info)
    sl = E2.optimization(wl)
    assert np.array_equal(buffers.summary_to_numpy(sl)["accept_mask"], so["accept_mask"])
    for k in ("pose", "speedbias"):
        dlo, dot = rel(wl.a[k], wo.a[k]), rel(wo.a[k], wt.a[k])
        print(f"[chained solve, reference-literal clamp vs the FP64 oracle's chain] {k}: {dlo:.2e}   (oracle vs exact-prior chain {dot:.2e})")
        assert dlo < CHAIN_LITERAL_VS_ORACLE[k], (k, dlo)
        assert dot < CHAIN_ORACLE_VS_EXACT[k], (k, dot)


# ---------------------------------------------------------------- HP-B
@pytest.mark.parametrize("H,nc,nu,mf,P", [(10, 80, 6, 30, 3), (13, 60, 0, 20, 2), (3, 30, 2, 10, 2), (5, 40, 0, 45, 1)])
def test_selector_information_and_ids(selector, oracle, H, nc, nu, mf, P):
    pr = synth.make_fsel(P, horizon=H, n_cand=nc, n_used=nu, max_features=mf)
    om, dl, va = selector.information(pr)
    oom, odl, ova = oracle.fsel_information(pr)
    assert rel(om, oom) < 1e-12
    assert np.array_equal(va, ova)
    assert rel(dl, odl) < 1e-10
    out = selector.select_batch(pr)
    oo = buffers.FselOutArrays.alloc(P, mf)
    oracle.fsel_select(pr, oo)
    assert np.array_equal(out.a["n_selected"], oo.a["n_selected"])
    assert np.array_equal(out.a["selected_ids"], oo.a["selected_ids"])  # bit-exact ids, in selection order
    n = int(oo.a["n_selected"][0])
    assert rel(out.a["fvalues"][0, :n], oo.a["fvalues"][0, :n]) < 1e-9


def test_selector_ids_over_many_frames(selector, oracle):
    """24 different frames (three horizons): selected ids identical to the oracle's, in selection order."""
    for H, nc, mf in ((10, 200, 60), (5, 150, 50), (13, 120, 30)):
        pr = synth.make_fsel(8, horizon=H, n_cand=nc, n_used=4, max_features=mf)
        out = selector.select_batch(pr)
        oo = buffers.FselOutArrays.alloc(8, mf)
        oracle.fsel_select(pr, oo, n_threads=8)
        assert np.array_equal(out.a["n_selected"], oo.a["n_selected"]) and (oo.a["n_selected"] > 0).all()
        assert np.array_equal(out.a["selected_ids"], oo.a["selected_ids"])


def _poisoned_frames():
    pr = synth.make_fsel(6, horizon=5, n_cand=40, n_used=3, n_cloud=20, max_features=12)
    pr.a["delta_imu"][0] = 0.0        # the reference's very first call: deltaF = 0 (feature_selector.cpp:85-91), Omega is not finite
    pr.a["hor_pos"][1, 2, 0] = np.nan  # one horizon frame is NaN: that frame sees nothing, the others still count
    pr.a["cand_xy"][2, 3] = np.nan     # one NaN candidate
    pr.a["cand_prob"][3, :] = 0.0      # no candidate adds information
    pr.a["cloud_depth"][4, :] = np.inf
    return pr


def test_selector_non_finite_inputs_match_the_oracle(selector, oracle):
    pr = _poisoned_frames()
    og = selector.select_batch(pr).to_host()
    oo = buffers.FselOutArrays.alloc(6, 12)
    oracle.fsel_select(pr, oo)
    assert oo.a["n_selected"].tolist() == [0, 9, 9, 9, 0, 9]
    assert np.array_equal(og.a["n_selected"], oo.a["n_selected"])
    assert np.array_equal(og.a["selected_ids"], oo.a["selected_ids"])


def test_selector_reference_horizon_at_scale(selector, oracle):
    """HORIZON = 13 (state_defs.h:8, the value the reference is compiled with), 800 candidates, 20 already tracked,
    maxFeatures 170: 150 greedy rounds on 39 x 39 position blocks - identical ids in identical order."""
    pr = synth.make_fsel(1, first_id=77, horizon=13, n_cand=800, n_used=20, n_cloud=150, max_features=170)
    og = selector.select_batch(pr).to_host()
    oo = buffers.FselOutArrays.alloc(1, 170)
    oracle.fsel_select(pr, oo)
    assert oo.a["n_selected"][0] == 150
    assert np.array_equal(og.a["n_selected"], oo.a["n_selected"])
    assert np.array_equal(og.a["selected_ids"], oo.a["selected_ids"])
    assert rel(og.a["fvalues"][0, :150], oo.a["fvalues"][0, :150]) < 1e-9


def test_depth_cloud_matches_oracle(selector, oracle):
    """B8 (first half): FeatureSelector::initKDTree's cloud on device; it then feeds select() unchanged."""
    B = 5
    w = synth.make_windows(B, tracks="sparse", n_feat=90, max_feat=150)
    w.a["inv_depth"][:, 3::7] *= -1.0
    w.a["n_feat"][4] = 0                                          # empty window -> empty cloud
    rng = np.random.default_rng(5)
    k1_pos = w.a["pose"][:, 10, :3] + 0.1 * rng.normal(size=(B, 3))
    k1_quat = w.a["pose"][:, 10, 3:].copy()
    for mc in (150, 9):
        n, xy, dep = selector.initKDTree(w, k1_pos, k1_quat, max_cloud=mc)
        on, oxy, odep = oracle.fsel_build_cloud(w, k1_pos, k1_quat, max_cloud=mc)
        assert np.array_equal(n, on) and n[4] == 0 and n[:4].min() > 0
        assert rel(xy, oxy) < 1e-13 and np.array_equal(dep, odep)
    # the device-built cloud drives the selector to the oracle's ids
    P = 2
    prob = synth.make_fsel(P, horizon=5, n_cand=60, n_cloud=40, max_features=15)
    mc = prob.a["cloud_xy"].shape[1]
    n, xy, dep = selector.initKDTree(w, k1_pos, k1_quat, max_cloud=mc)
    prob.a["n_cloud"][:], prob.a["cloud_xy"][:], prob.a["cloud_depth"][:] = n[:P], xy[:P], dep[:P]
    out = selector.select_batch(prob).to_host()
    oo = buffers.FselOutArrays.alloc(P, 15)
    oracle.fsel_select(prob, oo)
    assert np.array_equal(out.a["n_selected"], oo.a["n_selected"]) and np.array_equal(out.a["selected_ids"], oo.a["selected_ids"])


def test_horizon_generator_imu_matches_oracle(selector, oracle):
    """B4: HorizonGenerator::imu on device, and its output feeding select()."""
    rng = np.random.default_rng(11)
    for H in (3, 10, 13):
        q = rng.normal(size=(6, 2, 4)); q /= np.linalg.norm(q, axis=-1, keepdims=True)
        i = dict(k_pos=rng.normal(size=(6, 3)), k_quat=q[:, 0], k_ba=0.02 * rng.normal(size=(6, 3)), k1_pos=rng.normal(size=(6, 3)),
                 k1_vel=rng.normal(size=(6, 3)), k1_quat=q[:, 1], acc=np.array([0, 0, 9.8]) + rng.normal(size=(6, 3)),
                 gyr=0.3 * rng.normal(size=(6, 3)), nr_imu=rng.integers(0, 25, 6), delta_imu=np.full(6, 0.005))
        gp, gq = selector.generateFutureHorizon(H, **i)
        op, oq = oracle.fsel_horizon_imu(H, **i)
        assert rel(gp, op) < 1e-13 and rel(gq, oq) < 1e-13
    # a generated horizon drives the selector to the same ids as the oracle
    prob = synth.make_fsel(2, horizon=5, n_cand=60, n_cloud=40, max_features=15)
    P = 2
    hp, hq = prob.a["hor_pos"], prob.a["hor_quat"]
    vel = (hp[:, 1] - hp[:, 0]) / (prob.a["nr_imu"] * prob.a["delta_imu"])[:, None]
    args = dict(k_pos=hp[:, 0], k_quat=hq[:, 0], k_ba=np.zeros((P, 3)), k1_pos=hp[:, 1], k1_vel=vel, k1_quat=hq[:, 1],
                acc=np.tile([0.1, 0.0, 9.80665], (P, 1)), gyr=np.tile([0.0, 0.0, 0.1], (P, 1)), nr_imu=prob.a["nr_imu"], delta_imu=prob.a["delta_imu"])
    gp, gq = selector.generateFutureHorizon(5, **args)
    prob.a["hor_pos"], prob.a["hor_quat"] = gp, gq
    out = selector.select_batch(prob).to_host()
    oo = buffers.FselOutArrays.alloc(P, 15)
    oracle.fsel_select(prob, oo)
    assert np.array_equal(out.a["n_selected"], oo.a["n_selected"]) and np.array_equal(out.a["selected_ids"], oo.a["selected_ids"])


def test_selector_headline_500_to_150(selector, oracle):
    pr = synth.make_fsel(1, horizon=10, n_cand=500, n_used=0, max_features=150)
    out = selector.select_batch(pr)
    oo = buffers.FselOutArrays.alloc(1, 150)
    oracle.fsel_select(pr, oo)
    assert int(out.a["n_selected"][0]) == 150
    assert np.array_equal(out.a["selected_ids"], oo.a["selected_ids"])


def _mirror_frame(H=5, npairs=20, n_used=3, seed=0):
    """A frame whose candidates come in mirror pairs (x, y) / (-x, y) of equal probability in front of a camera that moves
    straight along its optical axis (identity attitudes, identity extrinsics): the DIAGONALS of the two Delta_l are
    bit-identical (every x enters them squared), the off-diagonals are not - equal Hadamard upper bounds, different logdets.
    Asymmetric already-tracked features make Omega asymmetric under the mirror."""
    rng = np.random.default_rng(seed)
    pr = synth.make_fsel(1, horizon=H, n_cand=2 * npairs, n_used=n_used, n_cloud=30, max_features=n_used + 12)
    a = pr.a
    a["hor_quat"][0, :] = [0, 0, 0, 1]
    a["hor_pos"][0, :, :] = 0
    a["hor_pos"][0, :, 2] = 0.15 * np.arange(H + 1)
    pr.scalars["q_ic"], pr.scalars["t_ic"] = np.array([0, 0, 0, 1.0]), np.zeros(3)
    xy = np.stack([rng.uniform(0.05, 0.5, npairs), rng.uniform(-0.3, 0.3, npairs)], 1)
    a["cand_xy"][0, 0:2 * npairs:2], a["cand_xy"][0, 1:2 * npairs:2] = xy, xy * np.array([-1, 1])
    p = rng.uniform(0.3, 1.0, npairs).astype(np.float32).astype(float)
    a["cand_prob"][0, 0:2 * npairs:2], a["cand_prob"][0, 1:2 * npairs:2] = p, p
    a["n_cloud"][0], a["cloud_xy"][0, 0], a["cloud_depth"][0, 0] = 1, [0, 0], 6.0      # one cloud point: the same depth for everybody
    a["used_xy"][0, :n_used] = np.stack([rng.uniform(0.1, 0.5, n_used), rng.uniform(-0.3, 0.3, n_used)], 1)
    return pr


def test_selector_equal_upper_bounds_follow_the_std_map_rule(selector, oracle, monkeypatch):
    """sortedlogDetUB stores the bounds in a std::map<double, int> (feature_selector.cpp:724): of two live candidates with
    bit-identical bounds only the higher id is scored in that round.  The oracle keeps the map; the device reproduces the
    rule in its pick.  With the rule switched off the same frame selects in a different order - i.e. the frame really
    exercises it."""
    for seed in (0, 1):
        pr = _mirror_frame(seed=seed)
        _, dl, va = oracle.fsel_information(pr)
        assert va.all() and np.array_equal(np.diag(dl[0, 0]), np.diag(dl[0, 1])) and np.abs(dl[0, 0] - dl[0, 1]).max() > 1e-3
        oo = buffers.FselOutArrays.alloc(1, pr.dims["max_features"])
        oracle.fsel_select(pr, oo)
        out = selector.select_batch(pr)
        assert np.array_equal(out.a["n_selected"], oo.a["n_selected"]) and np.array_equal(out.a["selected_ids"], oo.a["selected_ids"])
        # in every pair the higher id goes first, whatever the two logdets are
        ids = pr.a["cand_id"][0].tolist()
        order = [ids.index(s) for s in oo.a["selected_ids"][0, : oo.a["n_selected"][0]]]
        for k in range(0, 2 * 20, 2):   # while both members of a pair are live the lower id is shadowed: the higher id always goes first
            if k in order:
                assert k + 1 in order and order.index(k + 1) < order.index(k), (k, order)
    monkeypatch.setenv("AVM_FSEL_NO_KEY_RULE", "1")
    differs = 0
    for seed in (0, 1):
        pr = _mirror_frame(seed=seed)
        oo = buffers.FselOutArrays.alloc(1, pr.dims["max_features"])
        oracle.fsel_select(pr, oo)
        differs += int(not np.array_equal(selector.select_batch(pr).a["selected_ids"], oo.a["selected_ids"]))
    assert differs >= 1


def test_selector_single_frame_kernel_equals_the_launch_per_round_path(selector, oracle, monkeypatch):
    """A frame runs all its greedy rounds in one launch (csrc/fsel/frame_kernel.hpp, fsel_frame_kernel: a team of workgroups on one XCD by
    default, one team over all XCDs as the first fallback); AVM_FSEL_FRAME=0 forces one launch per round.  The three must agree
    to the bit - ids in selection order AND the fValues - and with the oracle's ids: the usual frames, the reference's
    HORIZON 13 (Delta not kept in LDS), the mirror-pair frames of the std::map rule, tiny / exhausted candidate sets."""
    frames = [synth.make_fsel(1, horizon=10, n_cand=500, n_used=0, max_features=150),
              synth.make_fsel(1, horizon=13, n_cand=300, n_used=5, max_features=60, first_id=3),
              synth.make_fsel(1, horizon=3, n_cand=10, n_used=4, max_features=4, n_cloud=0),
              synth.make_fsel(1, horizon=5, n_cand=12, n_used=0, max_features=20, n_cloud=5),
              _mirror_frame(seed=0), _mirror_frame(seed=1)]
    for pr in frames:
        oo = buffers.FselOutArrays.alloc(1, pr.dims["max_features"])
        oracle.fsel_select(pr, oo)
        outs = []
        for mode in ("0", "1", "2"):
            monkeypatch.setenv("AVM_FSEL_FRAME", mode)
            outs.append(selector.select_batch(pr))
        for o in outs:
            assert np.array_equal(o.a["n_selected"], oo.a["n_selected"]) and np.array_equal(o.a["selected_ids"], oo.a["selected_ids"])
            n = int(o.a["n_selected"][0])
            assert np.array_equal(o.a["fvalues"][0, :n], outs[0].a["fvalues"][0, :n])
    # a value that never arrives: the kernel's wait times out (20 ms), the select is re-run one mode down - twice - and the
    # context stays on the launch-per-round path
    monkeypatch.delenv("AVM_FSEL_FRAME")
    lib_m = __import__("importlib").import_module("anticipated-vins-mono_amd.lib")
    fs_m = __import__("importlib").import_module("anticipated-vins-mono_amd.feature_selector")
    FS2 = fs_m.FeatureSelector(ctx=lib_m.Context(0))
    pr = frames[1]
    oo = buffers.FselOutArrays.alloc(1, pr.dims["max_features"])
    oracle.fsel_select(pr, oo)
    monkeypatch.setenv("AVM_FSEL_TEST_DROP", "7")
    assert np.array_equal(FS2.select_batch(pr).a["selected_ids"], oo.a["selected_ids"])
    monkeypatch.delenv("AVM_FSEL_TEST_DROP")
    import time
    t0 = time.perf_counter()
    assert np.array_equal(FS2.select_batch(pr).a["selected_ids"], oo.a["selected_ids"])
    assert time.perf_counter() - t0 < 0.02   # (no 20 ms timeout any more: the context does not try the frame kernel again)
    # a device-resident frame takes the same path
    pr = frames[0]
    od = selector.select_batch(pr.to_device("cuda:0")).to_host()
    oo = buffers.FselOutArrays.alloc(1, pr.dims["max_features"])
    oracle.fsel_select(pr, oo)
    assert np.array_equal(od.a["selected_ids"], oo.a["selected_ids"])


def test_selector_batches_on_the_frame_kernel(selector, oracle, monkeypatch):
    """Batches run on the frame kernel too: the workgroups of every XCD form a team (two per XCD above eight frames), the teams
    take frames from a queue.  12 and 19 frames (more frames than teams; ragged candidate counts; the reference's HORIZON 13 keeps
    one team per XCD): ids identical to the oracle's, ids and fValues identical to the launch-per-round path to the bit."""
    for H, P, nc, mf in ((10, 12, 220, 50), (5, 19, 90, 30), (13, 11, 130, 25)):
        pr = synth.make_fsel(P, horizon=H, n_cand=nc, n_used=3, max_features=mf)
        pr.a["n_cand"][::3] = nc - 17          # ragged
        oo = buffers.FselOutArrays.alloc(P, mf)
        oracle.fsel_select(pr, oo, n_threads=8)
        monkeypatch.setenv("AVM_FSEL_FRAME", "2")
        a = selector.select_batch(pr)
        monkeypatch.setenv("AVM_FSEL_FRAME", "0")
        b = selector.select_batch(pr)
        monkeypatch.delenv("AVM_FSEL_FRAME")
        for o in (a, b):
            assert np.array_equal(o.a["n_selected"], oo.a["n_selected"]) and np.array_equal(o.a["selected_ids"], oo.a["selected_ids"])
        for q in range(P):
            n = int(a.a["n_selected"][q])
            # (to the bit where both paths evaluate in the DPP form; batches of more than eight frames with 3 H <= 30 evaluate on the
            #  matrix cores - a different order of the same operations on matrices with condition numbers of 1e6: 1e-11 relative)
            assert n > 0 and (np.array_equal(a.a["fvalues"][q, :n], b.a["fvalues"][q, :n]) if H == 13 else rel(a.a["fvalues"][q, :n], b.a["fvalues"][q, :n]) < 1e-10)


def test_selector_bench_batch_matches_the_oracle(selector, oracle):
    """The batch `bench.py` times (16 frames, 500 candidates -> 150, horizon 10: two teams per XCD on the frame kernel),
    device-resident as in the bench: every frame's ids are the oracle's, in selection order."""
    pr = synth.make_fsel(16, first_id=0)
    oo = buffers.FselOutArrays.alloc(16, pr.dims["max_features"])
    oracle.fsel_select(pr, oo, n_threads=8)
    out = selector.select_batch(pr.to_device("cuda:0")).to_host()
    assert (oo.a["n_selected"] == 150).all()
    assert np.array_equal(out.a["n_selected"], oo.a["n_selected"]) and np.array_equal(out.a["selected_ids"], oo.a["selected_ids"])


def test_selector_single_frames_from_two_host_threads_at_once(oracle):
    """One avm_ctx per host thread is the documented model.  Two threads that select a single frame at the same moment compete
    for the compute units the frame kernel's workgroups must hold together; whatever happens (both fit, or a wait times out and
    the call repeats itself one mode down) every call returns the oracle's ids."""
    import threading
    lib_m = __import__("importlib").import_module("anticipated-vins-mono_amd.lib")
    fs_m = __import__("importlib").import_module("anticipated-vins-mono_amd.feature_selector")
    frames = [synth.make_fsel(1, horizon=10, n_cand=300, n_used=0, max_features=60, first_id=k) for k in range(2)]
    want = []
    for pr in frames:
        oo = buffers.FselOutArrays.alloc(1, 60)
        oracle.fsel_select(pr, oo)
        want.append(oo.a["selected_ids"].copy())
    sels = [fs_m.FeatureSelector(ctx=lib_m.Context(0)) for _ in range(2)]
    bad = []

    def work(k):
        for _ in range(12):
            got = sels[k].select_batch(frames[k]).a["selected_ids"]
            if not np.array_equal(got, want[k]):
                bad.append(k)

    th = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    assert not any(x.is_alive() for x in th) and not bad


def test_selector_edge_cases(selector, oracle):
    for kw in (dict(n_cand=10, n_used=4, max_features=4, n_cloud=0), dict(n_cand=12, n_used=0, max_features=20, n_cloud=5)):
        pr = synth.make_fsel(1, horizon=3, **kw)
        out = selector.select_batch(pr)
        oo = buffers.FselOutArrays.alloc(1, kw["max_features"])
        oracle.fsel_select(pr, oo)
        assert np.array_equal(out.a["n_selected"], oo.a["n_selected"])
        assert np.array_equal(out.a["selected_ids"], oo.a["selected_ids"])


def test_window_roll_matches_oracle_and_chains_solves(ctx, oracle):
    """8(f)2: avm_slide_window on host and device buffers vs the oracle's list-based roll, then solve -> roll -> solve
    entirely on device-resident tables against the same chain through the oracle."""
    from test_oracle import _roll_inputs
    E = importlib_est().Estimator(ctx=ctx, options=abi.default_options())

    def same_tables(g, o):
        assert np.array_equal(g["pose"], o["pose"]) and np.array_equal(g["speedbias"], o["speedbias"]) and np.array_equal(g["n_feat"], o["n_feat"])
        assert np.array_equal(g["imu_n"], o["imu_n"]) and np.array_equal(g["imu_lin_ba"], o["imu_lin_ba"]) and np.array_equal(g["imu_lin_bg"], o["imu_lin_bg"])
        for b in range(len(g["n_feat"])):
            n = g["n_feat"][b]
            assert np.array_equal(g["feat_start"][b, :n], o["feat_start"][b, :n]) and np.array_equal(g["feat_nobs"][b, :n], o["feat_nobs"][b, :n])
            assert n == 0 or rel(g["inv_depth"][b, :n], o["inv_depth"][b, :n]) < 1e-13
            for e in range(n):
                no, gb, ob = g["feat_nobs"][b, e], g["feat_obs_begin"][b, e], o["feat_obs_begin"][b, e]
                assert np.array_equal(g["obs_xy"][b, gb:gb + no], o["obs_xy"][b, ob:ob + no]), (b, e)
            for j in range(10):
                m = g["imu_n"][b, j]
                assert np.array_equal(g["imu_dt"][b, j, :m], o["imu_dt"][b, j, :m])
                assert np.array_equal(g["imu_acc"][b, j, :m + 1], o["imu_acc"][b, j, :m + 1]) and np.array_equal(g["imu_gyr"][b, j, :m + 1], o["imu_gyr"][b, j, :m + 1])

    for flag, shift in ((abi.MARGIN_OLD, True), (abi.MARGIN_OLD, False), (abi.MARGIN_SECOND_NEW, True)):
        w = _roll_inputs()
        wo, wd = w.copy(), w.copy().to_device("cuda:0")
        assert oracle.slide_window(wo, flag, shift, 5.0) == 0
        E.slideWindow(w, flag, shift, 5.0)
        E.slideWindow(wd, flag, shift, 5.0)
        same_tables(w.a, wo.a)
        same_tables(wd.to_host().a, wo.a)
    # degenerate tables: no features at all, and an empty newest interval
    for flag in (abi.MARGIN_OLD, abi.MARGIN_SECOND_NEW):
        w = blank_windows(2)
        w.a["imu_n"][:, 9] = 0
        w.a["imu_n"][1, 8] = 0
        wo = w.copy()
        assert oracle.slide_window(wo, flag, True, 5.0) == 0
        E.slideWindow(w, flag, True, 5.0)
        same_tables(w.a, wo.a)
    w = _roll_inputs()
    w.a["imu_n"][:, 8], w.a["imu_n"][:, 9] = 30, 20
    lib_m = __import__("importlib").import_module("anticipated-vins-mono_amd.lib")
    with pytest.raises(lib_m.AvmError, match="max_samp"):   # AVM_ERR_CAPACITY
        E.slideWindow(w, abi.MARGIN_SECOND_NEW)
    # solve -> roll -> (new IMU samples arrive) -> solve: the rolled tables are valid solver input, and the chain through the
    # GPU agrees with the chain through the oracle
    o = abi.default_options()
    w = synth.make_windows(3, tracks="sparse", n_feat=50, max_feat=150, max_samp=40)
    from marg_sensitivity import truth_marginalize
    wg, wo = w.copy(), w.copy()
    E.optimization(wg)
    pg, po = E.last_marginalization_info, buffers.PriorOutArrays.alloc(3)
    oracle.window_solve(o, wo, po, buffers.summary_alloc(3))
    wt = wo.copy()
    pt = truth_marginalize(wo, o)[0]     # the exact prior (binary128) at the oracle's solution: the reference chain
    E.slideWindow(wg, abi.MARGIN_OLD, True, 5.0)
    assert oracle.slide_window(wo, abi.MARGIN_OLD, True, 5.0) == 0
    assert oracle.slide_window(wt, abi.MARGIN_OLD, True, 5.0) == 0
    for win, p in ((wg, pg), (wo, po), (wt, pt)):
        a = win.a
        a["prior_n"][:], a["prior_nblk"][:] = p.a["n"].astype(np.int32), p.a["nblk"]
        a["prior_blk_kind"][:], a["prior_blk_frame"][:] = p.a["blk_kind"], p.a["blk_frame"]
        a["prior_J"][:], a["prior_r"][:], a["prior_x0"][:] = p.a["J"], p.a["r"], p.a["x0"]
        assert (a["imu_n"][:, 9] == 0).all()
        a["imu_n"][:, 9] = a["imu_n"][:, 8]              # the next image's IMU interval: same motion as the one before
        a["imu_dt"][:, 9], a["imu_acc"][:, 9, 1:], a["imu_gyr"][:, 9, 1:] = a["imu_dt"][:, 8], a["imu_acc"][:, 8, 1:], a["imu_gyr"][:, 8, 1:]
        for b in range(3):
            n = a["n_feat"][b]
            assert n > 10 and (a["feat_nobs"][b, :n] >= 2).all() and (np.diff(a["feat_start"][b, :n]) >= 0).all() and (a["feat_start"][b, :n] < 9).all()
    o2 = abi.default_options()
    o2.marginalization_flag = abi.MARGIN_NONE
    E2 = importlib_est().Estimator(ctx=ctx, options=o2)
    E2.optimization(wg)
    oracle.window_solve(o2, wo, None, buffers.summary_alloc(3))
    oracle.window_solve(o2, wt, None, buffers.summary_alloc(3))
    for k in ("pose", "speedbias"):
        # against the chain with the exact prior (the FP64 oracle's own chain sits 1e-6 .. 1e-5 away from it)
        print(f"\n[solve -> roll -> solve vs exact-prior chain] {k}: gpu {rel(wg.a[k], wt.a[k]):.2e}  oracle {rel(wo.a[k], wt.a[k]):.2e}")
        assert rel(wg.a[k], wt.a[k]) < 1e-6, (k, rel(wg.a[k], wt.a[k]))
