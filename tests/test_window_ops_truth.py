"""triangulate_kernel, imu_propagate_kernel and projection_td_eval_kernel (csrc/triangulate.hip) against the extended-precision arbiter
(oracle/avm_truth.cpp: avmt_triangulate, avmt_imu_propagate, avmt_projection_td_eval) and a 50-digit reading.

The three kernels run in every solveOdometry() step of the stream loop.  What the suite had for them: the FP64 oracle - the same
Hestenes sweep with the same threshold, the same formulas - through helpers.rel, one number per batch (1e-9 for 150 depths, 1e-13 for a
pose table, 1e-10 for J[300, 2, 20] whose lambda column is hundreds of times larger than its pose blocks), on windows with one ex_pose,
tracks with start 0 and 11 observations or sparse ones, five windows (one block) for the dead-reckoning, equal dt in every sample.

Here (case sets and distance measures: tests/window_ops_cases.py):
  * the truth is the oracle's own function with binary128 as its scalar type, on the same FP64 tables, rounded once; its sweep
    converges to binary128's roundoff, not to the FP64 constant 2.3e-16;
  * that arbiter is pinned to an independent 50-digit reading written from the reference sources (tests/golden/window_ops_mp.npz) to
    1e-25, for the depth 1e-25 cond_d;
  * the depth is graded per feature, relative to cond_d - the first-order condition number of v[2] / v[3] under a normwise
    perturbation of the system, the measure under which the oracle's error is flat over the four decades of baseline in the sets -
    features whose truth falls back to init_depth exactly; the pose per window and per part; the factor per factor, the residual
    against s (|x / z| + |u|), the Jacobian per block against the block's largest entry, exact zeros where the truth has them;
  * the conditions on set T (cond_d <= 1e6 on every graded feature, no ratio near 0.1) are asserted on the arbiter's values, which
    the fixture pins to the 50-digit reading on twenty-one of the features;
  * set TX (tracks with one mismatched observation) is there for one reason: a sweep that stops at 1e-12 instead of 2.3e-16 stays
    inside the ten-fold margin on consistent tracks, where sigma_4 / sigma_1 is 1e-3, and shows where it is percents;
  * CPU tier: the FP64 oracle's worst distance per quantity (ORACLE_TO_TRUTH);
  * GPU tier: every item within ten times that and within 1e-12 (depth: 1e-12 cond_d); host and device mode the same bits; the
    output of an item does not depend on its row, window, block or lane, nor on what lies beyond the live counts (to the bit); depths
    that were positive and rows beyond n_feat come back untouched; a null Jacobian pointer gives the same residual bits.
"""
import ctypes as C
import functools
import os

import mpmath as mp
import numpy as np
import pytest

import window_ops_cases as WC
from helpers import abi
from preint_cases import PAD

TOL = 1e-12  # the suite's tolerance for product <-> oracle, here per item and against the truth (depth: times cond_d)
# The FP64 oracle's worst distance to the binary128 arbiter per quantity, over sets T70 + T150 + TX (213 graded features), P under both
# gravities (2 x 130 windows) and F (130 factors); for the Jacobian per block of WC.JAC_BLOCKS.  Measured by
# test_fp64_oracle_is_within_tolerance_of_the_truth (x86-64, g++ -O3 -march=x86-64-v3 as oracle/Makefile builds it); three digits,
# rounded up.
ORACLE_TO_TRUTH = {
    "depth": 8.30e-17,                # TX (T70: 7.37e-17, T150: 7.31e-17), in units of cond_d
    "P": 6.06e-16,                    # P, default gravity
    "V": 5.56e-16,                    # P, default gravity
    "q": 3.70e-16,                    # P, either gravity
    "residual": 2.59e-14,             # F, factor 3 (dep_j = 0.2: the division by dep_j amplifies the chain's rounding)
    "jacobian[pose_i.p]": 1.86e-14,   # F, factor 3
    "jacobian[pose_i.th]": 2.09e-14,  # F, factor 3
    "jacobian[pose_j.p]": 1.86e-14,   # F, factor 3
    "jacobian[pose_j.th]": 1.85e-14,  # F, factor 3
    "jacobian[ex.p]": 2.13e-14,       # F, factor 3
    "jacobian[ex.th]": 1.77e-14,      # F, factor 3
    "jacobian[lambda]": 4.15e-14,     # F, factor 56
    "jacobian[td]": 1.13e-14,         # F, factor 3
}
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "window_ops_mp.npz"))
GRAVITY = {"default": tuple(float(v) for v in abi.default_options().g), "tilted": WC.G_TILTED}
mp.mp.dps = 50


def _freeze(*dicts):
    for d in dicts:
        for v in d.values():
            v.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _tset(name):
    """(windows, the rows triangulate() has to fill, the arbiter's hi, its lo) of T70 / T150 / TX: computed once, changed by no test."""
    import oracle_py

    w = WC.T_SETS[name]()
    rows = WC.no_depth_rows(w)
    hi, lo = oracle_py.truth_triangulate(w, WC.INIT_DEPTH, rows)
    _freeze(w.a, hi, lo)
    return w, rows, hi, lo


@functools.lru_cache(maxsize=None)
def _pset(gname):
    import oracle_py

    w = _pwindows()
    hi, lo = oracle_py.truth_imu_propagate(w, GRAVITY[gname])
    _freeze(hi, lo)
    return w, GRAVITY[gname], hi, lo


@functools.lru_cache(maxsize=None)
def _pwindows():
    w = WC.set_p()
    _freeze(w.a)
    return w


@functools.lru_cache(maxsize=None)
def _fset():
    import oracle_py

    a = WC.set_f()
    hi, lo = oracle_py.truth_projection_td_eval(a, WC.TR, WC.ROW, WC.FOCAL)
    _freeze(a, hi, lo)
    return a, hi, lo


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, np.float64)).view(np.uint64)


def _assert_same_bits(got, want, what):
    same = _bits(got) == _bits(want)
    assert same.all(), (what, "first difference at", tuple(int(v[0]) for v in np.nonzero(~same)))


# ---- CPU tier -------------------------------------------------------------------------------------------------------------------------
def test_the_case_sets_hold_what_they_are_meant_to():
    # -- set T
    w70, w150 = _tset("T70")[0], _tset("T150")[0]
    assert (w70.dims["max_feat"], w70.a["n_feat"].tolist()) == (70, [70, 55, 1, 0]) and 70 % 64 != 0
    assert (w150.dims["max_feat"], w150.a["n_feat"].tolist()) == (150, [130])
    ex = np.concatenate([w70.a["ex_pose"], w150.a["ex_pose"]])
    assert len(np.unique(ex, axis=0)) == 5
    angle = np.rad2deg(2 * np.arccos(np.abs(ex[:, 6])))
    assert ((angle > 20) & (angle < 60)).all() and (np.linalg.norm(ex[:, :3], axis=1) > 5e-3).all() and (np.abs(ex[:, :3]) < 0.2).all()
    graded_cond, n_graded = [], 0
    wx = _tset("TX")[0]
    assert (wx.dims["max_feat"], wx.a["n_feat"].tolist()) == (150, [130])
    for name, scales in (("T70", WC.T70_SCALE), ("T150", WC.T150_SCALE), ("TX", WC.TX_SCALE)):
        w, rows, hi, lo = _tset(name)
        a, mf = w.a, w.dims["max_feat"]
        for b in range(w.n_windows):
            n = int(a["n_feat"][b])
            reach = np.linalg.norm(a["pose"][b, 1:, :3] - a["pose"][b, 0, :3], axis=1).max()
            assert 0.5 * scales[b] < reach < 1.5 * scales[b], (name, b, reach)
            live = [(int(a["feat_start"][b, e]), int(a["feat_nobs"][b, e])) for e in range(n)]
            if n >= 55:
                assert set(live) == set(WC.PAIRS), (name, b)  # every (start, nobs) with nobs 2 ... 11
            assert all(s >= 0 and no >= 2 and s + no <= 11 for s, no in live) and sorted(live, key=lambda p: p[0]) == live
            # the observation table: every row's block inside it, no two overlap, PAD behind each and everywhere else
            used = np.zeros(w.dims["max_obs"], bool)
            begin = a["feat_obs_begin"][b]
            for e in range(mf):
                ob, no = int(begin[e]), int(a["feat_nobs"][b, e])
                assert no >= 2 and a["feat_start"][b, e] + no <= 11 and not used[ob:ob + no].any() and ob + no < w.dims["max_obs"]
                used[ob:ob + no] = True
                assert (a["obs_xy"][b, ob + no] == PAD).all()
            assert (a["obs_xy"][b][~used] == PAD).all() and (np.abs(a["obs_xy"][b][used]) < 3).all()
            if n >= 2:
                assert (np.diff(begin[:n]) < 0).any() and (np.diff(begin[:n]) > 0).any()  # not monotone
            # depth slots
            keep = a["inv_depth"][b, :n] > 0
            assert np.array_equal(np.where(keep)[0], np.arange(1, n, 4)) and (a["inv_depth"][b, n:] == -1.0).all()
            if n >= 55:
                slots = a["inv_depth"][b, :n][~keep]
                assert np.isnan(slots).any() and (slots == -1.0).any() and ((slots == 0) & np.signbit(slots)).any() and ((slots == 0) & ~np.signbit(slots)).any()
        # the decisions, by construction, and nothing near 0.1
        for b, kinds in w.kinds.items():
            for e, d in kinds.items():
                assert (b, e) in rows and abs(hi["ratio"][b, e] - d) < 1e-9 * abs(d), (name, b, e)
                assert hi["depth"][b, e] == (WC.INIT_DEPTH if d < 0.1 else hi["ratio"][b, e])
        placed = sorted(d for kinds in w.kinds.values() for d in kinds.values())
        assert set(placed) == (set(WC.DECISIONS) if name != "TX" else {-2.0})
        cond = WC.cond_d(hi["sigma"], hi["V"])
        # how far from consistent the graded systems are: sigma_4 / sigma_1 is noise-sized in T70 and T150, percents in TX
        misfit = max(hi["sigma"][b, e, 3] / hi["sigma"][b, e, 0] for b, e in rows if hi["ratio"][b, e] >= 0.1)
        assert misfit > 0.02 if name == "TX" else misfit < 5e-3, (name, misfit)
        for b, e in rows:
            r = hi["ratio"][b, e]
            assert np.isfinite(r) and abs(r - 0.1) > WC.decision_margin(r, cond[b, e]), (name, b, e, r, cond[b, e])
            assert (hi["depth"][b, e] == r) == (r >= 0.1) and (r >= 0.1 or hi["depth"][b, e] == WC.INIT_DEPTH)
            if r >= 0.1:
                graded_cond.append(cond[b, e])
                n_graded += 1
    print("\n[window ops] set T: %d graded features, cond_d %.3g ... %.3g" % (n_graded, min(graded_cond), max(graded_cond)))
    assert n_graded >= 200 and max(graded_cond) <= WC.COND_MAX and min(graded_cond) < 20 and max(graded_cond) > 5e4
    # -- set P
    w = _pwindows()
    a, n = w.a, _pwindows().a["imu_n"]
    assert w.n_windows == 130 == 64 + 64 + 2 and w.dims["max_samp"] == 20 and n[:, 9].tolist() == [b % 21 for b in range(130)]
    live = np.arange(20)[None, None, :] < n[:, :, None]
    assert (a["imu_dt"][~live] == PAD).all() and a["imu_dt"][live].min() >= 0.7 / 400 and a["imu_dt"][live].max() <= 1.3 / 100
    for b in range(130):
        k = int(n[b, 9])
        assert len(set(a["imu_dt"][b, 9, :k].tolist())) == k  # every sample its own dt
        assert (a["imu_acc"][b, 9, k + 1:] == PAD).all() and (a["imu_gyr"][b, 9, k + 1:] == PAD).all() and (np.abs(a["imu_acc"][b, 9, :k + 1]) < 20).all()
        assert all((a[t][b, 9, 0] != a[t][b, j, 0]).all() for t in ("imu_acc", "imu_gyr") for j in range(9))  # other data in intervals 0 ... 8
        assert k == 0 or not np.isin(a["imu_dt"][b, 9, :k], a["imu_dt"][b, :9]).any()
        assert not np.array_equal(a["pose"][b, 10], a["pose"][b, 9]) and not np.array_equal(a["speedbias"][b, 10], a["speedbias"][b, 9])
    for k in ("pose", "speedbias"):
        assert len(np.unique(a[k][:, 10], axis=0)) == 130 and a[k][:, 10].all()
    assert sum(1 for v in GRAVITY["tilted"] if v != 0) == 3 and GRAVITY["default"] != GRAVITY["tilted"]
    assert len(set((WC.P_PERM // 64 != np.arange(130) // 64).nonzero()[0])) >= 60 and (WC.P_PERM % 64 != np.arange(130) % 64).all()
    assert sorted(WC.P_PERM.tolist()) == list(range(130)) and sorted(WC.F_PERM.tolist()) == list(range(130))
    # -- set F
    f, D = _fset()[0], WC.F_DESIGNED
    assert len(f["inv_depth"]) == 130
    assert all(abs(WC.td_forward(f, k)["dep_j"] - 0.2) < 1e-12 for k in D["dep_j"])
    assert (f["inv_depth"][list(D["lam_near"])] == 1 / 0.3).all() and (f["inv_depth"][list(D["lam_far"])] == 1 / 60.0).all()
    assert not f["vel_i"][list(D["vel_zero"] + D["vel_i_zero"])].any() and not f["vel_j"][list(D["vel_zero"] + D["vel_j_zero"])].any()
    assert f["vel_j"][list(D["vel_i_zero"])].all() and f["vel_i"][list(D["vel_j_zero"])].all()
    assert (f["row_i"][list(D["row_0"])] == 0).all() and (f["row_i"][list(D["row_full"])] == WC.ROW).all()
    for k in (i for v in D.values() for i in v):  # ... on either side of the block boundary
        assert 0 <= k < 130
    assert any(k >= 64 for k in D["dep_j"]) and any(k < 64 for k in D["dep_j"]) and 129 in D["vel_zero"]


def test_the_distance_measures_see_a_nan_or_an_infinity():
    """The truth itself has distance zero; with one entry poisoned the item's distance is infinite (max(0.0, nan) is 0.0), and a NaN in a
    block that is zero in the truth is reported."""
    w, rows, hi, lo = _tset("T70")
    lam = np.where(hi["ratio"] >= 0.1, 1.0 / hi["depth"], 1.0 / WC.INIT_DEPTH)
    d, cond, graded = WC.depth_distances(lam, hi, lo, rows)
    assert max(d.values()) < 2.3e-16 and sum(graded.values()) > 60  # (1 / hi: one rounding, divided by cond_d >= 10)
    g, fb = next(r for r in rows if graded[r]), next(r for r in rows if not graded[r])
    for poison in (np.nan, np.inf):
        for r in (g, fb):
            x = lam.copy()
            x[r] = poison
            d = WC.depth_distances(x, hi, lo, rows)[0]
            assert d[r] == np.inf and not d[r] < TOL and sum(1 for v in d.values() if v == np.inf) == 1
    x = lam.copy()
    x[fb] = np.nextafter(x[fb], 1.0)  # a fallback that is one ulp off is off
    assert WC.depth_distances(x, hi, lo, rows)[0][fb] == np.inf
    w, g_, hi, lo = _pset("default")
    same = WC.pose_distances(hi["pose"], hi["speedbias"], hi)
    assert all(not v.any() for v in same.values())
    for poison in (np.nan, np.inf):
        for col, key in ((1, "P"), (4, "q")):
            p = hi["pose"].copy()
            p[77, col] = poison
            d = WC.pose_distances(p, hi["speedbias"], hi)
            assert d[key][77] == np.inf and np.isinf(d[key]).sum() == 1
        s = hi["speedbias"].copy()
        s[129, 2] = poison
        assert WC.pose_distances(hi["pose"], s, hi)["V"][129] == np.inf
    a, hi, lo = _fset()
    same, bad = WC.factor_distances(hi["residual"], hi["jac"], hi, a)
    assert not bad and all(not v.any() for v in same.values())
    k = WC.F_DESIGNED["vel_zero"][0]
    assert not hi["jac"][k, :, 19].any()
    for poison in (np.nan, np.inf):
        r, J = hi["residual"].copy(), hi["jac"].copy()
        r[5, 1] = J[6, 0, 4] = J[k, 1, 19] = poison
        d, bad = WC.factor_distances(r, J, hi, a)
        assert d["residual"][5] == np.inf and d["pose_i.th"][6] == np.inf and len(bad) == 1 and "factor %d" % k in bad[0]


def _mpv(hi, lo):
    hi, lo = np.asarray(hi, float), np.asarray(lo, float)
    out = np.empty(hi.shape, dtype=object)
    for idx in np.ndindex(hi.shape):
        out[idx] = mp.mpf(float(hi[idx])) + mp.mpf(float(lo[idx]))
    return out


def test_binary128_arbiter_agrees_with_the_50_digit_reading_of_the_triangulation():
    """avmt_triangulate's hi + lo against tests/golden/window_ops_mp.npz (mp.svd_r of the system built in 50 digits) on twenty-one
    features: every (nobs, scale) corner, the five decision rows, two mismatched tracks.  The ratio to 1e-25 cond_d; the singular values to 1e-25 of the largest; each
    right singular vector, up to its sign, to 1e-25 times sigma_1 over its gap to the nearest other singular value."""
    worst = {}
    for i in range(len(GOLD["t_row"])):
        name, b, e = str(GOLD["t_set"][i]), int(GOLD["t_window"][i]), int(GOLD["t_row"][i])
        w, rows, hi, lo = _tset(name)
        no, ob = int(w.a["feat_nobs"][b, e]), int(w.a["feat_obs_begin"][b, e])
        assert (b, e) in rows and no == GOLD["t_nobs"][i] and w.a["feat_start"][b, e] == GOLD["t_start"][i] \
            and np.array_equal(w.a["obs_xy"][b, ob:ob + no], GOLD["t_obs"][i, :no]), "the fixture is of other case sets: regenerate it"
        A = {k: _mpv(hi[k][b, e], lo[k][b, e]) for k in ("ratio", "depth", "sigma", "V")}
        M = {k: _mpv(GOLD["t_%s_hi" % k][i], GOLD["t_%s_lo" % k][i]).reshape(A[k].shape) for k in A}
        cond = mp.mpf(float(WC.cond_d(hi["sigma"][b, e], hi["V"][b, e])))
        gaps = {"ratio": abs(A["ratio"][()] - M["ratio"][()]) / abs(M["ratio"][()]) / cond,
                "sigma": max(abs(x - y) for x, y in zip(A["sigma"], M["sigma"])) / M["sigma"][0]}
        if M["ratio"][()] >= mp.mpf("0.1"):
            gaps["depth"] = abs(A["depth"][()] - M["depth"][()]) / abs(M["depth"][()]) / cond
        else:
            assert A["depth"][()] == M["depth"][()] == mp.mpf(WC.INIT_DEPTH)
        for k in range(4):
            gap = min(abs(M["sigma"][k] - M["sigma"][j]) for j in range(4) if j != k)
            dv = min(max(abs(A["V"][r, k] - s * M["V"][r, k]) for r in range(4)) for s in (1, -1))
            gaps["V"] = max(gaps.get("V", mp.mpf(0)), dv / (M["sigma"][0] / gap))
        print("[mp pin] %-4s window %d row %3d (%2d obs, cond_d %8.3g): " % (name, b, e, no, float(cond)) + "  ".join("%s %s" % (k, mp.nstr(v, 2)) for k, v in gaps.items()))
        for k, v in gaps.items():
            worst[k] = max(worst.get(k, mp.mpf(0)), v)
            assert v < mp.mpf("1e-25"), (i, k, v)
    print("[mp pin] triangulation, worst: " + "  ".join("%s %s" % (k, mp.nstr(v, 2)) for k, v in worst.items()))
    assert set(worst) == {"ratio", "depth", "sigma", "V"} and len(GOLD["t_row"]) >= 16


def test_binary128_arbiter_agrees_with_the_50_digit_reading_of_the_dead_reckoning():
    """avmt_imu_propagate against the 50-digit run of the numpy statement on eight newest intervals (0, 1, 2, 5, 13 and 20 samples, fast
    turns, both gravities): P, V and the quaternion (sign-insensitive) to 1e-25, the bias columns exactly."""
    worst = {}
    for i in range(len(GOLD["p_window"])):
        b, g = int(GOLD["p_window"][i]), tuple(GOLD["p_g"][i].tolist())
        gname = next(k for k, v in GRAVITY.items() if v == g)
        w, _, hi, lo = _pset(gname)
        assert w.a["imu_n"][b, 9] == GOLD["p_n"][i] and np.array_equal(w.a["imu_dt"][b, 9], GOLD["p_dt"][i]), "the fixture is of other case sets: regenerate it"
        Ap, As = _mpv(hi["pose"][b], lo["pose"][b]), _mpv(hi["speedbias"][b], lo["speedbias"][b])
        Mp, Ms = _mpv(GOLD["p_pose_hi"][i], GOLD["p_pose_lo"][i]), _mpv(GOLD["p_speedbias_hi"][i], GOLD["p_speedbias_lo"][i])
        nrm = lambda v: mp.sqrt(sum((x * x for x in v), mp.mpf(0)))
        gaps = {"P": nrm(Ap[:3] - Mp[:3]) / nrm(Mp[:3]), "V": nrm(As[:3] - Ms[:3]) / nrm(Ms[:3]), "q": min(nrm(Ap[3:] - Mp[3:]), nrm(Ap[3:] + Mp[3:]))}
        assert all(x == y for x, y in zip(As[3:], Ms[3:])) and np.array_equal(hi["speedbias"][b, 3:], w.a["speedbias"][b, 10, 3:])
        print("[mp pin] window %3d (%2d samples, gravity %s): " % (b, GOLD["p_n"][i], gname) + "  ".join("%s %s" % (k, mp.nstr(v, 2)) for k, v in gaps.items()))
        for k, v in gaps.items():
            worst[k] = max(worst.get(k, mp.mpf(0)), v)
            assert v < mp.mpf("1e-25"), (i, k, v)
    print("[mp pin] dead-reckoning, worst: " + "  ".join("%s %s" % (k, mp.nstr(v, 2)) for k, v in worst.items()))
    assert len(GOLD["p_window"]) == 8 and sorted(set(GOLD["p_n"].tolist())) == [0, 1, 2, 5, 13, 20]


def test_binary128_arbiter_agrees_with_the_50_digit_reading_of_the_td_factor():
    """avmt_projection_td_eval against the 50-digit run of gen_solve_trace_x.projection_td_factor on sixteen factors, the designed rows
    among them: the residual against s (|x / z| + |u|) and every Jacobian block against its largest entry to 1e-25; a block that is
    zero in one is zero in the other."""
    a, hi, lo = _fset()
    worst = {}
    for i, k in enumerate(GOLD["f_index"].tolist()):
        assert np.array_equal(a["pose_i"][k], GOLD["f_pose_i"][i]) and a["inv_depth"][k] == GOLD["f_inv_depth"][i], "the fixture is of other case sets: regenerate it"
        Ar, AJ = _mpv(hi["residual"][k], lo["residual"][k]), _mpv(hi["jac"][k], lo["jac"][k])
        Mr, MJ = _mpv(GOLD["f_residual_hi"][i], GOLD["f_residual_lo"][i]), _mpv(GOLD["f_jac_hi"][i], GOLD["f_jac_lo"][i]).reshape(2, 20)
        sc = WC.td_forward(a, k)["scale"]
        gaps = {"residual": max(abs(Ar[c] - Mr[c]) / mp.mpf(float(sc[c])) for c in range(2))}
        for nm, c0, c1 in WC.JAC_BLOCKS:
            x, t = AJ[:, c0:c1].ravel(), MJ[:, c0:c1].ravel()
            if all(v == 0 for v in t):
                assert all(v == 0 for v in x), (k, nm)
            else:
                gaps[nm] = max(abs(p - q) for p, q in zip(x, t)) / max(abs(q) for q in t)
        print("[mp pin] factor %3d: " % k + "  ".join("%s %s" % (q, mp.nstr(v, 2)) for q, v in gaps.items()))
        for q, v in gaps.items():
            worst[q] = max(worst.get(q, mp.mpf(0)), v)
            assert v < mp.mpf("1e-25"), (k, q, v)
    print("[mp pin] td factor, worst: " + "  ".join("%s %s" % (k, mp.nstr(v, 2)) for k, v in worst.items()))
    assert len(GOLD["f_index"]) == 16 and set(worst) == {"residual"} | {nm for nm, _, _ in WC.JAC_BLOCKS}


def test_any_output_of_the_arbiter_may_be_left_out():
    import oracle_py

    L = oracle_py.truth_lib()
    none = C.cast(None, abi.c_dp)
    w, rows, hi, lo = _tset("T70")
    b, e = rows[7]
    s, out = w.struct(), np.zeros(4)
    L.avmt_triangulate.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_double] + [abi.c_dp] * 8
    assert L.avmt_triangulate(C.byref(s), b, e, WC.INIT_DEPTH, none, none, none, none, abi.dptr(out), none, none, none) == 0
    assert np.array_equal(out, hi["sigma"][b, e])
    assert L.avmt_triangulate(C.byref(s), 0, 70, WC.INIT_DEPTH, *([none] * 8)) == -1
    w, g, hi, lo = _pset("tilted")
    s, out, gg = w.struct(), np.zeros(9), np.array(g)
    assert L.avmt_imu_propagate(C.byref(s), 129, abi.dptr(gg), none, none, none, abi.dptr(out)) == 0
    assert np.array_equal(out, lo["speedbias"][129])
    a, hi, lo = _fset()
    f, out = abi.td_factor_batch(a, WC.TR, WC.ROW, WC.FOCAL), np.zeros(2)
    assert L.avmt_projection_td_eval(C.byref(f), 3, abi.dptr(out), none, none, none) == 0
    assert np.array_equal(out, hi["residual"][3])


def _record(worst, key, values):
    for v in np.atleast_1d(values):
        worst[key] = WC.worse(worst.get(key, 0.0), v)


def _tri_worst(inv_depth, name):
    """{"depth": worst distance over the rows to fill}, and the per-row record, of a triangulated inv_depth table of set `name`."""
    w, rows, hi, lo = _tset(name)
    d, cond, graded = WC.depth_distances(inv_depth, hi, lo, rows)
    return d, cond, graded


def _check(worst, limit_of):
    for k, v in worst.items():
        assert v <= limit_of(k) and v < TOL, (k, v, limit_of(k))


def _report(title, worst):
    print("\n%s: " % title + "  ".join("%s %.3e" % kv for kv in worst.items()))


@pytest.mark.parametrize("case", ["T70", "T150", "TX", "P-default", "P-tilted", "F"])
def test_fp64_oracle_is_within_tolerance_of_the_truth(oracle, case):
    """The FP64 oracle against the arbiter on a case set: every item within 1e-12 (the depth: 1e-12 cond_d), fallbacks, kept depths,
    frames 0 ... 9 and the bias columns exact - and ORACLE_TO_TRUTH, which the GPU tier's bound is ten times of, still describes this
    oracle (within a factor of four: another compiler's choice of fused multiply-adds moves single roundings, not the size of the
    distance; beyond that the constants are to be measured again)."""
    worst = {}
    if case in WC.T_SETS:
        w, rows, hi, lo = _tset(case)
        wo = w.copy()
        oracle.triangulate(wo, init_depth=WC.INIT_DEPTH)
        d, cond, graded = _tri_worst(wo.a["inv_depth"], case)
        _record(worst, "depth", list(d.values()) or [0.0])
        _assert_untouched(wo, w, rows)
    elif case.startswith("P"):
        w, g, hi, lo = _pset(case[2:])
        wo = w.copy()
        oracle.imu_propagate(wo, np.array(g))
        for k, v in WC.pose_distances(wo.a["pose"][:, 10], wo.a["speedbias"][:, 10], hi).items():
            _record(worst, k, v)
        _assert_rest_of_the_tables(wo, w)
    else:
        a, hi, lo = _fset()
        r, J = oracle.projection_td_eval(a, WC.TR, WC.ROW, WC.FOCAL)
        d, bad = WC.factor_distances(r, J, hi, a)
        assert not bad, bad
        for k, v in d.items():
            _record(worst, k if k == "residual" else "jacobian[%s]" % k, v)
    _report("[window ops truth] FP64 oracle -> binary128, %s" % case, worst)
    _check(worst, lambda k: 4 * ORACLE_TO_TRUTH[k])


def _assert_untouched(got, w, rows):
    """Depths that were positive, and every row beyond n_feat, bit for bit; every row to fill now holds a positive depth."""
    fill = np.zeros(w.a["inv_depth"].shape, bool)
    for b, e in rows:
        fill[b, e] = True
    _assert_same_bits(got.a["inv_depth"][~fill], w.a["inv_depth"][~fill], "slots that triangulate() has to leave alone")
    assert (got.a["inv_depth"][fill] > 0).all()
    for k in w.a:
        if k != "inv_depth":
            assert np.array_equal(got.a[k], w.a[k], equal_nan=True), k


def _assert_rest_of_the_tables(got, w):
    _assert_same_bits(got.a["pose"][:, :10], w.a["pose"][:, :10], "frames 0 ... 9")
    _assert_same_bits(got.a["speedbias"][:, :10], w.a["speedbias"][:, :10], "frames 0 ... 9")
    _assert_same_bits(got.a["speedbias"][:, 10, 3:], w.a["speedbias"][:, 10, 3:], "the bias columns of frame 10")
    zero = w.a["imu_n"][:, 9] == 0  # no samples: the position and velocity as they were (the quaternion goes through a rotation matrix)
    _assert_same_bits(got.a["pose"][zero, 10, :3], w.a["pose"][zero, 10, :3], "P without samples")
    _assert_same_bits(got.a["speedbias"][zero, 10, :3], w.a["speedbias"][zero, 10, :3], "V without samples")


# ---- GPU tier -------------------------------------------------------------------------------------------------------------------------
def _triangulate(E, w, device):
    x = w.copy().to_device("cuda:0") if device else w.copy()  # (the sets are read-only: always a copy)
    E.triangulate(x, init_depth=WC.INIT_DEPTH)
    return x.to_host() if device else x


def _propagate(E, w, g, device):
    x = w.copy().to_device("cuda:0") if device else w.copy()  # (the sets are read-only: always a copy)
    s = x.struct()
    rc = E.ctx._L.avm_imu_propagate_batch(E.ctx.h, x.mem, C.byref(s), (C.c_double * 3)(*[float(v) for v in g]))
    E.ctx.check(rc, "avm_imu_propagate_batch")
    return x.to_host() if device else x


def _td_eval(E, a, device, jac=True):
    """avm_projection_td_eval through the C ABI in host or device mode; jac=False passes a null Jacobian pointer."""
    n = len(a["inv_depth"])
    if not device:
        f = abi.td_factor_batch(a, WC.TR, WC.ROW, WC.FOCAL)
        r, J = np.zeros((n, 2)), np.full((n, 2, 20), np.nan)
        rc = E.ctx._L.avm_projection_td_eval(E.ctx.h, abi.AVM_MEM_HOST, C.byref(f), abi.dptr(r), abi.dptr(J) if jac else None)
        E.ctx.check(rc, "avm_projection_td_eval")
        return r, J
    import torch

    t = {k: torch.from_numpy(np.array(v, float)).to("cuda:0") for k, v in a.items()}  # (np.array: a writable copy of the read-only set)
    f = abi.TdFactorBatch()
    f.n = n
    for k, v in t.items():
        setattr(f, k, abi.dptr(v))
    f.tr, f.row, f.focal_length = WC.TR, WC.ROW, WC.FOCAL
    r = torch.zeros((n, 2), dtype=torch.float64, device="cuda:0")
    J = torch.full((n, 2, 20), float("nan"), dtype=torch.float64, device="cuda:0")
    rc = E.ctx._L.avm_projection_td_eval(E.ctx.h, abi.AVM_MEM_DEVICE, C.byref(f), abi.dptr(r), abi.dptr(J) if jac else None)
    E.ctx.check(rc, "avm_projection_td_eval")
    torch.cuda.synchronize()
    return r.cpu().numpy(), J.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WC.T_SETS))
def test_gpu_triangulation_is_as_close_to_the_binary128_one_as_the_fp64_oracle(estimator, name):
    """triangulate_kernel on a set: every graded depth within ten times the oracle's worst distance and within 1e-12, both times
    cond_d; every fallback exactly 1 / init_depth; depths that were positive and rows beyond n_feat untouched; device mode the bits of
    host mode.  (Ten times: the kernel contracts to FMAs and forms R1^T R0 directly where the oracle forms (R0^T R1)^T.)"""
    w, rows, hi, lo = _tset(name)
    got = _triangulate(estimator, w, device=False)
    dev = _triangulate(estimator, w, device=True)
    d, cond, graded = _tri_worst(got.a["inv_depth"], name)
    worst = {}
    _record(worst, "depth", list(d.values()) or [0.0])
    _report("[window ops truth] GPU -> binary128, %s (%d graded, %d fallbacks)" % (name, sum(graded.values()), len(rows) - sum(graded.values())), worst)
    r = max(rows, key=lambda k: d[k]) if rows else None
    print("  worst row %s: cond_d %.3g, ratio to ORACLE_TO_TRUTH %.2f" % (r, cond.get(r, 0), worst["depth"] / ORACLE_TO_TRUTH["depth"]))
    _assert_same_bits(dev.a["inv_depth"], got.a["inv_depth"], "device mode against host mode")
    _assert_untouched(got, w, rows)
    for k in rows:
        assert d[k] <= 10 * ORACLE_TO_TRUTH["depth"] and d[k] < TOL, (k, d[k], cond[k], graded[k])


@pytest.mark.gpu
@pytest.mark.parametrize("gname", list(GRAVITY))
def test_gpu_dead_reckoning_is_as_close_to_the_binary128_one_as_the_fp64_oracle(estimator, gname):
    """imu_propagate_kernel on the 130 windows of set P (three blocks): P, V and the quaternion of every window within ten times the
    oracle's worst distance and within 1e-12; frames 0 ... 9 and the bias columns untouched; device mode the bits of host mode."""
    w, g, hi, lo = _pset(gname)
    got = _propagate(estimator, w, g, device=False)
    dev = _propagate(estimator, w, g, device=True)
    d = WC.pose_distances(got.a["pose"][:, 10], got.a["speedbias"][:, 10], hi)
    worst = {}
    for k, v in d.items():
        _record(worst, k, v)
    _report("[window ops truth] GPU -> binary128, P under the %s gravity" % gname, worst)
    print("  ratios to ORACLE_TO_TRUTH: " + "  ".join("%s %.2f" % (k, v / ORACLE_TO_TRUTH[k]) for k, v in worst.items()))
    for k in ("pose", "speedbias"):
        _assert_same_bits(dev.a[k], got.a[k], "device mode against host mode: " + k)
    _assert_rest_of_the_tables(got, w)
    for k, v in d.items():
        for b in range(130):
            assert v[b] <= 10 * ORACLE_TO_TRUTH[k] and v[b] < TOL, (k, b, v[b])


@pytest.mark.gpu
def test_gpu_td_factor_is_as_close_to_the_binary128_one_as_the_fp64_oracle(estimator):
    """projection_td_eval_kernel on the 130 factors of set F: the residual and every Jacobian block of every factor within ten times the
    oracle's worst distance for that block and within 1e-12; blocks that are zero in the truth exactly zero; device mode the bits of host
    mode; with a null Jacobian pointer the residual bits of the full call, in both modes."""
    a, hi, lo = _fset()
    r, J = _td_eval(estimator, a, device=False)
    rd, Jd = _td_eval(estimator, a, device=True)
    d, bad = WC.factor_distances(r, J, hi, a)
    worst = {}
    for k, v in d.items():
        _record(worst, k if k == "residual" else "jacobian[%s]" % k, v)
    _report("[window ops truth] GPU -> binary128, F", worst)
    print("  ratios to ORACLE_TO_TRUTH: " + "  ".join("%s %.2f" % (k, v / ORACLE_TO_TRUTH[k]) for k, v in worst.items()))
    _assert_same_bits(rd, r, "device mode against host mode: residual")
    _assert_same_bits(Jd, J, "device mode against host mode: jac")
    for device in (False, True):
        r0, J0 = _td_eval(estimator, a, device=device, jac=False)
        _assert_same_bits(r0, r, "null Jacobian pointer, device %s" % device)
        assert np.isnan(J0).all()
    assert not bad, bad
    for k, v in d.items():
        q = k if k == "residual" else "jacobian[%s]" % k
        for i in range(130):
            assert v[i] <= 10 * ORACLE_TO_TRUTH[q] and v[i] < TOL, (q, i, v[i])


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(WC.T_SETS))
def test_a_depth_does_not_depend_on_its_row_its_window_or_its_observation_rows(estimator, name):
    """A set with its windows in another order, the rows of every window rotated within their groups of equal feat_start (the table
    contract keeps feat_start ascending), the ghost rows rotated, every row's observations at another place of obs_xy: every row's
    inverse depth, moved back, is the unpermuted call's to the bit."""
    w = _tset(name)[0]
    wp, where = WC.permuted_t(w)
    n_moved = sum(1 for b in range(w.n_windows) for e in range(int(w.a["n_feat"][b])) if tuple(where[b, e]) != (b, e))
    assert n_moved == sum(w.a["n_feat"])  # every live row is somewhere else
    base = _triangulate(estimator, w, device=False).a["inv_depth"]
    moved = _triangulate(estimator, wp, device=False).a["inv_depth"]
    back = moved[where[..., 0], where[..., 1]]
    _assert_same_bits(back, base, "permuted rows")


@pytest.mark.gpu
def test_a_window_does_not_depend_on_its_block_or_lane(estimator):
    """Set P with window i moved to (37 i + 11) mod 130 - every window on another lane, most in another block: pose and speed-bias,
    moved back, to the bit."""
    w, g, _, _ = _pset("tilted")
    base = _propagate(estimator, w, g, device=False)
    moved = _propagate(estimator, WC.permuted_p(w), g, device=False)
    for k in ("pose", "speedbias"):
        _assert_same_bits(moved.a[k][WC.P_PERM], base.a[k], "permuted windows: " + k)


@pytest.mark.gpu
def test_a_factor_does_not_depend_on_its_place(estimator):
    """Set F with factor i moved to (47 i + 29) mod 130: residual and Jacobian, moved back, to the bit."""
    a = _fset()[0]
    r, J = _td_eval(estimator, a, device=False)
    rp, Jp = _td_eval(estimator, WC.permuted_f(a, WC.F_PERM), device=False)
    _assert_same_bits(rp[WC.F_PERM], r, "permuted factors: residual")
    _assert_same_bits(Jp[WC.F_PERM], J, "permuted factors: jac")


@pytest.mark.gpu
def test_nothing_beyond_the_live_counts_reaches_the_result(estimator):
    """NaN in place of the sentinel - every row of obs_xy outside a live feature's own, the observations of the rows beyond n_feat,
    every entry of imu_dt / imu_acc / imu_gyr beyond an interval's sample count: no output bit changes."""
    for name in WC.T_SETS:
        w = _tset(name)[0]
        wn = WC.nan_padded_t(w)
        assert np.isnan(wn.a["obs_xy"]).sum() > w.dims["max_obs"] and not np.isnan(w.a["obs_xy"]).any()
        base = _triangulate(estimator, w, device=False).a["inv_depth"]
        got = _triangulate(estimator, wn, device=False).a["inv_depth"]
        _assert_same_bits(got, base, "NaN beyond the live rows, " + name)
    w, g, _, _ = _pset("default")
    wn = WC.nan_padded_p(w)
    assert np.isnan(wn.a["imu_dt"]).sum() == (20 - w.a["imu_n"]).sum()
    base, got = _propagate(estimator, w, g, device=False), _propagate(estimator, wn, g, device=False)
    for k in ("pose", "speedbias"):
        _assert_same_bits(got.a[k], base.a[k], "NaN beyond the sample counts: " + k)
