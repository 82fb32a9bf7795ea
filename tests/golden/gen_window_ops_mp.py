"""Generates tests/golden/window_ops_mp.npz: independent 50-digit readings (mpmath) of the three small operations around the solve, on
items of the case sets of tests/window_ops_cases.py.  Each is written from the reference sources, not from oracle/:

  triangulation     feature_manager.cpp:209-249, the rows as _numpy_triangulate of tests/test_oracle.py states them, built in 50 digits
                    from the FP64 poses and observations; mp.svd_r of that matrix (not an eigendecomposition of A^T A, which divides by
                    zero on near-degenerate systems): the ratio v[2] / v[3], the depth after `< 0.1 -> INIT_DEPTH`, the four singular
                    values and the right singular vectors;
  dead-reckoning    estimator.cpp:100-107, the numpy statement of test_newest_frame_dead_reckoning_matches_numpy, followed by Eigen's
                    Quaterniond(Matrix3d) (gen_visual_align.R2q) as vector2double forms the pose quaternion (estimator.cpp:486);
  td factor         gen_solve_trace_x.projection_td_factor (projection_td_factor.cpp:34-141) with the module's numpy replaced by
                    gen_solve_trace_mp.NpProxy - nothing of it is rewritten; sqrt_info = FOCAL_LENGTH / 1.5 is the FP64 quotient.

The binary128 arbiter (oracle/avm_truth.cpp: avmt_triangulate, avmt_imu_propagate, avmt_projection_td_eval) is oracle/'s reading of
the same formulas in a wider scalar; tests/test_window_ops_truth.py compares its hi + lo pairs with the ones stored here, together
with the inputs they were computed from.

Run once (a few seconds):  python tests/golden/gen_window_ops_mp.py
"""
import os
import sys

import mpmath as mp
import numpy as real_np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (HERE, os.path.dirname(HERE), ROOT, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_solve_trace_mp import MPF, NpProxy, obj  # noqa: E402  (sets mp.dps = 50)

# (set, window, row): (start, nobs) and what the row is are asserted below
T_PICKS = [("T70", 0, 0), ("T70", 0, 12), ("T70", 0, 34), ("T70", 0, 50), ("T70", 0, 68), ("T70", 1, 3), ("T70", 1, 20), ("T70", 1, 42),
           ("T70", 1, 54), ("T70", 2, 0), ("T150", 0, 2), ("T150", 0, 60), ("T150", 0, 100), ("T150", 0, 128),
           ("TX", 0, 4), ("TX", 0, 90)]
# + every decision row of T70 window 1 (true depth 0.05, 0.09, 0.11, 0.2, -2): appended in main()
P_PICKS = [("default", 0), ("default", 1), ("default", 2), ("default", 5), ("default", 20), ("default", 83), ("tilted", 13), ("tilted", 125)]
F_PICKS = [0, 1, 2, 3, 10, 11, 20, 21, 22, 30, 31, 64, 65, 70, 100, 129]


def split(vals):
    hi = real_np.array([float(v) for v in vals])
    lo = real_np.array([float(v - MPF(h)) if real_np.isfinite(h) else real_np.nan for v, h in zip(vals, hi)])
    return hi, lo


def q2R(q):  # x y z w
    x, y, z, w = q
    return mp.matrix([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                      [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def vec(x):
    return mp.matrix([MPF(float(v)) for v in x])


def triangulate(a, b, e, init_depth):
    """feature_manager.cpp:209-249 for row e of window b: (ratio, depth, sigma [4], V [4][4] with column k belonging to sigma[k])."""
    ex = a["ex_pose"][b]
    tic, ric = vec(ex[:3]), q2R(vec(ex[3:]))
    st, no, ob = int(a["feat_start"][b, e]), int(a["feat_nobs"][b, e]), int(a["feat_obs_begin"][b, e])
    P_ = lambda f: vec(a["pose"][b, f, :3])
    R_ = lambda f: q2R(vec(a["pose"][b, f, 3:]))
    t0, R0 = P_(st) + R_(st) * tic, R_(st) * ric
    A = mp.zeros(2 * no, 4)
    for k in range(no):
        j = st + k
        t1, R1 = P_(j) + R_(j) * tic, R_(j) * ric
        t, R = R0.T * (t1 - t0), R0.T * R1
        mt = -(R.T * t)
        P = [[R[c, r] for c in range(3)] + [mt[r]] for r in range(3)]  # [R^T | -R^T t]
        f = [MPF(float(a["obs_xy"][b, ob + k, 0])), MPF(float(a["obs_xy"][b, ob + k, 1])), MPF(1)]
        nf = mp.sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])
        f = [c / nf for c in f]
        for c in range(4):
            A[2 * k, c] = f[0] * P[2][c] - f[2] * P[0][c]
            A[2 * k + 1, c] = f[1] * P[2][c] - f[2] * P[1][c]
    U, S, V = mp.svd_r(A, compute_uv=True)  # A = U diag(S) V, S descending
    assert all(S[k] >= S[k + 1] for k in range(3))
    ratio = V[3, 2] / V[3, 3]
    depth = ratio if ratio >= MPF("0.1") else MPF(float(init_depth))
    return ratio, depth, [S[k] for k in range(4)], [[V[k, i] for k in range(4)] for i in range(4)]


class _Be:
    sqrt = staticmethod(mp.sqrt)


def propagate(a, b, g):
    """estimator.cpp:100-107 on interval 9 of window b, from frame 10's pose and speed-bias: (pose [7], speedbias [9])."""
    from gen_visual_align import R2q

    P, V = vec(a["pose"][b, 10, :3]), vec(a["speedbias"][b, 10, :3])
    Ba, Bg = vec(a["speedbias"][b, 10, 3:6]), vec(a["speedbias"][b, 10, 6:9])
    R = q2R(vec(a["pose"][b, 10, 3:]))
    acc, gyr, dt = a["imu_acc"][b, 9], a["imu_gyr"][b, 9], a["imu_dt"][b, 9]
    g = vec(g)
    a0, w0 = vec(acc[0]), vec(gyr[0])
    half = MPF(1) / 2
    for s in range(int(a["imu_n"][b, 9])):
        a1, w1, h = vec(acc[s + 1]), vec(gyr[s + 1]), MPF(float(dt[s]))
        ua0 = R * (a0 - Ba) - g
        ug = half * (w0 + w1) - Bg
        R = R * q2R([ug[0] * h / 2, ug[1] * h / 2, ug[2] * h / 2, MPF(1)])
        ua = half * (ua0 + R * (a1 - Ba) - g)
        P, V = P + h * V + half * h * h * ua, V + h * ua
        a0, w0 = a1, w1
    q = R2q(_Be, R)  # w x y z
    return list(P) + [q[1], q[2], q[3], q[0]], list(V) + list(Ba) + list(Bg)


def main():
    import gen_golden as GG
    import gen_solve_trace as GS
    import gen_solve_trace_x as GX
    import window_ops_cases as WC
    from helpers import abi

    assert mp.mp.dps == 50
    out = {}
    # ---- triangulation
    sets = {k: make() for k, make in WC.T_SETS.items()}
    picks = list(T_PICKS) + [("T70", 1, e) for e in sorted(sets["T70"].kinds[1])]
    keys = ("ratio", "depth", "sigma", "V")
    res = {k + s: [] for k in keys for s in ("_hi", "_lo")}
    meta = dict(set=[], window=[], row=[], start=[], nobs=[], obs=[])
    for name, b, e in picks:
        a = sets[name].a
        assert e < a["n_feat"][b] and not a["inv_depth"][b, e] > 0, (name, b, e)
        ratio, depth, sig, V = triangulate(a, b, e, WC.INIT_DEPTH)
        for k, vals in zip(keys, ([ratio], [depth], sig, [V[i][k] for i in range(4) for k in range(4)])):
            hi, lo = split(vals)
            res[k + "_hi"].append(hi), res[k + "_lo"].append(lo)
        st, no, ob = int(a["feat_start"][b, e]), int(a["feat_nobs"][b, e]), int(a["feat_obs_begin"][b, e])
        obs = real_np.full((11, 2), real_np.nan)
        obs[:no] = a["obs_xy"][b, ob:ob + no]
        for k, v in zip(("set", "window", "row", "start", "nobs", "obs"), (name, b, e, st, no, obs)):
            meta[k].append(v)
        print("T %-4s window %d row %3d (start %d, %2d obs): ratio %s  sigma %s" % (name, b, e, st, no, mp.nstr(ratio, 8), [mp.nstr(s, 3) for s in sig]), flush=True)
    out.update({"t_" + k: real_np.array(v) for k, v in res.items()})
    out.update({"t_" + k: real_np.array(v) for k, v in meta.items()})
    # ---- dead-reckoning
    wp = WC.set_p()
    gs = dict(default=[float(v) for v in abi.default_options().g], tilted=list(WC.G_TILTED))
    res = {k + s: [] for k in ("pose", "speedbias") for s in ("_hi", "_lo")}
    meta = dict(g=[], window=[], n=[], dt=[])
    for gname, b in P_PICKS:
        pose, sb = propagate(wp.a, b, gs[gname])
        for k, vals in (("pose", pose), ("speedbias", sb)):
            hi, lo = split(vals)
            res[k + "_hi"].append(hi), res[k + "_lo"].append(lo)
        for k, v in zip(("g", "window", "n", "dt"), (gs[gname], b, int(wp.a["imu_n"][b, 9]), wp.a["imu_dt"][b, 9].copy())):
            meta[k].append(v)
        print("P window %3d (%2d samples, gravity %s): P %s" % (b, wp.a["imu_n"][b, 9], gname, [mp.nstr(v, 6) for v in pose[:3]]), flush=True)
    out.update({"p_" + k: real_np.array(v) for k, v in res.items()})
    out.update({"p_" + k: real_np.array(v) for k, v in meta.items()})
    # ---- td factor
    proxy = NpProxy()
    for mod in (GG, GS, GX):
        mod.np = proxy
    GX.TR, GX.ROW = MPF(WC.TR), MPF(WC.ROW)
    s = MPF(WC.FOCAL / 1.5)
    fa = WC.set_f()
    res = {k + s_: [] for k in ("residual", "jac") for s_ in ("_hi", "_lo")}
    for i in F_PICKS:
        aux = lambda side: obj([fa["vel_" + side][i, 0], fa["vel_" + side][i, 1], fa["td_" + side][i], fa["row_" + side][i]])
        r, Ji, Jj, Jex, Je, Jtd = GX.projection_td_factor(obj(fa["pose_i"][i]), obj(fa["pose_j"][i]), obj(fa["ex_pose"][i]), MPF(float(fa["inv_depth"][i])),
                                                          MPF(float(fa["td"][i])), obj(list(fa["pts_i"][i]) + [1.0]), obj(list(fa["pts_j"][i]) + [1.0]),
                                                          aux("i"), aux("j"), s)
        J = [list(Ji[c]) + list(Jj[c]) + list(Jex[c]) + [Je[c], Jtd[c]] for c in range(2)]
        for k, vals in (("residual", list(r)), ("jac", J[0] + J[1])):
            hi, lo = split(vals)
            res[k + "_hi"].append(hi), res[k + "_lo"].append(lo)
        print("F factor %3d: residual %s" % (i, [mp.nstr(v, 8) for v in r]), flush=True)
    out.update({"f_" + k: real_np.array(v) for k, v in res.items()})
    out.update(f_index=real_np.array(F_PICKS, real_np.int64), f_pose_i=fa["pose_i"][F_PICKS], f_inv_depth=fa["inv_depth"][F_PICKS], dps=real_np.int64(mp.mp.dps))
    path = os.path.join(HERE, "window_ops_mp.npz")
    real_np.savez_compressed(path, **out)
    print("wrote window_ops_mp.npz: %d features, %d intervals, %d factors, %d bytes" % (len(picks), len(P_PICKS), len(F_PICKS), os.path.getsize(path)))


if __name__ == "__main__":
    main()
