"""Test infrastructure: the case sets of tests/test_window_ops_truth.py and tests/golden/gen_window_ops_mp.py, and the distance
measures that triangulate_kernel, imu_propagate_kernel and projection_td_eval_kernel (csrc/triangulate.hip) are graded with.

Why sets of their own: synth.make_windows gives every window the same ex_pose, tracks that are dense (start 0, 11 observations) or
sparse, a feat_obs_begin without holes, equal dt in every IMU sample and at most a handful of windows per test - nothing in which a
mistake in the kernels' addressing (gid / max_feat, one observation past nobs, another window's biases beyond lane 63, dt[0] for
every sample) changes a number.

Set T, triangulation.  `set_t70()`: four windows at max_feat 70 (no multiple of the 64-thread block: windows 1 ... 3 begin inside a
wavefront) with n_feat 70, 55, 1 and 0; `set_t150()`: one window at max_feat 150 with n_feat 130.  Per window: an ex_pose of its own
(a rotation of 20 ... 60 degrees, tic of centimetres), frame positions scaled about frame 0 by 1, 1e-3, 0.1, 0.01 (T70) and 0.01
(T150), every (start, nobs) pair with nobs 2 ... 11 in each window of 55 rows or more, a feat_obs_begin laid out in a shuffled order
with one to three rows of PAD behind every feature, and valid-looking tracks with inv_depth -1 in the rows beyond n_feat.  Observations
are projections of one point at depth 1 ... 12 m plus 1e-3 of noise from the second on; a quarter of the rows keep a positive inverse
depth, the others hold 0.0, -0.0, -1.0 or NaN in turn.  Decision rows (no noise) sit at true depth 0.05, 0.09 (fall back to
init_depth), 0.11, 0.2 (kept) and -2 (behind the camera: falls back) in the windows whose scale keeps the camera's motion far below
0.05 m.  A plain feature is drawn again (same generator, next numbers) until a numpy estimate keeps its cond_d below 3e5 and its
ratio clear of 0.1: the seeds and this rule are what makes the conditions of test_the_case_sets_hold_what_they_are_meant_to hold.
`set_tx()`, mismatched tracks: one window at max_feat 150 with n_feat 130 and scale 1 in which every track has one observation that is
off by 0.02 ... 0.1, as an outlier of the front end is.  In T70 and T150 sigma_4 / sigma_1 is noise-sized (1e-3) and what a sweep
that stops early leaves between the last column and the others moves the depth by that factor times the leftover - inside the
margin the device is given; in TX the factor is percents, and a threshold of 1e-12 in place of 2.3e-16 shows.

Set P, dead-reckoning.  130 windows (blocks of 64 + 64 + 2), max_samp 20, the newest interval's sample count cycling through
0 ... 20, every sample its own dt from [0.7 / 400, 1.3 / 100], PAD beyond the count, biases, velocity and pose of frame 10 of its own
per window (and different from frame 9's), other data in intervals 0 ... 8.  Run with the default gravity and with G_TILTED.

Set F, td factor.  130 factors drawn like test_projection_td_factor_matches_oracle's, with designed rows: dep_j = 0.2, lambda =
1 / 0.3 and 1 / 60, zero velocities on one or both sides, row_i = 0 and row_i = ROW.
"""
import numpy as np

from helpers import blank_windows
from preint_cases import PAD, worse

INIT_DEPTH = 5.0
G_TILTED = (1.3, -2.1, 9.2)
TR, ROW, FOCAL = 0.033, 480.0, 460.0
NO_DEPTH = (0.0, -0.0, -1.0, np.nan)
PAIRS = [(s, n) for s in range(10) for n in range(2, 12 - s)]  # the 55 (start, nobs) with nobs 2 ... 11, start 0 ... 11 - nobs
DECISIONS = (0.05, 0.09, 0.11, 0.2, -2.0)
COND_MAX = 1e6
JAC_BLOCKS = (("pose_i.p", 0, 3), ("pose_i.th", 3, 6), ("pose_j.p", 6, 9), ("pose_j.th", 9, 12), ("ex.p", 12, 15), ("ex.th", 15, 18),
              ("lambda", 18, 19), ("td", 19, 20))
assert len(PAIRS) == 55


def q2R(q):  # x y z w, Eigen's toRotationMatrix (no normalization)
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _axis_angle_q(axis, angle):
    axis = axis / np.linalg.norm(axis)
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])


def _qmul(a, b):  # x y z w
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


# ---- set T ----------------------------------------------------------------------------------------------------------------------------
def system_rows(a, w, e):
    """The (2 nobs) x 4 system of feature_manager.cpp:209-249 for row e of window w, in FP64 numpy (the generator's estimate only)."""
    ex = a["ex_pose"][w]
    tic, ric = ex[:3], q2R(ex[3:])
    st, no, ob = int(a["feat_start"][w, e]), int(a["feat_nobs"][w, e]), int(a["feat_obs_begin"][w, e])
    cam = lambda f: (q2R(a["pose"][w, f, 3:]) @ ric, a["pose"][w, f, :3] + q2R(a["pose"][w, f, 3:]) @ tic)
    R0, t0 = cam(st)
    rows = []
    for k in range(no):
        R1, t1 = cam(st + k)
        R, t = R0.T @ R1, R0.T @ (t1 - t0)
        P = np.hstack([R.T, (-R.T @ t)[:, None]])
        f = np.array([a["obs_xy"][w, ob + k, 0], a["obs_xy"][w, ob + k, 1], 1.0])
        f /= np.linalg.norm(f)
        rows += [f[0] * P[2] - f[2] * P[0], f[1] * P[2] - f[2] * P[1]]
    return np.array(rows)


def cond_d(sigma, V):
    """The first-order condition number of d = v[2] / v[3] (v: the last right singular vector) under a normwise perturbation of the
    system: sigma_1 * sum_{i < 4} |V[2, i] / v[2] - V[3, i] / v[3]| / (sigma_i - sigma_4).  sigma [..., 4] descending, V [..., 4, 4]
    with column k belonging to sigma[k]."""
    sigma, V = np.asarray(sigma, float), np.asarray(V, float)
    with np.errstate(all="ignore"):
        c = np.zeros(sigma.shape[:-1])
        for i in range(3):
            c = c + np.abs(V[..., 2, i] / V[..., 2, 3] - V[..., 3, i] / V[..., 3, 3]) / (sigma[..., i] - sigma[..., 3])
        return sigma[..., 0] * c


def decision_margin(ratio, cond):
    """How far from 0.1 a ratio has to stay for rounding to decide no fallback: 1e3 * cond_d * 2.2e-16 * |d|."""
    return 1e3 * cond * 2.2e-16 * np.abs(ratio)


def _tri_window(a, w, n_feat, scale, decisions, rng, gross=False):
    mf, mo = a["inv_depth"].shape[1], a["obs_xy"].shape[1]
    # this window's extrinsic and body frames
    a["ex_pose"][w, :3] = rng.normal(0, 0.03, 3)
    a["ex_pose"][w, 3:] = _axis_angle_q(rng.normal(size=3), np.deg2rad(rng.uniform(20, 60)))
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    step_axis, vel, P0 = rng.normal(size=3), rng.normal(size=3), rng.normal(0, 2.0, 3)
    vel /= np.linalg.norm(vel)
    for f in range(11):
        a["pose"][w, f, :3] = P0 + scale * (0.1 * f * vel + (rng.normal(0, 0.02, 3) if f else 0.0))
        a["pose"][w, f, 3:] = q
        q = _qmul(q, _axis_angle_q(step_axis + 0.3 * rng.normal(size=3), np.deg2rad(rng.uniform(0.8, 1.6))))
        q /= np.linalg.norm(q)
    # the rows: the live ones sorted by start (the table contract, BAD_ORDER), every start at least twice; ghosts behind them
    if n_feat >= 55:
        live = PAIRS + ([(9, 2)] + [PAIRS[int(k)] for k in rng.integers(0, 55, n_feat - 56)] if n_feat > 55 else [])
    else:
        live = [(3, 4)][:n_feat]
    live = sorted(live[:n_feat], key=lambda p: p[0])
    rows = live + [PAIRS[int(k)] for k in rng.integers(0, 55, mf - n_feat)]
    a["n_feat"][w] = n_feat
    a["feat_start"][w], a["feat_nobs"][w] = [p[0] for p in rows], [p[1] for p in rows]
    a["obs_xy"][w] = PAD
    at = 2
    for e in rng.permutation(mf):
        a["feat_obs_begin"][w, e] = at
        at += rows[e][1] + int(rng.integers(1, 4))
    assert at <= mo
    # depth slots: every fourth live row keeps a depth; decision rows among the short tracks of the others
    a["inv_depth"][w] = -1.0
    kind = {}
    short = [e for e in range(n_feat) if e % 4 != 1 and rows[e][1] <= 4]
    for d, e in zip(decisions, short[::max(1, len(short) // max(1, len(decisions)))]):
        kind[e] = d
    assert len(kind) == len(decisions)
    k = 0
    for e in range(n_feat):
        if e % 4 == 1:
            a["inv_depth"][w, e] = rng.uniform(0.05, 1.0)
        else:
            a["inv_depth"][w, e] = NO_DEPTH[k % 4]
            k += 1
    ric, tic = q2R(a["ex_pose"][w, 3:]), a["ex_pose"][w, :3]

    def observe(e, depth, noise):
        st, no, ob = rows[e][0], rows[e][1], int(a["feat_obs_begin"][w, e])
        xy = rng.uniform(-0.2, 0.2, 2) if e in kind else rng.uniform(-0.5, 0.5, 2)
        cam = lambda f: (q2R(a["pose"][w, f, 3:]) @ ric, a["pose"][w, f, :3] + q2R(a["pose"][w, f, 3:]) @ tic)
        R0, t0 = cam(st)
        pw = R0 @ (depth * np.array([xy[0], xy[1], 1.0])) + t0
        for j in range(no):
            R1, t1 = cam(st + j)
            pc = R1.T @ (pw - t1)
            a["obs_xy"][w, ob + j] = pc[:2] / pc[2] + (rng.normal(0, noise, 2) if j else 0.0)
        if gross and noise:  # a mismatched observation, as a front end's outlier: the system is far from consistent
            a["obs_xy"][w, ob + int(rng.integers(1, no))] += rng.choice([-1.0, 1.0], 2) * rng.uniform(0.02, 0.1, 2)

    for e in range(mf):
        if e in kind:
            observe(e, kind[e], 0.0)
            continue
        for _ in range(200):
            observe(e, rng.uniform(1.0, 12.0), 1e-3)
            _, s, Vt = np.linalg.svd(system_rows(a, w, e))
            c, d = cond_d(s, Vt.T), Vt[3, 2] / Vt[3, 3]
            if c <= 3e5 and abs(d - 0.1) > 10 * decision_margin(d, c) + 1e-6:
                break
        else:
            raise AssertionError("no admissible draw for row %d of window %d" % (e, w))
    return kind


def _tri_set(max_feat, n_feats, scales, decision_windows, seed, gross=False):
    B = len(n_feats)
    w = blank_windows(B, max_feat=max_feat, max_obs=15 * max_feat, max_samp=1, max_prior=1, max_pblk=1)
    w.a["imu_n"][:] = 0
    kinds = {}
    for b in range(B):
        rng = np.random.Generator(np.random.Philox(key=seed + b))
        kinds[b] = _tri_window(w.a, b, n_feats[b], scales[b], DECISIONS if b in decision_windows else (DECISIONS[-1:] if n_feats[b] >= 55 else ()), rng, gross)
    w.kinds = kinds  # {window: {row: true depth of a decision row}}
    return w


T70_NFEAT, T70_SCALE = (70, 55, 1, 0), (1.0, 1e-3, 0.1, 0.01)
T150_NFEAT, T150_SCALE = (130,), (0.01,)
TX_NFEAT, TX_SCALE = (130,), (1.0,)


def set_t70():
    return _tri_set(70, T70_NFEAT, T70_SCALE, (1,), 0x7A1170)


def set_t150():
    return _tri_set(150, T150_NFEAT, T150_SCALE, (0,), 0x7A1150)


def set_tx():
    """Mismatched tracks: one window of 130 rows at max_feat 150 in which every plain track has one observation that is off by 0.02 ... 0.1."""
    return _tri_set(150, TX_NFEAT, TX_SCALE, (), 0x7A1171, gross=True)


T_SETS = {"T70": set_t70, "T150": set_t150, "TX": set_tx}


def no_depth_rows(w):
    """[(window, row)] of the live rows that triangulate() has to fill: inv_depth not > 0."""
    a = w.a
    return [(b, e) for b in range(w.n_windows) for e in range(int(a["n_feat"][b])) if not a["inv_depth"][b, e] > 0]


def permuted_t(w, seed=0x7A11FF):
    """A copy of `w` with the windows in another order, the live rows of every window rotated by one place within their group of equal
    feat_start (the table contract keeps feat_start ascending), the ghost rows rotated among themselves, and every row's observations
    moved to a fresh shuffled layout (other holes).  Returns (copy, where): where[b, e] = (b', e') of the row that holds what row e of
    window b of `w` holds."""
    a, B = w.a, w.n_windows
    mf, mo = w.dims["max_feat"], w.dims["max_obs"]
    out = w.copy()
    o = out.a
    wperm = [(b + 1) % B for b in range(B)] if B > 1 else [0]
    where = np.zeros((B, mf, 2), np.int64)
    rng = np.random.Generator(np.random.Philox(key=seed))
    for b in range(B):
        nb, n = wperm[b], int(a["n_feat"][b])
        groups = [[e for e in range(n) if a["feat_start"][b, e] == s] for s in range(11)] + [list(range(n, mf))]
        dest = np.arange(mf)
        for g in groups:
            for i, e in enumerate(g):
                dest[e] = g[(i + 1) % len(g)]
        for k in ("pose", "speedbias", "ex_pose", "n_feat"):
            o[k][nb] = a[k][b]
        o["obs_xy"][nb] = PAD
        begin = np.zeros(mf, np.int64)
        at = 1
        for e in rng.permutation(mf):
            begin[e] = at
            at += int(a["feat_nobs"][b, e]) + int(rng.integers(1, 4))
        assert at <= mo
        for e in range(mf):
            d, no, ob = dest[e], int(a["feat_nobs"][b, e]), int(a["feat_obs_begin"][b, e])
            for k in ("feat_start", "feat_nobs", "inv_depth"):
                o[k][nb, d] = a[k][b, e]
            o["feat_obs_begin"][nb, d] = begin[e]
            o["obs_xy"][nb, begin[e]:begin[e] + no] = a["obs_xy"][b, ob:ob + no]
            where[b, e] = (nb, d)
    return out, where


def nan_padded_t(w):
    """`w` with NaN in place of every PAD row of obs_xy and in the observations of the rows beyond n_feat."""
    out = w.copy()
    o = out.a
    o["obs_xy"][o["obs_xy"] == PAD] = np.nan
    for b in range(w.n_windows):
        for e in range(int(o["n_feat"][b]), w.dims["max_feat"]):
            ob, no = int(o["feat_obs_begin"][b, e]), int(o["feat_nobs"][b, e])
            o["obs_xy"][b, ob:ob + no] = np.nan
    return out


# ---- set P ----------------------------------------------------------------------------------------------------------------------------
def set_p():
    B, S = 130, 20
    w = blank_windows(B, max_feat=1, max_obs=11, max_samp=S, max_prior=1, max_pblk=1)
    rng = np.random.Generator(np.random.Philox(key=0x7A1190))
    a = w.a
    a["imu_n"][:, :9] = rng.integers(0, S + 1, (B, 9))
    a["imu_n"][:, 9] = np.arange(B) % (S + 1)
    base = rng.uniform(1.0 / 400, 1.0 / 100, (B, 10, 1))
    a["imu_dt"][:] = base * (1.0 + rng.uniform(-0.3, 0.3, (B, 10, S)))
    a["imu_acc"][:] = rng.normal(0, 0.5, (B, 10, S + 1, 3)) + np.array([0, 0, 9.8])
    a["imu_gyr"][:] = rng.normal(0, 0.2, (B, 10, S + 1, 3))
    for b in range(0, B, 5):  # every fifth window: the fastest sample of the newest interval turns at 3 rad/s
        g = a["imu_gyr"][b, 9, :a["imu_n"][b, 9] + 1]
        g *= 3.0 / np.linalg.norm(g, axis=1).max()
    for b in range(B):
        for j in range(10):
            n = a["imu_n"][b, j]
            a["imu_dt"][b, j, n:] = PAD
            a["imu_acc"][b, j, n + 1:] = PAD
            a["imu_gyr"][b, j, n + 1:] = PAD
    a["pose"][:, :, :3] = rng.normal(0, 3.0, (B, 11, 3))
    q = rng.normal(size=(B, 11, 4))
    a["pose"][:, :, 3:] = q / np.linalg.norm(q, axis=-1, keepdims=True)
    a["speedbias"][:, :, 0:3] = rng.normal(0, 1.0, (B, 11, 3))
    a["speedbias"][:, :, 3:6] = rng.normal(0, 0.02, (B, 11, 3))
    a["speedbias"][:, :, 6:9] = rng.normal(0, 0.002, (B, 11, 3))
    return w


P_PERM = (37 * np.arange(130) + 11) % 130


def permuted_p(w, perm=P_PERM):
    """A copy of `w` whose window perm[i] holds what window i of `w` holds."""
    out = w.copy()
    for k, v in w.a.items():
        out.a[k][perm] = v
    return out


def nan_padded_p(w):
    out = w.copy()
    a = out.a
    for b in range(w.n_windows):
        for j in range(10):
            n = a["imu_n"][b, j]
            a["imu_dt"][b, j, n:] = np.nan
            a["imu_acc"][b, j, n + 1:] = np.nan
            a["imu_gyr"][b, j, n + 1:] = np.nan
    return out


# ---- set F ----------------------------------------------------------------------------------------------------------------------------
F_DESIGNED = dict(dep_j=(3, 70), lam_near=(10, 64), lam_far=(11, 65), vel_zero=(20, 66, 129), vel_i_zero=(21,), vel_j_zero=(22,), row_0=(30, 67), row_full=(31, 68))


def set_f():
    rng = np.random.Generator(np.random.Philox(key=0x7A11F0))
    n = 130

    def unit(x):
        return x / np.linalg.norm(x, axis=-1, keepdims=True)

    def pose(scale):
        return np.hstack([scale * rng.normal(size=(n, 3)), unit(np.array([0, 0, 0, 1.0]) + 0.2 * rng.normal(size=(n, 4)))])

    a = dict(pose_i=pose(0.5), pose_j=pose(0.5), ex_pose=pose(0.05), inv_depth=1.0 / rng.uniform(2, 15, n), td=0.01 * rng.normal(size=n),
             pts_i=0.4 * rng.normal(size=(n, 2)), pts_j=0.4 * rng.normal(size=(n, 2)), vel_i=0.3 * rng.normal(size=(n, 2)),
             vel_j=0.3 * rng.normal(size=(n, 2)), td_i=0.01 * rng.normal(size=n), td_j=0.01 * rng.normal(size=n),
             row_i=rng.uniform(0, ROW, n), row_j=rng.uniform(0, ROW, n))
    D = F_DESIGNED
    a["inv_depth"][list(D["lam_near"])] = 1.0 / 0.3
    a["inv_depth"][list(D["lam_far"])] = 1.0 / 60.0
    for k in D["vel_zero"]:
        a["vel_i"][k] = a["vel_j"][k] = 0.0
    a["vel_i"][list(D["vel_i_zero"])] = 0.0
    a["vel_j"][list(D["vel_j_zero"])] = 0.0
    a["row_i"][list(D["row_0"])] = 0.0
    a["row_i"][list(D["row_full"])] = ROW
    for k in D["dep_j"]:  # frame j keeps its rotation and is placed so that the point lies 0.2 in front of its camera
        pci = td_forward(a, k)["pts_camera_i"]
        Ri, Rj, ric, tic = q2R(a["pose_i"][k, 3:]), q2R(a["pose_j"][k, 3:]), q2R(a["ex_pose"][k, 3:]), a["ex_pose"][k, :3]
        pw = Ri @ (ric @ pci + tic) + a["pose_i"][k, :3]
        a["pose_j"][k, :3] = pw - Rj @ (ric @ np.array([0.05, -0.03, 0.2]) + tic)
    return a


def td_forward(a, i):
    """The forward chain of ProjectionTdFactor::Evaluate for factor i in FP64 numpy: the scales of the residual measure
    (projection_td_factor.cpp:56-73)."""
    s = FOCAL / 1.5
    vi, vj = np.append(a["vel_i"][i], 0.0), np.append(a["vel_j"][i], 0.0)
    pi_td = np.append(a["pts_i"][i], 1.0) - (a["td"][i] - a["td_i"][i] + TR / ROW * (a["row_i"][i] - ROW / 2)) * vi
    pj_td = np.append(a["pts_j"][i], 1.0) - (a["td"][i] - a["td_j"][i] + TR / ROW * (a["row_j"][i] - ROW / 2)) * vj
    Ri, Rj, ric = q2R(a["pose_i"][i, 3:]), q2R(a["pose_j"][i, 3:]), q2R(a["ex_pose"][i, 3:])
    tic = a["ex_pose"][i, :3]
    pci = pi_td / a["inv_depth"][i]
    pw = Ri @ (ric @ pci + tic) + a["pose_i"][i, :3]
    pcj = ric.T @ (Rj.T @ (pw - a["pose_j"][i, :3]) - tic)
    return dict(pts_camera_i=pci, pts_camera_j=pcj, dep_j=pcj[2], scale=s * (np.abs(pcj[:2] / pcj[2]) + np.abs(pj_td[:2])))


def permuted_f(a, perm):
    """Factor perm[i] of the copy holds what factor i of `a` holds."""
    out = {k: np.empty_like(v) for k, v in a.items()}
    for k, v in a.items():
        out[k][perm] = v
    return out


F_PERM = (47 * np.arange(130) + 29) % 130


# ---- the distance measures ------------------------------------------------------------------------------------------------------------
assert np.finfo(np.longdouble).eps < 2e-19, "the depth distance subtracts in x87 extended precision"


def depth_distances(inv_depth, hi, lo, rows, init_depth=INIT_DEPTH):
    """`inv_depth` [B, max_feat] against the arbiter's (hi, lo) of oracle_py.truth_triangulate over `rows` [(window, row)]:
      graded rows (the truth keeps its ratio: >= 0.1)   |lambda - lambda_t| / (|lambda_t| cond_d), lambda_t = 1 / (hi + lo) of the ratio
      fallback rows (ratio < 0.1, or NaN)               1 / init_depth, the same bits on every side: 0 or infinity
    A NaN or an infinity counts as an infinite distance.  Returns {(window, row): distance}, the cond_d of every row and the graded mask."""
    out, cond, graded = {}, {}, {}
    c_all = cond_d(hi["sigma"], hi["V"])
    for b, e in rows:
        r = hi["ratio"][b, e]
        graded[b, e] = bool(r >= 0.1)
        cond[b, e] = float(c_all[b, e])
        x = inv_depth[b, e]
        if not graded[b, e]:
            out[b, e] = 0.0 if np.float64(x).tobytes() == np.float64(1.0 / init_depth).tobytes() else np.inf
            continue
        lt = np.longdouble(1.0) / (np.longdouble(r) + np.longdouble(lo["ratio"][b, e]))
        out[b, e] = worse(0.0, float(abs(np.longdouble(x) - lt) / (abs(lt) * np.longdouble(cond[b, e]))))
    return out, cond, graded


def pose_distances(pose10, sb10, hi):
    """Frame 10 after the dead-reckoning, pose10 [B, 7] and sb10 [B, 9], against the arbiter's hi: per window |P - P_t| / |P_t|,
    |V - V_t| / |V_t|, and the quaternion sign-insensitive against 1.  Returns {"P" / "V" / "q": [B] distances}."""
    out = {k: np.zeros(len(pose10)) for k in ("P", "V", "q")}
    with np.errstate(all="ignore"):
        for b in range(len(pose10)):
            tp, tv, tq = hi["pose"][b, :3], hi["speedbias"][b, :3], hi["pose"][b, 3:]
            out["P"][b] = worse(0.0, np.linalg.norm(pose10[b, :3] - tp) / np.linalg.norm(tp))
            out["V"][b] = worse(0.0, np.linalg.norm(sb10[b, :3] - tv) / np.linalg.norm(tv))
            dq = (np.linalg.norm(pose10[b, 3:] - tq), np.linalg.norm(pose10[b, 3:] + tq))
            out["q"][b] = worse(0.0, np.inf if not np.isfinite(dq).all() else min(dq))
    return out


def factor_distances(r, J, hi, a):
    """residual [n, 2] and jac [n, 2, 20] against the arbiter's hi: the residual per factor and component against
    s (|x / z| + |u|) (a difference: its own size is no scale), the Jacobian per factor and block of JAC_BLOCKS against the block's
    largest entry in the truth; a block that is exactly zero there has to be exactly zero.  Returns ({"residual": [n], block: [n]},
    [messages about blocks that should be zero and are not])."""
    n = len(r)
    out, bad = {"residual": np.zeros(n)}, []
    out.update({k: np.zeros(n) for k, _, _ in JAC_BLOCKS})
    with np.errstate(all="ignore"):
        for i in range(n):
            sc = td_forward(a, i)["scale"]
            out["residual"][i] = worse(0.0, (np.abs(r[i] - hi["residual"][i]) / sc).max() if np.isfinite(r[i]).all() else np.inf)
            for k, c0, c1 in JAC_BLOCKS:
                x, t = J[i, :, c0:c1], hi["jac"][i, :, c0:c1]
                if not t.any():
                    if x.any() or not np.isfinite(x).all():
                        bad.append("factor %d: block %s is zero in the truth, not here" % (i, k))
                else:
                    out[k][i] = worse(0.0, np.abs(x - t).max() / np.abs(t).max() if np.isfinite(x).all() else np.inf)
    return out, bad
