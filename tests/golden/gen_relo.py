"""Generates tests/golden/relo.npz: the outputs of double2vector()'s relocalization block (estimator.cpp:588-604) for seeded cases, from
an independent statement written from that block, utility.h:66-108,130-139 (R2ypr, ypr2R, normalizeAngle) and Eigen's quaternion <->
matrix conversions - run once in FP64 (numpy scalars) and once with mpmath at 50 digits.

Per case the inputs are relo_pose as the solve returns it (relo_t | quaternion of relo_r, x y z w), the window pose of relo_frame
(Ps | quaternion of Rs), prev_relo_t and prev_relo_q.  The quaternions of relo_pose and of the window pose are a few parts in 1e3 away
from unit length - the reference normalises both (:593, :551) -, prev_relo_q is used as it is (estimator_node.cpp:293-294).

Stored: the inputs, m_<quantity> (the 50-digit values, rounded to double) and err_fp64_<quantity> [N] (the FP64 run's distance from the
50-digit run, per case).  Distances are absolute: angles / 180, vectors / max(1, largest input coordinate of the case), quaternions
entry by entry after sign alignment.

The generator asserts that its inputs are well posed: every yaw and both yaw differences at least 1 degree away from +-180 (atan2's and
normalizeAngle's jumps), every pitch within +-80 degrees.

    python tests/golden/gen_relo.py        # rewrites relo.npz next to this file
"""
import os

import numpy as np

QUANTITIES = ("drift_correct_yaw", "drift_correct_t", "relo_relative_t", "relo_relative_q", "relo_relative_yaw")
ANGLES, QUATS = ("drift_correct_yaw", "relo_relative_yaw"), ("relo_relative_q",)
N_RANDOM = 24
# (yaw of prev_relo_r, yaw of relo_r, yaw of Rs) of the cases in which normalizeAngle wraps: |yaw(Rs) - yaw(relo_r)| > 180
WRAP_YAWS = ((40.0, -150.0, 160.0), (-100.0, 170.0, -120.0), (10.0, 120.0, -110.0))


class FP64:
    pi = np.float64(np.pi)
    num = staticmethod(np.float64)
    sqrt, atan2, cos, sin, floor = (staticmethod(f) for f in (np.sqrt, np.arctan2, np.cos, np.sin, np.floor))


def mp50():
    import mpmath

    mpmath.mp.dps = 50

    class MP:
        pi = +mpmath.pi
        num = staticmethod(lambda x: mpmath.mpf(float(x)))
        sqrt, atan2, cos, sin, floor = (staticmethod(f) for f in (mpmath.sqrt, mpmath.atan2, mpmath.cos, mpmath.sin, mpmath.floor))

    return MP


# ---------------------------------------------------------------- the statement (scalars of M; matrices are lists of rows)
def q_normalized(q, M):                                                     # q = (x, y, z, w)
    n = M.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return [v / n for v in q]


def q_to_R(q):                                                              # Eigen::Quaternion::toRotationMatrix (no normalisation)
    x, y, z, w = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return [[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]


def R_to_q(R, M):                                                           # Eigen::Quaternion(Matrix3): x y z w
    t = R[0][0] + R[1][1] + R[2][2]
    if t > 0:
        t = M.sqrt(t + 1)
        w = t / 2
        t = 1 / (2 * t)
        return [(R[2][1] - R[1][2]) * t, (R[0][2] - R[2][0]) * t, (R[1][0] - R[0][1]) * t, w]
    i = 0
    if R[1][1] > R[0][0]:
        i = 1
    if R[2][2] > R[i][i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = M.sqrt(R[i][i] - R[j][j] - R[k][k] + 1)
    v = [None] * 3
    v[i] = t / 2
    t = 1 / (2 * t)
    w = (R[k][j] - R[j][k]) * t
    v[j] = (R[j][i] + R[i][j]) * t
    v[k] = (R[k][i] + R[i][k]) * t
    return v + [w]


def yaw_deg(R, M):                                                          # Utility::R2ypr(R).x()
    return M.atan2(R[1][0], R[0][0]) / M.pi * 180


def pitch_deg(R, M):                                                        # Utility::R2ypr(R).y()
    y = M.atan2(R[1][0], R[0][0])
    return M.atan2(-R[2][0], R[0][0] * M.cos(y) + R[1][0] * M.sin(y)) / M.pi * 180


def normalize_angle(a, M):                                                  # Utility::normalizeAngle
    return a - 360 * M.floor((a + 180) / 360) if a > 0 else a + 360 * M.floor((-a + 180) / 360)


def matvec(R, v):
    return [R[i][0] * v[0] + R[i][1] * v[1] + R[i][2] * v[2] for i in range(3)]


def transposed(R):
    return [[R[j][i] for j in range(3)] for i in range(3)]


def matmul(A, B):
    return [[A[i][0] * B[0][j] + A[i][1] * B[1][j] + A[i][2] * B[2][j] for j in range(3)] for i in range(3)]


def finish_statement(relo_pose, frame_pose, prev_t, prev_q, M=FP64):
    """estimator.cpp:597-603 for one window.  Returns a dict of the five quantities (lists of M's scalars) and the three yaws / pitches."""
    rp, fp, pt, pq = ([M.num(v) for v in a] for a in (relo_pose, frame_pose, prev_t, prev_q))
    relo_r, Rs, prev_r = q_to_R(q_normalized(rp[3:7], M)), q_to_R(q_normalized(fp[3:7], M)), q_to_R(pq)
    relo_t, Ps = rp[:3], fp[:3]
    dyaw = yaw_deg(prev_r, M) - yaw_deg(relo_r, M)
    y = dyaw / 180 * M.pi
    Rz = [[M.cos(y), -M.sin(y), 0], [M.sin(y), M.cos(y), 0], [0, 0, 1]]     # ypr2R(dyaw, 0, 0): Ry and Rx are the identity
    rot = matvec(Rz, relo_t)
    rT = transposed(relo_r)
    rel_yaw = yaw_deg(Rs, M) - yaw_deg(relo_r, M)
    return {"drift_correct_yaw": [dyaw], "drift_correct_t": [pt[i] - rot[i] for i in range(3)],
            "relo_relative_t": matvec(rT, [Ps[i] - relo_t[i] for i in range(3)]), "relo_relative_q": R_to_q(matmul(rT, Rs), M),
            "relo_relative_yaw": [normalize_angle(rel_yaw, M)],
            "_yaws": [yaw_deg(prev_r, M), yaw_deg(relo_r, M), yaw_deg(Rs, M)], "_pitches": [pitch_deg(R, M) for R in (prev_r, relo_r, Rs)],
            "_rel_yaw_raw": rel_yaw}


def distance(q, got, want, scale):
    """the metric of this fixture: `got`, `want` sequences of one quantity of one case; scale = max(1, largest input coordinate)"""
    d = [abs(g - w) for g, w in zip(got, want)]
    if q in QUATS:
        d = min(d, [abs(g + w) for g, w in zip(got, want)], key=max)
    return float(max(d)) / (180.0 if q in ANGLES else (scale if q.endswith("_t") else 1.0))


# ---------------------------------------------------------------- the cases
def _quat_ypr(y, p, r):
    """x y z w of Rz(y) Ry(p) Rx(r), degrees"""
    cy, sy, cp, sp, cr, sr = (f(np.deg2rad(a) / 2) for a in (y, p, r) for f in (np.cos, np.sin))
    return np.array([cy * cp * sr - sy * sp * cr, cy * sp * cr + sy * cp * sr, sy * cp * cr - cy * sp * sr, cy * cp * cr + sy * sp * sr])


def cases(seed=11):
    rng = np.random.default_rng(seed)
    yaws = [tuple(rng.uniform(-160, 160, 3)) for _ in range(N_RANDOM)] + list(WRAP_YAWS)
    out = dict(relo_pose=[], frame_pose=[], prev_relo_t=[], prev_relo_q=[])
    for k, (y_prev, y_relo, y_fr) in enumerate(yaws):
        ok = k >= N_RANDOM
        while not ok:                                                       # (random cases: redraw what sits on a jump)
            ok = all(abs(abs(d) - 180) > 5 for d in (y_prev - y_relo, y_fr - y_relo))
            if not ok:
                y_prev, y_relo, y_fr = rng.uniform(-160, 160, 3)
        pr = rng.uniform(-60, 60, (3, 2))
        scale = rng.choice([0.1, 1.0, 10.0])
        relo_t, Ps, prev_t = rng.uniform(-scale, scale, (3, 3))
        Ps = relo_t + rng.uniform(-0.3, 0.3, 3) * scale                     # the loop frame and the window frame see the same place
        out["relo_pose"].append(np.r_[relo_t, _quat_ypr(y_relo, *pr[0]) * rng.uniform(0.997, 1.003)])
        out["frame_pose"].append(np.r_[Ps, _quat_ypr(y_fr, *pr[1]) * rng.uniform(0.997, 1.003)])
        out["prev_relo_t"].append(prev_t)
        out["prev_relo_q"].append(_quat_ypr(y_prev, *pr[2]))
    return {k: np.array(v) for k, v in out.items()}


def main():
    c = cases()
    N = len(c["relo_pose"])
    MP = mp50()
    gold = dict(c)
    for q in QUANTITIES:
        gold["m_" + q], gold["err_fp64_" + q] = [], np.zeros(N)
    wraps = 0
    for k in range(N):
        args = [c[key][k] for key in ("relo_pose", "frame_pose", "prev_relo_t", "prev_relo_q")]
        f, m = finish_statement(*args, M=FP64), finish_statement(*args, M=MP)
        # well posed: away from the jumps of atan2 and normalizeAngle, and from the gimbal lock
        assert all(abs(abs(float(v)) - 180) >= 1 for v in m["_yaws"]), (k, m["_yaws"])
        assert all(abs(abs(float(v)) - 180) >= 1 for v in (m["drift_correct_yaw"][0], m["_rel_yaw_raw"])), k
        assert all(abs(float(v)) <= 80 for v in m["_pitches"]), (k, m["_pitches"])
        wraps += abs(float(m["_rel_yaw_raw"])) > 180
        scale = max(1.0, max(np.abs(a).max() for a in args))
        for q in QUANTITIES:
            gold["m_" + q].append([float(v) for v in m[q]])
            gold["err_fp64_" + q][k] = distance(q, [MP.num(v) for v in f[q]], m[q], scale)
    assert N >= 24 and wraps >= 2, (N, wraps)
    for q in QUANTITIES:
        gold["m_" + q] = np.array(gold["m_" + q])
        print("%-18s worst err_fp64 %.3g (non-zero: %s)" % (q, gold["err_fp64_" + q].max(), gold["err_fp64_" + q].max() > 0))
        assert gold["err_fp64_" + q].max() > 0
    np.savez(os.path.join(os.path.dirname(os.path.abspath(__file__)), "relo.npz"), **gold)


if __name__ == "__main__":
    main()
