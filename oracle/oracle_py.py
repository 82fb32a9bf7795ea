"""ctypes loader for the CPU oracle (TEST INFRASTRUCTURE ONLY).

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this.
"""
import ctypes as C
import functools
import importlib
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# The functions that take a handle or scalars ctypes would not convert by itself: name -> (restype, argtypes), applied by _load() to
# whichever of them a library exports.  (Every other function takes byref() structs, pointers and ints only.)
_vp, _dp_t, _ip_t, _fp_t = C.c_void_p, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_float)
PROTOTYPES = {
    "avmo_triangulate_batch": (C.c_int, [_vp, C.c_double, C.c_int]),
    "avmo_slide_window": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double]),
    "avmo_gt_from_rows": (_vp, [_dp_t, C.c_int]),
    "avmo_gt_free": (None, [_vp]),
    "avmo_gt_seek": (C.c_int, [_vp]),
    "avmo_fsel_horizon_ground_truth": (C.c_int, [_vp, C.c_int, C.c_double, _dp_t, _dp_t, C.c_double, _dp_t, _dp_t]),
    "avmo_image_from_pointcloud": (C.c_int, [C.c_int, _fp_t, C.POINTER(_fp_t), C.c_int, _ip_t, _ip_t, _dp_t]),
    "avmt_triangulate": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double] + [_dp_t] * 8),
}


def _load(path):
    L = C.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        if hasattr(L, name):
            f = getattr(L, name)
            f.restype, f.argtypes = restype, argtypes
    return L


def build():
    subprocess.check_call(["make", "-C", _HERE, "-s"])


def lib():
    global _LIB
    if _LIB is None:
        path = os.path.join(_HERE, "libavm_oracle.so")
        if not os.path.exists(path):
            build()
        _LIB = _load(path)
    return _LIB


def use_library(path):
    """Switch to another build of the same oracle (bench.py compiles one with -march=native on the host it times)."""
    global _LIB
    _LIB = _load(path)
    return _LIB


# (the package's name has a hyphen: no import statement can name it, and it is imported on first use)
@functools.lru_cache(None)
def _abi():
    return importlib.import_module("anticipated-vins-mono_amd.abi")


@functools.lru_cache(None)
def _buffers():
    return importlib.import_module("anticipated-vins-mono_amd.buffers")


def _dp(a):
    return _abi().dptr(a)


def _ip(a):
    return _abi().iptr(a)


def window_solve(opt, win, prior_out=None, summary=None, n_threads=1):
    """In-place Estimator::optimization() on host WindowArrays."""
    s = win.struct()
    po = prior_out.struct() if prior_out is not None else None
    sp = _buffers().summary_ptr(summary) if summary is not None else None
    rc = lib().avmo_window_solve_batch(C.byref(opt), C.byref(s), C.byref(po) if po is not None else None, sp, int(n_threads))
    assert rc == 0
    return rc


def fsel_select(fsel, out, n_threads=1):
    s, o = fsel.struct(), out.struct()
    n = C.c_int64(0)
    rc = lib().avmo_fsel_select_batch(C.byref(s), C.byref(o), int(n_threads), C.byref(n))
    assert rc == 0
    return n.value


def preintegrate(opt, win):
    B = win.n_windows
    d, j, cv, sd, sq = np.zeros((B, 10, 10)), np.zeros((B, 10, 15, 15)), np.zeros((B, 10, 15, 15)), np.zeros((B, 10)), np.zeros((B, 10, 15, 15))
    s = win.struct()
    rc = lib().avmo_imu_preintegrate_batch(C.byref(opt), C.byref(s), _dp(d), _dp(j), _dp(cv), _dp(sd), _dp(sq))
    assert rc == 0
    return d, j, cv, sd, sq


_TRUTH = None


def truth_lib():
    """libavm_truth.so: the oracle with binary128 as its scalar type (oracle/avm_truth.cpp)."""
    global _TRUTH
    if _TRUTH is None:
        path = os.path.join(_HERE, "libavm_truth.so")
        if not os.path.exists(path):
            subprocess.check_call(["make", "-C", _HERE, "-s", "libavm_truth.so"])
        _TRUTH = _load(path)
    return _TRUTH


def truth_preintegrate(opt, win, sqrt_info=True):
    """avmt_imu_preintegrate on every window of host WindowArrays: the pre-integration in binary128 from the imu_* tables and the
    options' noise.  Returns (hi, lo): two dicts of delta [B,10,10], jacobian, covariance [B,10,15,15], sum_dt [B,10] and
    sqrt_info [B,10,15,15]; hi is the value rounded once to FP64, hi + lo the value to 32 digits."""
    B = win.n_windows
    shapes = dict(delta=(B, 10, 10), jacobian=(B, 10, 15, 15), covariance=(B, 10, 15, 15), sum_dt=(B, 10), sqrt_info=(B, 10, 15, 15))
    hi, lo = {k: np.zeros(s) for k, s in shapes.items()}, {k: np.zeros(s) for k, s in shapes.items()}
    s = win.struct()
    L = truth_lib()
    for w in range(B):
        ptrs = []
        for k in shapes:
            skip = k == "sqrt_info" and not sqrt_info
            ptrs += [None if skip else _dp(hi[k][w]), None if skip else _dp(lo[k][w])]
        rc = L.avmt_imu_preintegrate(C.byref(opt), C.byref(s), w, *ptrs)
        assert rc == 0
    return hi, lo


def _hilo(shapes):
    return {k: np.zeros(s) for k, s in shapes.items()}, {k: np.zeros(s) for k, s in shapes.items()}


def truth_triangulate(win, init_depth=5.0, features=None):
    """avmt_triangulate on host WindowArrays: FeatureManager::triangulate in binary128 for every (window, feature) pair of `features`
    (default: every row e < n_feat; rows with fewer than two observations included - their ratio is whatever a rank-2 system gives).
    Returns (hi, lo): dicts of ratio [B, max_feat] (v[2] / v[3] before the 0.1 rule), depth [B, max_feat] (after it), sigma
    [B, max_feat, 4] (descending) and V [B, max_feat, 4, 4] (column k belongs to sigma[k]); NaN where nothing was asked for."""
    B, mf = win.n_windows, win.dims["max_feat"]
    hi, lo = _hilo(dict(ratio=(B, mf), depth=(B, mf), sigma=(B, mf, 4), V=(B, mf, 4, 4)))
    for d in (hi, lo):
        for v in d.values():
            v[:] = np.nan
    if features is None:
        features = [(w, e) for w in range(B) for e in range(int(win.a["n_feat"][w]))]
    s = win.struct()
    L = truth_lib()
    for w, e in features:
        ptrs = []
        for k in ("ratio", "depth", "sigma", "V"):
            ptrs += [_dp(hi[k][w, e:e + 1]), _dp(lo[k][w, e:e + 1])]
        rc = L.avmt_triangulate(C.byref(s), int(w), int(e), float(init_depth), *ptrs)
        assert rc == 0, (w, e)
    return hi, lo


def truth_imu_propagate(win, g):
    """avmt_imu_propagate on every window of host WindowArrays (nothing is changed in place).  Returns (hi, lo): dicts of pose [B, 7]
    and speedbias [B, 9] of frame 10 after the dead-reckoning."""
    B = win.n_windows
    hi, lo = _hilo(dict(pose=(B, 7), speedbias=(B, 9)))
    gg = np.ascontiguousarray(g, float)
    s = win.struct()
    L = truth_lib()
    for w in range(B):
        rc = L.avmt_imu_propagate(C.byref(s), w, _dp(gg), _dp(hi["pose"][w]), _dp(lo["pose"][w]), _dp(hi["speedbias"][w]),
                                  _dp(lo["speedbias"][w]))
        assert rc == 0, w
    return hi, lo


def truth_projection_td_eval(arrays, tr, row, focal_length=460.0):
    """avmt_projection_td_eval on every factor of `arrays` (abi.td_factor_batch).  Returns (hi, lo): dicts of residual [n, 2], jac [n, 2, 20]."""
    f = _abi().td_factor_batch(arrays, tr, row, focal_length)
    hi, lo = _hilo(dict(residual=(f.n, 2), jac=(f.n, 2, 20)))
    L = truth_lib()
    for i in range(f.n):
        rc = L.avmt_projection_td_eval(C.byref(f), i, _dp(hi["residual"][i]), _dp(lo["residual"][i]), _dp(hi["jac"][i]),
                                       _dp(lo["jac"][i]))
        assert rc == 0, i
    return hi, lo


def eval_factors(opt, win, apply_loss=False):
    B, mo, mp = win.n_windows, win.dims["max_obs"], win.dims["max_prior"]
    out = dict(proj_r=np.zeros((B, mo, 2)), proj_J=np.zeros((B, mo, 2, 13)), imu_r=np.zeros((B, 10, 15)),
               imu_J=np.zeros((B, 10, 15, 30)), prior_res=np.zeros((B, mp)), cost=np.zeros(B))
    s = win.struct()
    rc = lib().avmo_window_eval_factors(C.byref(opt), C.byref(s), int(apply_loss),
                                        *[_dp(out[k]) for k in ("proj_r", "proj_J", "imu_r", "imu_J", "prior_res", "cost")])
    assert rc == 0
    return out


def fsel_information(fsel):
    P, H, mc = fsel.n_problems, fsel.dims["horizon"], fsel.dims["max_cand"]
    N, T = 9 * (H + 1), 3 * H
    om, dl, va = np.zeros((P, N, N)), np.zeros((P, mc, T, T)), np.zeros((P, mc), np.int32)
    s = fsel.struct()
    rc = lib().avmo_fsel_information(C.byref(s), _dp(om), _dp(dl), _ip(va))
    assert rc == 0
    return om, dl, va


def set_fast_linalg(on: bool):
    """bench.py's second CPU leg ("port_blocked"): vectorisable Schur / Cholesky / forward-substitution loops, bit-identical results."""
    lib().avmo_set_fast_linalg(1 if on else 0)


def fsel_nn_depth(fsel):
    """findNNDepth of every candidate, [P, max_cand]."""
    out = np.zeros((fsel.n_problems, fsel.dims["max_cand"]))
    s = fsel.struct()
    assert lib().avmo_fsel_nn_depth(C.byref(s), _dp(out)) == 0
    return out


def triangulate(win, init_depth=5.0, n_threads=1):
    """FeatureManager::triangulate in place on host WindowArrays (inverse depths <= 0 are replaced)."""
    s = win.struct()
    rc = lib().avmo_triangulate_batch(C.byref(s), float(init_depth), int(n_threads))
    assert rc == 0


def smallest_right_singular_vector(A):
    A = np.ascontiguousarray(A, float)
    v = np.zeros(4)
    rc = lib().avmo_smallest_right_singular_vector(int(A.shape[0]), _dp(A), _dp(v))
    assert rc == 0
    return v


def imu_propagate(win, g):
    """Estimator::processIMU dead-reckoning of the newest frame, in place on host WindowArrays."""
    s = win.struct()
    gg = np.ascontiguousarray(g, float)
    rc = lib().avmo_imu_propagate_batch(C.byref(s), _dp(gg))
    assert rc == 0


def fsel_horizon_imu(horizon, k_pos, k_quat, k_ba, k1_pos, k1_vel, k1_quat, acc, gyr, nr_imu, delta_imu):
    s = _abi().horizon_in(horizon, k_pos, k_quat, k_ba, k1_pos, k1_vel, k1_quat, acc, gyr, nr_imu, delta_imu)
    hp, hq = np.zeros((s.n_problems, horizon + 1, 3)), np.zeros((s.n_problems, horizon + 1, 4))
    rc = lib().avmo_fsel_horizon_imu(C.byref(s), _dp(hp), _dp(hq))
    assert rc == 0
    return hp, hq


def projection_td_eval(arrays, tr, row, focal_length=460.0):
    f = _abi().td_factor_batch(arrays, tr, row, focal_length)
    r, J = np.zeros((f.n, 2)), np.zeros((f.n, 2, 20))
    rc = lib().avmo_projection_td_eval(C.byref(f), _dp(r), _dp(J))
    assert rc == 0
    return r, J


def fsel_build_cloud(win, k1_pos, k1_quat, max_cloud=150):
    B = win.n_windows
    kp, kq = np.ascontiguousarray(k1_pos, float), np.ascontiguousarray(k1_quat, float)
    n, xy, dep = np.zeros(B, np.int32), np.zeros((B, max_cloud, 2)), np.zeros((B, max_cloud))
    s = win.struct()
    rc = lib().avmo_fsel_build_cloud(C.byref(s), _dp(kp), _dp(kq), int(max_cloud), _ip(n), _dp(xy), _dp(dep))
    assert rc == 0
    return n, xy, dep


class GroundTruth:
    def __init__(self, rows):
        r = np.ascontiguousarray(rows, float)
        self._L = lib()
        self._g = self._L.avmo_gt_from_rows(_dp(r), r.shape[0])

    @property
    def seek_idx(self):
        return int(self._L.avmo_gt_seek(self._g))

    def horizon(self, H, t0, k_pos, k_quat, deltaFrame):
        kp, kq = np.ascontiguousarray(k_pos, float), np.ascontiguousarray(k_quat, float)
        pos, quat = np.zeros((H + 1, 3)), np.zeros((H + 1, 4))
        rc = self._L.avmo_fsel_horizon_ground_truth(self._g, H, float(t0), _dp(kp), _dp(kq), float(deltaFrame), _dp(pos), _dp(quat))
        return rc, pos, quat

    def __del__(self):
        try:
            self._L.avmo_gt_free(self._g)
        except Exception:
            pass


def image_from_pointcloud(points, channels, num_cam=1):
    pts = np.ascontiguousarray(points, np.float32).reshape(-1, 3)
    n = pts.shape[0]
    ch = [np.ascontiguousarray(c, np.float32) for c in channels]
    arr = (C.POINTER(C.c_float) * 6)(*[c.ctypes.data_as(C.POINTER(C.c_float)) for c in ch])
    fid, cam, out = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros((n, 8))
    rc = lib().avmo_image_from_pointcloud(n, pts.ctypes.data_as(C.POINTER(C.c_float)), arr, int(num_cam), _ip(fid), _ip(cam), _dp(out))
    return rc, fid, cam, out


def slide_window(win, flag, shift_depth=True, init_depth=5.0):
    """Estimator::slideWindow on host WindowArrays, in place; returns the status (0, or -3 on sample-capacity overflow)."""
    s = win.struct()
    return lib().avmo_slide_window(C.byref(s), int(flag), int(bool(shift_depth)), float(init_depth))
