"""Test infrastructure: tests/host_cpp/align_shim.cpp (the hooks around avm_host::Estimator::visualInitialAlign) compiled with g++ into
a temporary directory and driven through ctypes."""
import ctypes as C
import os
import subprocess

import numpy as np

from helpers import PKG, abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def build_shim(tmpdir):
    import torch  # noqa: F401  (its bundled HIP runtime has to be the first one in the process, see lib.py)

    so = os.path.join(str(tmpdir), "libavm_align_shim.so")
    pkg = os.path.join(ROOT, PKG)
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O2", "-Wall", "-Wextra", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                           "-o", so, os.path.join(HERE, "host_cpp", "align_shim.cpp"), "-L" + pkg, "-lavm_hip", "-Wl,-rpath," + pkg])
    L = C.CDLL(so)
    L.as_create.restype = C.c_void_p
    L.as_last_error.restype = C.c_char_p
    L.as_stamp.restype = C.c_double
    return L


class AlignHost:
    """One avm_host::Estimator behind the shim."""

    def __init__(self, L, device=0):
        self.L = L
        self.h = C.c_void_p(L.as_create(int(device)))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.as_destroy(self.h)
            self.h = None

    def err(self):
        return self.L.as_last_error().decode()

    def load(self, al, win=None, w=0, drop_header=-1):
        sa = al.struct()
        sw = win.struct() if win is not None else None
        return self.L.as_load(self.h, C.byref(sa), C.byref(sw) if sw is not None else None, int(w), int(drop_header))

    def marshal(self, max_frames, max_samp):
        MF, MS = max_frames, max_samp
        out = dict(frame_R=np.zeros((MF, 9)), frame_T=np.zeros((MF, 3)), tic=np.zeros(3), imu_n=np.zeros(MF - 1, np.int32), imu_dt=np.zeros((MF - 1, MS)),
                   imu_acc=np.zeros((MF - 1, MS + 1, 3)), imu_gyr=np.zeros((MF - 1, MS + 1, 3)), imu_lin_ba=np.zeros((MF - 1, 3)),
                   imu_lin_bg=np.zeros((MF - 1, 3)), key_index=np.zeros(11, np.int32))
        dims = np.array([MF, MS, 0], np.int32)
        rc = self.L.as_marshal(self.h, abi.iptr(dims), abi.dptr(out["frame_R"]), abi.dptr(out["frame_T"]), abi.dptr(out["tic"]), abi.iptr(out["imu_n"]),
                               abi.dptr(out["imu_dt"]), abi.dptr(out["imu_acc"]), abi.dptr(out["imu_gyr"]), abi.dptr(out["imu_lin_ba"]),
                               abi.dptr(out["imu_lin_bg"]), abi.iptr(out["key_index"]))
        out["n_frames"] = int(dims[2])
        return rc, out

    def align(self):
        res = C.c_int32(-1)
        rc = self.L.as_align(self.h, C.byref(res))
        return rc, int(res.value)

    def state(self, n_frames, n_feat):
        F = n_frames
        out = dict(pose=np.zeros((11, 7)), speedbias=np.zeros((11, 9)), inv_depth=np.zeros(max(n_feat, 1)), g=np.zeros(3), delta_bg=np.zeros(3),
                   x=np.zeros(3 * F + 1), lin=np.zeros((10, 6)), lin_all=np.zeros((F - 1, 6)), is_key=np.zeros(F, np.int32))
        out["solver_flag"] = self.L.as_state(self.h, *[abi.dptr(out[k]) for k in ("pose", "speedbias", "inv_depth", "g", "delta_bg", "x", "lin", "lin_all")],
                                             abi.iptr(out["is_key"]))
        return out
