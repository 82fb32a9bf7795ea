"""Host-side mirror of FeatureSelector::select() (vins_estimator/src/feature_selector.h:49-50,
feature_selector.cpp:74-202) over the C ABI.

The reference mutates `image` in place and returns {trackedFeatures_, selectedIds}; the host
bookkeeping around the scoring loop (splitOnFeatureId :208-219, the tracked list :108-120,192-196)
is plain index work and stays on the host, the information matrices and the greedy logdet
scoring run on the GPU through avm_fsel_select_batch.  select_stream() is the same function for a batch
of streams whose images and selector state live where the tables live: avm_fsel_select_image_batch does
that bookkeeping in kernels around the same selection.
"""
import ctypes as C

import numpy as np

from . import abi, buffers
from .lib import Context


class FeatureSelector:
    def __init__(self, ctx: Context = None, device: int = 0):
        self.ctx = ctx or Context(device)
        self.trackedFeatures_ = []  # feature_selector.h:93
        self.lastFeatureId_ = 0

    def select_batch(self, problems: buffers.FselArrays, want_fvalues: bool = True, want_min_gap: bool = False):
        """Greedy selection for P independent frames. Returns (n_selected[P], ids[P, max_features], fvalues[, min_gap: how firmly every
        round was decided, avm_fsel_out::min_gap])."""
        P, mf = problems.n_problems, problems.dims["max_features"]
        dev = "cuda:%d" % self.ctx.device if problems.on_device else None
        out = buffers.FselOutArrays.alloc(P, mf, dev, want_min_gap=want_min_gap)
        if not want_fvalues:
            out.a["fvalues"] = None
        s, o = problems.struct(), out.struct()
        rc = self.ctx._L.avm_fsel_select_batch(self.ctx.h, problems.mem, C.byref(s), C.byref(o))
        self.ctx.check(rc, "avm_fsel_select_batch")
        return out

    def generateFutureHorizon(self, horizon, k_pos, k_quat, k_ba, k1_pos, k1_vel, k1_quat, acc, gyr, nr_imu, delta_imu):
        """FeatureSelector::generateFutureHorizon in IMU mode = HorizonGenerator::imu (horizon_generator.cpp:25-69) for P
        frames: returns hor_pos [P, H+1, 3], hor_quat [P, H+1, 4] (x y z w), the arrays avm_fsel_batch consumes.  Host arrays give
        host arrays; device tensors (all eleven inputs then) give device tensors, nothing crossing to the host."""
        if hasattr(k_pos, "data_ptr"):
            import torch

            f64 = lambda a, n: a.to(torch.float64).reshape(-1, n).contiguous()
            keep = dict(k_pos=f64(k_pos, 3), k_quat=f64(k_quat, 4), k_ba=f64(k_ba, 3), k1_pos=f64(k1_pos, 3), k1_vel=f64(k1_vel, 3),
                        k1_quat=f64(k1_quat, 4), acc=f64(acc, 3), gyr=f64(gyr, 3), delta_imu=delta_imu.to(torch.float64).reshape(-1).contiguous())
            nr = nr_imu.to(torch.int32).reshape(-1).contiguous()
            s = abi.FselHorizonIn()
            s.n_problems, s.horizon = keep["k_pos"].shape[0], int(horizon)
            for k, v in keep.items():
                setattr(s, k, abi.dptr(v))
            s.nr_imu = abi.iptr(nr)
            P, dev = s.n_problems, keep["k_pos"].device
            hp, hq = torch.zeros((P, horizon + 1, 3), dtype=torch.float64, device=dev), torch.zeros((P, horizon + 1, 4), dtype=torch.float64, device=dev)
            mem = abi.AVM_MEM_DEVICE
        else:
            s = abi.horizon_in(horizon, k_pos, k_quat, k_ba, k1_pos, k1_vel, k1_quat, acc, gyr, nr_imu, delta_imu)
            P = s.n_problems
            hp, hq = np.zeros((P, horizon + 1, 3)), np.zeros((P, horizon + 1, 4))
            mem = abi.AVM_MEM_HOST
        rc = self.ctx._L.avm_fsel_horizon_imu(self.ctx.h, mem, C.byref(s), abi.dptr(hp), abi.dptr(hq))
        self.ctx.check(rc, "avm_fsel_horizon_imu")
        return hp, hq

    def initKDTree(self, windows: buffers.WindowArrays, k1_pos, k1_quat, max_cloud: int = 150):
        """The depth cloud FeatureSelector::initKDTree() builds (feature_selector.cpp:380-433), one per window: returns
        n_cloud [B], cloud_xy [B, max_cloud, 2], cloud_depth [B, max_cloud], where the windows live (host arrays or device tensors;
        k1_pos / k1_quat are taken there too)."""
        B = windows.n_windows
        if windows.on_device:
            import torch

            dev = windows.a["pose"].device
            conv = lambda x: (x if hasattr(x, "data_ptr") else torch.from_numpy(np.ascontiguousarray(x, float))).to(device=dev, dtype=torch.float64).contiguous()
            kp, kq = conv(k1_pos), conv(k1_quat)
            n = torch.zeros(B, dtype=torch.int32, device=dev)
            xy, dep = torch.zeros((B, max_cloud, 2), dtype=torch.float64, device=dev), torch.zeros((B, max_cloud), dtype=torch.float64, device=dev)
        else:
            kp, kq = np.ascontiguousarray(k1_pos, float), np.ascontiguousarray(k1_quat, float)
            n, xy, dep = np.zeros(B, np.int32), np.zeros((B, max_cloud, 2)), np.zeros((B, max_cloud))
        s = windows.struct()
        rc = self.ctx._L.avm_fsel_build_cloud(self.ctx.h, windows.mem, C.byref(s), abi.dptr(kp), abi.dptr(kq), int(max_cloud), abi.iptr(n),
                                              abi.dptr(xy), abi.dptr(dep))
        self.ctx.check(rc, "avm_fsel_build_cloud")
        return n, xy, dep

    def select_stream(self, image: buffers.ImageArrays, state: buffers.SelectorState, problem: buffers.FselArrays, initialized=None,
                      init_thresh: int = None, prune_lost: bool = False, want_min_gap: bool = False, image_out: buffers.ImageArrays = None,
                      out: buffers.FselOutArrays = None):
        """FeatureSelector::select() (feature_selector.cpp:74-202) for one image per stream, where the arrays live (all host or all
        device): avm_fsel_select_image_batch.  `image` carries the tracker's points and their `prob` array; `state` is updated in
        place; `problem` gives the horizon, nr_imu, delta_imu, the cloud and the strides, and its n_cand / cand_* / n_used / used_*
        arrays are written.  initialized: [B] (None: every stream has solver_flag == NON_LINEAR).  Returns (out, image_out): the
        selection's FselOutArrays and the ImageArrays addFeatureCheckParallax takes (allocated with the image's max_pts unless given)."""
        B, mp = image.n_windows, image.dims["max_pts"]
        assert problem.n_problems == B and state.n_windows == B and image.on_device == state.on_device == problem.on_device and "prob" in image.a
        dev = "cuda:%d" % self.ctx.device if image.on_device else None
        out = out or buffers.FselOutArrays.alloc(B, problem.dims["max_features"], dev, want_min_gap=want_min_gap)
        if image_out is None:
            a = {"n_pts": np.zeros(B, np.int32), "feature_id": np.zeros((B, mp), np.int32), "xy": np.zeros((B, mp, 2))}
            if "vel_td" in image.a:
                a["vel_td"] = np.zeros((B, mp, 4))
            image_out = buffers.ImageArrays({"n_windows": B, "max_pts": mp}, a)
            image_out = image_out.to_device(dev) if dev else image_out
        thresh = getattr(self, "initThresh_", 0) if init_thresh is None else init_thresh
        si, ss, sp, so, sio = image.struct(), state.struct(), problem.struct(), out.struct(), image_out.struct()
        rc = self.ctx._L.avm_fsel_select_image_batch(self.ctx.h, image.mem, C.byref(si), abi.dptr(image.a["prob"]), abi.iptr(initialized),
                                                     int(thresh), int(bool(prune_lost)), C.byref(ss), C.byref(sp), C.byref(so), C.byref(sio))
        self.ctx.check(rc, "avm_fsel_select_image_batch")
        return out, image_out

    def information(self, problems: buffers.FselArrays):
        """Omega_kkH (+prior) [P,N,N], compact Delta_ell [P,max_cand,3H,3H], valid [P,max_cand] (host arrays)."""
        assert not problems.on_device
        P, H, mc = problems.n_problems, problems.dims["horizon"], problems.dims["max_cand"]
        N, T = 9 * (H + 1), 3 * H
        om, dl, va = np.zeros((P, N, N)), np.zeros((P, mc, T, T)), np.zeros((P, mc), np.int32)
        s = problems.struct()
        rc = self.ctx._L.avm_fsel_information(self.ctx.h, problems.mem, C.byref(s), abi.dptr(om), abi.dptr(dl), abi.iptr(va))
        self.ctx.check(rc, "avm_fsel_information")
        return om, dl, va

    def nn_depth(self, problems: buffers.FselArrays):
        """FeatureSelector::findNNDepth (feature_selector.cpp:437-459) of every candidate: [P, max_cand] (host array)."""
        assert not problems.on_device
        out = np.zeros((problems.n_problems, problems.dims["max_cand"]))
        s = problems.struct()
        self.ctx.check(self.ctx._L.avm_fsel_nn_depth(self.ctx.h, problems.mem, C.byref(s), abi.dptr(out)), "avm_fsel_nn_depth")
        return out

    def setParameters(self, enable=True, maxFeatures=150, initThresh=0):
        """The bookkeeping half of FeatureSelector::setParameters (feature_selector.cpp:24-34); the noise parameters and
        the horizon mode travel with the FselArrays the problem_builder returns."""
        self.enable_, self.maxFeatures_, self.initThresh_ = bool(enable), int(maxFeatures), int(initThresh)

    def select(self, image: dict, problem_builder, initialized: bool = True):
        """Single-frame select() with the reference's bookkeeping (feature_selector.cpp:74-202): `image` maps feature id ->
        8-vector (x y 1 u v vx vy prob) and is replaced by the subset handed to the back end; `problem_builder(new_ids,
        used_ids)` returns a 1-problem FselArrays for those ids (only called when `initialized`, i.e. solver_flag ==
        NON_LINEAR).  Returns (trackedFeatures_, selectedIds); () when disabled.  include/avm_host.hpp holds the C++
        statement of the same function, including the horizon / depth-cloud marshalling."""
        if not getattr(self, "enable_", True):
            return ()
        ids = sorted(image)
        new_ids = [i for i in ids if i > self.lastFeatureId_]  # splitOnFeatureId
        old = {i: image[i] for i in ids if i <= self.lastFeatureId_}
        if new_ids:
            self.lastFeatureId_ = new_ids[-1]
        subset = {f: old[f] for f in self.trackedFeatures_ if f in old}
        selected = []
        if initialized:
            prob = problem_builder(new_ids, sorted(subset))
            out = self.select_batch(prob).to_host()
            n = int(out.a["n_selected"][0])
            selected = [int(v) for v in out.a["selected_ids"][0, :n]]
            for f in selected:
                subset[f] = image[f]
        elif getattr(self, "firstImage_", True):
            subset = {f: image[f] for f in new_ids}  # the whole first image initializes the back end
            self.trackedFeatures_.extend(new_ids)
            self.firstImage_ = False
        if not initialized and len(subset) < getattr(self, "initThresh_", 0):
            subset.update(old)
        image.clear()
        image.update(subset)
        self.trackedFeatures_.extend(selected)
        return list(self.trackedFeatures_), selected
