"""Caller-owned buffers behind the C ABI structs (include/avm.h).

A *Arrays object owns a dict of arrays — numpy (host) or torch CUDA tensors (HBM
resident) — and builds the matching ctypes struct with raw pointers.  PyTorch is used
only as the device allocator here; no torch types cross the ABI.
"""
import ctypes as C

import numpy as np

from . import abi


def _device(where):
    """None when `where` - a *Arrays object, or one array - is host memory (numpy), else the torch device it lives on."""
    first = next(iter(where.a.values())) if hasattr(where, "a") else where
    return None if isinstance(first, np.ndarray) else first.device


def _torch_dtype(dtype):
    import torch

    return None if dtype is None else torch.int32 if dtype == np.int32 else torch.float64


def like(arrays, x, dtype, shape=None):
    """x contiguous, of `dtype` (np.int32 / np.float64; None: its own), in the memory space of `arrays`: a numpy array beside host
    arrays, a tensor on their device beside device ones.  shape: asserted when given."""
    dev = _device(arrays)
    if dev is None:
        out = np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x, dtype)
    else:
        import torch

        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x, dtype))
        out = t.to(device=dev, dtype=_torch_dtype(dtype)).contiguous()
    assert shape is None or tuple(out.shape) == tuple(shape), (tuple(out.shape), tuple(shape))
    return out


def zeros_like_space(arrays, shape, dtype):
    """zeros of `shape` and `dtype` (np.int32 / np.float64) in the memory space of `arrays`"""
    dev = _device(arrays)
    if dev is None:
        return np.zeros(shape, dtype)
    import torch

    return torch.zeros(shape, dtype=_torch_dtype(dtype), device=dev)


class _Arrays:
    """A subclass names its struct type as STRUCT; F64 / I32, the keys of `a` that become its double* / int32_t* members (an absent
    key or a None value: NULL), follow from it.  PER_STREAM: the [B] array that gives n_windows where dims has none."""
    STRUCT = None
    PER_STREAM = None
    F64: list = []
    I32: list = []

    def __init_subclass__(cls):
        if "STRUCT" in cls.__dict__:
            cls.F64, cls.I32 = abi.pointer_members(cls.STRUCT)

    def __init__(self, dims: dict, arrays: dict):
        self.dims = dict(dims)
        self.a = dict(arrays)

    @property
    def on_device(self) -> bool:
        return _device(self) is not None

    @property
    def mem(self) -> int:
        return abi.AVM_MEM_DEVICE if self.on_device else abi.AVM_MEM_HOST

    @property
    def n_windows(self) -> int:
        return self.dims["n_windows"] if "n_windows" in self.dims else self.a[self.PER_STREAM].shape[0]

    def struct(self):
        return self._fill(self.STRUCT())

    def slice(self, lo: int, hi: int):
        d = dict(self.dims)
        d["n_windows"] = hi - lo
        return type(self)(d, {k: v[lo:hi] for k, v in self.a.items()})

    def copy(self):
        if self.on_device:
            return type(self)(self.dims, {k: v.clone() for k, v in self.a.items()})
        return type(self)(self.dims, {k: v.copy() for k, v in self.a.items()})

    def to_device(self, device="cuda:0"):
        import torch

        out = {}
        for k, v in self.a.items():
            out[k] = torch.from_numpy(np.ascontiguousarray(v)).to(device) if isinstance(v, np.ndarray) else v.to(device)
        return type(self)(self.dims, out)

    def to_host(self):
        if not self.on_device:
            return self.copy()
        return type(self)(self.dims, {k: v.cpu().numpy() for k, v in self.a.items()})

    def _fill(self, s):
        for k, v in self.dims.items():
            setattr(s, k, v)
        for k in self.F64:
            setattr(s, k, abi.dptr(self.a.get(k)))
        for k in self.I32:
            setattr(s, k, abi.iptr(self.a.get(k)))
        return s


class WindowArrays(_Arrays):
    """avm_window_batch: the inputs/outputs of Estimator::optimization() for B windows."""

    STRUCT = abi.WindowBatch


TRACK_KEYS = ("n_feat", "feat_start", "feat_nobs", "feat_obs_begin", "obs_xy", "inv_depth", "obs_vel_td")   # what avm_solve_view_batch writes


class ImageArrays(_Arrays):
    """avm_image_batch: one image per window, what processImage gets from the tracker (camera 0): n_pts [B], feature_id [B, max_pts]
    strictly ascending, xy [B, max_pts, 2] and, with the time offset, vel_td [B, max_pts, 4] (velocity.x, velocity.y, cur_td, uv.y).
    Optionally `prob` [B, max_pts], the fPROB channel: not a member of the struct, the array FeatureSelector.select_stream takes beside it."""

    STRUCT = abi.ImageBatch

    @staticmethod
    def from_maps(images, max_pts: int, with_td: bool = False, prob=None) -> "ImageArrays":
        """images: per window a dict {feature id: (x, y)} or, with_td, {feature id: (x, y, vx, vy, cur_td, v)}; std::map order = sorted ids.
        prob: per window a dict {feature id: probability} (the `prob` array), or None."""
        B = len(images)
        a = {"n_pts": np.zeros(B, np.int32), "feature_id": np.zeros((B, max_pts), np.int32), "xy": np.zeros((B, max_pts, 2))}
        if with_td:
            a["vel_td"] = np.zeros((B, max_pts, 4))
        if prob is not None:
            a["prob"] = np.zeros((B, max_pts))
            for b, im in enumerate(images):
                a["prob"][b, :len(im)] = [prob[b][fid] for fid in sorted(im)]
        for b, im in enumerate(images):
            ids = sorted(im)
            assert len(ids) <= max_pts
            a["n_pts"][b] = len(ids)
            for i, fid in enumerate(ids):
                a["feature_id"][b, i] = fid
                a["xy"][b, i] = im[fid][:2]
                if with_td:
                    a["vel_td"][b, i] = im[fid][2:6]
        return ImageArrays({"n_windows": B, "max_pts": max_pts}, a)


class SelectorState(_Arrays):
    """avm_select_state: the members of FeatureSelector that outlive a call, one row per stream - last_feature_id [B] (lastFeatureId_),
    n_tracked [B] and tracked_id [B, max_tracked] (trackedFeatures_, append order), first_image [B] (firstImage_).  alloc() gives the
    state of freshly constructed selectors; copy / to_device / to_host as every *Arrays."""

    STRUCT, PER_STREAM = abi.SelectState, "n_tracked"

    @staticmethod
    def alloc(n_windows: int, max_tracked: int, device=None) -> "SelectorState":
        a = {"last_feature_id": np.zeros(n_windows, np.int32), "n_tracked": np.zeros(n_windows, np.int32),
             "tracked_id": np.zeros((n_windows, max_tracked), np.int32), "first_image": np.ones(n_windows, np.int32)}
        s = SelectorState({"max_tracked": max_tracked}, a)
        return s.to_device(device) if device else s


class ReloMsgArrays(_Arrays):
    """avm_relo_msg_batch: the loop-closure message of estimator_node.cpp:274-297, one row per stream - has_msg [B], frame_stamp [B],
    n_match [B], match_id [B, max_match] strictly ascending, match_xy [B, max_match, 2], prev_relo_t [B, 3], prev_relo_q [B, 4] (x y z w)."""

    STRUCT = abi.ReloMsgBatch

    @staticmethod
    def from_messages(messages, max_match: int) -> "ReloMsgArrays":
        """messages: per window None (no message) or a dict with frame_stamp, matches [(id, x, y), ...] in the message's order (match_points:
        ascending ids), prev_relo_t (3) and prev_relo_q (x y z w)."""
        B = len(messages)
        a = {"has_msg": np.zeros(B, np.int32), "frame_stamp": np.zeros(B), "n_match": np.zeros(B, np.int32),
             "match_id": np.zeros((B, max_match), np.int32), "match_xy": np.zeros((B, max_match, 2)), "prev_relo_t": np.zeros((B, 3)),
             "prev_relo_q": np.tile([0.0, 0.0, 0.0, 1.0], (B, 1))}
        for b, m in enumerate(messages):
            if m is None:
                continue
            n = len(m["matches"])
            assert n <= max_match
            a["has_msg"][b], a["frame_stamp"][b], a["n_match"][b] = 1, m["frame_stamp"], n
            for k, (fid, x, y) in enumerate(m["matches"]):
                a["match_id"][b, k], a["match_xy"][b, k] = fid, (x, y)
            a["prev_relo_t"][b], a["prev_relo_q"][b] = m["prev_relo_t"], m["prev_relo_q"]
        return ReloMsgArrays({"n_windows": B, "max_match": max_match}, a)


class ReloState(_Arrays):
    """avm_relo_state: the Estimator members of the relocalization that outlive a call, one row per stream.  alloc() gives the state of
    freshly constructed estimators: no relocalization pending, relo_pose rows (0, 0, 0, 0, 0, 0, 1)."""

    STRUCT, PER_STREAM = abi.ReloState, "n_match"

    @staticmethod
    def alloc(n_windows: int, max_match: int, device=None) -> "ReloState":
        B, unit = n_windows, [0.0, 0.0, 0.0, 1.0]
        a = {"relocalization_info": np.zeros(B, np.int32), "relo_frame": np.zeros(B, np.int32), "relo_stamp": np.zeros(B),
             "n_match": np.zeros(B, np.int32), "match_id": np.zeros((B, max_match), np.int32), "match_xy": np.zeros((B, max_match, 2)),
             "prev_relo_t": np.zeros((B, 3)), "prev_relo_q": np.tile(unit, (B, 1)), "relo_pose": np.tile([0.0, 0.0, 0.0] + unit, (B, 1)),
             "drift_correct_yaw": np.zeros(B), "drift_correct_t": np.zeros((B, 3)), "relo_relative_t": np.zeros((B, 3)),
             "relo_relative_q": np.tile(unit, (B, 1)), "relo_relative_yaw": np.zeros(B)}
        s = ReloState({"max_match": max_match}, a)
        return s.to_device(device) if device else s


PRIOR_KEYS = ("n", "nblk", "blk_kind", "blk_frame", "J", "r", "x0")   # avm_prior_out's arrays; the batch's are prior_<key>


class TrackTables:
    """The tables of a batch of streams whose feature manager lives in the library (include/avm.h, "the feature manager on
    device-resident tables"): `full` holds the whole f_manager.feature list of every window (strides up to MAX_FEAT_WIDE /
    MAX_OBS_WIDE), `feat_id` [B, max_feat] its ids, `view` is what triangulate() and optimization() take - a WindowArrays of the solve's
    strides whose track arrays (TRACK_KEYS) are its own and whose every other array IS the array of `full` (the same object: poses, IMU,
    prior) - and `view_row` [B, view max_feat] the row of `full` behind every row of the view.  Estimator.solve_view() fills the view,
    Estimator.setDepth() carries its depths back."""

    def __init__(self, full: WindowArrays, feat_id, max_feat: int = abi.MAX_FEAT, max_obs: int = abi.MAX_OBS, view_tracks: dict = None, view_row=None):
        self.full, self.feat_id = full, feat_id
        B = full.n_windows
        dims = dict(full.dims)
        dims["max_feat"], dims["max_obs"] = max_feat, max_obs
        shapes = {"n_feat": (B,), "feat_start": (B, max_feat), "feat_nobs": (B, max_feat), "feat_obs_begin": (B, max_feat),
                  "obs_xy": (B, max_obs, 2), "inv_depth": (B, max_feat), "obs_vel_td": (B, max_obs, 4)}
        a = {k: v for k, v in full.a.items() if k not in TRACK_KEYS and not k.startswith("relo_")}
        for k in TRACK_KEYS:
            if k in full.a:
                a[k] = view_tracks[k] if view_tracks else zeros_like_space(full, shapes[k], np.int32 if k in WindowArrays.I32 else np.float64)
        self.view = WindowArrays(dims, a)
        self.view_row = view_row if view_row is not None else zeros_like_space(full, (B, max_feat), np.int32)

    @property
    def on_device(self) -> bool:
        return self.full.on_device

    def swap_prior(self, prior: "PriorOutArrays"):
        """The prior hand-over behind Estimator.keep_prior(): the seven arrays of `prior` and the batch's prior_* change places, in `full` and
        in `view` (they share them).  `prior` then holds the slots the next solve may write.  Raises on unequal strides."""
        d = self.full.dims
        if (prior.dims["max_prior"], prior.dims["max_pblk"]) != (d["max_prior"], d["max_pblk"]):
            raise ValueError("swap_prior: the prior slots' strides %r differ from the batch's %r" %
                             ((prior.dims["max_prior"], prior.dims["max_pblk"]), (d["max_prior"], d["max_pblk"])))
        for k in PRIOR_KEYS:
            mine = self.full.a["prior_" + k]
            self.full.a["prior_" + k] = self.view.a["prior_" + k] = prior.a[k]
            prior.a[k] = mine

    def _rebuilt(self, conv, full):
        d = self.view.dims
        tracks = {k: conv(self.view.a[k]) for k in TRACK_KEYS if k in self.view.a}
        return TrackTables(full, conv(self.feat_id), d["max_feat"], d["max_obs"], tracks, conv(self.view_row))

    def copy(self) -> "TrackTables":
        return self._rebuilt((lambda v: v.clone()) if self.on_device else (lambda v: v.copy()), self.full.copy())

    def to_device(self, device="cuda:0") -> "TrackTables":
        full = self.full.to_device(device)
        return self._rebuilt(lambda v: like(full, v, None), full)

    def to_host(self) -> "TrackTables":
        return self._rebuilt(lambda v: v.copy() if isinstance(v, np.ndarray) else v.cpu().numpy(), self.full.to_host())


class PriorOutArrays(_Arrays):
    STRUCT = abi.PriorOut

    @staticmethod
    def alloc(n_windows: int, max_prior: int = 96, max_pblk: int = 16, device=None) -> "PriorOutArrays":
        shapes = {
            "n": ((n_windows,), "i4"),
            "nblk": ((n_windows,), "i4"),
            "blk_kind": ((n_windows, max_pblk), "i4"),
            "blk_frame": ((n_windows, max_pblk), "i4"),
            "J": ((n_windows, max_prior, max_prior), "f8"),
            "r": ((n_windows, max_prior), "f8"),
            "x0": ((n_windows, max_pblk, 9), "f8"),
        }
        if device:
            import torch  # zero-filled in HBM directly (J alone is 74 KB per window: never staged through the host)

            a = {k: torch.zeros(sh, dtype=torch.int32 if dt == "i4" else torch.float64, device=device) for k, (sh, dt) in shapes.items()}
        else:
            a = {k: np.zeros(sh, np.int32 if dt == "i4" else np.float64) for k, (sh, dt) in shapes.items()}
        return PriorOutArrays({"max_prior": max_prior, "max_pblk": max_pblk}, a)


class FselArrays(_Arrays):
    """avm_fsel_batch: the inputs of FeatureSelector::select() for P frames."""

    STRUCT = abi.FselBatch

    def __init__(self, dims, arrays, scalars=None):
        super().__init__(dims, arrays)
        self.scalars = dict(scalars or {})

    def copy(self):
        c = super().copy()
        c.scalars = dict(self.scalars)
        return c

    def to_device(self, device="cuda:0"):
        c = super().to_device(device)
        c.scalars = dict(self.scalars)
        return c

    def struct(self) -> abi.FselBatch:
        s = super().struct()
        for k, v in self.scalars.items():
            if k in ("q_ic", "t_ic"):
                arr = getattr(s, k)
                for i, x in enumerate(v):
                    arr[i] = float(x)
            else:
                setattr(s, k, v)
        return s

    @property
    def n_problems(self) -> int:
        return self.dims["n_problems"]


class FselOutArrays(_Arrays):
    STRUCT = abi.FselOut

    @staticmethod
    def alloc(n_problems: int, max_features: int, device=None, want_min_gap: bool = False) -> "FselOutArrays":
        a = {
            "n_selected": np.zeros(n_problems, np.int32),
            "selected_ids": np.full((n_problems, max_features), -1, np.int32),
            "fvalues": np.zeros((n_problems, max_features)),
        }
        if want_min_gap:  # avm_fsel_out::min_gap (nullable: an absent key is a NULL pointer)
            a["min_gap"] = np.zeros((n_problems, max_features))
        o = FselOutArrays({}, a)
        return o.to_device(device) if device else o


class AlignArrays(_Arrays):
    """avm_align_batch: all_image_frame (SfM poses and raw IMU) of B windows, the inputs of Estimator::visualInitialAlign()."""

    STRUCT = abi.AlignBatch


class AlignOutArrays(_Arrays):
    STRUCT = abi.AlignOut

    @staticmethod
    def alloc(n_windows: int, max_frames: int, device=None, want_deltas: bool = True) -> "AlignOutArrays":
        a = {"ok": np.zeros(n_windows, np.int32), "delta_bg": np.zeros((n_windows, 3)), "g_c0": np.zeros((n_windows, 3)),
             "x": np.zeros((n_windows, 3 * max_frames + 1)), "g_world": np.zeros((n_windows, 3))}
        if want_deltas:
            a["deltas"] = np.zeros((n_windows, max_frames - 1, 10))
        o = AlignOutArrays({}, a)
        return o.to_device(device) if device else o


class SfmArrays(_Arrays):
    """What Estimator::initialStructure hands GlobalSFM::construct and its PnP loop, one row per stream (synth.make_sfm; the reference
    statement tests/golden/gen_global_sfm.py reads these tables): relativePose's result - l [B], relative_R [B, 9] row-major,
    relative_T [B, 3] -, all_image_frame - n_frames [B], key_index [B, 11] - and the image of every frame - frame_n_pts [B, max_frames],
    frame_pt_id [B, max_frames, max_pts] strictly ascending, frame_pt_xy [..., 2].  dims: n_windows, max_frames, max_pts and the BA's
    ba_max_num_iterations / ba_max_solver_time_s.  A table container only (copy / to_device / to_host / slice): the C ABI has no entry
    point that takes it yet, so there is no struct()."""

    F64 = ["relative_R", "relative_T", "frame_pt_xy"]
    I32 = ["l", "n_frames", "key_index", "frame_n_pts", "frame_pt_id"]


def summary_alloc(n_windows: int, device=None):
    """[B] avm_solve_summary records (numpy structured array, or a raw byte tensor on device)."""
    if device is None:
        return np.zeros(n_windows, abi.SUMMARY_DTYPE)
    import torch

    return torch.zeros(n_windows * abi.SUMMARY_DTYPE.itemsize, dtype=torch.uint8, device=device)


def summary_ptr(s):
    if isinstance(s, np.ndarray):
        return s.ctypes.data_as(C.POINTER(abi.SolveSummary))
    return C.cast(s.data_ptr(), C.POINTER(abi.SolveSummary))


def summary_to_numpy(s):
    if isinstance(s, np.ndarray):
        return s
    return np.frombuffer(s.cpu().numpy().tobytes(), dtype=abi.SUMMARY_DTYPE).copy()
