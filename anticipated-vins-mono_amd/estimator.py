"""Host-side mirror of the reference's Estimator::optimization() call surface
(vins_estimator/src/estimator.h:47, estimator.cpp:661-994) over the C ABI.

The reference method takes no arguments and works on member arrays (para_Pose,
para_SpeedBias, para_Ex_Pose, para_Feature, pre_integrations, f_manager.feature,
last_marginalization_info).  Here those members live in a WindowArrays batch (host numpy or
HBM-resident torch tensors); optimization() solves all B windows in place and hands back the
new prior, exactly like the reference leaves last_marginalization_info behind.
"""
import ctypes as C

import numpy as np

from . import abi, buffers, init_buffers
from .lib import Context


class Estimator:
    def __init__(self, ctx: Context = None, options: abi.Options = None, device: int = 0):
        self.ctx = ctx or Context(device)
        self.options = options or abi.default_options()
        self.last_summary = None
        self.last_marginalization_info = None  # PriorOutArrays after a MARGIN_OLD / SECOND_NEW solve

    # the reference's name
    def optimization(self, windows: buffers.WindowArrays, want_summary: bool = True, prior_out: buffers.PriorOutArrays = None,
                     summary_out=None, marginalization_flags=None, relo_active=None):
        """Solve all windows in place.  `prior_out` lets a caller that solves batch after batch hand the same
        output slots back in (the reference allocates a new MarginalizationInfo per call; the slots are plain data);
        `summary_out` (buffers.summary_alloc) likewise for the per-window summaries: every record is rewritten by a call.
        `marginalization_flags`: [B] int32 where the windows live (numpy / device tensor), one MARGIN_OLD / MARGIN_SECOND_NEW /
        MARGIN_NONE per window instead of options.marginalization_flag (keyframe_decision() gives them); every window that reports
        n < 0 - MARGIN_NONE, or MARGIN_SECOND_NEW with nothing to drop - then keeps the prior it was solved with.
        `relo_active`: [B] int32 where the windows live, != 0 for the windows with a relocalization pending
        (avm_window_solve_batch_relo: the others are solved as if the batch had no relocalization arrays and their relo_pose rows stay
        as they are); True: the table resolve_relo(split=True) remembered on the windows.  None: the calls as they always were."""
        B = windows.n_windows
        s = windows.struct()
        dev = self.ctx.device_str if windows.on_device else None
        summ = (summary_out if summary_out is not None else buffers.summary_alloc(B, dev)) if want_summary else None
        prior = None
        if marginalization_flags is not None or self.options.marginalization_flag != abi.MARGIN_NONE:
            prior = prior_out or buffers.PriorOutArrays.alloc(B, windows.dims["max_prior"], windows.dims["max_pblk"], dev)
        po = prior.struct() if prior is not None else None
        head = (C.byref(self.options), windows.mem, C.byref(s))
        tail = (C.byref(po) if po is not None else None, buffers.summary_ptr(summ) if summ is not None else None)
        flags = None if marginalization_flags is None else self._flags(windows, marginalization_flags)
        if relo_active is not None:
            active = self._flags(windows, windows._relo_active if relo_active is True else relo_active)
            self.ctx.call("avm_window_solve_batch_relo", *head, abi.iptr(flags), abi.iptr(active), *tail)
        elif flags is None:
            self.ctx.call("avm_window_solve_batch", *head, *tail)
        else:
            self.ctx.call("avm_window_solve_batch_flags", *head, abi.iptr(flags), *tail)
        self.last_summary = summ
        if prior is not None and (marginalization_flags is not None or self.options.marginalization_flag == abi.MARGIN_SECOND_NEW):
            if windows.on_device and prior.on_device:
                self.keep_prior(windows, prior)      # (one kernel: no table crosses to the host)
            else:
                self._keep_old_prior_where_nothing_was_dropped(prior, windows)
        self.last_marginalization_info = prior
        return summ

    @staticmethod
    def _flags(windows, flags):
        """[B] int32 flags in the memory space of `windows`: a host array for host windows, a device tensor for device ones."""
        return buffers.like(windows, flags, np.int32, (windows.n_windows,))

    @staticmethod
    def _decision_out(windows):
        """the outputs of the keyframe decision where the windows live: marginalization_flags [B], last_track_num [B], parallax [B, 2]"""
        B = windows.n_windows
        return tuple(buffers.zeros_like_space(windows, sh, dt) for sh, dt in (((B,), np.int32), ((B,), np.int32), ((B, 2), np.float64)))

    def keyframe_decision(self, windows: buffers.WindowArrays, min_parallax: float):
        """FeatureManager::addFeatureCheckParallax's verdict (feature_manager.cpp:74-96) for every window, on tables that already hold
        the new image's observations: returns (marginalization_flags [B] int32, last_track_num [B] int32, parallax [B, 2] = sum, num),
        arrays where the windows live.  MARGIN_OLD = keyframe.  min_parallax: MIN_PARALLAX (configured pixels / FOCAL_LENGTH)."""
        flags, ltn, par = self._decision_out(windows)
        s = windows.struct()
        self.ctx.call("avm_keyframe_decision_batch", windows.mem, C.byref(s), float(min_parallax), abi.iptr(flags), abi.iptr(ltn), abi.dptr(par))
        return flags, ltn, par

    def failureDetection(self, windows: buffers.WindowArrays, last_P):
        """Estimator::failureDetection (estimator.cpp:612-658) for every window: [B] int32, 0 or the number of the first rule that fired
        (1: |Ba[10]| > 2.5, 2: |Bg[10]| > 1, 3: |P[10] - last_P| > 5, 4: |dP.z| > 1).  last_P: [B, 3] where the windows live."""
        B = windows.n_windows
        lp = buffers.like(windows, last_P, np.float64, (B, 3))
        failed = buffers.zeros_like_space(windows, (B,), np.int32)
        s = windows.struct()
        self.ctx.call("avm_failure_detection_batch", windows.mem, C.byref(s), abi.dptr(lp), abi.iptr(failed))
        return failed

    @staticmethod
    def _keep_old_prior_where_nothing_was_dropped(prior, windows):
        """MARGIN_SECOND_NEW leaves last_marginalization_info untouched when pose[WINDOW_SIZE - 1] is not in the old prior
        (or there is none): estimator.cpp:926-927.  The library reports that as n == -1; those windows keep the prior
        they were solved with (the batch's prior_* tables), so that the returned slots can always be chained."""
        n = prior.a["n"]
        keep = (n < 0)
        if not bool(keep.any()):
            return
        pa, wa = prior.a, windows.a
        mp = min(prior.dims["max_prior"], windows.dims["max_prior"])
        mb = min(prior.dims["max_pblk"], windows.dims["max_pblk"])
        idx = keep.nonzero()[0] if isinstance(n, np.ndarray) else keep.nonzero().flatten()
        for i in idx.tolist():
            pa["n"][i] = wa["prior_n"][i]
            pa["nblk"][i] = wa["prior_nblk"][i]
            pa["blk_kind"][i, :mb] = wa["prior_blk_kind"][i, :mb]
            pa["blk_frame"][i, :mb] = wa["prior_blk_frame"][i, :mb]
            pa["J"][i, :mp, :mp] = wa["prior_J"][i, :mp, :mp]
            pa["r"][i, :mp] = wa["prior_r"][i, :mp]
            pa["x0"][i, :mb] = wa["prior_x0"][i, :mb]

    def keep_prior(self, windows: buffers.WindowArrays, prior: buffers.PriorOutArrays):
        """estimator.cpp:926-927 on the slots: every window that reported n < 0 gets the used part of the prior it was solved with (the
        batch's prior_* tables), in place.  Afterwards `prior` can always be chained: TrackTables.swap_prior(prior) is the hand-over."""
        assert prior.on_device == windows.on_device
        s, po = windows.struct(), prior.struct()
        self.ctx.call("avm_prior_keep_batch", windows.mem, C.byref(s), C.byref(po))

    def headers_step(self, windows: buffers.WindowArrays, stamp, marginalization_flags=None, new_stamp=None):
        """The frame stamps Headers[i].stamp of B streams, stamp [B, 11] where the windows live, in place: slideWindow's moves for the
        flags (estimator.cpp:1015,1021,1064) - call it behind the roll -, then Headers[10] = new_stamp (:126) - on the next image."""
        B = windows.n_windows
        assert tuple(stamp.shape) == (B, abi.NFRAMES)
        flags = None if marginalization_flags is None else self._flags(windows, marginalization_flags)
        new = None if new_stamp is None else buffers.like(windows, new_stamp, np.float64, (B,))
        self.ctx.call("avm_headers_step_batch", windows.mem, B, abi.dptr(stamp), abi.iptr(flags), abi.dptr(new))

    # the reference's name
    def setReloFrame(self, windows: buffers.WindowArrays, stamp, msg: buffers.ReloMsgArrays, state: buffers.ReloState):
        """Estimator::setReloFrame (estimator.cpp:1109-1127) for every stream with a message: the message goes into `state`; a frame
        0 .. WINDOW_SIZE - 1 whose stamp equals frame_stamp (the last one) makes the relocalization pending, relo_pose = its pose."""
        assert msg.on_device == windows.on_device == state.on_device and tuple(stamp.shape) == (windows.n_windows, abi.NFRAMES)
        s, sm, ss = windows.struct(), msg.struct(), state.struct()
        self.ctx.call("avm_set_relo_frame_batch", windows.mem, C.byref(s), abi.dptr(stamp), C.byref(sm), C.byref(ss))

    def resolve_relo(self, tables: buffers.TrackTables, state: buffers.ReloState, split: bool = False) -> int:
        """The match loop of optimization() (estimator.cpp:765-790) on tables.view (behind solve_view()): with a relocalization pending
        in some window, tables.view gets relo_n / relo_frame / relo_feat / relo_xy and relo_pose (state's own array: the solve returns the
        loop frame's pose into it), and optimization() takes the extended kernel; with none they are removed.  Returns the number of
        windows with a relocalization pending.
        split=True: the arrays are attached whether or not a window is active, and tables.view remembers state's relocalization_info
        as the table optimization(relo_active=True) passes: only the windows it marks take the extended kernel."""
        v = tables.view
        B, mf = v.n_windows, v.dims["max_feat"]
        out = getattr(tables, "_relo_out", None)
        if out is None:
            shapes = {"relo_n": ((B,), np.int32), "relo_frame": ((B,), np.int32), "relo_feat": ((B, mf), np.int32), "relo_xy": ((B, mf, 2), np.float64)}
            out = tables._relo_out = {k: buffers.zeros_like_space(v, sh, dt) for k, (sh, dt) in shapes.items()}
        n_active = C.c_int32(0)
        s, ss = v.struct(), state.struct()
        self.ctx.call("avm_relo_resolve_batch", v.mem, C.byref(s), abi.iptr(tables.feat_id), int(tables.full.dims["max_feat"]),
                      abi.iptr(tables.view_row), C.byref(ss), abi.iptr(out["relo_n"]), abi.iptr(out["relo_frame"]), abi.iptr(out["relo_feat"]),
                      abi.dptr(out["relo_xy"]), C.byref(n_active))
        for k in ("relo_n", "relo_frame", "relo_feat", "relo_xy", "relo_pose"):
            v.a.pop(k, None)
        v._relo_active = state.a["relocalization_info"] if split else None
        if split or n_active.value > 0:
            v.a.update(out)
            v.a["relo_pose"] = state.a["relo_pose"]
        return int(n_active.value)

    def relo_finish(self, windows: buffers.WindowArrays, state: buffers.ReloState):
        """The outputs of double2vector() (estimator.cpp:588-604) behind optimization(): drift_correct_yaw / _t and relo_relative_t / _q /
        _yaw of every window with a relocalization pending, whose relocalization_info then returns to 0."""
        s, ss = windows.struct(), state.struct()
        self.ctx.call("avm_relo_finish_batch", windows.mem, C.byref(s), C.byref(ss))

    # the reference's name
    def visualInitialAlign(self, align: buffers.AlignArrays, windows: buffers.WindowArrays = None, out: buffers.AlignOutArrays = None):
        """Estimator::visualInitialAlign (estimator.cpp:355-431) for B windows.  windows=None: VisualIMUAlignment only
        (initial_aligment.cpp:199-207).  With windows: pose, velocities, gyro biases and inverse depths are set in place; a window
        whose `ok` is 0 keeps them, except for the bias increment.  Returns the AlignOutArrays (ok, delta_bg, g_c0, x, g_world,
        deltas).  Before the first optimization() call reset_linearization_biases(windows)."""
        out = out or buffers.AlignOutArrays.alloc(align.n_windows, align.dims["max_frames"], self.ctx.device_str if align.on_device else None)
        sa, so = align.struct(), out.struct()
        sw = windows.struct() if windows is not None else None
        self.ctx.call("avm_visual_initial_align_batch", C.byref(self.options), align.mem, C.byref(sa), C.byref(sw) if sw is not None else None,
                      C.byref(so))
        return out

    def globalSFM(self, sfm: buffers.SfmArrays, full: buffers.WindowArrays, feat_id, out: init_buffers.SfmOutArrays = None,
                  align: buffers.AlignArrays = None):
        """The deterministic half of Estimator::initialStructure (estimator.cpp:247-344) for B streams: GlobalSFM::construct and the PnP
        of every frame (avm_global_sfm_batch, include/avm_init.h).  sfm: relativePose's result and the frames' images (synth.make_sfm);
        full: the whole f_manager.feature list (its track tables and ex_pose are read, nothing is written); feat_id [B, max_feat] where
        the tables live.  With `align`, frame_R / frame_T of the result ARE align's own arrays (its max_frames must be sfm's): the
        alignment reads what the SfM wrote, with no copy.  Returns the SfmOutArrays; a stream writes only the rows its ok allows."""
        sfm = init_buffers.SfmBatchArrays.of(sfm)
        MF, MFE = sfm.dims["max_frames"], full.dims["max_feat"]
        out = out or init_buffers.SfmOutArrays.alloc(sfm.n_windows, MF, MFE, self.ctx.device_str if sfm.on_device else None)
        if align is not None:
            assert align.dims["max_frames"] == MF and align.on_device == sfm.on_device
            out.a["frame_R"], out.a["frame_T"] = align.a["frame_R"], align.a["frame_T"]
        ss, sw, so = sfm.struct(), full.struct(), out.struct()
        self.ctx.call("avm_global_sfm_batch", sfm.mem, C.byref(ss), C.byref(sw), abi.iptr(buffers.like(sfm, feat_id, np.int32, (sfm.n_windows, MFE))),
                      C.byref(so))
        return out

    def initialStructure(self, sfm: buffers.SfmArrays, full: buffers.WindowArrays, feat_id, align: buffers.AlignArrays,
                         windows: buffers.WindowArrays = None):
        """Estimator::initialStructure after relativePose: globalSFM() into align's frame_R / frame_T, then visualInitialAlign(align,
        windows); on the device the two calls chain with no host trip.  Returns (SfmOutArrays, AlignOutArrays).
        A stream whose SfM failed (ok != 0) wrote no frame pose; this method then sets that stream's frame_R / frame_T rows of `align`
        to NaN, which the alignment answers with ITS ok = 0 (non-finite input ends that window alone, include/avm.h) and leaves the
        window's state alone.  The caller prefills nothing; it loses what those rows held."""
        so = self.globalSFM(sfm, full, feat_id, align=align)
        bad = so.a["ok"] != 0
        align.a["frame_R"][bad] = np.nan
        align.a["frame_T"][bad] = np.nan
        return so, self.visualInitialAlign(align, windows)

    @staticmethod
    def reset_linearization_biases(windows: buffers.WindowArrays):
        """pre_integrations[i]->repropagate(0, Bgs[i]) of visualInitialAlign (estimator.cpp:391-394): the solve pre-integrates from
        imu_lin_ba / imu_lin_bg, so they become 0 and the (new) gyro biases of the frames."""
        windows.a["imu_lin_ba"][:] = 0.0
        windows.a["imu_lin_bg"][:] = windows.a["speedbias"][:, : abi.WINDOW_SIZE, 6:9]

    def triangulate(self, windows: buffers.WindowArrays, init_depth: float = 5.0):
        """FeatureManager::triangulate (feature_manager.cpp:202-257), the step before optimization() in solveOdometry():
        features whose inverse depth is <= 0 get 1 / depth from the multi-view linear triangulation, in place."""
        s = windows.struct()
        self.ctx.call("avm_triangulate_batch", windows.mem, C.byref(s), float(init_depth))

    def projection_td_eval(self, arrays: dict, tr: float, row: float, focal_length: float = 460.0):
        """ProjectionTdFactor::Evaluate (projection_td_factor.cpp:34-141) for n factors given as host arrays
        (abi.td_factor_batch): returns residual [n, 2] and Jacobian [n, 2, 20] (pose_i 6 | pose_j 6 | ex 6 | lambda | td)."""
        f = abi.td_factor_batch(arrays, tr, row, focal_length)
        r, J = np.zeros((f.n, 2)), np.zeros((f.n, 2, 20))
        self.ctx.call("avm_projection_td_eval", abi.AVM_MEM_HOST, C.byref(f), abi.dptr(r), abi.dptr(J))
        return r, J

    def imu_propagate(self, windows: buffers.WindowArrays):
        """Estimator::processIMU's dead-reckoning of the newest frame (estimator.cpp:100-107), in place."""
        s = windows.struct()
        g = (C.c_double * 3)(*[float(x) for x in self.options.g])
        self.ctx.call("avm_imu_propagate_batch", windows.mem, C.byref(s), g)

    def push_imu(self, windows: buffers.WindowArrays, n, dt, acc, gyr):
        """The buffer half of Estimator::processIMU (estimator.cpp:92-98) for the samples between two images: n [B] samples per window,
        dt [B, max_in], acc / gyr [B, max_in, 3], appended to interval WINDOW_SIZE - 1 in place.  imu_propagate() is the other half."""
        dt = buffers.like(windows, dt, np.float64)
        B, max_in = windows.n_windows, int(dt.shape[1])
        assert tuple(dt.shape) == (B, max_in)
        n = buffers.like(windows, n, np.int32, (B,))
        acc, gyr = buffers.like(windows, acc, np.float64, (B, max_in, 3)), buffers.like(windows, gyr, np.float64, (B, max_in, 3))
        s = windows.struct()
        self.ctx.call("avm_imu_push_batch", windows.mem, C.byref(s), abi.iptr(n), max_in, abi.dptr(dt), abi.dptr(acc), abi.dptr(gyr))

    # the reference's name
    def addFeatureCheckParallax(self, full: buffers.WindowArrays, feat_id, image: buffers.ImageArrays, min_parallax: float):
        """FeatureManager::addFeatureCheckParallax (feature_manager.cpp:45-96) on the full tables, in place: every image point is appended
        to the track of its id in feat_id [B, max_feat] or starts a new row, the observation table is rewritten dense in list order.
        Returns keyframe_decision()'s (marginalization_flags, last_track_num, parallax) on the result."""
        B = full.n_windows
        assert image.on_device == full.on_device and tuple(feat_id.shape) == (B, full.dims["max_feat"])   # (n_windows: the library refuses it)
        flags, ltn, par = self._decision_out(full)
        s, si = full.struct(), image.struct()
        self.ctx.call("avm_add_image_batch", full.mem, C.byref(s), abi.iptr(feat_id), C.byref(si), float(min_parallax), abi.iptr(flags),
                      abi.iptr(ltn), abi.dptr(par))
        return flags, ltn, par

    def solve_view(self, tables: buffers.TrackTables) -> buffers.WindowArrays:
        """The rows of tables.full that pass used_num >= 2 && start_frame < WINDOW_SIZE - 2 (estimator.cpp:715), gathered into
        tables.view (and tables.view_row): what triangulate() and optimization() take.  Returns tables.view."""
        sf, sv = tables.full.struct(), tables.view.struct()
        self.ctx.call("avm_solve_view_batch", tables.full.mem, C.byref(sf), C.byref(sv), abi.iptr(tables.view_row))
        return tables.view

    # the reference's name
    def setDepth(self, tables: buffers.TrackTables):
        """FeatureManager::setDepth's copy (feature_manager.cpp:141-159): the inverse depths of tables.view back into the rows of
        tables.full they came from."""
        sf, sv = tables.full.struct(), tables.view.struct()
        self.ctx.call("avm_solve_view_store_depths", tables.full.mem, C.byref(sf), C.byref(sv), abi.iptr(tables.view_row))

    def slideWindow(self, windows: buffers.WindowArrays, marginalization_flag=None, shift_depth=True, init_depth=5.0, remove_failures=False,
                    feat_id=None):
        """Estimator::slideWindow (estimator.cpp:996-1107) + removeBackShiftDepth / removeBack / removeFront
        (feature_manager.cpp:275-352), in place on the batch tables (host or device resident).  marginalization_flag: one int for the
        batch, or an array / tensor of B flags, one per window.  remove_failures: f_manager.removeFailures() behind the roll
        (estimator.cpp:197-198): the features the solve left with a negative inverse depth are erased.  feat_id [B, max_feat] (where
        the windows live): the ids of the rows, compacted with them; the rows of obs_vel_td then move with their observations."""
        flag = self.options.marginalization_flag if marginalization_flag is None else marginalization_flag
        s = windows.struct()
        if feat_id is None and np.ndim(flag) == 0 and not remove_failures:
            self.ctx.call("avm_slide_window", windows.mem, C.byref(s), int(flag), int(bool(shift_depth)), float(init_depth))
            return
        flags = self._flags(windows, np.full(windows.n_windows, int(flag), np.int32) if np.ndim(flag) == 0 else flag)
        tail = (abi.iptr(flags), int(bool(shift_depth)), float(init_depth), int(bool(remove_failures)))
        if feat_id is not None:
            assert tuple(feat_id.shape) == (windows.n_windows, windows.dims["max_feat"])
            self.ctx.call("avm_slide_window_tracks", windows.mem, C.byref(s), abi.iptr(feat_id), *tail)
        else:
            self.ctx.call("avm_slide_window_flags", windows.mem, C.byref(s), *tail)

    def preintegrate(self, windows: buffers.WindowArrays):
        """IntegrationBase for every interval: returns delta [B,10,10], jacobian, covariance [B,10,15,15], sum_dt [B,10]."""
        assert not windows.on_device
        B = windows.n_windows
        d, j, cv, sd = np.zeros((B, 10, 10)), np.zeros((B, 10, 15, 15)), np.zeros((B, 10, 15, 15)), np.zeros((B, 10))
        s = windows.struct()
        self.ctx.call("avm_imu_preintegrate_batch", C.byref(self.options), windows.mem, C.byref(s), abi.dptr(d), abi.dptr(j), abi.dptr(cv), abi.dptr(sd))
        return d, j, cv, sd

    def sqrt_info(self, n_windows: int):
        out = np.zeros((n_windows, 10, 15, 15))
        self.ctx.call("avm_debug_copy_sqrt_info", n_windows, abi.dptr(out))
        return out

    def eval_factors(self, windows: buffers.WindowArrays, apply_loss: bool = False):
        assert not windows.on_device
        B, mo, mp = windows.n_windows, windows.dims["max_obs"], windows.dims["max_prior"]
        out = dict(proj_r=np.zeros((B, mo, 2)), proj_J=np.zeros((B, mo, 2, 13)), imu_r=np.zeros((B, 10, 15)),
                   imu_J=np.zeros((B, 10, 15, 30)), prior_res=np.zeros((B, mp)), cost=np.zeros(B))
        s = windows.struct()
        self.ctx.call("avm_window_eval_factors", C.byref(self.options), windows.mem, C.byref(s), int(apply_loss),
                      *[abi.dptr(out[k]) for k in ("proj_r", "proj_J", "imu_r", "imu_J", "prior_res", "cost")])
        return out
