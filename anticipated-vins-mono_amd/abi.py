"""ctypes mirror of include/avm.h (POD structs only).

Field order and types must match the header exactly; tests/test_abi.py checks
sizeof() of every struct against the values the C library reports.
"""
import ctypes as C

import numpy as np

WINDOW_SIZE = 10
NFRAMES = WINDOW_SIZE + 1
MAX_ITER_TRACE = 16
# table limits of an avm_window_batch (include/avm.h): the solve's, and the per-feature entry points' around it
MAX_FEAT, MAX_FEAT_WIDE = 150, 384
MAX_OBS, MAX_OBS_WIDE = MAX_FEAT * NFRAMES, MAX_FEAT_WIDE * NFRAMES

AVM_MEM_HOST, AVM_MEM_DEVICE = 0, 1
# avm_status (include/avm.h)
AVM_OK, AVM_ERR_INVALID, AVM_ERR_UNSUPPORTED, AVM_ERR_NO_DEVICE, AVM_ERR_HIP, AVM_ERR_CAPACITY = 0, -1, -2, -3, -4, -5
BLK_POSE, BLK_SPEEDBIAS, BLK_EXPOSE, BLK_TD = 0, 1, 2, 3
MARGIN_OLD, MARGIN_SECOND_NEW, MARGIN_NONE = 0, 1, 2
TERM_NAMES = ["NO_CONVERGENCE", "GRADIENT_TOL", "PARAMETER_TOL", "FUNCTION_TOL", "MIN_RADIUS", "FAILURE"]

c_dp = C.POINTER(C.c_double)
c_ip = C.POINTER(C.c_int32)


class Options(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32),
        ("estimate_extrinsic", C.c_int32),
        ("estimate_td", C.c_int32),
        ("marginalization_flag", C.c_int32),
        ("focal_length", C.c_double),
        ("g", C.c_double * 3),
        ("acc_n", C.c_double),
        ("gyr_n", C.c_double),
        ("acc_w", C.c_double),
        ("gyr_w", C.c_double),
        ("cauchy_a", C.c_double),
        ("max_sum_dt", C.c_double),
        ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double),
        ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double),
        ("function_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
        ("max_num_consecutive_invalid_steps", C.c_int32),
        ("jacobi_scaling", C.c_int32),
        ("marg_eps", C.c_double),
        ("tr", C.c_double),
        ("row", C.c_double),
        ("max_solver_time_s", C.c_double),
        ("marg_noise_rel", C.c_double),
    ]


class WindowBatch(C.Structure):
    _fields_ = [
        ("n_windows", C.c_int32),
        ("max_feat", C.c_int32),
        ("max_obs", C.c_int32),
        ("max_samp", C.c_int32),
        ("max_prior", C.c_int32),
        ("max_pblk", C.c_int32),
        ("pose", c_dp),
        ("speedbias", c_dp),
        ("ex_pose", c_dp),
        ("inv_depth", c_dp),
        ("n_feat", c_ip),
        ("feat_start", c_ip),
        ("feat_nobs", c_ip),
        ("feat_obs_begin", c_ip),
        ("obs_xy", c_dp),
        ("imu_n", c_ip),
        ("imu_dt", c_dp),
        ("imu_acc", c_dp),
        ("imu_gyr", c_dp),
        ("imu_lin_ba", c_dp),
        ("imu_lin_bg", c_dp),
        ("prior_n", c_ip),
        ("prior_nblk", c_ip),
        ("prior_blk_kind", c_ip),
        ("prior_blk_frame", c_ip),
        ("prior_J", c_dp),
        ("prior_r", c_dp),
        ("prior_x0", c_dp),
        ("obs_vel_td", c_dp),
        ("td", c_dp),
        ("relo_n", c_ip),
        ("relo_frame", c_ip),
        ("relo_feat", c_ip),
        ("relo_xy", c_dp),
        ("relo_pose", c_dp),
        ("failure_occur", c_ip),
        ("last_pose0", c_dp),
    ]


class PriorOut(C.Structure):
    _fields_ = [
        ("max_prior", C.c_int32),
        ("max_pblk", C.c_int32),
        ("n", c_ip),
        ("nblk", c_ip),
        ("blk_kind", c_ip),
        ("blk_frame", c_ip),
        ("J", c_dp),
        ("r", c_dp),
        ("x0", c_dp),
    ]


class SolveSummary(C.Structure):
    _fields_ = [
        ("termination", C.c_int32),
        ("num_iterations", C.c_int32),
        ("num_successful", C.c_int32),
        ("accept_mask", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
        ("cost_trace", C.c_double * MAX_ITER_TRACE),
        ("radius_trace", C.c_double * MAX_ITER_TRACE),
    ]


SUMMARY_DTYPE = np.dtype(SolveSummary)


class TdFactorBatch(C.Structure):
    """avm_td_factor_batch (include/avm.h): inputs of ProjectionTdFactor, one entry per factor."""
    _fields_ = [("n", C.c_int32)] + [(k, c_dp) for k in ("pose_i", "pose_j", "ex_pose", "inv_depth", "td", "pts_i", "pts_j", "vel_i", "vel_j",
                                                        "td_i", "td_j", "row_i", "row_j")] + [("tr", C.c_double), ("row", C.c_double), ("focal_length", C.c_double)]


def td_factor_batch(arrays: dict, tr: float, row: float, focal_length: float = 460.0):
    """Build an avm_td_factor_batch from host numpy arrays (kept alive on the returned struct)."""
    keep = {k: np.ascontiguousarray(np.asarray(v, float)) for k, v in arrays.items()}
    s = TdFactorBatch()
    s.n = keep["inv_depth"].shape[0]
    for k, v in keep.items():
        setattr(s, k, dptr(v))
    s.tr, s.row, s.focal_length = float(tr), float(row), float(focal_length)
    s._keep = keep
    return s


class FselHorizonIn(C.Structure):
    """avm_fsel_horizon_in (include/avm.h): inputs of HorizonGenerator::imu."""
    _fields_ = [
        ("n_problems", C.c_int32),
        ("horizon", C.c_int32),
        ("k_pos", c_dp), ("k_quat", c_dp), ("k_ba", c_dp),
        ("k1_pos", c_dp), ("k1_vel", c_dp), ("k1_quat", c_dp),
        ("acc", c_dp), ("gyr", c_dp),
        ("nr_imu", c_ip), ("delta_imu", c_dp),
    ]


def horizon_in(horizon, k_pos, k_quat, k_ba, k1_pos, k1_vel, k1_quat, acc, gyr, nr_imu, delta_imu):
    """Build an avm_fsel_horizon_in from host arrays or from torch tensors, all eleven of one kind (a mix raises).  The converted
    arrays are kept alive on the returned struct as `_keep`; its `mem` is AVM_MEM_HOST for arrays, AVM_MEM_DEVICE for tensors."""
    given = dict(k_pos=k_pos, k_quat=k_quat, k_ba=k_ba, k1_pos=k1_pos, k1_vel=k1_vel, k1_quat=k1_quat, acc=acc, gyr=gyr, nr_imu=nr_imu,
                 delta_imu=delta_imu)
    tensors = [k for k, a in given.items() if hasattr(a, "data_ptr")]
    if tensors and len(tensors) != len(given):
        raise ValueError("horizon_in: host arrays and tensors mixed (tensors: %s)" % ", ".join(tensors))
    if tensors:
        import torch
    cols = dict(k_pos=3, k_quat=4, k_ba=3, k1_pos=3, k1_vel=3, k1_quat=4, acc=3, gyr=3)   # nr_imu and delta_imu are [P]
    keep = {}
    for k, a in given.items():
        shape = (-1, cols[k]) if k in cols else (-1,)
        if tensors:
            keep[k] = a.to(torch.int32 if k == "nr_imu" else torch.float64).reshape(shape).contiguous()
        else:
            keep[k] = np.ascontiguousarray(np.asarray(a, np.int32 if k == "nr_imu" else float).reshape(shape))
    s = FselHorizonIn()
    s.n_problems, s.horizon = keep["k_pos"].shape[0], int(horizon)
    for k, v in keep.items():
        setattr(s, k, iptr(v) if k == "nr_imu" else dptr(v))
    s._keep, s.mem = keep, AVM_MEM_DEVICE if tensors else AVM_MEM_HOST
    return s


class FselBatch(C.Structure):
    _fields_ = [
        ("n_problems", C.c_int32),
        ("horizon", C.c_int32),
        ("max_cand", C.c_int32),
        ("max_used", C.c_int32),
        ("max_cloud", C.c_int32),
        ("max_features", C.c_int32),
        ("hor_pos", c_dp),
        ("hor_quat", c_dp),
        ("nr_imu", c_ip),
        ("delta_imu", c_dp),
        ("acc_var", C.c_double),
        ("acc_bias_var", C.c_double),
        ("q_ic", C.c_double * 4),
        ("t_ic", C.c_double * 3),
        ("fx", C.c_double),
        ("fy", C.c_double),
        ("cx", C.c_double),
        ("cy", C.c_double),
        ("k1", C.c_double),
        ("k2", C.c_double),
        ("p1", C.c_double),
        ("p2", C.c_double),
        ("image_width", C.c_int32),
        ("image_height", C.c_int32),
        ("n_cand", c_ip),
        ("cand_id", c_ip),
        ("cand_xy", c_dp),
        ("cand_prob", c_dp),
        ("n_used", c_ip),
        ("used_id", c_ip),
        ("used_xy", c_dp),
        ("n_cloud", c_ip),
        ("cloud_xy", c_dp),
        ("cloud_depth", c_dp),
    ]


class FselOut(C.Structure):
    _fields_ = [("n_selected", c_ip), ("selected_ids", c_ip), ("fvalues", c_dp), ("min_gap", c_dp)]


MAX_ALIGN_FRAMES = 64  # AVM_MAX_ALIGN_FRAMES


class AlignBatch(C.Structure):
    """avm_align_batch (include/avm.h): the inputs of VisualIMUAlignment for B windows."""
    _fields_ = [("n_windows", C.c_int32), ("max_frames", C.c_int32), ("max_samp", C.c_int32),
                ("n_frames", c_ip), ("frame_R", c_dp), ("frame_T", c_dp), ("tic", c_dp),
                ("imu_n", c_ip), ("imu_dt", c_dp), ("imu_acc", c_dp), ("imu_gyr", c_dp), ("imu_lin_ba", c_dp), ("imu_lin_bg", c_dp),
                ("key_index", c_ip)]


class AlignOut(C.Structure):
    """avm_align_out (include/avm.h)."""
    _fields_ = [("ok", c_ip), ("delta_bg", c_dp), ("g_c0", c_dp), ("x", c_dp), ("g_world", c_dp), ("deltas", c_dp)]


AVM_ABI_VERSION = 6  # include/avm.h: avm_create() refuses a caller built against another header


class Config(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("max_windows", C.c_int32),
        ("max_problems", C.c_int32),
        ("abi_version", C.c_int32),
        ("reserved", C.c_int32 * 4),
    ]


MAX_IMAGE_PTS = 1024  # AVM_MAX_IMAGE_PTS


class ImageBatch(C.Structure):
    """avm_image_batch (include/avm.h): one image per window, the `image` map of processImage (camera 0)."""
    _fields_ = [("n_windows", C.c_int32), ("max_pts", C.c_int32), ("n_pts", c_ip), ("feature_id", c_ip), ("xy", c_dp), ("vel_td", c_dp)]


class SelectState(C.Structure):
    """avm_select_state (include/avm.h): the members of FeatureSelector that outlive a call, one row per stream."""
    _fields_ = [("max_tracked", C.c_int32), ("last_feature_id", c_ip), ("n_tracked", c_ip), ("tracked_id", c_ip), ("first_image", c_ip)]


class ReloMsgBatch(C.Structure):
    """avm_relo_msg_batch (include/avm.h): the loop-closure message of estimator_node.cpp:274-297, one row per stream."""
    _fields_ = [("n_windows", C.c_int32), ("max_match", C.c_int32), ("has_msg", c_ip), ("frame_stamp", c_dp), ("n_match", c_ip),
                ("match_id", c_ip), ("match_xy", c_dp), ("prev_relo_t", c_dp), ("prev_relo_q", c_dp)]


class ReloState(C.Structure):
    """avm_relo_state (include/avm.h): the Estimator members of the relocalization that outlive a call, one row per stream."""
    _fields_ = [("max_match", C.c_int32), ("relocalization_info", c_ip), ("relo_frame", c_ip), ("relo_stamp", c_dp), ("n_match", c_ip),
                ("match_id", c_ip), ("match_xy", c_dp), ("prev_relo_t", c_dp), ("prev_relo_q", c_dp), ("relo_pose", c_dp),
                ("drift_correct_yaw", c_dp), ("drift_correct_t", c_dp), ("relo_relative_t", c_dp), ("relo_relative_q", c_dp),
                ("relo_relative_yaw", c_dp)]


def pointer_members(struct):
    """(names of the double* members, names of the int32_t* members) of a struct type, in declaration order."""
    return [k for k, t in struct._fields_ if t is c_dp], [k for k, t in struct._fields_ if t is c_ip]


# Every function the package binds: name -> (restype, argtypes); lib.py applies the table in one loop.  The 51 declarations of
# include/avm.h under the header's own headings, then the avm_debug_* hooks (csrc/api/debug.hpp).  avm_ctx* is a void pointer,
# avm_mem an int; restype None is ctypes' void.
_vp, _int, _i32, _f64, _P = C.c_void_p, C.c_int, C.c_int32, C.c_double, C.POINTER
_opt, _win, _prior, _summ, _fsel, _img, _rs = _P(Options), _P(WindowBatch), _P(PriorOut), _P(SolveSummary), _P(FselBatch), _P(ImageBatch), _P(ReloState)
_ints, _i64s = _P(C.c_int), _P(C.c_int64)
PROTOTYPES = {
    # lifecycle
    "avm_default_options": (_int, [_opt]),
    "avm_create": (_int, [_P(Config), _P(_vp)]),
    "avm_destroy": (None, [_vp]),
    "avm_last_error": (C.c_char_p, [_vp]),
    "avm_version": (C.c_char_p, []),
    "avm_abi_version": (_int, []),
    # HP-A: Estimator::optimization() for a batch of independent windows, and the steps around it
    "avm_window_solve_batch": (_int, [_vp, _opt, _int, _win, _prior, _summ]),
    "avm_window_solve_batch_flags": (_int, [_vp, _opt, _int, _win, c_ip, _prior, _summ]),
    "avm_window_solve_batch_relo": (_int, [_vp, _opt, _int, _win, c_ip, c_ip, _prior, _summ]),
    "avm_window_solve": (_int, [_vp, _opt, _int, _win, _prior, _summ]),
    "avm_imu_preintegrate_batch": (_int, [_vp, _opt, _int, _win] + [c_dp] * 4),
    "avm_triangulate_batch": (_int, [_vp, _int, _win, _f64]),
    "avm_imu_propagate_batch": (_int, [_vp, _int, _win, c_dp]),
    "avm_fsel_horizon_imu": (_int, [_vp, _int, _P(FselHorizonIn), c_dp, c_dp]),
    "avm_projection_td_eval": (_int, [_vp, _int, _P(TdFactorBatch), c_dp, c_dp]),
    "avm_fsel_build_cloud": (_int, [_vp, _int, _win, c_dp, c_dp, _i32, c_ip, c_dp, c_dp]),
    "avm_slide_window": (_int, [_vp, _int, _win, _i32, _i32, _f64]),
    "avm_slide_window_flags": (_int, [_vp, _int, _win, c_ip, _i32, _f64, _i32]),
    "avm_keyframe_decision_batch": (_int, [_vp, _int, _win, _f64, c_ip, c_ip, c_dp]),
    "avm_failure_detection_batch": (_int, [_vp, _int, _win, c_dp, c_ip]),
    # the feature manager on device-resident tables
    "avm_add_image_batch": (_int, [_vp, _int, _win, c_ip, _img, _f64, c_ip, c_ip, c_dp]),
    "avm_imu_push_batch": (_int, [_vp, _int, _win, c_ip, _i32, c_dp, c_dp, c_dp]),
    "avm_solve_view_batch": (_int, [_vp, _int, _win, _win, c_ip]),
    "avm_solve_view_store_depths": (_int, [_vp, _int, _win, _win, c_ip]),
    "avm_slide_window_tracks": (_int, [_vp, _int, _win, c_ip, c_ip, _i32, _f64, _i32]),
    # the selector in the stream loop
    "avm_fsel_select_image_batch": (_int, [_vp, _int, _img, c_dp, c_ip, _i32, _i32, _P(SelectState), _fsel, _P(FselOut), _img]),
    # relocalization and the prior hand-over in the stream loop
    "avm_headers_step_batch": (_int, [_vp, _int, _i32, c_dp, c_ip, c_dp]),
    "avm_set_relo_frame_batch": (_int, [_vp, _int, _win, c_dp, _P(ReloMsgBatch), _rs]),
    "avm_relo_resolve_batch": (_int, [_vp, _int, _win, c_ip, _i32, c_ip, _rs, c_ip, c_ip, c_ip, c_dp, _P(_i32)]),
    "avm_relo_finish_batch": (_int, [_vp, _int, _win, _rs]),
    "avm_prior_keep_batch": (_int, [_vp, _int, _win, _prior]),
    # Estimator::visualInitialAlign
    "avm_visual_initial_align_batch": (_int, [_vp, _opt, _int, _P(AlignBatch), _win, _P(AlignOut)]),
    # host-side format adapters (no ctx), and the per-factor parity surface declared behind them
    "avm_gt_load_csv": (_vp, [C.c_char_p]),
    "avm_gt_from_rows": (_vp, [c_dp, _i32]),
    "avm_gt_free": (None, [_vp]),
    "avm_gt_size": (_int, [_vp]),
    "avm_gt_seek": (_int, [_vp]),
    "avm_fsel_horizon_ground_truth": (_int, [_vp, _i32, _f64, c_dp, c_dp, _f64, c_dp, c_dp]),
    "avm_image_from_pointcloud": (_int, [_i32, _P(C.c_float), _P(_P(C.c_float)), _i32, c_ip, c_ip, c_dp]),
    "avm_window_eval_factors": (_int, [_vp, _opt, _int, _win, _int] + [c_dp] * 6),
    # HP-B: FeatureSelector::select() for a batch of independent frames
    "avm_fsel_select_batch": (_int, [_vp, _int, _fsel, _P(FselOut)]),
    "avm_fsel_select": (_int, [_vp, _int, _fsel, c_ip, c_ip, c_dp]),
    "avm_fsel_fallback_stats": (_int, [_vp, _i64s]),
    "avm_fsel_nn_depth": (_int, [_vp, _int, _fsel, c_dp]),
    "avm_fsel_information": (_int, [_vp, _int, _fsel, c_dp, c_dp, c_ip]),
    # multi-GPU: the library's own communicator
    "avm_comm_unique_id": (_int, [_vp, _vp]),
    "avm_comm_init": (_int, [_vp, _i32, _i32, _vp]),
    "avm_gather_states": (_int, [_vp, c_dp, c_dp, C.c_size_t]),
    "avm_comm_destroy": (_int, [_vp]),
    # the ctx stream, and the timing of the last call on it
    "avm_ctx_stream": (_int, [_vp, _P(_vp)]),
    "avm_last_kernel_ms": (_int, [_vp, C.c_char_p, _P(C.c_float)]),
    # test / bench hooks, not in avm.h
    "avm_debug_copy_sqrt_info": (_int, [_vp, _int, c_dp]),
    "avm_debug_last_solve_form": (_int, [_vp]),
    "avm_debug_last_marg_form": (_int, [_vp]),
    "avm_debug_last_fsel_form": (_int, [_vp]),
    "avm_debug_last_split": (_int, [_vp, _i64s]),
    "avm_debug_counters": (_int, [_vp, _i64s]),
    "avm_debug_preint_cache": (_int, [_vp, _i64s]),
    "avm_debug_fsel_evaluations": (_int, [_vp, _i64s]),
    "avm_debug_solve_tp_occupancy": (_int, [_ints]),
    "avm_debug_solve_tp_list_occupancy": (_int, [_ints]),
    "avm_debug_solve_pattern": (_int, [_int, _ints]),
    "avm_debug_solve_tp_pattern": (_int, [_ints]),
    "avm_debug_table_limits": (_int, [_ints]),
    "avm_debug_struct_sizes": (_int, [_ints]),
    "avm_debug_track_struct_sizes": (_int, [_ints]),
    "avm_debug_relo_struct_sizes": (_int, [_ints]),
    "avm_debug_align_layout": (_int, [_ints]),
}


class SfmBatch(C.Structure):
    """avm_sfm_batch (include/avm_init.h): relativePose's result, all_image_frame and every frame's image, one row per stream."""
    _fields_ = [("n_windows", C.c_int32), ("max_frames", C.c_int32), ("max_pts", C.c_int32), ("ba_max_num_iterations", C.c_int32),
                ("ba_max_solver_time_s", C.c_double),
                ("l", c_ip), ("n_frames", c_ip), ("key_index", c_ip), ("frame_n_pts", c_ip), ("frame_pt_id", c_ip),
                ("relative_R", c_dp), ("relative_T", c_dp), ("frame_pt_xy", c_dp)]


class SfmOut(C.Structure):
    """avm_sfm_out (include/avm_init.h)."""
    _fields_ = [("ok", c_ip), ("frame_R", c_dp), ("frame_T", c_dp), ("q", c_dp), ("T", c_dp), ("point", c_dp), ("point_state", c_ip),
                ("ba_counts", c_ip), ("ba_cost", c_dp), ("pnp_q", c_dp), ("pnp_t", c_dp)]


# The declarations of include/avm_init.h, the initialisation phase: a table of its own, applied by lib.lib() like the one above
PROTOTYPES_INIT = {
    "avm_global_sfm_batch": (_int, [_vp, _int, _P(SfmBatch), _win, c_ip, _P(SfmOut)]),
}


def default_options() -> Options:
    """Values the reference runs with (estimator.cpp:794-806, euroc_config.yaml:54-63) + Ceres defaults.

    Kept in Python so that host code can build options without loading any native library;
    tests check it against avm_default_options() of the product and the oracle.
    """
    o = Options()
    o.max_num_iterations = 8
    o.estimate_extrinsic = 0
    o.estimate_td = 0
    o.marginalization_flag = MARGIN_OLD
    o.focal_length = 460.0
    o.g[0], o.g[1], o.g[2] = 0.0, 0.0, 9.81007
    o.acc_n, o.gyr_n, o.acc_w, o.gyr_w = 0.08, 0.004, 0.00004, 2.0e-6
    o.cauchy_a = 1.0
    o.max_sum_dt = 10.0
    o.initial_trust_region_radius = 1e4
    o.max_trust_region_radius = 1e16
    o.min_trust_region_radius = 1e-32
    o.min_relative_decrease = 1e-3
    o.function_tolerance = 1e-6
    o.gradient_tolerance = 1e-10
    o.parameter_tolerance = 1e-8
    o.min_lm_diagonal = 1e-6
    o.max_lm_diagonal = 1e32
    o.max_num_consecutive_invalid_steps = 5
    o.jacobi_scaling = 1
    o.marg_eps = 1e-8
    o.tr, o.row = 0.0, 480.0  # global shutter (euroc_config.yaml:66), image_height 480
    o.max_solver_time_s = 0.0  # no wall-clock cap (estimator.cpp:803-806 sets SOLVER_TIME; off for parity and the bench)
    o.marg_noise_rel = 1e-18   # the eigenvalue clamp also tests against the rounding noise of the eigenvector's variables (0: reference-literal)
    return o


def _ptr(a, ctype):
    """Pointer to a numpy array (host) or a torch tensor (host or device)."""
    if a is None:
        return C.cast(None, C.POINTER(ctype))
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(C.POINTER(ctype))
    # torch tensor
    assert a.is_contiguous()
    return C.cast(a.data_ptr(), C.POINTER(ctype))


def dptr(a):
    return _ptr(a, C.c_double)


def iptr(a):
    return _ptr(a, C.c_int32)
