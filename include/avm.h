/*
 * avm.h — C ABI of the MI355X-native hot paths of Anticipated-VINS-Mono.
 *
 * The reference has no FFI/plugin interface: both hot paths are C++ member
 * functions on stateful objects called from one thread
 * (vins_estimator/src/estimator_node.cpp:340,360).  This header is the boundary
 * a maintainer would bind instead of
 *
 *   HP-A  void Estimator::optimization()                       vins_estimator/src/estimator.h:47
 *                                                              (body estimator.cpp:661-994)
 *   HP-B  std::pair<std::vector<int>,std::vector<int>>
 *         FeatureSelector::select(image_t&, const Header&, int) vins_estimator/src/feature_selector.h:49-50
 *                                                              (body feature_selector.cpp:74-202)
 *
 * Conventions
 *   - plain pointers + sizes, FP64 everywhere, row-major, no exceptions cross
 *     the ABI; every function returns AVM_OK (0) or a negative avm_status.
 *   - the index tables of a batch (feature tracks, IMU sample counts, prior block
 *     tables, the selector's counts) are validated before any kernel indexes with
 *     them - host tables on the host, device-resident ones by a one-thread-per-window
 *     kernel: AVM_ERR_INVALID, avm_last_error() names the first bad window and the
 *     rule, nothing has been modified.  (avm_window_solve_batch on device-resident
 *     tables reads that kernel's verdict while the pre-integration - which writes
 *     library-owned buffers only and clamps the one entry it indexes with - is already
 *     running; nothing else is launched before the verdict is in.)
 *   - all buffers are caller owned.  `mem` says whether the pointers are host
 *     pointers (the library stages them over PCIe) or device pointers already
 *     resident in HBM (what bench.py times).
 *   - one avm_ctx per host thread (re-entrant, no statics — the reference's
 *     function-local statics at feature_selector.cpp:85,383,424 are NOT
 *     reproduced); the ctx owns device scratch + one HIP stream.
 *   - stream ordering of AVM_MEM_DEVICE buffers: the ctx stream is a BLOCKING stream,
 *     i.e. it is ordered after everything submitted to the legacy default (NULL) stream
 *     before the call (PyTorch's default current stream, plain hipMemcpy), and every
 *     entry point returns only after its own work has finished.  A caller that fills
 *     device buffers on some other non-blocking stream must order that stream itself
 *     before calling in (synchronize it, or record an event and hipStreamWaitEvent on
 *     avm_ctx_stream()).
 *   - quaternions are stored (x,y,z,w) exactly like para_Pose
 *     (estimator.cpp:484-488).
 *
 * Struct layouts in this header are shared verbatim by the CPU oracle
 * (oracle/, test infrastructure only) so the same buffers can be handed to both.
 */
#ifndef AVM_H_
#define AVM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AVM_WINDOW_SIZE 10               /* parameters.h:14  */
#define AVM_NFRAMES (AVM_WINDOW_SIZE + 1)
#define AVM_SIZE_POSE 7                  /* parameters.h:53  */
#define AVM_SIZE_SPEEDBIAS 9             /* parameters.h:54  */
#define AVM_MAX_ITER_TRACE 16

typedef enum avm_status {
  AVM_OK = 0,
  AVM_ERR_INVALID = -1,     /* bad argument / size */
  AVM_ERR_UNSUPPORTED = -2, /* not available on this host: a selector HORIZON without a kernel instance (2,3,5,10,13 are built),
                               or librccl.so.1 cannot be loaded for avm_comm_* */
  AVM_ERR_NO_DEVICE = -3,   /* no HIP device: there is NO CPU fallback */
  AVM_ERR_HIP = -4,         /* HIP runtime error, see avm_last_error() */
  AVM_ERR_CAPACITY = -5     /* problem larger than avm_config limits */
} avm_status;

typedef enum avm_mem { AVM_MEM_HOST = 0, AVM_MEM_DEVICE = 1 } avm_mem;

/* prior block kinds (replaces the pointer-keyed addr_shift map, estimator.cpp:904-916) */
enum { AVM_BLK_POSE = 0, AVM_BLK_SPEEDBIAS = 1, AVM_BLK_EXPOSE = 2, AVM_BLK_TD = 3 /* para_Td, 1 value */ };

/* marginalization_flag, estimator.h:33-37 */
enum { AVM_MARGIN_OLD = 0, AVM_MARGIN_SECOND_NEW = 1, AVM_MARGIN_NONE = 2 };

/* termination, mirrors ceres::TerminationType as far as this path can reach it */
enum {
  AVM_TERM_NO_CONVERGENCE = 0, /* max_num_iterations reached */
  AVM_TERM_GRADIENT_TOL = 1,
  AVM_TERM_PARAMETER_TOL = 2,
  AVM_TERM_FUNCTION_TOL = 3,
  AVM_TERM_MIN_RADIUS = 4,
  AVM_TERM_FAILURE = 5         /* too many invalid steps / linear solver failure */
};

/* Solver + model options.  Defaults (avm_default_options) are the values the
 * reference runs with: estimator.cpp:794-806, config/euroc/euroc_config.yaml:54-63,
 * parameters.cpp:11, estimator.cpp:17, and the Ceres defaults listed in SURVEY.md §5.9. */
typedef struct avm_options {
  int32_t max_num_iterations;        /* NUM_ITERATIONS = 8 (the wall-clock cap: max_solver_time_s below) */
  int32_t estimate_extrinsic;        /* 0: ex_pose constant (SetParameterBlockConstant, estimator.cpp:677-681); != 0: a variable of the solve */
  int32_t estimate_td;               /* != 0: every vision factor is a ProjectionTdFactor and para_Td is a variable (estimator.cpp:684-688,732-747) */
  int32_t marginalization_flag;      /* AVM_MARGIN_* */
  double focal_length;               /* FOCAL_LENGTH 460; sqrt_info = focal/1.5 * I2 (estimator.cpp:17) */
  double g[3];                       /* G = (0,0,g_norm) parameters.cpp:11,127 */
  double acc_n, gyr_n, acc_w, gyr_w; /* integration_base.h:21-27 */
  double cauchy_a;                   /* CauchyLoss(1.0) estimator.cpp:666 */
  double max_sum_dt;                 /* 10.0: IMU factor skipped above (estimator.cpp:705) */
  /* Ceres trust-region defaults (not overridden by the reference) */
  double initial_trust_region_radius; /* 1e4  */
  double max_trust_region_radius;     /* 1e16 */
  double min_trust_region_radius;     /* 1e-32 */
  double min_relative_decrease;       /* 1e-3 */
  double function_tolerance;          /* 1e-6 */
  double gradient_tolerance;          /* 1e-10 */
  double parameter_tolerance;         /* 1e-8 */
  double min_lm_diagonal;             /* 1e-6 */
  double max_lm_diagonal;             /* 1e32 */
  int32_t max_num_consecutive_invalid_steps; /* 5 */
  int32_t jacobi_scaling;                    /* 1 */
  double marg_eps;                           /* 1e-8 marginalization_factor.h:70 */
  double tr, row;                            /* TR (rolling-shutter read-out time, 0 for a global shutter) and ROW (image height), parameters.cpp:
                                                only read by the td factor (projection_td_factor.cpp:19-20,50-52) */
  double max_solver_time_s;                  /* options.max_solver_time_in_seconds (estimator.cpp:803-806: SOLVER_TIME, x 4/5 under MARGIN_OLD;
                                                config/euroc/euroc_config.yaml:54).  0 (the default) = no cap, which is what the parity
                                                tests and the bench run with.  > 0: checked like Ceres' MaxSolverTimeReached at the top of
                                                every iteration, before the iteration limit, against a device wall clock that starts when the
                                                window's solve starts on the GPU (staging and pre-integration are not counted); the
                                                minimizer then stops at the current point with AVM_TERM_NO_CONVERGENCE.  Non-finite values
                                                and anything above 1e9 s mean "no cap".  Both forms of the solve kernel check it (round 5:
                                                a batch larger than the CU count keeps the throughput form under a cap) */
  double marg_noise_rel;                     /* The eigenvalue clamp of marginalization_factor.cpp:284-285 keeps S > marg_eps.  With
                                                marg_noise_rel > 0 (default 1e-18) an eigenvalue is kept only if it ALSO exceeds the
                                                rounding noise of the variables its eigenvector lives on,
                                                S^2 > marg_noise_rel * v^T diag(s) v, s_i the magnitude the diagonal entry A'_ii was
                                                formed at: the exact zeros of a rank-deficient A' (the first marginalization of a run,
                                                ragged tracks) are dropped as exact arithmetic would drop them, where the reference's own
                                                FP64 run keeps some of them as rounding noise.  The default is
                                                set so that NO genuine direction is dropped: along eight 20-frame streams the states
                                                stay as close to the exact-prior stream as with the literal clamp (round 5; 1e-16, the
                                                default of rounds 2-4, dropped weak genuine directions on 11 of 160 frames).  0 = the
                                                reference-literal clamp, nothing but S > marg_eps (AVM_PRIOR_LITERAL=1 does the same and
                                                also forces the eigen-decomposition path) */
} avm_options;

/* Table sizes of an avm_window_batch.  AVM_MAX_FEAT_WIDE / AVM_MAX_OBS_WIDE are the largest strides the API accepts for a
 * window: avm_imu_preintegrate_batch and avm_triangulate_batch take them (their kernels hold nothing per feature on chip;
 * the cap is this contract, not a kernel limit), larger strides get AVM_ERR_CAPACITY naming it.  avm_slide_window and
 * avm_fsel_build_cloud take tables of any size.  AVM_MAX_FEAT / AVM_MAX_OBS are what the solve kernels are built for
 * today: avm_window_solve_batch, avm_window_solve and avm_window_eval_factors keep the window's inverse depths in a compute
 * unit's LDS and refuse larger strides with AVM_ERR_CAPACITY. */
#define AVM_MAX_FEAT 150
#define AVM_MAX_OBS (AVM_MAX_FEAT * AVM_NFRAMES)           /* 1650 */
#define AVM_MAX_FEAT_WIDE 384
#define AVM_MAX_OBS_WIDE (AVM_MAX_FEAT_WIDE * AVM_NFRAMES) /* 4224 */

/* A batch of independent sliding windows, struct-of-arrays over the window index.
 * [B] = n_windows.  Strides are the max_* fields so that one batch can hold
 * ragged windows.  Maps the inputs of Estimator::optimization() (SURVEY §8 A1,A14). */
typedef struct avm_window_batch {
  int32_t n_windows;
  int32_t max_feat;  /* stride of per-feature arrays (>= max n_feat); limits above */
  int32_t max_obs;   /* stride of per-observation arrays (>= max total observations); limits above */
  int32_t max_samp;  /* stride of IMU sample arrays (>= max samples per interval) */
  int32_t max_prior; /* leading dimension of prior_J / prior_r (>= max prior_n) */
  int32_t max_pblk;  /* stride of prior block tables */

  /* ---- state, in/out: para_Pose / para_SpeedBias / para_Ex_Pose / para_Feature (estimator.h:109-115) */
  double* pose;      /* [B][11][7]  x y z qx qy qz qw */
  double* speedbias; /* [B][11][9]  v ba bg */
  double* ex_pose;   /* [B][7]      tic, qic */
  double* inv_depth; /* [B][max_feat]  1/estimated_depth, feature_manager.cpp:184-200 */

  /* ---- feature tracks (already filtered by used_num>=2 && start_frame<WINDOW_SIZE-2, estimator.cpp:715) */
  const int32_t* n_feat;         /* [B] */
  const int32_t* feat_start;     /* [B][max_feat] start_frame (imu_i); must be non-decreasing in e (std::list order) */
  const int32_t* feat_nobs;      /* [B][max_feat] feature_per_frame.size(); frames start..start+nobs-1 */
  const int32_t* feat_obs_begin; /* [B][max_feat] offset of the first observation in obs_xy */
  const double* obs_xy;          /* [B][max_obs][2] normalized-plane point.x, point.y (z == 1) */

  /* ---- IMU raw samples per interval j=0..9 (pre_integrations[j+1], between frames j and j+1) */
  const int32_t* imu_n; /* [B][10] number of push_back() samples */
  const double* imu_dt; /* [B][10][max_samp] */
  const double* imu_acc; /* [B][10][max_samp+1][3]; row 0 = acc_0 of the constructor (integration_base.h:13) */
  const double* imu_gyr; /* [B][10][max_samp+1][3] */
  const double* imu_lin_ba; /* [B][10][3] linearized_ba */
  const double* imu_lin_bg; /* [B][10][3] linearized_bg */

  /* ---- marginalization prior in (last_marginalization_info), prior_n == 0: none */
  const int32_t* prior_n;         /* [B] residual dimension n */
  const int32_t* prior_nblk;      /* [B] number of kept blocks */
  const int32_t* prior_blk_kind;  /* [B][max_pblk] AVM_BLK_* */
  const int32_t* prior_blk_frame; /* [B][max_pblk] frame index the block is applied to (already addr_shift'ed) */
  const double* prior_J;          /* [B][max_prior][max_prior] linearized_jacobians (n x n used) */
  const double* prior_r;          /* [B][max_prior] linearized_residuals */
  const double* prior_x0;         /* [B][max_pblk][9] keep_block_data (pose uses 7, speedbias 9, td 1) */

  /* ---- optional members of the problem; NULL = absent -------------------------------------------------------- */
  /* time offset (opt->estimate_td != 0): per OBSERVATION slot FeaturePerFrame::velocity.x, .y, cur_td, uv.y()
   * (estimator.cpp:734-736) and para_Td */
  const double* obs_vel_td;      /* [B][max_obs][4] */
  double* td;                    /* [B] in/out */
  /* relocalization (estimator.cpp:760-792, 588-604): these five arrays present <=> relocalization_info.  The loop over
   * f_manager.feature / match_points (ids ascending) is resolved by the host into feature INDICES of this batch
   * (ascending, only features with start_frame <= relo_frame_local_index) - or, for device-resident tables, by
   * avm_relo_resolve_batch below.  relo_n[w] == 0 (no feature matched): no factor
   * references relo_Pose and the solve leaves it alone, but it still comes back through double2vector's gauge fix
   * (relo_t / relo_r of :590-596), as in the reference; a window without relocalization simply ignores its relo_pose. */
  const int32_t* relo_n;         /* [B] number of matched features */
  const int32_t* relo_frame;     /* [B] relo_frame_local_index (only needed by the host for the outputs of :598-604) */
  const int32_t* relo_feat;      /* [B][max_feat] feature index of match k */
  const double* relo_xy;         /* [B][max_feat][2] match_points[k].x, .y */
  double* relo_pose;             /* [B][7] relo_Pose, in: as set by setReloFrame (:1135-1141); out: relo_t | quaternion of
                                    relo_r of double2vector (:590-596), i.e. the optimized loop-frame pose after the gauge fix */
  /* failure_occur re-anchoring of double2vector (estimator.cpp:526-531) */
  const int32_t* failure_occur;  /* [B] != 0: origin_R0 / origin_P0 come from last_pose0 instead of pose[0] */
  const double* last_pose0;      /* [B][7] last_P0, last_R0 as a quaternion x y z w */
} avm_window_batch;

/* new prior produced by the post-solve marginalization (estimator.cpp:817-990) */
typedef struct avm_prior_out {
  int32_t max_prior, max_pblk;
  int32_t* n;         /* [B] */
  int32_t* nblk;      /* [B] */
  int32_t* blk_kind;  /* [B][max_pblk] */
  int32_t* blk_frame; /* [B][max_pblk] frame index AFTER addr_shift */
  double* J;          /* [B][max_prior][max_prior] */
  double* r;          /* [B][max_prior] */
  double* x0;         /* [B][max_pblk][9] */
} avm_prior_out;

/* per-window solve report (subset of ceres::Solver::Summary) */
typedef struct avm_solve_summary {
  int32_t termination;      /* AVM_TERM_* */
  int32_t num_iterations;   /* step attempts (iteration 0 not counted) */
  int32_t num_successful;   /* accepted steps */
  int32_t accept_mask;      /* bit k set: attempt k+1 accepted */
  double initial_cost;
  double final_cost;
  double cost_trace[AVM_MAX_ITER_TRACE]; /* x_cost after each attempt */
  double radius_trace[AVM_MAX_ITER_TRACE];
} avm_solve_summary;

/* One feature-selection problem = the inputs FeatureSelector::select() reads from its
 * members + estimator.  H is a runtime parameter (state_defs.h:8 fixes 13). */
typedef struct avm_fsel_batch {
  int32_t n_problems;
  int32_t horizon;   /* HORIZON; Omega is 9(H+1) square */
  int32_t max_cand;  /* stride of candidate arrays */
  int32_t max_used;  /* stride of already-tracked ("subset") arrays */
  int32_t max_cloud; /* stride of depth cloud arrays */
  int32_t max_features; /* maxFeatures_ */

  /* horizon states state_kkH[0..H] (state_defs.h:15-19): pos, vel, ba, quaternion(x,y,z,w) */
  const double* hor_pos;  /* [P][H+1][3] */
  const double* hor_quat; /* [P][H+1][4] x y z w */
  const int32_t* nr_imu;  /* [P] nrImuMeasurements */
  const double* delta_imu; /* [P] deltaImu */
  /* IMU noise passed to setParameters (std-devs passed where variances are expected — kept) */
  double acc_var, acc_bias_var;
  /* extrinsics + pinhole camera (config/euroc/euroc_config.yaml:11-22,30-42) */
  double q_ic[4]; /* x y z w */
  double t_ic[3];
  double fx, fy, cx, cy, k1, k2, p1, p2;
  int32_t image_width, image_height;

  /* new candidates (image_new), ascending feature id */
  const int32_t* n_cand;  /* [P] */
  const int32_t* cand_id; /* [P][max_cand] */
  const double* cand_xy;  /* [P][max_cand][2] normalized plane x,y (z==1) */
  const double* cand_prob; /* [P][max_cand] fPROB channel (float32-rounded upstream) */
  /* already tracked features present in this frame (subset) */
  const int32_t* n_used;  /* [P] */
  const int32_t* used_id; /* [P][max_used] */
  const double* used_xy;  /* [P][max_used][2] */
  /* depth cloud of initKDTree(): nip points w.r.t camera k+1 and their depths (feature_selector.cpp:396-419) */
  const int32_t* n_cloud;   /* [P] */
  const double* cloud_xy;   /* [P][max_cloud][2] */
  const double* cloud_depth; /* [P][max_cloud] */
} avm_fsel_batch;

typedef struct avm_fsel_out {
  int32_t* n_selected;   /* [P] */
  int32_t* selected_ids; /* [P][max_features] in selection order (blacklist order) */
  double* fvalues;       /* [P][max_features] fMax of each round (nullable) */
  double* min_gap;       /* [P][max_features] (nullable; round 5) fMax of the round minus the largest fValue among the OTHER candidates that
                            took part in it (+inf when there was no other): how firmly the round was decided.  Every round compares FP64
                            log-determinants, so a pick whose gap is of the order of their rounding errors (1e-12 of the value) is decided by
                            rounding - a host can see that here and need not expect another FP64 implementation (the reference's own run
                            included) to make the same pick.  Exact in the forms that score every candidate every round; in the lazy form of
                            large batches exact whenever it is below 1e-8 of the value and a lower bound otherwise.  Candidates the
                            std::map equal-key rule of sortedlogDetUB keeps out of the round are not counted as far as the pick meets them. */
} avm_fsel_out;

/* B4: FeatureSelector::generateFutureHorizon in IMU mode = HorizonGenerator::imu
 * (utility/horizon_generator.cpp:25-69; state_defs.h:15-19,37-41).  Inputs are what
 * setNextStateFromImuPropagation latched (feature_selector.cpp:38-70): state_k_ (tail of the window), state_k1_
 * (IMU-propagated current frame), the body acceleration / angular rate a_k1, w_k1. */
typedef struct avm_fsel_horizon_in {
  int32_t n_problems;
  int32_t horizon;          /* H: states 0..H are produced */
  const double* k_pos;      /* [P][3] state_k_  position */
  const double* k_quat;     /* [P][4] state_k_  attitude x y z w */
  const double* k_ba;       /* [P][3] state_k_  accelerometer bias (held constant over the horizon) */
  const double* k1_pos;     /* [P][3] state_k1_ position */
  const double* k1_vel;     /* [P][3] state_k1_ velocity */
  const double* k1_quat;    /* [P][4] state_k1_ attitude x y z w */
  const double* acc;        /* [P][3] a_k1 */
  const double* gyr;        /* [P][3] w_k1 */
  const int32_t* nr_imu;    /* [P] nrImuMeasurements */
  const double* delta_imu;  /* [P] deltaImu */
} avm_fsel_horizon_in;

/* A7: inputs of ProjectionTdFactor (factor/projection_td_factor.cpp:6-32,34-141; call site estimator.cpp:732-747),
 * one entry per factor: the factor on its own (the solve uses it through avm_window_batch::obs_vel_td when
 * opt->estimate_td != 0), for hosts that assemble problems themselves and for the parity tests. */
typedef struct avm_td_factor_batch {
  int32_t n;
  const double* pose_i;    /* [n][7] x y z qx qy qz qw */
  const double* pose_j;    /* [n][7] */
  const double* ex_pose;   /* [n][7] */
  const double* inv_depth; /* [n] */
  const double* td;        /* [n] current time offset (para_Td) */
  const double* pts_i;     /* [n][2] normalized plane, z == 1 */
  const double* pts_j;     /* [n][2] */
  const double* vel_i;     /* [n][2] image velocity of the feature in frame i (FeaturePerFrame::velocity) */
  const double* vel_j;     /* [n][2] */
  const double* td_i;      /* [n] cur_td when frame i was taken */
  const double* td_j;      /* [n] */
  const double* row_i;     /* [n] image row (uv.y()), before the ROW / 2 shift of the constructor */
  const double* row_j;     /* [n] */
  double tr, row;          /* TR (rolling shutter read-out time), ROW (image height): parameters.cpp */
  double focal_length;     /* sqrt_info = focal_length / 1.5 * I2 (estimator.cpp:17) */
} avm_td_factor_batch;

typedef struct avm_config {
  int32_t device;       /* HIP device ordinal */
  int32_t max_windows;  /* capacity of one avm_window_solve_batch call */
  int32_t max_problems; /* capacity of one avm_fsel_select_batch call */
  int32_t abi_version;  /* AVM_ABI_VERSION of the header the caller was compiled against.  avm_create() refuses any other value
                         * (AVM_ERR_INVALID): the structs of this header carry no size fields, so a host built against an older
                         * header - avm_fsel_out had three members before min_gap - must not get as far as a call that reads them. */
  int32_t reserved[4];
} avm_config;
#define AVM_ABI_VERSION 6 /* bumped whenever a struct of this header changes its layout or an entry point its meaning */

typedef struct avm_ctx avm_ctx;

/* ---- lifecycle -------------------------------------------------------------- */
int avm_default_options(avm_options* opt);
int avm_create(const avm_config* cfg, avm_ctx** out);
void avm_destroy(avm_ctx* ctx);
const char* avm_last_error(const avm_ctx* ctx);
const char* avm_version(void);
int avm_abi_version(void); /* AVM_ABI_VERSION the library was built with */

/* ---- HP-A: Estimator::optimization() for a batch of independent windows ------ */
/* solve in place (states updated like double2vector+vector2double leave them),
 * optionally producing the new prior.  prior_out may be NULL iff
 * opt->marginalization_flag == AVM_MARGIN_NONE.  summary may be NULL. */
int avm_window_solve_batch(avm_ctx* ctx, const avm_options* opt, avm_mem mem,
                           const avm_window_batch* batch, avm_prior_out* prior_out,
                           avm_solve_summary* summary /* [B], host or device per mem */);

/* The same solve with a marginalization flag PER WINDOW: a batch of streams, each of which took its own keyframe decision
 * (estimator.cpp:117-120; avm_keyframe_decision_batch below).  marginalization_flags: [B] in `mem` space, each AVM_MARGIN_OLD,
 * AVM_MARGIN_SECOND_NEW or AVM_MARGIN_NONE; anything else is AVM_ERR_INVALID naming the window, before any kernel reads a flag.
 * NULL: opt->marginalization_flag for every window - that is avm_window_solve_batch, which is this call with NULL.
 * Window w is solved and marginalized exactly (bit for bit) as avm_window_solve_batch does it in a batch whose
 * opt->marginalization_flag is marginalization_flags[w]; opt->marginalization_flag itself is not read when flags are given, and
 * prior_out must be given.  A window whose flag is AVM_MARGIN_NONE is not marginalized and reports prior_out->n = -1, nblk = 0, exactly
 * as a MARGIN_SECOND_NEW window whose prior does not hold pose[WINDOW_SIZE - 1]: both mean "the caller keeps the prior it had".  (A
 * batch whose flags are all AVM_MARGIN_NONE launches no marginalization and reports the same.)
 * opt->max_solver_time_s stays ONE cap per call.  The reference gives a MARGIN_OLD frame 4/5 of SOLVER_TIME (estimator.cpp:803-806);
 * which cap a mixed batch runs under is the caller's choice, there is no cap per window. */
int avm_window_solve_batch_flags(avm_ctx* ctx, const avm_options* opt, avm_mem mem, const avm_window_batch* batch,
                                 const int32_t* marginalization_flags /* [B], in `mem` space; NULL = opt's */,
                                 avm_prior_out* prior_out, avm_solve_summary* summary);

/* The same call for a batch of streams of which SOME have a relocalization pending: every window takes the kernel form of its own
 * problem, instead of the relocalization arrays sending the whole batch to the extended kernel.
 * relo_active: [B] in `mem` space, or NULL.  NULL is avm_window_solve_batch_flags, call for call.  Otherwise:
 *  - relo_active[w] != 0: window w has a relocalization pending - the test avm_relo_resolve_batch applies to
 *    state->relocalization_info, and that array can be passed as it is.  relo_n, relo_frame, relo_feat, relo_xy and relo_pose of the
 *    batch must then be present (AVM_ERR_INVALID otherwise, whatever the values of relo_active).  The window is solved exactly (bit for
 *    bit) as avm_window_solve_batch_flags solves it in this batch with the arrays; relo_n[w] == 0 keeps its meaning: the loop frame
 *    takes part in the gauge fix without a factor.
 *  - relo_active[w] == 0: none of the window's relo_* rows is read (they may hold anything) and its relo_pose row is NOT written.
 *    With opt->estimate_extrinsic == opt->estimate_td == 0 the window is solved by the kernel form it would get in this same batch
 *    without the relocalization arrays - chosen from n_windows of the WHOLE batch, not from the number of such windows - so its result
 *    is, to the bit, what it would have been had no stream of the batch been relocalizing.  A prior that does not fit the throughput
 *    form sends the batch's plain windows to the latency form, as it does without the arrays (the rule stays per batch).
 *  - With opt->estimate_extrinsic or opt->estimate_td set every window takes the extended kernel as before; relo_active then only
 *    decides which windows have a relocalization frame (the first two points hold unchanged).
 *  - The marginalization runs once, on the whole batch, and reads no relocalization data.  It takes its throughput form when the plain
 *    windows' solve does or when n_windows exceeds the number of compute units (unless a prior does not fit it, or AVM_MARG_TP=0).
 *  - marginalization_flags, summary, opt->max_solver_time_s and prior_out behave as in avm_window_solve_batch_flags;
 *    avm_last_kernel_ms("window_solve") covers both launches of the solve. */
int avm_window_solve_batch_relo(avm_ctx* ctx, const avm_options* opt, avm_mem mem, const avm_window_batch* batch,
                                const int32_t* marginalization_flags /* [B] or NULL, as avm_window_solve_batch_flags */,
                                const int32_t* relo_active /* [B], in `mem` space, or NULL */,
                                avm_prior_out* prior_out, avm_solve_summary* summary);

/* the single-call form, exactly one Estimator::optimization() (estimator.h:47): the same arguments with
 * batch->n_windows == 1 (AVM_ERR_INVALID otherwise).  One window occupies one compute unit; see DESIGN.md for its latency. */
int avm_window_solve(avm_ctx* ctx, const avm_options* opt, avm_mem mem, const avm_window_batch* window,
                     avm_prior_out* prior_out, avm_solve_summary* summary);

/* A4 only: IntegrationBase for every interval of every window (integration_base.h:13-158).
 * out_* are [B][10][...]: delta (p3,q4 xyzw,v3 = 10), jacobian 15x15, covariance 15x15, sum_dt.
 *
 * The ctx remembers its last pre-integration - this call's, and the one inside avm_window_solve_batch* and
 * avm_window_eval_factors - together with a copy of the inputs every interval was integrated from (imu_n, the samples and
 * dt up to imu_n, imu_lin_ba / imu_lin_bg; about 1.2 KB per interval at max_samp = 20).  The next call compares every
 * interval's inputs with that copy, bit by bit, on the device, and integrates only the intervals that differ; a call with
 * another n_windows, max_samp or noise density integrates all of them, and avm_slide_window* moves the remembered
 * intervals with the window.  Content decides, nothing else: there is nothing to invalidate or to tell the ctx, the
 * results are those of integrating everything, and changing a sample in place is seen.  AVM_PREINT_CACHE=0 in the
 * environment (read on every call) integrates every interval on every call. */
int avm_imu_preintegrate_batch(avm_ctx* ctx, const avm_options* opt, avm_mem mem,
                               const avm_window_batch* batch, double* out_delta, double* out_jacobian,
                               double* out_covariance, double* out_sum_dt);

/* SURVEY 8(f)1 - the step right before optimization() in solveOdometry() (estimator.cpp:471):
 * FeatureManager::triangulate (feature_manager.cpp:202-257).  Every feature whose inv_depth is <= 0
 * ("no depth yet": estimated_depth = -1 at construction, feature_manager.h:61) gets 1 / depth from the linear
 * multi-view triangulation over all of its observations, in the camera frame of its first observation: the
 * smallest right singular vector v of the (2 nobs) x 4 system, depth = v[2] / v[3]; depths < 0.1 fall back to
 * init_depth (INIT_DEPTH = 5.0, parameters.cpp:113).  In place on batch->inv_depth; reads pose, ex_pose and the
 * feature tables only.  (IntegrationBase::repropagate, the other half of that row, is
 * avm_imu_preintegrate_batch() with the new linearization biases in imu_lin_ba / imu_lin_bg.) */
int avm_triangulate_batch(avm_ctx* ctx, avm_mem mem, avm_window_batch* batch, double init_depth);

/* SURVEY 8(f)1, second half: the dead-reckoning of the newest frame in Estimator::processIMU (estimator.cpp:100-107).
 * Frame AVM_WINDOW_SIZE of every window (which slideWindow() left holding a copy of the previous newest frame) is
 * carried through the raw samples of the last interval (imu_* [B][AVM_WINDOW_SIZE-1], row 0 of acc/gyr = the sample
 * the interval was constructed with): world-frame midpoint integration with the biases of that frame and gravity g;
 * Rs is propagated as a matrix times the rotation matrix of the UNNORMALIZED deltaQ, as the reference does, and turned
 * into the pose quaternion at the end.  In place on batch->pose[.][10] and batch->speedbias[.][10][0..2]. */
int avm_imu_propagate_batch(avm_ctx* ctx, avm_mem mem, avm_window_batch* batch, const double g[3]);

/* B4 (see avm_fsel_horizon_in): constant body acceleration / angular rate propagation of states 2..H with
 * Qimu = deltaQ(w * deltaImu) - UNNORMALIZED and never renormalized in the loop (horizon_generator.cpp:46,54) - and
 * gravity (0, 0, -9.80665).  Writes hor_pos [P][H+1][3] and hor_quat [P][H+1][4] (x y z w), the layout
 * avm_fsel_batch consumes. */
int avm_fsel_horizon_imu(avm_ctx* ctx, avm_mem mem, const avm_fsel_horizon_in* in, double* hor_pos, double* hor_quat);

/* A7: ProjectionTdFactor::Evaluate for n factors: residual [n][2], jac [n][2][20] with columns
 * pose_i 6 | pose_j 6 | ex_pose 6 | inv_depth 1 | td 1 (local 6-column pose blocks, like avm_window_eval_factors). */
int avm_projection_td_eval(avm_ctx* ctx, avm_mem mem, const avm_td_factor_batch* f, double* residual, double* jac);

/* B8, first half: the depth cloud FeatureSelector::initKDTree() builds (feature_selector.cpp:380-433), one cloud per
 * window: every feature of the window (they all pass used_num >= 2 && start_frame < WINDOW_SIZE - 2 by construction)
 * with start_frame <= WINDOW_SIZE * 3 / 4 and solve_flag == 1 (depth = 1 / inv_depth >= 0, feature_manager.cpp:141-159)
 * is lifted to the world with its first observation and its depth, moved into camera k+1 (state_k1_: k1_pos [B][3],
 * k1_quat [B][4] x y z w; extrinsic = the window's ex_pose) and projected to the normalized plane.  Output in feature
 * order, the layout avm_fsel_batch consumes: n_cloud [B], cloud_xy [B][max_cloud][2], cloud_depth [B][max_cloud].
 * (The nearest-neighbour lookup itself, findNNDepth, runs inside avm_fsel_select_batch.) */
int avm_fsel_build_cloud(avm_ctx* ctx, avm_mem mem, const avm_window_batch* windows, const double* k1_pos, const double* k1_quat,
                         int32_t max_cloud, int32_t* n_cloud, double* cloud_xy, double* cloud_depth);

/* the window roll, Estimator::slideWindow (estimator.cpp:996-1107) with FeatureManager::removeBackShiftDepth /
 * removeBack / removeFront (feature_manager.cpp:275-352), applied IN PLACE to the batch so that the next solve can run on
 * the same (device-resident) tables; the prior hand-off is already part of avm_window_solve_batch (blk_frame carries the
 * addr_shift).  frame_count == WINDOW_SIZE is assumed.  The const qualifiers of the batch's table pointers are cast away:
 * the caller owns writable memory of the declared strides.
 *   AVM_MARGIN_OLD:        poses / speed-biases / IMU intervals move down by one (frame 10 keeps its values, interval 9
 *                          becomes empty: imu_n = 0, row 0 of imu_acc / imu_gyr = the last sample pushed, linearization
 *                          biases = those of frame 10); a feature with start_frame != 0 starts one frame earlier, the
 *                          others lose their first observation and are erased when fewer than 2 remain (shift_depth != 0,
 *                          i.e. solver_flag == NON_LINEAR; their depth is re-anchored in the new first frame, init_depth
 *                          where it comes out non-positive) or when none remains (shift_depth == 0).
 *   AVM_MARGIN_SECOND_NEW: frame 10 overwrites frame 9, the samples of interval 9 are appended to interval 8
 *                          (AVM_ERR_CAPACITY if that exceeds max_samp); a feature that starts in frame 10 starts in 9,
 *                          the others lose their frame-9 observation if they were still tracked in frame 9, and are
 *                          erased when none remains.
 * Erasing compacts the per-feature arrays in order (std::list order); observations stay where they are, only
 * feat_obs_begin / feat_nobs change (one element moves for removeFront).  inv_depth holds 1 / estimated_depth.
 * This entry point and avm_slide_window_flags do not move obs_vel_td: avm_slide_window_tracks does. */
int avm_slide_window(avm_ctx* ctx, avm_mem mem, avm_window_batch* windows, int32_t marginalization_flag, int32_t shift_depth, double init_depth);

/* The roll with a flag per window: marginalization_flags [B] in `mem` space, each AVM_MARGIN_OLD or AVM_MARGIN_SECOND_NEW (anything
 * else, AVM_MARGIN_NONE included: AVM_ERR_INVALID naming the window, nothing written).  Window w is rolled exactly as avm_slide_window
 * rolls it under marginalization_flags[w]; avm_slide_window is the uniform case with remove_failures = 0.  AVM_ERR_CAPACITY as there,
 * also when a single MARGIN_SECOND_NEW window overflows max_samp (the other windows were rolled).
 * remove_failures != 0: `slideWindow(); f_manager.removeFailures();`, the order of processImage (estimator.cpp:197-198).  A feature
 * is a failure if BEFORE the roll it passed the solve's filter (feat_nobs >= 2 && feat_start < WINDOW_SIZE - 2) and its inv_depth
 * is < 0: setDepth's solve_flag = 2 (feature_manager.cpp:141-159).  It is erased after the roll whatever the roll did to its depth
 * (removeBackShiftDepth rewrites a non-positive re-anchored depth to init_depth), compacting in list order like the roll's own
 * erasures.  A feature that never entered the solve is never erased by this rule: it carries inv_depth = 1 / (-1), "no depth yet". */
int avm_slide_window_flags(avm_ctx* ctx, avm_mem mem, avm_window_batch* windows, const int32_t* marginalization_flags /* [B] */,
                           int32_t shift_depth, double init_depth, int32_t remove_failures);

/* The keyframe decision of every window: the return value of FeatureManager::addFeatureCheckParallax (feature_manager.cpp:74-96,
 * compensatedParallax2 :355-388) for frame_count == WINDOW_SIZE, on tables that ALREADY hold the new image's observations (frame 10).
 *   last_track_num = features with feat_nobs >= 2 whose last observation is in frame 10 (the ones the new image extended);
 *   parallax sum / num over the features with start <= 8 && start + nobs - 1 >= 9, in list order: sqrt(du^2 + dv^2) between their
 *   frame-8 and frame-9 observations (the observations are normalized, z == 1: the "compensated" branch is the same number);
 *   flag = AVM_MARGIN_OLD (keyframe) if last_track_num < 20, or num == 0, or sum / num >= min_parallax (MIN_PARALLAX, i.e. the
 *   configured pixels / FOCAL_LENGTH); else AVM_MARGIN_SECOND_NEW.
 * The decision is discrete, so the arithmetic is the reference's and not a tolerance: every term without FMA contraction, the terms
 * added one after the other in list order.  Outputs in `mem` space: marginalization_flags [B]; last_track_num [B] and parallax [B][2]
 * (sum, num - both over the whole list, also where last_track_num < 20 decided) may be NULL.
 * It is the reference's decision when the tables hold the whole f_manager.feature list (as avm_host::Estimator::slideWindow
 * marshals it).  On the solve's FILTERED tables (start < WINDOW_SIZE - 2) the tracks that start in frame 8 are missing from the mean.
 * Tables up to AVM_MAX_FEAT_WIDE / AVM_MAX_OBS_WIDE; they are validated before the kernel indexes with them. */
int avm_keyframe_decision_batch(avm_ctx* ctx, avm_mem mem, const avm_window_batch* windows, double min_parallax,
                                int32_t* marginalization_flags /* [B] out */, int32_t* last_track_num /* [B] out, nullable */,
                                double* parallax /* [B][2] out, nullable: sum, num */);

/* Estimator::failureDetection (estimator.cpp:612-658) after the solve: failed[w] = 0, or the number of the first rule that fired, in
 * the reference's order:  1: |Ba[10]| > 2.5   2: |Bg[10]| > 1.0   3: |P[10] - last_P| > 5   4: |P[10].z - last_P.z| > 1
 * (Euclidean norms; the reference's commented-out rules and the ones that only log are not rules here).  last_P: [B][3], the newest
 * frame's position after the previous image (estimator.cpp:209); reads windows->pose and windows->speedbias only. */
int avm_failure_detection_batch(avm_ctx* ctx, avm_mem mem, const avm_window_batch* windows, const double* last_P /* [B][3] */,
                                int32_t* failed /* [B] out */);

/* ---- the feature manager on device-resident tables: a batch of streams takes an image without a host rewriting its tables ----------
 * Two kinds of tables.  The FULL tables hold the whole f_manager.feature list of every window: strides up to AVM_MAX_FEAT_WIDE /
 * AVM_MAX_OBS_WIDE, every track of the list a row, in list order.  The keyframe decision, the roll and removeFailures work on them.
 * The feature ids are a table BESIDE the batch, feat_id [B][max_feat] in `mem` space (the struct keeps its layout).  The VIEW is what
 * the solve and the triangulation take: the rows with feat_nobs >= 2 && feat_start < WINDOW_SIZE - 2 (estimator.cpp:715), gathered
 * into tables of the solve's strides by avm_solve_view_batch; avm_solve_view_store_depths carries the depths back (setDepth).
 * Every call below takes frame_count == WINDOW_SIZE, validates every index table before a kernel indexes with it, and is all or nothing:
 * on AVM_ERR_INVALID / AVM_ERR_CAPACITY the message names the first offending window and no table of any window has been written.
 * avm_last_kernel_ms keys: "add_image", "imu_push", "solve_view", "store_depths" (device time of the checks and the kernels). */
#define AVM_MAX_IMAGE_PTS 1024

typedef struct avm_image_batch {      /* one image per window: the `image` map of processImage, camera 0 (id_pts.second[0]) */
  int32_t n_windows, max_pts;         /* max_pts <= AVM_MAX_IMAGE_PTS */
  const int32_t* n_pts;               /* [B] */
  const int32_t* feature_id;          /* [B][max_pts] strictly ascending (std::map order) */
  const double* xy;                   /* [B][max_pts][2] point.x, point.y (z == 1) */
  const double* vel_td;               /* nullable [B][max_pts][4]: velocity.x, velocity.y, cur_td, uv.y - the layout of obs_vel_td;
                                         must be given iff windows->obs_vel_td is */
} avm_image_batch;

/* FeatureManager::addFeatureCheckParallax (feature_manager.cpp:45-96) on the full tables.  For every image point, in ascending id order:
 * an id found in feat_id[0 .. n_feat) gets the point appended to that track (feat_nobs + 1, its vel_td row with it); every other id
 * starts a new row behind the list: feat_id = id, feat_start = WINDOW_SIZE, feat_nobs = 1, inv_depth = -1.0 (1 / estimated_depth with
 * estimated_depth = -1, "no depth yet").  The observation table of the window is then rewritten dense in list order,
 * feat_obs_begin[e] = feat_nobs[0] + ... + feat_nobs[e - 1] (the roll leaves holes; obs_vel_td moves with obs_xy when present); slots at
 * and beyond the new total keep what they held.  Then the keyframe decision on the result - the kernel of avm_keyframe_decision_batch,
 * so flags_out, last_track_num and parallax are that call's on the same tables, to the bit.
 * AVM_ERR_INVALID: n_pts outside [0, max_pts]; ids not strictly ascending; a row with feat_start + feat_nobs > WINDOW_SIZE (the tables
 * already hold an observation of frame 10); an id that matches a track whose last observation is not in frame WINDOW_SIZE - 1 (the
 * reference would append it to the wrong frame; a tracker never re-issues a lost id); a duplicate in feat_id[0 .. n_feat).
 * AVM_ERR_CAPACITY: n_feat + new tracks > max_feat, or the new total of observations > max_obs; max_pts > AVM_MAX_IMAGE_PTS. */
int avm_add_image_batch(avm_ctx* ctx, avm_mem mem, avm_window_batch* windows, int32_t* feat_id /* [B][max_feat] in/out */,
                        const avm_image_batch* image, double min_parallax, int32_t* flags_out /* [B] */,
                        int32_t* last_track_num /* [B], nullable */, double* parallax /* [B][2], nullable */);

/* The buffer half of Estimator::processIMU (estimator.cpp:92-98): n[w] samples are appended to interval WINDOW_SIZE - 1 of window w -
 * imu_dt[9][imu_n ..], rows imu_n + 1 .. of imu_acc / imu_gyr, imu_n[9] += n.  n: [B], each in [0, max_in] (AVM_ERR_INVALID); dt
 * [B][max_in], acc / gyr [B][max_in][3].  AVM_ERR_CAPACITY if a window would hold more than max_samp samples.  The dead-reckoning half
 * is avm_imu_propagate_batch, called after it. */
int avm_imu_push_batch(avm_ctx* ctx, avm_mem mem, avm_window_batch* windows, const int32_t* n, int32_t max_in, const double* dt,
                       const double* acc, const double* gyr);

/* The solve's view of the full tables.  `view` is a batch of the caller's with the solve's strides (max_feat <= AVM_MAX_FEAT, max_obs <=
 * AVM_MAX_OBS, else AVM_ERR_CAPACITY); the library WRITES its n_feat, feat_start, feat_nobs, feat_obs_begin, obs_xy, inv_depth and, when
 * view->obs_vel_td is given (then full->obs_vel_td must be), obs_vel_td - the const qualifiers are cast away as in avm_slide_window; these
 * arrays must not be the full tables' own.  All its other pointers are the caller's business: normally they alias the full batch's.
 * The rows of `full` with feat_nobs >= 2 && feat_start < WINDOW_SIZE - 2 are gathered in list order, their observations dense in that
 * order; view_row[k] is the full row of view row k.  AVM_ERR_CAPACITY if a window has more such rows than view->max_feat or more
 * observations than view->max_obs. */
int avm_solve_view_batch(avm_ctx* ctx, avm_mem mem, const avm_window_batch* full, avm_window_batch* view,
                         int32_t* view_row /* [B][view->max_feat] out */);

/* FeatureManager::setDepth's copy (feature_manager.cpp:141-159): full.inv_depth[view_row[k]] = view.inv_depth[k] for k < view.n_feat.
 * view_row is validated first: inside [0, full.n_feat) and strictly increasing (AVM_ERR_INVALID). */
int avm_solve_view_store_depths(avm_ctx* ctx, avm_mem mem, avm_window_batch* full, const avm_window_batch* view, const int32_t* view_row);

/* avm_slide_window_flags on the full tables with their ids: the rows of feat_id [B][max_feat] are compacted together with the other
 * per-feature arrays, and when windows->obs_vel_td is given removeFront shifts its rows together with obs_xy, so the td channels stay
 * with their observations. */
int avm_slide_window_tracks(avm_ctx* ctx, avm_mem mem, avm_window_batch* windows, int32_t* feat_id /* [B][max_feat] in/out */,
                            const int32_t* marginalization_flags /* [B] */, int32_t shift_depth, double init_depth, int32_t remove_failures);

/* ---- the selector in the stream loop: FeatureSelector::select() (feature_selector.cpp:74-202) on device-resident images ------------
 * In the reference every image goes through select() before processImage (estimator_node.cpp:331-360).  This call is its bookkeeping
 * around the selection - splitOnFeatureId (:208-219), the tracked-feature list (:108-120, 192-196), image.swap(subset) (:192) - for
 * one image per window: it writes the selector problem from the image, runs the selection of avm_fsel_select_batch on it, and emits the
 * image avm_add_image_batch takes.  Everything is in `mem` space. */
typedef struct avm_select_state {  /* the members of FeatureSelector that outlive a call, one row per stream; in/out, `mem` space */
  int32_t max_tracked;
  int32_t* last_feature_id;  /* [B]               lastFeatureId_ */
  int32_t* n_tracked;        /* [B] */
  int32_t* tracked_id;       /* [B][max_tracked]  trackedFeatures_, in the reference's order (append order) */
  int32_t* first_image;      /* [B]               firstImage_ */
} avm_select_state;

/* prob: [B][image->max_pts], the fPROB channel of the image's points.  initialized: [B] (NULL: every window), non-zero where
 * solver_flag == NON_LINEAR.  init_thresh: initThresh_.
 * `problem` is the caller's avm_fsel_batch with n_problems == image->n_windows.  The caller gives the horizon, nr_imu, delta_imu, the
 * noise, camera and extrinsics, the cloud, max_features and the strides; the library WRITES n_cand, cand_id, cand_xy, cand_prob, n_used,
 * used_id, used_xy into the caller's buffers (the const qualifiers are cast away, as in avm_solve_view_batch).  `image_out` is the
 * caller's buffers in the same way: n_pts, feature_id, xy and, if and only if image->vel_td is given, vel_td are written.  None of its
 * arrays may be an array of `image` (AVM_ERR_INVALID).  Slots of these arrays that the call does not write keep what they held.
 * For every window, feature_selector.cpp:98-120, 156-196:
 *   1. split: the points with id > last_feature_id (upper_bound) are NEW, the others OLD; if any are new, last_feature_id becomes the
 *      image's last id.  A tracked id is looked up among the old points only (the reference searches `image` after the split), so a
 *      tracked id above last_feature_id is never found.
 *   2. used_* = the old points whose id is in tracked_id[0 .. n_tracked), ascending (n_used of every window).  An initialized window:
 *      cand_* = the new points, ascending, with their prob, n_cand their number.  An uninitialized window: n_cand = 0 (that is what the
 *      selection sees and the caller reads back; nothing is selected), its cand_* rows are not written.
 *   3. the selection of avm_fsel_select_batch on exactly these arrays, kappa = max(0, max_features - n_used); `out` is its avm_fsel_out.
 *   4. an uninitialized window with first_image != 0: the subset BECOMES the new points, every new id is appended to tracked_id in
 *      ascending order, first_image = 0 (:172-181).  Then, for any uninitialized window whose subset has fewer than init_thresh points,
 *      every old point joins the subset (:185-187).
 *   5. image_out = the subset (the used points, or rule 4's) plus the selected points, in ascending id order (std::map order), which
 *      is what avm_add_image_batch takes; xy and vel_td rows are copied bit for bit.
 *   6. the selected ids are appended to tracked_id in selection order (:196).  prune_lost != 0: the tracked ids that were not found in
 *      this image are dropped first, the others keeping their order.  The reference never prunes; its list grows without bound.  Pruning
 *      gives the same `problem`, `out` and image_out on every later image as long as the tracker never issues a lost id again (the rule
 *      avm_add_image_batch already requires of its caller) and no tracked id lies above last_feature_id: a dropped id could never be
 *      found again.
 * The state - last_feature_id, n_tracked, tracked_id, first_image - and image_out are written by the last kernel, after the selection
 * (its re-runs in a slower mode included) has finished: a refused or failed call leaves them as they were.
 * A check runs first and refuses the batch as a whole, naming the first offending window, before anything is written.  AVM_ERR_INVALID:
 * n_pts outside [0, max_pts]; ids not strictly ascending; n_tracked outside [0, max_tracked]; a NULL member; image_out sharing an array
 * with image.  AVM_ERR_CAPACITY: max_pts > AVM_MAX_IMAGE_PTS; an initialized window with more new points than problem->max_cand; more
 * used points than problem->max_used; a window whose image_out can exceed image_out->max_pts, or whose tracked list can exceed
 * state->max_tracked.  These two bounds are decided BEFORE the selection and are conservative on purpose: they take the selection to
 * pick min(kappa, new points) ids, although it may end with fewer.  image_out: n_used + min(kappa, n_new) when initialized, what rule 4
 * gives when not.  tracked list: the ids kept (n_tracked; with prune_lost the entries found in the image) plus min(kappa, n_new) when
 * initialized, plus n_new when uninitialized with first_image != 0, plus nothing otherwise.
 * (The tables of `problem` the caller gives - n_cloud, nr_imu - are checked as avm_fsel_select_batch checks them, behind the split.)
 * avm_last_kernel_ms keys: "select_split" (the check and the split), "select_merge"; "fsel_select" is the selection's, as ever. */
int avm_fsel_select_image_batch(avm_ctx* ctx, avm_mem mem, const avm_image_batch* image, const double* prob /* [B][image->max_pts] */,
                                const int32_t* initialized /* [B], nullable */, int32_t init_thresh, int32_t prune_lost,
                                avm_select_state* state, avm_fsel_batch* problem, avm_fsel_out* out, avm_image_batch* image_out);

/* ---- relocalization and the prior hand-over in the stream loop: what a batch of streams left to the host besides the initialisation ----
 * Everything below is in `mem` space and all or nothing, like the feature manager's calls: a check kernel runs first, and on
 * AVM_ERR_INVALID / AVM_ERR_CAPACITY the message names the first offending window and nothing has been written.  n_windows == 0: AVM_OK.
 * avm_last_kernel_ms keys: "headers_step", "set_relo", "relo_resolve", "relo_finish", "prior_keep".
 *
 * The frame stamps, Headers[i].stamp.toSec(), are a table BESIDE the batch like feat_id: stamp [B][11].  Step one, if
 * marginalization_flags is given: slideWindow's moves per window - AVM_MARGIN_OLD: Headers[i] = Headers[i + 1] for i < 10, then
 * Headers[10] = Headers[9] (estimator.cpp:1015,1021); AVM_MARGIN_SECOND_NEW: Headers[9] = Headers[10] (:1064); any other value is
 * AVM_ERR_INVALID.  Step two, if new_stamp is given: Headers[10] = new_stamp (:126).  A caller calls it behind the roll with the flags and
 * on the next image's arrival with new_stamp. */
int avm_headers_step_batch(avm_ctx* ctx, avm_mem mem, int32_t n_windows, double* stamp /* [B][11] in/out */,
                           const int32_t* marginalization_flags /* [B], nullable */, const double* new_stamp /* [B], nullable */);

typedef struct avm_relo_msg_batch {   /* the message of estimator_node.cpp:274-297, one row per stream */
  int32_t n_windows, max_match;       /* max_match <= AVM_MAX_IMAGE_PTS */
  const int32_t* has_msg;             /* [B] 0: no message for this stream, its row is not read */
  const double*  frame_stamp;         /* [B] */
  const int32_t* n_match;             /* [B] */
  const int32_t* match_id;            /* [B][max_match] (int)match_points[k].z(), strictly ascending */
  const double*  match_xy;            /* [B][max_match][2] */
  const double*  prev_relo_t;         /* [B][3] */
  const double*  prev_relo_q;         /* [B][4] x y z w */
} avm_relo_msg_batch;

typedef struct avm_relo_state {       /* the Estimator members that outlive the call; in/out, `mem` space */
  int32_t max_match;                  /* <= AVM_MAX_IMAGE_PTS */
  int32_t* relocalization_info;       /* [B] */
  int32_t* relo_frame;                /* [B] relo_frame_local_index */
  double*  relo_stamp;                /* [B] */
  int32_t* n_match;                   /* [B]               match_points.size() */
  int32_t* match_id;                  /* [B][max_match] */
  double*  match_xy;                  /* [B][max_match][2] */
  double*  prev_relo_t;               /* [B][3] */
  double*  prev_relo_q;               /* [B][4] x y z w */
  double*  relo_pose;                 /* [B][7]; the caller initialises rows to a finite pose (0 0 0 0 0 0 1) */
  double*  drift_correct_yaw;         /* [B]    outputs of :597-603, written by avm_relo_finish_batch only */
  double*  drift_correct_t;           /* [B][3] */
  double*  relo_relative_t;           /* [B][3] */
  double*  relo_relative_q;           /* [B][4] x y z w */
  double*  relo_relative_yaw;         /* [B] */
} avm_relo_state;

/* Estimator::setReloFrame (estimator.cpp:1109-1127) per window with has_msg != 0: frame_stamp, the first n_match matches and prev_relo_*
 * are copied into the state whether or not a frame matches (:1111-1116; match slots beyond n_match keep what they held); then for
 * i = 0 .. WINDOW_SIZE - 1 in order, stamp[w][i] == frame_stamp sets relo_frame = i, relocalization_info = 1 and relo_pose = pose[w][i] -
 * frame 10 is not searched and the last match wins, as the loop without a break does.  Windows without a message are untouched.
 * DEVIATION: the reference copies para_Pose[i], which at that point still holds what the PREVIOUS optimization's Ceres run left - before
 * the gauge fix and before the roll.  The tables have Ps / Rs only, so relo_pose starts from the current pose of frame i.  It is the start
 * value of a free variable of the solve; only with zero matched features does it reach the outputs unchanged.
 * AVM_ERR_INVALID: n_match outside [0, max_match]; ids not strictly ascending; msg->n_windows != windows->n_windows.
 * AVM_ERR_CAPACITY: state->max_match < msg->max_match; max_match > AVM_MAX_IMAGE_PTS. */
int avm_set_relo_frame_batch(avm_ctx* ctx, avm_mem mem, const avm_window_batch* windows /* pose is read */, const double* stamp /* [B][11] */,
                             const avm_relo_msg_batch* msg, avm_relo_state* state);

/* The match loop of optimization() (estimator.cpp:765-790) on the solve's view.  For a window with relocalization_info != 0: the view rows
 * k in order with feat_start[k] <= relo_frame, their id feat_id[view_row[k]]; for every such id that also occurs in match_id[0 .. n_match),
 * in ascending order, the next slot gets relo_feat = k and relo_xy = match_xy of that match.  relo_n is the count, relo_frame the
 * state's; slots at and beyond relo_n keep what they held.  A window with relocalization_info == 0 gets relo_n = 0 and relo_frame = 0.
 * *n_active (a host int, nullable) is the number of windows with relocalization_info != 0: the caller passes the four arrays and
 * state->relo_pose to the solve as the five optional members of avm_window_batch - and so takes the extended kernel - only when it is > 0.
 * DEVIATIONS: both id sequences must ascend (the reference's two-pointer loop presumes it; a tracker's ids do).  The reference advances
 * retrive_feature_index without a bound and reads past match_points when a list id exceeds every match id; here the matches simply end.
 * AVM_ERR_INVALID: view_row not strictly increasing inside [0, full_max_feat); on a window with relocalization_info != 0: relo_frame
 * outside [0, WINDOW_SIZE), n_match outside [0, state->max_match], the view rows' ids or the match ids not strictly ascending.
 * AVM_ERR_CAPACITY: view->max_feat > AVM_MAX_FEAT; state->max_match > AVM_MAX_IMAGE_PTS. */
int avm_relo_resolve_batch(avm_ctx* ctx, avm_mem mem, const avm_window_batch* view, const int32_t* feat_id /* [B][full_max_feat] */,
                           int32_t full_max_feat, const int32_t* view_row /* [B][view->max_feat] */, const avm_relo_state* state,
                           int32_t* relo_n /* [B] */, int32_t* relo_frame /* [B] */, int32_t* relo_feat /* [B][view->max_feat] */,
                           double* relo_xy /* [B][view->max_feat][2] */, int32_t* n_active /* host int, nullable */);

/* The outputs of double2vector() (estimator.cpp:588-604) for every window with relocalization_info != 0.  With relo_t | relo_r =
 * state->relo_pose as the solve returned it (after the gauge fix; the quaternion normalised as on :593), Ps | Rs = pose[w][relo_frame]
 * (the quaternion normalised as on :551) and prev_relo_r = prev_relo_q.toRotationMatrix():
 *   drift_correct_yaw = yaw(prev_relo_r) - yaw(relo_r)   in degrees
 *   drift_correct_t   = prev_relo_t - Rz(drift_correct_yaw) relo_t
 *   relo_relative_t   = relo_r^T (Ps - relo_t)
 *   relo_relative_q   = the quaternion of relo_r^T Rs
 *   relo_relative_yaw = normalizeAngle(yaw(Rs) - yaw(relo_r))
 * with R2ypr / ypr2R / normalizeAngle of utility.h:66-108,130-139; then relocalization_info = 0.  The other windows keep all five outputs.
 * Non-finite input gives non-finite output for that window only.  AVM_ERR_INVALID: relo_frame outside [0, WINDOW_SIZE) on such a window. */
int avm_relo_finish_batch(avm_ctx* ctx, avm_mem mem, const avm_window_batch* windows /* pose AFTER the solve */, avm_relo_state* state);

/* The prior hand-over (estimator.cpp:926-927).  The solve reports prior->n[w] < 0 for a window whose prior it left alone (MARGIN_NONE, or
 * MARGIN_SECOND_NEW with nothing to drop).  For every such window the slot becomes the prior the window was solved with, windows->prior_*:
 * n, nblk, the first nblk rows of blk_kind / blk_frame / x0, the leading n x n of J and n of r, each table with its own stride.  Windows
 * with n >= 0 and everything outside the used parts are untouched.  Afterwards `prior` is always chainable: with equal strides the caller
 * exchanges its seven pointers with the batch's prior_*, and that exchange is the whole hand-over.
 * AVM_ERR_INVALID: the window's own prior tables are inconsistent.  AVM_ERR_CAPACITY: a kept prior does not fit prior->max_prior / max_pblk. */
int avm_prior_keep_batch(avm_ctx* ctx, avm_mem mem, const avm_window_batch* windows, avm_prior_out* prior);

/* ---- Estimator::visualInitialAlign (estimator.cpp:355-431) with VisualIMUAlignment (initial/initial_aligment.cpp): the step that
 * moves solver_flag from INITIAL to NON_LINEAR.  It starts from the up-to-scale camera trajectory of initialStructure (relativePose,
 * GlobalSFM, solvePnP stay with the host: OpenCV and a Ceres BA) and is dense FP64 algebra on the raw IMU of all_image_frame. */
#define AVM_MAX_ALIGN_FRAMES 64   /* all_image_frame.size(); 63 intervals = one lane per interval of a wavefront */

typedef struct avm_align_batch {          /* the inputs of VisualIMUAlignment(all_image_frame, Bgs, g, x) */
  int32_t n_windows, max_frames, max_samp;
  const int32_t* n_frames;   /* [B] all_image_frame.size(), 2 .. max_frames */
  const double* frame_R;     /* [B][max_frames][9] ImageFrame::R row-major (= R_c0_ck * RIC^T, estimator.cpp:288,342) */
  const double* frame_T;     /* [B][max_frames][3] ImageFrame::T (camera position in c0, up to scale) */
  const double* tic;         /* [B][3] TIC[0] */
  /* raw IMU of interval j (frame j -> j+1), same conventions as avm_window_batch with 10 -> max_frames-1 */
  const int32_t* imu_n;      /* [B][max_frames-1] */
  const double *imu_dt, *imu_acc, *imu_gyr, *imu_lin_ba, *imu_lin_bg;
  const int32_t* key_index;  /* [B][11] position of Headers[i] in all_image_frame, strictly increasing; only read when windows != NULL */
} avm_align_batch;

typedef struct avm_align_out {
  int32_t* ok;        /* [B] the bool visualInitialAlign returns */
  double* delta_bg;   /* [B][3] */
  double* g_c0;       /* [B][3] g after RefineGravity, in c0 */
  double* x;          /* [B][3*max_frames+1] body-frame velocities of all frames, then s (already /100, :190-191) */
  double* g_world;    /* [B][3] R0 * g (:418); only written when windows != NULL */
  double* deltas;     /* nullable [B][max_frames-1][10]: delta p,q,v after the repropagation - parity surface */
} avm_align_out;

/* windows == NULL: exactly VisualIMUAlignment (initial_aligment.cpp:199-207) - solveGyroscopeBias, the repropagation of every interval
 * with (0, Bgs[0]), LinearAlignment, RefineGravity.  Bgs[0] is then the linearization bias of interval 0, imu_lin_bg[b][0].
 * windows != NULL: the whole of visualInitialAlign, in place on windows->pose, speedbias[.][.][0..2], speedbias[.][.][6..8] and
 * inv_depth; Bgs are speedbias[.][i][6..8].  A window with ok == 0 keeps its pose, velocities and depths; its gyro biases are still
 * incremented by delta_bg (the reference does that before it can fail).  G.norm() is the norm of opt->g, RIC the quaternion of
 * windows->ex_pose, INIT_DEPTH 5.0 (parameters.cpp:113).  ok, delta_bg, g_c0 and x must be given (g_world too with windows).
 *   x of a window with n_frames < max_frames: velocities at [0, 3 n_frames), zeros up to 3 max_frames, s at index 3 max_frames.
 *   x (s included), g_c0 and g_world of a window with ok == 0 are zero, wherever it failed; delta_bg and deltas are what was computed.
 * Quirks of the reference that are kept: RefineGravity never clears or un-scales its A and b between the four passes
 * (:63-66, :115-116); Vs[kv] = R_key(kv) * x.segment<3>(kv * 3) indexes x by the key-frame counter, not by the frame's position in
 * all_image_frame (estimator.cpp:397-406).
 * Deviations: the solves are Cholesky factorizations without pivoting.  Non-finite inputs, or a pivot that is not a positive finite
 * number, end THAT window with ok = 0 (delta_bg = 0 if it is the 3 x 3 system of the gyroscope bias) - Eigen's pivoted LDLT would
 * return some vector for a singular system, which the reference gives no meaning to.  n_frames < 4 (6 (F - 1) equations for 3 F + 4
 * unknowns) is refused the same way.  FromTwoVectors' antipodal branch (g along -z of c0; Eigen takes an SVD there) uses a unit axis
 * perpendicular to g, which is all that branch defines.
 * What the reference does next and this call cannot: it repropagates the window's pre_integrations with (0, Bgs[i]) (:391-394).  The
 * solve pre-integrates from the caller's const tables imu_lin_ba / imu_lin_bg: the caller sets imu_lin_ba = 0 and
 * imu_lin_bg[.][j] = speedbias[.][j][6..8] before the first avm_window_solve_batch.
 * Statuses: max_frames > AVM_MAX_ALIGN_FRAMES, or more windows than avm_config::max_windows (when that is > 0): AVM_ERR_CAPACITY;
 * n_frames / imu_n / key_index out of range or not increasing: AVM_ERR_INVALID before any kernel indexes with them.
 * avm_last_kernel_ms keys: "align_gyro_bias", "align_solve", "align_apply". */
int avm_visual_initial_align_batch(avm_ctx* ctx, const avm_options* opt, avm_mem mem, const avm_align_batch* align,
                                   avm_window_batch* windows /* nullable */, avm_align_out* out);

/* ---- SURVEY 8(f)4 + B4 (ground-truth mode): host-side format adapters.  Pure host bookkeeping like their
 * reference counterparts: no device work, no avm_ctx, usable without a GPU. ---------------------------------------- */

/* EuRoC ground-truth table with the reference's seek cursor (HorizonGenerator::truth_, seek_idx_, horizon_generator.h). */
typedef struct avm_gt avm_gt;
/* HorizonGenerator::loadGroundTruth (horizon_generator.cpp:169-196): first line = header, then
 * timestamp[ns], p(3), q(w x y z), v(3), w(3), a(3); the timestamp is stod(field) * 1e-9.  NULL on I/O / parse error. */
avm_gt* avm_gt_load_csv(const char* data_csv);
/* the same table from memory: rows [n][17], column 0 already in nanoseconds as a double */
avm_gt* avm_gt_from_rows(const double* rows, int32_t n);
void avm_gt_free(avm_gt* gt);
int32_t avm_gt_size(const avm_gt* gt);
int32_t avm_gt_seek(const avm_gt* gt); /* current seek_idx_ */
/* HorizonGenerator::groundTruth (horizon_generator.cpp:73-123) incl. getNextFrameTruth (:200-210): the H future poses
 * from the relative motion of the ground truth, starting at state k (timestamp, k_pos [3], k_quat [4] x y z w).
 * Stateful like the reference: the seek cursor only moves forward (and moves by at least one row per call).
 * Out: hor_pos [H+1][3], hor_quat [H+1][4] (x y z w; the products are not renormalized, as in the reference).
 * AVM_ERR_INVALID where the reference would read past the end of the table. */
int avm_fsel_horizon_ground_truth(avm_gt* gt, int32_t horizon, double timestamp_k, const double* k_pos, const double* k_quat,
                                  double delta_frame, double* hor_pos, double* hor_quat);

/* The feature message decode of estimator_node.cpp:303-321 (sensor_msgs::PointCloud -> image_t): points [n][3] float32
 * (geometry_msgs/Point32), channels[0..5] = id_of_point, u, v, velocity_x, velocity_y, probability (float32 each, [n]).
 * feature_id = int(ch0 + 0.5) / num_cam, camera_id = ... % num_cam; xyz_uv_velocity [n][8] = x y z u v vx vy prob.
 * Output in image_t order: ascending feature_id (std::map), message order within an id.  AVM_ERR_INVALID if a z != 1
 * (ROS_ASSERT(z == 1), :317). */
int avm_image_from_pointcloud(int32_t n_points, const float* points_xyz, const float* const* channels, int32_t num_cam,
                              int32_t* feature_id, int32_t* camera_id, double* xyz_uv_velocity);

/* A5/A6/A8 only: evaluate every factor once at the current state and return
 * residuals/Jacobians (local 6-column pose blocks).  Used by the per-factor parity tests.
 *   proj_r [B][max_obs][2], proj_J [B][max_obs][2][13]  (pose_i 6 | pose_j 6 | inv_depth 1), index = observation slot
 *   imu_r  [B][10][15],     imu_J  [B][10][15][30]      (pose_i 6 | sb_i 9 | pose_j 6 | sb_j 9)
 *   prior_res [B][max_prior]
 * robust loss (Cauchy) correction is applied to proj_* when apply_loss != 0. */
int avm_window_eval_factors(avm_ctx* ctx, const avm_options* opt, avm_mem mem,
                            const avm_window_batch* batch, int apply_loss, double* proj_r, double* proj_J,
                            double* imu_r, double* imu_J, double* prior_res, double* cost /* [B] */);

/* ---- HP-B: FeatureSelector::select() for a batch of independent frames ------- */
int avm_fsel_select_batch(avm_ctx* ctx, avm_mem mem, const avm_fsel_batch* batch, avm_fsel_out* out);
/* the single-call form, one FeatureSelector::select() (feature_selector.h:49-50): frame->n_problems == 1
 * (AVM_ERR_INVALID otherwise); selected_ids has room for frame->max_features ids (selection order), fvalues_opt may be NULL. */
int avm_fsel_select(avm_ctx* ctx, avm_mem mem, const avm_fsel_batch* frame, int32_t* selected_ids, int32_t* n_selected,
                    double* fvalues_opt);

/* how often this ctx's select calls had to fall back from the all-rounds-in-one-launch kernel (csrc/fsel/frame_kernel.hpp): counters since
 * avm_create.  out[0] = CALLS that had to be re-run in a slower mode (once per call), out[1] = LAUNCHES that reported a timed-out
 * wait or an unfinished frame (a call that falls two modes counts twice here), out[2] = the mode the next call starts in (2 = a
 * team per XCD, 1 = one team over all XCDs, 0 = one launch per round), out[3] = select calls so far.  A degraded call costs at most
 * the 20 ms spin time-out of the failed launch plus the slower mode's run time; the ctx probes the fast mode again after 16 calls,
 * and after 32, 64 ... 4096 if the probes keep failing (back to 16 once a fast-mode call has gone through). */
int avm_fsel_fallback_stats(const avm_ctx* ctx, int64_t out[4]);

/* B8, second half as a parity surface: FeatureSelector::findNNDepth (feature_selector.cpp:437-459) for every candidate of every
 * frame - the depth of the cloud point the reference's kd-tree search returns for the candidate on the normalized plane (exact
 * 1-NN, squared Euclidean distance as nanoflann's L2_Simple_Adaptor, feature_selector.h:143; 1.0 for an empty cloud,
 * feature_selector.cpp:444).  depth [P][max_cand] (entries beyond n_cand: 0).  The same search runs inside
 * avm_fsel_select_batch / avm_fsel_information; this entry exists so that it can be checked against the reference's own nanoflann
 * (tests/golden/nanoflann_nn.npz, nanoflann_nn2.npz).  Round 5: the tree is built and walked as nanoflann builds and walks it
 * (csrc/fsel/kdtree.hpp: fsel_kdtree_kernel, kd_depth), so among cloud points at bit-identical distances the answer is nanoflann's too - the
 * point its traversal meets first; every query of the two fixtures is answered bit for bit.  max_cloud <= 4096 (the tree is built in LDS). */
int avm_fsel_nn_depth(avm_ctx* ctx, avm_mem mem, const avm_fsel_batch* batch, double* depth);

/* B5/B6 only: Omega_kkH (+prior) [P][N][N] and compact Delta_ell position blocks
 * [P][max_cand][3H][3H] (+ valid flag [P][max_cand]); for parity tests. */
int avm_fsel_information(avm_ctx* ctx, avm_mem mem, const avm_fsel_batch* batch, double* omega,
                         double* delta_cand, int32_t* cand_valid);

/* ---- multi-GPU: windows and selector frames are independent, so a job is one process per GPU, each with its
 * own ctx and a contiguous block of the work; the only exchange is a gather of the final states.  The library owns a raw
 * RCCL communicator for it (rccl.h over xGMI; librccl.so.1 is dlopen'ed on first use, a single-GPU host never loads it).
 *   avm_comm_unique_id   rank 0 creates the 128-byte ncclUniqueId; the caller carries it to the other ranks (any channel)
 *   avm_comm_init        collective over all ranks: ncclCommInitRank on this ctx's device
 *   avm_gather_states    ncclAllGather of `count` doubles per rank, device pointers, on the ctx stream; returns when done.
 *                        recv is [n_ranks][count]; rank r's block lands at recv + r * count on every rank
 *   avm_comm_destroy     (also done by avm_destroy) */
#define AVM_COMM_ID_BYTES 128
int avm_comm_unique_id(avm_ctx* ctx, void* id /* AVM_COMM_ID_BYTES */);
int avm_comm_init(avm_ctx* ctx, int32_t n_ranks, int32_t rank, const void* id);
int avm_gather_states(avm_ctx* ctx, const double* send, double* recv, size_t count);
int avm_comm_destroy(avm_ctx* ctx);

/* the HIP stream (hipStream_t) every call on this ctx is enqueued on, for callers that produce device-resident inputs
 * on streams of their own (see "stream ordering" above) */
int avm_ctx_stream(const avm_ctx* ctx, void** stream);

/* ---- timing of the last call on the ctx stream (HIP events), milliseconds ---- */
int avm_last_kernel_ms(const avm_ctx* ctx, const char* which, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* AVM_H_ */
