/* avm_init.h - the initialisation phase: the deterministic half of Estimator::initialStructure on the device.
 *
 * GlobalSFM::construct (initial/initial_sfm.cpp:117-312) and "solve pnp for all frame" (estimator.cpp:277-344) for B streams in one
 * call.  relativePose (OpenCV's RANSAC on OpenCV's RNG) stays with the caller: its result (l, relative_R, relative_T) is an input.
 * What follows, visualInitialAlign, is avm_visual_initial_align_batch of avm.h; the two calls chain on the device (below).
 * This header adds to avm.h: AVM_ABI_VERSION stays as it is and no struct of avm.h changes.
 *
 * The statement this call is tested against is tests/golden/gen_global_sfm.py.  Deviations from the reference, all of
 * them the statement's readings:
 *   - cv::solvePnP(useExtrinsicGuess, ITERATIVE) is CvLevMarq on 6 parameters with K = I: points and observations enter as
 *     (double)(float)x, cvRodrigues2 without its SVD re-orthonormalisation (theta = pi fails the call), lambda from 1e-3 with
 *     1 + lambda on the diagonal, a step that makes the error grow retried with lambda * 10, 20 kept steps or
 *     |dparam| / |param| < FLT_EPSILON.  The 6 x 6 solve is a Cholesky factorization where OpenCV takes an SVD: a pivot that is not
 *     positive fails the call.
 *   - GlobalSFM::triangulatePoint takes the last right singular vector from a one-sided Jacobi SVD (Eigen: JacobiSVD).
 *   - The BA is Ceres' TrustRegionMinimizer with LEVENBERG_MARQUARDT and DENSE_SCHUR at its defaults, restated: Jacobi scaling fixed at
 *     the first point, D^2 = clamp(diag) / radius, analytic Jacobians, the points eliminated one 3 x 3 block at a time, the reduced
 *     camera system solved by a Cholesky factorization.  There is NO wall-clock cap (the reference sets 0.2 s): the iteration cap alone
 *     ends it, so a result never depends on the machine's load.  ba_max_solver_time_s must be 0.
 *   - Sums run in the device's fixed order (per thread by index, then a fixed reduction tree) with FMA contraction: results agree with the
 *     statement's FP64 run to rounding, and are the same bits from call to call, for any batch, position in the batch and strides.
 */
#ifndef AVM_INIT_H_
#define AVM_INIT_H_

#include "avm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct avm_sfm_batch {            /* one row per stream; tables as buffers.SfmArrays / synth.make_sfm lay them out */
  int32_t n_windows, max_frames, max_pts, ba_max_num_iterations;
  double  ba_max_solver_time_s;           /* must be 0 (no cap) in this version; anything else: AVM_ERR_INVALID */
  const int32_t *l, *n_frames, *key_index /*[B,11]*/, *frame_n_pts /*[B,max_frames]*/, *frame_pt_id /*[B,max_frames,max_pts]*/;
  const double  *relative_R /*[B,9]*/, *relative_T /*[B,3]*/, *frame_pt_xy /*[B,max_frames,max_pts,2]*/;
} avm_sfm_batch;

typedef struct avm_sfm_out {
  int32_t *ok;            /* [B] 0, or 1..4 as DESIGN.md 2.24 / the statement define them */
  double  *frame_R, *frame_T;   /* [B,max_frames,9] / [B,max_frames,3]: layout of avm_align_batch::frame_R / frame_T */
  double  *q, *T;         /* [B,11,4] (w x y z) / [B,11,3] after the BA */
  double  *point;         /* [B,max_feat,3] */
  int32_t *point_state;   /* [B,max_feat] */
  int32_t *ba_counts;     /* [B,3] iterations, successful steps, termination (the statement's TERM codes) */
  double  *ba_cost;       /* [B,2] initial, final */
  double  *pnp_q, *pnp_t; /* optional (NULL allowed): the chain's camera poses before the BA, [B,11,4] / [B,11,3] */
} avm_sfm_out;

/* ok per stream: 0 success; 1 a frame of the chain has fewer than 10 triangulated points or its PnP fails; 2 the BA neither converged
 * nor ended below a cost of 5e-3; 3 a non-key frame has fewer than 6 known points or its PnP fails; 4 relative_R / relative_T or a final
 * frame pose is not finite.  Non-finite input is no refusal: it ends that stream alone with a non-zero ok (every loop is bounded by its
 * iteration cap), the other streams' results do not change by a bit.
 *
 * Tables read from `full`, the whole f_manager.feature list with the wide strides (max_feat <= AVM_MAX_FEAT_WIDE, max_obs <=
 * AVM_MAX_OBS_WIDE): n_feat, feat_start, feat_nobs, feat_obs_begin, obs_xy, ex_pose.  Nothing is written into it.  feat_id [B,max_feat]:
 * the features' ids (in `mem` space); it need not ascend, the first row with an id wins.
 *
 * Written per stream: ok always; ba_counts / ba_cost once the BA ran (ok != 1, 4-at-the-start); pnp_q / pnp_t once the chain completed;
 * q, T, point, point_state (rows below n_feat) when ok is 0 or 3; frame_R / frame_T (rows below n_frames) only when ok == 0.  Every
 * other row is left as the caller passed it.
 *
 * Chaining: frame_R / frame_T may be the very pointers of the avm_align_batch handed to avm_visual_initial_align_batch next, on the
 * same ctx (or ordered against avm_ctx_stream()): no host trip in between.  A stream whose SfM failed leaves its rows as they were;
 * the caller makes the alignment refuse such a stream (ok = 0) through what it prefilled there - non-finite frame_R does it.
 *
 * A bad batch is refused as a whole before any kernel indexes with the tables: AVM_ERR_INVALID, avm_last_error names the first stream
 * and rule, nothing is written.  Rules: l within 0..9; 11 <= n_frames <= max_frames; key_index strictly ascending within [0, n_frames);
 * 0 <= frame_n_pts <= max_pts and frame_pt_id strictly ascending within a frame (frames below n_frames); ba_max_num_iterations >= 1;
 * ba_max_solver_time_s == 0; the track tables as every call checks them.  AVM_ERR_CAPACITY: max_frames > AVM_MAX_ALIGN_FRAMES, max_pts >
 * AVM_MAX_IMAGE_PTS, the strides of `full` beyond the wide limits, more streams than avm_config::max_windows (when that is > 0).
 * n_windows == 0 returns AVM_OK.  AVM_MEM_HOST and AVM_MEM_DEVICE give the same bytes.
 * avm_last_kernel_ms keys: "sfm_chain_ba", "sfm_frame_pnp". */
int avm_global_sfm_batch(avm_ctx* ctx, avm_mem mem, const avm_sfm_batch* sfm, const avm_window_batch* full, const int32_t* feat_id,
                         avm_sfm_out* out);

#ifdef __cplusplus
}
#endif
#endif /* AVM_INIT_H_ */
