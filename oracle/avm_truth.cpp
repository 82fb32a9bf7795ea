// oracle/avm_truth.cpp - TEST INFRASTRUCTURE ONLY.  The extended-precision ARBITER of the marginalization parity tests
// (VERDICT round 2, item 2): the oracle's own restatement of
//   MarginalizationInfo::addResidualBlockInfo / preMarginalize / marginalize   marginalization_factor.cpp:89-297
//   as driven by Estimator::optimization()                                       estimator.cpp:817-990
// (oracle/solver.hpp: marginalize(), with the factors of oracle/factors.hpp and the Eigen restatements of linalg.hpp)
// compiled with __float128 as the scalar type.  It follows the reference's algorithm literally - the joint
// SelfAdjointEigenSolver pseudo-inverse of Amm with the 1e-8 clamp (:267-272), the Schur complement (:275-281), the eigen
// square root (:283-291) - on the SAME FP64 inputs (states, observations, raw IMU samples, the old prior), from the
// pre-integration on.  With a unit roundoff of 1e-34 against entries that span 1e12 its rounding noise (1e-22) is far below
// the 1e-8 clamp and below anything FP64 can resolve: its result, rounded once to FP64 at the very end, is the value the
// reference's algorithm DEFINES for these inputs.  The FP64 oracle and the GPU are both measured against it.
//
// Nothing under anticipated-vins-mono_amd/ may include, link or call this file.
#include "quad_prelude.hpp"

#include "window_io.hpp"  // (-> solver.hpp -> factors.hpp -> linalg.hpp, all in the wide scalar type from here on)
#include "fsel_io.hpp"    // (-> fsel.hpp)
#include "triangulate.hpp"

#undef double

using namespace avmo;

extern "C" {

// The marginalization of window w of the batch at the state the batch holds (what avmo_window_solve_batch does after a solve
// with max_num_iterations = 0, minus the gauge-fix round trip, which is the identity on these states up to rounding).
// Outputs (all FP64, rounded from binary128 at the end; any pointer may be NULL):
//   n_out, nblk_out, blk_kind / blk_frame [max_pblk], x0 [max_pblk][9]
//   J [n][n] row-major linearized_jacobians, r [n] linearized_residuals          (eigenvector signs are arbitrary)
//   H [n][n] = J^T J, g [n] = J^T r, cost = 1/2 |r|^2                             (what a consumer of the prior sees)
//   A [n][n], b [n]: the Schur complement before the square root
//   ev_mm [cap_mm], n_mm: eigenvalues of Amm (ascending); ev_rr [n]: eigenvalues of the Schur complement
// returns 0, or -1 when MARGIN_SECOND_NEW has nothing to drop (the old prior stays, estimator.cpp:926-927).
int avmt_marginalize(const avm_options* opt, const avm_window_batch* batch, int w, int max_pblk, int32_t* n_out, int32_t* nblk_out,
                     int32_t* blk_kind, int32_t* blk_frame, double* x0, double* J, double* r, double* H, double* g, double* cost,
                     double* A, double* b, double* ev_mm, int cap_mm, int32_t* n_mm, double* ev_rr) {
  Window W;
  load_window(*opt, *batch, w, W);
  Prior np;
  MargDiag D;
  marginalize(W, W.x, *opt, np, &D);
  if (n_out) *n_out = np.n;
  if (np.n < 0) return -1;
  const int n = np.n, nb = (int)np.blk_kind.size();
  if (nblk_out) *nblk_out = nb;
  for (int k = 0; k < nb && k < max_pblk; k++) {
    if (blk_kind) blk_kind[k] = np.blk_kind[k];
    if (blk_frame) blk_frame[k] = np.blk_frame[k];
    if (x0)
      for (size_t q = 0; q < np.x0[k].size(); q++) x0[(size_t)k * 9 + q] = (double)np.x0[k][q];
  }
  for (int i = 0; i < n; i++) {
    if (r) r[i] = (double)np.r[i];
    for (int j = 0; j < n; j++) {
      if (J) J[(size_t)i * n + j] = (double)np.J(i, j);
      if (A) A[(size_t)i * n + j] = (double)D.A_rr(i, j);
    }
    if (b) b[i] = (double)D.b_rr[i];
    if (ev_rr) ev_rr[i] = (double)D.ev_rr[i];
  }
  if (H || g || cost) {
    avmo_real c = 0;
    for (int i = 0; i < n; i++) {
      c += np.r[i] * np.r[i];
      avmo_real gi = 0;
      for (int k = 0; k < n; k++) gi += np.J(k, i) * np.r[k];
      if (g) g[i] = (double)gi;
      if (H)
        for (int j = 0; j < n; j++) {
          avmo_real h = 0;
          for (int k = 0; k < n; k++) h += np.J(k, i) * np.J(k, j);
          H[(size_t)i * n + j] = (double)h;
        }
    }
    if (cost) *cost = (double)(c / 2);
  }
  if (n_mm) *n_mm = D.m;
  if (ev_mm)
    for (int i = 0; i < D.m && i < cap_mm; i++) ev_mm[i] = (double)D.ev_mm[i];
  return 0;
}

// The solve of window w in the wide scalar type: Problem::build + trust_region_solve (the restated Ceres 1.14 dogleg minimizer,
// oracle/solver.hpp) + the gauge-fix round trip of double2vector (estimator.cpp:206-284), from the pre-integration on, on the
// same FP64 inputs.  What comes back, rounded once to FP64, is the state the reference's ALGORITHM defines for these inputs when
// no arithmetic error is made on the way; the FP64 oracle and the GPU are both measured against it (tests/test_solve_truth.py).
// Outputs (any pointer may be NULL): pose [11][7], speedbias [11][9], ex_pose [7], td [1], relo_pose [7], inv_depth [n_feat];
// summary: the oracle's record (costs, iterations, termination), its doubles rounded from binary128.
int avmt_solve(const avm_options* opt, const avm_window_batch* batch, int w, double* pose, double* speedbias, double* ex_pose, double* td,
               double* relo_pose, double* inv_depth, avm_solve_summary* summary) {
  Window W;
  load_window(*opt, *batch, w, W);
  Problem P;
  P.build(W, *opt);
  SolveResult R = trust_region_solve(P, W.x);
  State out;
  out.lam = R.x.lam;
  gauge_fix_roundtrip(W.x, R.x, out, W.failure_occur ? W.last_pose0 : nullptr, W.has_relo);
  for (int f = 0; f < AVM_NFRAMES; f++) {
    if (pose)
      for (int k = 0; k < 7; k++) pose[f * 7 + k] = (double)out.pose[f][k];
    if (speedbias)
      for (int k = 0; k < 9; k++) speedbias[f * 9 + k] = (double)out.sb[f][k];
  }
  for (int k = 0; k < 7; k++) {
    if (ex_pose) ex_pose[k] = (double)out.ex[k];
    if (relo_pose && W.has_relo) relo_pose[k] = (double)out.relo[k];
  }
  if (td) *td = (double)out.td;
  if (inv_depth)
    for (size_t e = 0; e < out.lam.size(); e++) inv_depth[e] = (double)out.lam[e];
  if (summary) *summary = R.sum;
  return 0;
}

// The same solve with its result handed out BEYOND FP64: Ceres' own solution (before double2vector's gauge fix) as pose [11][7] |
// speed-bias [11][9] | inverse depths [n_feat] | ex_pose [7] | td [1] | relo_Pose [7], and the cost at the start point and at the solution, each as a double-double pair
// hi + lo (the binary128 value to 32 digits), followed by the cost after every iteration.  For tests/test_solve_trace_mp.py: the 50-digit run of the independent numpy minimizer
// (tests/golden/gen_solve_trace_mp.py) against this restatement.  cost_hi / cost_lo: [2 + AVM_MAX_ITER_TRACE]; returns the number of iterations.
int avmt_solve_dd(const avm_options* opt, const avm_window_batch* batch, int w, double* x_hi, double* x_lo, double* cost_hi, double* cost_lo,
                  int32_t* accept_mask) {
  Window W;
  load_window(*opt, *batch, w, W);
  Problem P;
  P.build(W, *opt);
  SolveResult R = trust_region_solve(P, W.x);
  auto put = [](avmo_real v, double* hi, double* lo) {
    *hi = (double)v;
    *lo = (double)(v - (avmo_real)*hi);
  };
  size_t q = 0;
  for (int f = 0; f < AVM_NFRAMES; f++)
    for (int k = 0; k < 7; k++, q++) put(R.x.pose[f][k], x_hi + q, x_lo + q);
  for (int f = 0; f < AVM_NFRAMES; f++)
    for (int k = 0; k < 9; k++, q++) put(R.x.sb[f][k], x_hi + q, x_lo + q);
  for (size_t e = 0; e < R.x.lam.size(); e++, q++) put(R.x.lam[e], x_hi + q, x_lo + q);
  for (int k = 0; k < 7; k++, q++) put(R.x.ex[k], x_hi + q, x_lo + q);   // (the optional members: constants of the base problem)
  put(R.x.td, x_hi + q, x_lo + q), q++;
  for (int k = 0; k < 7; k++, q++) put(R.x.relo[k], x_hi + q, x_lo + q);
  put(P.evaluate(W.x, false), cost_hi, cost_lo);
  put(P.evaluate(R.x, false), cost_hi + 1, cost_lo + 1);
  for (size_t k = 0; k < R.cost_after.size(); k++) put(R.cost_after[k], cost_hi + 2 + k, cost_lo + 2 + k);
  if (accept_mask) *accept_mask = R.sum.accept_mask;
  return R.sum.num_iterations;
}

// The pre-integration of the ten intervals of window w in the wide scalar type: PreIntegration::push_back over the raw samples and
// imu_sqrt_info, as load_window runs them per interval (oracle/window_io.hpp) - from the batch's imu_* tables and the options' noise
// densities alone, so a batch without features (or without any other table) is fine.  The sample loop is load_window's, repeated here
// and not shared with it: the FP64 build of that header decides its fused multiply-adds by how load_window is inlined, a helper called
// from both moved the last bits of the FP64 oracle's covariances and, through them, every stream test that amplifies them.
// Every output is rounded once to FP64 (the `hi` array) and, where the `lo` array is given, followed by lo = (double)(x - hi): the pair
// carries the binary128 value to 32 digits (tests/test_preint_truth.py against tests/golden/preint_mp.npz).  Per interval: delta [10]
// in the ABI's order p | qx qy qz qw | v, jacobian [225], covariance [225], sum_dt [1], sqrt_info [225].  Any pointer may be NULL.
int avmt_imu_preintegrate(const avm_options* opt, const avm_window_batch* batch, int w, double* delta_hi, double* delta_lo,
                          double* jacobian_hi, double* jacobian_lo, double* covariance_hi, double* covariance_lo, double* sum_dt_hi,
                          double* sum_dt_lo, double* sqrt_info_hi, double* sqrt_info_lo) {
  const avm_window_batch& B = *batch;
  auto put = [](avmo_real v, double* hi, double* lo, size_t at) {
    const double h = (double)v;
    if (hi) hi[at] = h;
    if (lo) lo[at] = (double)(v - (avmo_real)h);
  };
  ImuNoise nz{opt->acc_n, opt->gyr_n, opt->acc_w, opt->gyr_w};
  for (int j = 0; j < AVM_WINDOW_SIZE; j++) {
    const size_t iv = (size_t)w * AVM_WINDOW_SIZE + j;
    const auto* acc = B.imu_acc + iv * (B.max_samp + 1) * 3;
    const auto* gyr = B.imu_gyr + iv * (B.max_samp + 1) * 3;
    const auto* dt = B.imu_dt + iv * B.max_samp;
    const auto* lba = B.imu_lin_ba + iv * 3;
    const auto* lbg = B.imu_lin_bg + iv * 3;
    PreIntegration p(V3(acc[0], acc[1], acc[2]), V3(gyr[0], gyr[1], gyr[2]), V3(lba[0], lba[1], lba[2]), V3(lbg[0], lbg[1], lbg[2]), nz);
    const int ns = B.imu_n[iv];
    for (int s = 0; s < ns; s++)
      p.push_back(dt[s], V3(acc[3 * (s + 1)], acc[3 * (s + 1) + 1], acc[3 * (s + 1) + 2]),
                  V3(gyr[3 * (s + 1)], gyr[3 * (s + 1) + 1], gyr[3 * (s + 1) + 2]));
    const avmo_real d[10] = {p.delta_p.x, p.delta_p.y, p.delta_p.z, p.delta_q.x, p.delta_q.y, p.delta_q.z, p.delta_q.w,
                             p.delta_v.x, p.delta_v.y, p.delta_v.z};
    for (int k = 0; k < 10; k++) put(d[k], delta_hi, delta_lo, (size_t)j * 10 + k);
    put(p.sum_dt, sum_dt_hi, sum_dt_lo, (size_t)j);
    for (int k = 0; k < 225; k++) {
      put(p.jacobian.a[k], jacobian_hi, jacobian_lo, (size_t)j * 225 + k);
      put(p.covariance.a[k], covariance_hi, covariance_lo, (size_t)j * 225 + k);
    }
    if (sqrt_info_hi || sqrt_info_lo) {
      const Mat U = imu_sqrt_info(p);
      for (int k = 0; k < 225; k++) put(U.a[k], sqrt_info_hi, sqrt_info_lo, (size_t)j * 225 + k);
    }
  }
  return 0;
}

// ---- the small per-feature / per-window / per-factor operations around the solve (tests/test_window_ops_truth.py) ----------------------
// Each is the oracle's own function (triangulate.hpp, factors.hpp) on the same FP64 tables, converted exactly; each output is rounded
// once to FP64 (`hi`) and, where a `lo` array is given, followed by lo = (double)(x - hi).  Any output pointer may be NULL.
namespace {
struct HiLo {
  static void put(avmo_real v, double* hi, double* lo, size_t at) {
    const double h = (double)v;
    if (hi) hi[at] = h;
    if (lo) lo[at] = (double)(v - (avmo_real)h);
  }
};
}  // namespace

// FeatureManager::triangulate of feature e of window w (triangulate_feature; its Hestenes sweep converges to binary128's roundoff,
// AVMO_SVD_TOL of quad_prelude.hpp): ratio = v[2] / v[3] as it comes out of the SVD, depth = the same after `< 0.1 -> init_depth`,
// sigma [4] the singular values of the (2 nobs) x 4 system in descending order, V [4][4] its right singular vectors (column k belongs
// to sigma[k]; the last column is v, up to the sign the sweep happened to give it).  Whatever inv_depth holds for the feature is not read.
int avmt_triangulate(const avm_window_batch* batch, int w, int e, double init_depth, double* ratio_hi, double* ratio_lo, double* depth_hi,
                     double* depth_lo, double* sigma_hi, double* sigma_lo, double* V_hi, double* V_lo) {
  const avm_window_batch& B = *batch;
  if (w < 0 || w >= B.n_windows || e < 0 || e >= B.max_feat) return -1;
  const size_t k = (size_t)w * B.max_feat + e;
  const int start = B.feat_start[k], nobs = B.feat_nobs[k];
  if (start < 0 || nobs < 1 || start + nobs > AVM_NFRAMES) return -1;
  avmo_real pose[AVM_NFRAMES][7], ex[7];
  for (int f = 0; f < AVM_NFRAMES; f++)
    for (int c = 0; c < 7; c++) pose[f][c] = B.pose[((size_t)w * AVM_NFRAMES + f) * 7 + c];
  for (int c = 0; c < 7; c++) ex[c] = B.ex_pose[(size_t)w * 7 + c];
  std::vector<avmo_real> obs((size_t)2 * nobs);
  const auto* src = B.obs_xy + ((size_t)w * B.max_obs + B.feat_obs_begin[k]) * 2;
  for (int c = 0; c < 2 * nobs; c++) obs[c] = src[c];
  TriDetail D;
  tri_detail() = &D;
  const avmo_real depth = triangulate_feature(pose, ex, start, nobs, obs.data(), (avmo_real)init_depth);
  tri_detail() = nullptr;
  HiLo::put(D.ratio, ratio_hi, ratio_lo, 0);
  HiLo::put(depth, depth_hi, depth_lo, 0);
  for (int c = 0; c < 4; c++) HiLo::put(D.sig[c], sigma_hi, sigma_lo, c);
  for (int c = 0; c < 16; c++) HiLo::put(D.V[c], V_hi, V_lo, c);
  return 0;
}

// Estimator::processIMU's dead-reckoning of the newest frame (propagate_newest_frame) on interval 9 of window w, from pose [10] and
// speedbias [10] of the batch and gravity g: pose_out [7] (p | qx qy qz qw), sb_out [9] (v, and the biases as they went in).
int avmt_imu_propagate(const avm_window_batch* batch, int w, const double* g, double* pose_hi, double* pose_lo, double* sb_hi, double* sb_lo) {
  const avm_window_batch& B = *batch;
  if (w < 0 || w >= B.n_windows) return -1;
  const size_t iv = (size_t)w * AVM_WINDOW_SIZE + (AVM_WINDOW_SIZE - 1);
  const int n = B.imu_n[iv];
  if (n < 0 || n > B.max_samp) return -1;
  avmo_real pose[7], sb[9];
  for (int c = 0; c < 7; c++) pose[c] = B.pose[((size_t)w * AVM_NFRAMES + AVM_WINDOW_SIZE) * 7 + c];
  for (int c = 0; c < 9; c++) sb[c] = B.speedbias[((size_t)w * AVM_NFRAMES + AVM_WINDOW_SIZE) * 9 + c];
  std::vector<avmo_real> dt(n), acc((size_t)3 * (n + 1)), gyr((size_t)3 * (n + 1));
  for (int s = 0; s < n; s++) dt[s] = B.imu_dt[iv * B.max_samp + s];
  for (int c = 0; c < 3 * (n + 1); c++) acc[c] = B.imu_acc[iv * (B.max_samp + 1) * 3 + c], gyr[c] = B.imu_gyr[iv * (B.max_samp + 1) * 3 + c];
  propagate_newest_frame(pose, sb, n, dt.data(), acc.data(), gyr.data(), V3(g[0], g[1], g[2]));
  for (int c = 0; c < 7; c++) HiLo::put(pose[c], pose_hi, pose_lo, c);
  for (int c = 0; c < 9; c++) HiLo::put(sb[c], sb_hi, sb_lo, c);
  return 0;
}

// ProjectionTdFactor::Evaluate of factor i of the batch (projection_td_factor_evaluate): residual [2], jac [2][20].
int avmt_projection_td_eval(const avm_td_factor_batch* f, int i, double* residual_hi, double* residual_lo, double* jac_hi, double* jac_lo) {
  if (i < 0 || i >= f->n) return -1;
  auto two = [&](const double* p, avmo_real out[2]) { out[0] = p[2 * i], out[1] = p[2 * i + 1]; };
  auto seven = [&](const double* p, avmo_real out[7]) {
    for (int c = 0; c < 7; c++) out[c] = p[7 * (size_t)i + c];
  };
  avmo_real pts_i[2], pts_j[2], vel_i[2], vel_j[2], pose_i[7], pose_j[7], ex[7], r[2], J[40];
  two(f->pts_i, pts_i), two(f->pts_j, pts_j), two(f->vel_i, vel_i), two(f->vel_j, vel_j);
  seven(f->pose_i, pose_i), seven(f->pose_j, pose_j), seven(f->ex_pose, ex);
  const bool want_jac = jac_hi || jac_lo;
  projection_td_factor_evaluate(pts_i, pts_j, vel_i, vel_j, f->td_i[i], f->td_j[i], f->row_i[i], f->row_j[i], f->tr, f->row,
                                (avmo_real)(f->focal_length / 1.5) /* sqrt_info is an FP64 constant (estimator.cpp:17) */, pose_i, pose_j, ex, f->inv_depth[i], f->td[i], r,
                                want_jac ? J : nullptr);
  for (int c = 0; c < 2; c++) HiLo::put(r[c], residual_hi, residual_lo, c);
  if (want_jac)
    for (int c = 0; c < 40; c++) HiLo::put(J[c], jac_hi, jac_lo, c);
  return 0;
}

// FeatureSelector::select of frame p of the batch in the wide scalar type (oracle/fsel.hpp: calcInfoFromRobotMotion,
// calcInfoFromFeatures, the lazy greedy of selectInformativeFeatures with sortedlogDetUB's std::map, Utility::logdet by Cholesky -
// feature_selector.cpp:239-728): the ids the reference's algorithm selects when no logdet comparison is decided by rounding.
// selected_ids [max_features], fvalues [max_features] (rounded to FP64; may be NULL); returns the number selected.
int avmt_fsel_select(const avm_fsel_batch* batch, int p, int32_t* selected_ids, double* fvalues) {
  FselProblem P;
  load_fsel(*batch, p, P);
  FselResult R = fsel_select(P);
  for (size_t i = 0; i < R.selected.size(); i++) {
    selected_ids[i] = R.selected[i];
    if (fvalues) fvalues[i] = (double)R.fvalues[i];
  }
  return (int)R.selected.size();
}

// Omega (calcInfoFromRobotMotion incl. addOmegaPrior) [N][N] and every candidate's Delta [max_cand][N][N] (zero when the
// candidate is not triangulable) of frame p, formed in binary128 and rounded to FP64 (either pointer may be NULL).
int avmt_fsel_information(const avm_fsel_batch* batch, int p, double* omega, double* delta_full) {
  FselProblem P;
  load_fsel(*batch, p, P);
  const int N = 9 * (P.H + 1);
  Mat Om = calcInfoFromRobotMotion(P);
  if (omega)
    for (int i = 0; i < N * N; i++) omega[i] = (double)Om.a[i];
  if (delta_full) {
    std::map<int, Mat> D = calcInfoFromFeatures(P, P.cand_id, P.cand_x, P.cand_y);
    for (size_t c = 0; c < P.cand_id.size(); c++) {
      auto it = D.find(P.cand_id[c]);
      for (int i = 0; i < N * N; i++) delta_full[c * N * N + i] = it == D.end() ? 0.0 : (double)it->second.a[i];
    }
  }
  return 0;
}

int avmt_digits(void) { return FLT128_DIG; }

}  // extern "C"
