// solve/eval_factors_kernel.hpp - per-factor evaluation kernel (latency build only)
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// Per-factor evaluation at the input state (no solve): parity-test surface for A5/A6/A8.
__global__ __launch_bounds__(NT) void eval_factors_kernel(EvalArgs A) {
  lds_base_check();
  double* lds = LDS();
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  const int t = threadIdx.x;
  const avm_options& o = lds_opt();
  const avm_window_batch& B = A.b;
  const int w = blockIdx.x;
  WinCtx cl;
  cl.sc = nullptr, cl.osf = nullptr, cl.w = w;
  cl.nf = B.n_feat[w];
  cl.obs = as_global(B.obs_xy + (size_t)w * B.max_obs * 2);
  cl.pdelta = as_global(A.pre_delta + (size_t)w * 100), cl.pjac = as_global(A.pre_jac + (size_t)w * 2250), cl.psqrt = as_global(A.pre_sqrt + (size_t)w * 2250);
  cl.psum = as_global(A.pre_sum_dt + (size_t)w * 10);
  cl.lba = as_global(B.imu_lin_ba + (size_t)w * 30), cl.lbg = as_global(B.imu_lin_bg + (size_t)w * 30);
  cl.pn = B.prior_n ? B.prior_n[w] : 0;
  cl.pnblk = cl.pn > 0 ? B.prior_nblk[w] : 0;
  cl.ldp = B.max_prior;
  cl.pJ = as_global(B.prior_J + (size_t)w * B.max_prior * B.max_prior);
  cl.pr = as_global(B.prior_r + (size_t)w * B.max_prior);
  cl.px0 = as_global(B.prior_x0 + (size_t)w * B.max_pblk * 9);
  cl.prof = nullptr, cl.cov = nullptr, cl.nobs_tot = 0;
  lds_store_ctx(cl, A.opt);
  __syncthreads();
  const WinCtx& c = lds_ctx();
  for (int i = t; i < 77; i += NT) lds[L_X + i] = B.pose[(size_t)w * 77 + i];
  for (int i = t; i < 99; i += NT) lds[L_X + XSB + i] = B.speedbias[(size_t)w * 99 + i];
  for (int i = t; i < MAXE; i += NT) lds[L_X + XLAM + i] = i < c.nf ? B.inv_depth[(size_t)w * B.max_feat + i] : 1.0;
  for (int i = t; i < MAXPRIOR; i += NT) lds[L_DXP + i] = 0.0, lds[L_RP + i] = 0.0;
  for (int i = t; i < 10 * 465; i += NT) lds[L_S + i] = 0.0;
  if (t < 7) lds[L_RIC + 12 + t] = B.ex_pose[(size_t)w * 7 + t];
  if (t == 0) {
    const double* ex = B.ex_pose + (size_t)w * 7;
    double R[9];
    q2R(quat{ex[6], ex[3], ex[4], ex[5]}, R);
    for (int k = 0; k < 9; k++) lds[L_RIC + k] = R[k];
    for (int k = 0; k < 3; k++) lds[L_RIC + 9 + k] = ex[k];
    int off = 0;
    for (int k = 0; k < c.pnblk; k++) {
      const int kind = B.prior_blk_kind[(size_t)w * B.max_pblk + k], fr = B.prior_blk_frame[(size_t)w * B.max_pblk + k];
      ids[I_PBLK + k * 3] = kind, ids[I_PBLK + k * 3 + 1] = fr, ids[I_PBLK + k * 3 + 2] = off;
      off += kind == AVM_BLK_SPEEDBIAS ? 9 : 6;
    }
  }
  __syncthreads();
  build_frames(L_X, 0);
  __syncthreads();
  Frames fr{lds + L_FR, lds + L_FR + 99};
  const double sqi = o.focal_length / 1.5;
  double acc = 0;
  if (t >= NT - 64 && t < NT - 64 + 10) {
    const int i = t - (NT - 64);
    imu_raw<true>(lds + L_X, fr.R, o, c.pdelta + i * 10, c.pjac + i * 225, c.psum[i], c.lba + i * 3, c.lbg + i * 3, i, lds + L_S + i * 465);
  }
  for (int e = 0; e < c.nf; e++) {  // thread per observation of feature e
    const int s0 = B.feat_obs_begin[(size_t)w * B.max_feat + e], no = B.feat_nobs[(size_t)w * B.max_feat + e];
    const int fa = B.feat_start[(size_t)w * B.max_feat + e];
    for (int k = 1 + t; k < no; k += NT) {
      const int s = s0 + k;
      double r[2], Ji[12], Jj[12], Je[2];
      acc += proj_eval<true>(lds + L_X, fr, lds + L_RIC, lds + L_RIC + 9, c.obs[2 * s0], c.obs[2 * s0 + 1], c.obs[2 * s], c.obs[2 * s + 1],
                             lds[L_X + XLAM + e], fa, fa + k, sqi, o.cauchy_a, A.apply_loss != 0, r, Ji, Jj, Je);
      const size_t ob = (size_t)w * B.max_obs + s;
      if (A.proj_r) A.proj_r[ob * 2] = r[0], A.proj_r[ob * 2 + 1] = r[1];
      if (A.proj_J)
        for (int rr = 0; rr < 2; rr++) {
          for (int q = 0; q < 6; q++) A.proj_J[ob * 26 + rr * 13 + q] = Ji[rr * 6 + q], A.proj_J[ob * 26 + rr * 13 + 6 + q] = Jj[rr * 6 + q];
          A.proj_J[ob * 26 + rr * 13 + 12] = Je[rr];
        }
    }
  }
  __syncthreads();
  for (int idx = t; idx < 10 * 465; idx += NT) {
    const int i = idx / 465, rc = idx % 465, r = rc / 31, cc = rc % 31;
    double s = 0;
    for (int k = r; k < 15; k++) s += c.psqrt[i * 225 + r * 15 + k] * lds[L_S + i * 465 + k * 31 + cc];
    const size_t iv = (size_t)w * 10 + i;
    if (cc == 0) {
      if (A.imu_r) A.imu_r[iv * 15 + r] = s;
      if (c.psum[i] <= o.max_sum_dt) acc += 0.5 * s * s;
    } else if (A.imu_J) {
      A.imu_J[(iv * 15 + r) * 30 + cc - 1] = s;
    }
  }
  if (c.pn > 0) {
    prior_residual_dev(c, L_X);
    if (t < c.pn) {
      acc += 0.5 * lds[L_RP + t] * lds[L_RP + t];
      if (A.prior_res) A.prior_res[(size_t)w * B.max_prior + t] = lds[L_RP + t];
    }
  }
  const double cost = block_sum<NT>(acc, lds + L_RED);
  if (t == 0 && A.cost) A.cost[w] = cost;
}
