// solve/jac_times_vec.hpp - jac_times_vec_sq: |J' u|^2 for the Cauchy point
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// || J' u ||^2 with J' the Jacobi-scaled Jacobian, u in lds[L_ST] (scaled space), at state lds[L_X].
// Only needed when the Gauss-Newton step leaves the trust region (Cauchy point), so the factors are
// simply re-evaluated here instead of keeping their Jacobians around.
AVM_NOINL double jac_times_vec_sq(const WinCtx&, const avm_options&) {
  const WinCtx& c = lds_ctx();
  const avm_options& o = lds_opt();
  double* lds = LDS();
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  (void)ids;
  const int t = threadIdx.x;
  const double* u = lds + L_ST;
  const double* scl = lds + L_SC;
  const double* xs = lds + L_X;
  Frames fr{lds + L_FR, lds + L_FR + 9 * NFRP};
  const double* ric = ric_of(0);
  const double sqi = o.focal_length / 1.5;
  double acc = 0;
#ifdef AVM_X
  // regular factors, then the relocalization factors (slot index >= nobs_tot: match k against frame 11)
  for (int s = t; s < c.nobs_tot + c.relo_n; s += NT) {
    const bool relo = s >= c.nobs_tot;
    const int e = relo ? c.cov[(NFRP - 1) * MAXE + (s - c.nobs_tot)] : min(max(c.osf[s], 0), c.nf - 1);
    const int s0 = ids[I_FOBS + e];
    if (!relo && (s <= s0 || s >= s0 + ids[I_FNOBS + e])) continue;  // first observation, or a hole of the table (see eval_cost)
    const int fa = ids[I_FSTART + e], fb = relo ? NFRP - 1 : fa + (s - s0);
    double ob[4] = {c.obs[2 * s0], c.obs[2 * s0 + 1], 0, 0}, ai[4] = {0, 0, 0, 0}, aj[4] = {0, 0, 0, 0};
    if (relo)
      ob[2] = c.relo_xy[2 * (s - c.nobs_tot)], ob[3] = c.relo_xy[2 * (s - c.nobs_tot) + 1];
    else
      ob[2] = c.obs[2 * s], ob[3] = c.obs[2 * s + 1];
    const bool use_td = c.est_td && !relo;
    if (use_td) {
#pragma unroll
      for (int k = 0; k < 4; k++) ai[k] = c.aux[4 * s0 + k], aj[k] = c.aux[4 * s + k];
      td_shift(ob, ai, aj, xs[XTD], o.tr, o.row);
    }
    double r[2], Ji[12], Jj[12], Je[2], Jx[12], Jt[2];
    proj_eval<true>(xs, fr, ric, ric + 9, ob[0], ob[1], ob[2], ob[3], xs[XLAM + e], fa, fb, sqi, o.cauchy_a, true, r, Ji, Jj, Je, Jx, Jt,
                    ai[0], ai[1], aj[0], aj[1]);
    double y0 = 0, y1 = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double va = u[fa * 6 + k] * scl[fa * 6 + k], vb = u[fb * 6 + k] * scl[fb * 6 + k];
      const double vx = c.est_ex ? u[XC_EX + k] * scl[XC_EX + k] : 0.0;
      y0 += Ji[k] * va + Jj[k] * vb + Jx[k] * vx;
      y1 += Ji[6 + k] * va + Jj[6 + k] * vb + Jx[6 + k] * vx;
    }
    const double ve = u[NF + e] * scl[NF + e], vt = use_td ? u[XC_TD] * scl[XC_TD] : 0.0;
    y0 += Je[0] * ve + Jt[0] * vt;
    y1 += Je[1] * ve + Jt[1] * vt;
    acc += y0 * y0 + y1 * y1;
  }
#else
  for (int s = t; s < c.nobs_tot; s += NT) {
    const int e = min(max(c.osf[s], 0), c.nf - 1);
    const int s0 = ids[I_FOBS + e];
    if (s <= s0 || s >= s0 + ids[I_FNOBS + e]) continue;  // first observation, or a hole of the table (see eval_cost)
    const int fa = ids[I_FSTART + e], fb = fa + (s - s0);
    double r[2], Ji[12], Jj[12], Je[2];
    proj_eval<true>(xs, fr, ric, ric + 9, c.obs[2 * s0], c.obs[2 * s0 + 1], c.obs[2 * s], c.obs[2 * s + 1], xs[XLAM + e],
                    fa, fb, sqi, o.cauchy_a, true, r, Ji, Jj, Je);
    double y0 = 0, y1 = 0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const double va = u[fa * 6 + k] * scl[fa * 6 + k], vb = u[fb * 6 + k] * scl[fb * 6 + k];
      y0 += Ji[k] * va + Jj[k] * vb;
      y1 += Ji[6 + k] * va + Jj[6 + k] * vb;
    }
    const double ve = u[NF + e] * scl[NF + e];
    y0 += Je[0] * ve;
    y1 += Je[1] * ve;
    acc += y0 * y0 + y1 * y1;
  }
#endif
  // IMU: y = sqrt_info * (raw_J * v), raw Jacobians of the last eval_jac are still in the scratch slot.  Two steps with one trip to
  // the slot each (thread (i, k): row k of raw_J times v, thirty loads in flight; thread (i, r): row r of sqrt_info times that) - as
  // nested loops from k = r every thread made up to fifteen trips of its own, and every row of raw_J v was computed up to 15 times
  double* rvb = lds + L_WCH;  // [150] (the factorization's scratch is dead here)
  if (t < 150) {
    const int i = t / 15, k = t % 15;
    const double* IJR = c.sc + Scratch::IJRAW + i * IJBLK;
    double jv[30];
#pragma unroll
    for (int p = 0; p < 30; p++) jv[p] = IJR[k * 31 + 1 + p];
    double rv = 0;
#pragma unroll
    for (int p = 0; p < 30; p++) {
      const int col = imu_col(i, p);
      rv += jv[p] * (u[col] * scl[col]);
    }
    rvb[t] = rv;
  }
  // the prior's rows meanwhile: J0 row i times v, sixteen loads in flight (behind `pidx[k] >= 0` they were up to 75 trips)
  if (c.pn > 0 && t >= PT0 && t < PT0 + c.pn) {
    const int i = t - PT0;
    const int* pidx = ids + I_PIDX;
    const int pn1 = c.pn - 1;
    double y = 0;
    for (int k0 = 0; k0 < c.pn; k0 += 16) {
      double pj[16];
#pragma unroll
      for (int q = 0; q < 16; q++) pj[q] = c.pJ[(size_t)i * c.ldp + min(k0 + q, pn1)];
#pragma unroll
      for (int q = 0; q < 16; q++) {
        const int ix = pidx[min(k0 + q, pn1)], ic = max(ix, 0);
        y += (k0 + q <= pn1 && ix >= 0) ? pj[q] * (u[ic] * scl[ic]) : 0.0;
      }
    }
    acc += y * y;
  }
  __syncthreads();
  if (t < 150) {
    const int i = t / 15, r = t % 15;
    if (c.psum[i] <= o.max_sum_dt) {
      double ps[15];
#pragma unroll
      for (int k = 0; k < 15; k++) ps[k] = c.psqrt[i * 225 + r * 15 + k];
      double y = 0;
#pragma unroll
      for (int k = 0; k < 15; k++) y += k >= r ? ps[k] * rvb[i * 15 + k] : 0.0;
      acc += y * y;
    }
  }
  return block_sum1(acc);
}
