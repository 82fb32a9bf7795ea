// solve/eval_cost.hpp - eval_cost: the residual-only cost of a candidate state
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// residual-only cost at state xs (frames slot `which` must be built). Uses lds[L_S..] as IMU staging.
AVM_NOINL double eval_cost(const WinCtx&, const avm_options&, int xs_off, int which) {
  const WinCtx& c = lds_ctx();
  const avm_options& o = lds_opt();
  double* lds = LDS();
  const double* xs = lds + xs_off;
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  (void)ids;
  const int t = threadIdx.x;
  Frames fr{lds + L_FR + which * FRS, lds + L_FR + which * FRS + 9 * NFRP};
  const double* ric = ric_of(which);
  const double sqi = o.focal_length / 1.5;
  double acc = 0;
  // IMU raw residuals by threads of the last wave (so they overlap with projection work of the others)
  for (int i = t; i < 10 * 31 * 15; i += NT) lds[L_S + i] = 0.0;
  __syncthreads();
  if (t >= NT - 64 && t < NT - 64 + 10) {
    const int i = t - (NT - 64);
    if (c.psum[i] <= o.max_sum_dt)
      imu_raw<false>(xs, fr.R, o, c.pdelta + i * 10, c.pjac + i * 225, c.psum[i], c.lba + i * 3, c.lbg + i * 3, i, lds + L_S + i * 465);
  }
  if (c.nobs_tot > 0) {
    // thread per observation slot; the feature id and the two observations of every slot a thread owns are
    // fetched up front (two dependent rounds of loads in total instead of two per slot); slots past the end are
    // clamped to the last valid one, so every address stays inside the window's tables
    constexpr int NSL = (MAXOBS + NT - 1) / NT;
    int es[NSL], s0s[NSL];
    double ob[NSL][4];
#pragma unroll
    for (int u = 0; u < NSL; u++) es[u] = min(max(c.osf[min(t + u * NT, c.nobs_tot - 1)], 0), c.nf - 1);
#pragma unroll
    for (int u = 0; u < NSL; u++) {
      const int s = min(t + u * NT, c.nobs_tot - 1);
      s0s[u] = ids[I_FOBS + es[u]];
      ob[u][0] = c.obs[2 * s0s[u]], ob[u][1] = c.obs[2 * s0s[u] + 1], ob[u][2] = c.obs[2 * s], ob[u][3] = c.obs[2 * s + 1];
    }
#pragma unroll
    for (int u = 0; u < NSL; u++) {
      const int s = t + u * NT;
      const int e = es[u];
      // the observation table may have holes (avm_slide_window drops a feature's first observation in place): a slot
      // belongs to the feature the slot map names only if it lies inside that feature's range of the CURRENT table
      if (s >= c.nobs_tot || s <= s0s[u] || s >= s0s[u] + ids[I_FNOBS + e]) continue;
      const int fa = ids[I_FSTART + e], fb = fa + (s - s0s[u]);
      double r[2];
#ifdef AVM_X
      if (c.est_td) {
        double ai[4], aj[4];
#pragma unroll
        for (int k = 0; k < 4; k++) ai[k] = c.aux[4 * s0s[u] + k], aj[k] = c.aux[4 * s + k];
        td_shift(ob[u], ai, aj, xs[XTD], o.tr, o.row);
      }
#endif
      acc += proj_eval<false>(xs, fr, ric, ric + 9, ob[u][0], ob[u][1], ob[u][2], ob[u][3], xs[XLAM + e], fa, fb, sqi,
                              o.cauchy_a, true, r, nullptr, nullptr, nullptr);
    }
  }
#ifdef AVM_X
  // relocalization factors (estimator.cpp:760-792): plain ProjectionFactors against relo_Pose = frame 11
  for (int k = t; k < c.relo_n; k += NT) {
    const int e = c.cov[(NFRP - 1) * MAXE + k], s0 = ids[I_FOBS + e];
    double r[2];
    acc += proj_eval<false>(xs, fr, ric, ric + 9, c.obs[2 * s0], c.obs[2 * s0 + 1], c.relo_xy[2 * k], c.relo_xy[2 * k + 1], xs[XLAM + e],
                            ids[I_FSTART + e], NFRP - 1, sqi, o.cauchy_a, true, r, nullptr, nullptr, nullptr);
  }
#endif
  // the prior on the last wavefront (the same code, hence the same rounding, as in eval_jac)
  if (t >= NT - 64 && c.pn > 0) {
    const double pc = prior_wave<false>(xs_off, 0, c.pn, L_DXP);
    if (t == NT - 64) acc += pc;
  }
  __syncthreads();
  if (t < 150) {
    const int i = t / 15, r = t % 15;
    if (c.psum[i] <= o.max_sum_dt) {
      double ps[15], s = 0;  // (all fifteen loads in flight: from k = r every step was a trip to memory of its own)
#pragma unroll
      for (int k = 0; k < 15; k++) ps[k] = c.psqrt[i * 225 + r * 15 + k];
#pragma unroll
      for (int k = 0; k < 15; k++) s += k >= r ? ps[k] * lds[L_S + i * 465 + k * 31] : 0.0;
      acc += 0.5 * s * s;
    }
  }

  return block_sum1(acc);
}
