// solve/frame_task_x.hpp - the frame task of the extended build
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// The same task with every optional member of the problem: staged row [Jj | Ji | r | Jex | Jtd] (20 columns, two 16-wide
// operand tiles), frame 11 = the relocalization frame (its "observations" are the match points, its pose relo_Pose).
// X^T X now has three tiles: D00 = [Jj Ji r]^2 as before, D10 = [Jex Jtd]^T [Jj Ji r] and D11 = [Jex Jtd]^2.
//   D00, per start-frame run a:  (b,a), (a,a) -> PART[b][a], g_a;        total: (b,b), g_b
//   D10, per run:  [Jex Jtd]^T Ji -> PART[b][a][SP_XA..];                 total: [Jex Jtd]^T Jj -> S rows 72..78 x cols 6b.. (owned by
//        this frame), [Jex Jtd]^T r -> PARTX[b][28..34]
//   D11, total: -> PARTX[b][0..27]
// Members that are switched off (estimate_extrinsic / estimate_td == 0) stage exact zeros, so their blocks come out zero.
AVM_DEV double frame_task(const WinCtx&, const avm_options&, int b, int stage_off) {
  const WinCtx& c = lds_ctx();
  const avm_options& o = lds_opt();
  double* lds = LDS();
  double* stage = lds + stage_off;
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  const int lane = threadIdx.x & 63;
  const int ncov = ids[I_NCOV + b];
  const int32_t* cov = c.cov + b * MAXE;
  Frames fr{lds + L_FR, lds + L_FR + 9 * NFRP};
  const double* ric = ric_of(0);
  const double* xs = lds + L_X;
  const double sqi = o.focal_length / 1.5;
  const bool relo = b == NFRP - 1;
  const bool use_td = c.est_td && !relo;  // the relocalization factors are plain ProjectionFactors (estimator.cpp:783)
  const double exm = c.est_ex ? 1.0 : 0.0;
  const double td = xs[XTD];
  double* W = c.sc + Scratch::W;
  double* PF = c.sc + Scratch::PF;
  double* PART = c.sc + Scratch::PART + (size_t)b * NFR * SPARTW;
  double* PX = c.sc + Scratch::PART + PARTX0 + (size_t)b * PARTX;
  const double* scl = lds + L_SC;
  d4 Dtot = {0, 0, 0, 0}, D00 = {0, 0, 0, 0}, E00 = {0, 0, 0, 0}, D10 = {0, 0, 0, 0}, E10 = {0, 0, 0, 0}, D10tot = {0, 0, 0, 0},
     D11 = {0, 0, 0, 0}, E11 = {0, 0, 0, 0};
  int a_run = -1, pmask = 0;
  double cost = 0;
  const int drow = lane >> 4, dcol = lane & 15;
  auto flush = [&]() {
    if (a_run < 0) return;
    D00 += E00, D10 += E10;
    E00 = E10 = d4{0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = drow + 4 * r;
      const double v = D00[r];
      if (row < 6 && dcol >= 6 && dcol < 12) lds[L_S + roff(6 * b + row) + 6 * a_run + (dcol - 6)] = v * (scl[6 * b + row] * scl[6 * a_run + (dcol - 6)]);  // Jj^T Ji (S is written Jacobi-scaled, as in the other builds)
      if (row >= 6 && row < 12) {
        const int i = row - 6;
        if (dcol >= 6 && dcol < 12 && dcol - 6 <= i) PART[a_run * SPARTW + SP_AA + i * (i + 1) / 2 + (dcol - 6)] = v;  // Ji^T Ji (lower)
        if (dcol == 12) PART[a_run * SPARTW + SP_GA + i] = v;                                                  // Ji^T r
      }
      if (row < 7 && dcol >= 6 && dcol < 12) PART[a_run * SPARTW + SP_XA + row * 6 + (dcol - 6)] = D10[r];      // [Jex Jtd]^T Ji
    }
    pmask |= 1 << a_run;
    Dtot += D00, D10tot += D10;
    D00 = D10 = d4{0, 0, 0, 0};
  };
  for (int chunk0 = 0; chunk0 < ncov; chunk0 += 64) {
    const int idx = chunk0 + lane;
    const bool act = idx < ncov;
    const int e = cov[min(idx, ncov - 1)];
    const int fa = ids[I_FSTART + e];
    const int s0 = ids[I_FOBS + e], s = s0 + (b - fa);
    double ob[4];
    ob[0] = c.obs[2 * s0], ob[1] = c.obs[2 * s0 + 1];
    if (relo)
      ob[2] = c.relo_xy[2 * min(idx, ncov - 1)], ob[3] = c.relo_xy[2 * min(idx, ncov - 1) + 1];
    else
      ob[2] = c.obs[2 * s], ob[3] = c.obs[2 * s + 1];
    double ai[4] = {0, 0, 0, 0}, aj[4] = {0, 0, 0, 0};
    if (use_td) {
#pragma unroll
      for (int k = 0; k < 4; k++) ai[k] = c.aux[4 * s0 + k], aj[k] = c.aux[4 * s + k];
      td_shift(ob, ai, aj, td, o.tr, o.row);
    }
    double r[2] = {0, 0}, Ji[12], Jj[12], Je[2] = {0, 0}, Jx[12], Jt[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 12; k++) Ji[k] = 0, Jj[k] = 0, Jx[k] = 0;
    if (act) {
      cost += proj_eval<true>(xs, fr, ric, ric + 9, ob[0], ob[1], ob[2], ob[3], xs[XLAM + e], fa, b, sqi, o.cauchy_a, true, r, Ji, Jj, Je, Jx,
                              Jt, ai[0], ai[1], aj[0], aj[1]);
#pragma unroll
      for (int k = 0; k < 12; k++) Jx[k] *= exm;
      if (!use_td) Jt[0] = Jt[1] = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) {
        W[(6 * b + k) * WLE + e] = Jj[k] * Je[0] + Jj[6 + k] * Je[1];
        if (k >= 3) PF[((PQ_JI + k) * NFRP + b) * WLE + e] = Ji[k] * Je[0] + Ji[6 + k] * Je[1];  // (k < 3: minus W's entry, see the base build's frame task)
        PF[((PQ_JEX + k) * NFRP + b) * WLE + e] = Jx[k] * Je[0] + Jx[6 + k] * Je[1];
      }
      PF[(PQ_HEE * NFRP + b) * WLE + e] = Je[0] * Je[0] + Je[1] * Je[1];
      PF[(PQ_GE * NFRP + b) * WLE + e] = Je[0] * r[0] + Je[1] * r[1];
      PF[(PQ_JTD * NFRP + b) * WLE + e] = Jt[0] * Je[0] + Jt[1] * Je[1];
    }
    // The staging tile holds HALF a chunk (lanes 0-31 stage and the wavefront multiplies, then lanes 32-63: the scheme of the throughput build
    // and of marg_frame_task).  A run that straddles the two halves simply continues: the switch below only acts on a new start frame.
    const int nact = min(64, ncov - chunk0);
    const int fav = act ? fa : -1;
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
      const int h0 = 32 * half, lim = min(nact, h0 + 32);
      if (h0 >= nact) break;  // (uniform)
      if ((lane >> 5) == half) {
        dv2* st = reinterpret_cast<dv2*>(stage) + (lane & 31);
#pragma unroll
        for (int k = 0; k < 6; k++) {
          st[k * (XRS_X / 2)] = dv2{Jj[k], Jj[6 + k]};
          st[(6 + k) * (XRS_X / 2)] = dv2{Ji[k], Ji[6 + k]};
          st[(13 + k) * (XRS_X / 2)] = dv2{Jx[k], Jx[6 + k]};
        }
        st[12 * (XRS_X / 2)] = dv2{r[0], r[1]};
        st[19 * (XRS_X / 2)] = dv2{Jt[0], Jt[1]};
      }
      wave_lds_sync();
      int l = h0;
      while (l < lim) {
        const int a_cur = __shfl(fav, l, 64);
        const int l_end = min(l + __popcll(__ballot(act && fa == a_cur && lane >= l)), lim);
        if (a_cur != a_run) {
          flush();
          a_run = a_cur;
        }
        const int j_end = (l_end - h0 + 3) >> 2;
#pragma unroll 1
        for (int j0 = (l - h0) >> 2; j0 < j_end; j0 += 4) {
          // D10 / D11 have seven rows ([Jex Jtd]): two four-row strips on v_mfma_f64_4x4x4 each (18 cycles of the FP64 pipe an issue against
          // 64; schur_strip4's operand layout: A = row li % 4 of the strip in every quad, B as the 16 x 16 tile takes it, D = register r of the
          // tile's accumulator for strip r) - 128 + 8 x 18 = 272 instead of 384 cycles per step: 5.78 -> 5.60 ms per 1024 windows (round 5)
          dv2 u0[4], u1[4], ua[4], ub[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int ro = 8 * min(j0 + u, 7) + 2 * drow;
            u0[u] = *reinterpret_cast<const dv2*>(stage + min(dcol, 12) * XRS_X + ro);
            u1[u] = *reinterpret_cast<const dv2*>(stage + (13 + min(dcol, 6)) * XRS_X + ro);
            ua[u] = *reinterpret_cast<const dv2*>(stage + (13 + (dcol & 3)) * XRS_X + ro);
            ub[u] = *reinterpret_cast<const dv2*>(stage + (13 + min(4 + (dcol & 3), 6)) * XRS_X + ro);
          }
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int f = h0 + 4 * (j0 + u) + drow;
            const bool in = f >= l && f < l_end;
            const double a0 = (in && dcol < 13) ? u0[u][0] : 0.0, a1 = (in && dcol < 13) ? u0[u][1] : 0.0;
            const double x0 = (in && dcol < 7) ? u1[u][0] : 0.0, x1 = (in && dcol < 7) ? u1[u][1] : 0.0;
            const double p0 = in ? ua[u][0] : 0.0, p1 = in ? ua[u][1] : 0.0;
            const double q0 = (in && (dcol & 3) < 3) ? ub[u][0] : 0.0, q1 = (in && (dcol & 3) < 3) ? ub[u][1] : 0.0;
            D00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, D00, 0, 0, 0);
            D10[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(p0, a0, D10[0], 0, 0, 0), D10[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(q0, a0, D10[1], 0, 0, 0);
            D11[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(p0, x0, D11[0], 0, 0, 0), D11[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(q0, x0, D11[1], 0, 0, 0);
            E00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, E00, 0, 0, 0);
            E10[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(p1, a1, E10[0], 0, 0, 0), E10[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(q1, a1, E10[1], 0, 0, 0);
            E11[0] = __builtin_amdgcn_mfma_f64_4x4x4f64(p1, x1, E11[0], 0, 0, 0), E11[1] = __builtin_amdgcn_mfma_f64_4x4x4f64(q1, x1, E11[1], 0, 0, 0);
          }
        }
        l = l_end;
      }
      wave_lds_sync();
    }
  }
  flush();
  D11 += E11;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int row = drow + 4 * r;
    if (row < 6 && dcol <= row) lds[L_S + roff(6 * b + row) + 6 * b + dcol] = Dtot[r] * (scl[6 * b + row] * scl[6 * b + dcol]);   // (b,b) lower
    if (row < 6 && dcol == 12) lds[L_G + 6 * b + row] = Dtot[r];                         // g_b (the gradient is scaled afterwards, as a vector)
    if (row < 7) {
      if (dcol < 6) lds[L_S + roff(XC_EX + row) + 6 * b + dcol] = D10tot[r] * (scl[XC_EX + row] * scl[6 * b + dcol]);  // ([ex td], pose b)
      if (dcol == 12) PX[28 + row] = D10tot[r];                                          // [Jex Jtd]^T r
      if (dcol <= row) PX[row * (row + 1) / 2 + dcol] = D11[r];                          // ([ex td], [ex td]) lower
    }
  }
  if (lane == 0) ids[I_PMASK + b] = pmask;
  return cost;
}
