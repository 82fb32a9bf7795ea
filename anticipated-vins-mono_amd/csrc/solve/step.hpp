// solve/step.hpp - from the reduced solution to a candidate state: back_substitute, scale_system, state_plus
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// back substitution y_e = (g'_e - W'_e y_p) / (hee' + mu D_e^2) with W'[e][c] = s_e s_c W[e][c] (W unscaled in the
// slot): 4 lanes per feature, every lane's loads in flight at once; returns 1 if y is not finite
AVM_NOINL double back_substitute(const WinCtx&, double mu) {
  const WinCtx& c = lds_ctx();
  double* lds = LDS();
  const int t = threadIdx.x;
  gcdouble* W = c.sc + Scratch::W;
  const double* scl = lds + L_SC;
  double* ys = lds + L_WCH;  // s_c y_c
  constexpr int NQ4 = (NPOSE + 3) / 4;  // W rows dealt to the 4 lanes of a feature, a quarter each: 17 (20)
  if (t < NPOSE) ys[t] = scl[t] * lds[L_Y + t];
  if (t >= NPOSE && t < 4 * NQ4 + 4) ys[t] = 0.0;
  __syncthreads();
  AVM_PRIO_BULK();  // (150 independent dot products from the slot: bulk work; measured 12.54 -> 12.46 ms against leaving it at the light level)
  const int part = t & 3;
#pragma unroll
  for (int pass = 0; pass < (MAXE + NT / 4 - 1) / (NT / 4); pass++) {
    const int e = (t >> 2) + (NT / 4) * pass;
    double sacc = 0;
    if (e < c.nf) {
      gcdouble* We = W + e;  // Wt[c][e]
      double v[NQ4];
#pragma unroll
      for (int j = 0; j < NQ4; j++) v[j] = (part + 4 * j < NPOSE) ? We[(size_t)(part + 4 * j) * WLE] : 0.0;
#pragma unroll
      for (int j = 0; j < NQ4; j++) sacc += v[j] * ys[part + 4 * j];
    }
    sacc += lane_xor<1>(sacc);
    sacc += lane_xor<2>(sacc);
    if (e < c.nf && part == 0) {
      const double he = lds[L_HEE + e] + mu * lds[L_DD + NF + e] * lds[L_DD + NF + e];
      lds[L_Y + NF + e] = (lds[L_G + NF + e] - scl[NF + e] * sacc) / he;
    }
  }
  AVM_PRIO_LIGHT();
  __syncthreads();
  double bad = 0;
  for (int i = t; i < NF + c.nf; i += NT)
    if (!isfinite(lds[L_Y + i])) bad = 1;
  return block_max1(bad);
}

// Jacobi column scaling of the assembled system: H' = S H S, hee', g'  (W stays unscaled: see schur_reduce)
// `matrix`: also the entries of S.  In the base build that is needed once per solve, after the evaluation that fixes the
// scaling: from then on the evaluations write S scaled (frame_task, the (a,a) sums, imu_factor_mfma) and the packed prior
// in the slot is scaled in place here, once.
AVM_NOINL void scale_system(const WinCtx&, bool matrix) {
  const WinCtx& c = lds_ctx();
  double* lds = LDS();
  const int t = threadIdx.x;
  const double* scl = lds + L_SC;
  if (matrix && c.pn > 0) {
    const int* pidx = reinterpret_cast<const int*>(lds + L_INT) + I_PIDX;
    gdouble* HPk = c.sc + Scratch::HP;
    const int npk = c.pn * (c.pn + 1) / 2;
    for (int idx = t; idx < npk; idx += NT) {
      int gi = (int)((__builtin_sqrtf(8.0f * (float)idx + 1.0f) - 1.0f) * 0.5f);
      while (gi * (gi + 1) / 2 > idx) gi--;
      while ((gi + 1) * (gi + 2) / 2 <= idx) gi++;
      const int gj = idx - gi * (gi + 1) / 2;
      const int ip = pidx[gi], iq = pidx[gj];
      if (ip >= 0 && iq >= 0) HPk[idx] *= scl[ip] * scl[iq];
    }
  }
#ifdef AVM_TP
  if (matrix) {
    // once per solve: the pose rows of the packed triangle entry by entry, then the speed-bias rows in their structural form
    for (int idx = t; idx < NPOSE * NPOSE; idx += NT) {
      const int r = idx / NPOSE, cc = idx - r * NPOSE;
      if (cc <= r) lds[L_S + roff(r) + cc] *= scl[r] * scl[cc];
    }
    for (int idx = t; idx < 99 * SBW; idx += NT) {
      const int q = idx / SBW, p = idx - q * SBW, i = q / 9;
      const int cc = p < 18 ? 6 * (i - 1) + p : NPOSE + 9 * (i - 1) + (p - 18);
      if (cc >= 0 && (p >= 18 || cc < NPOSE)) lds[L_SBC + idx] *= scl[NPOSE + q] * scl[cc];
    }
    const int psb = reinterpret_cast<const int*>(lds + L_INT)[I_PSB];
    for (int idx = t; idx < 9 * NPOSE; idx += NT) {
      const int a = idx / NPOSE, cc = idx - a * NPOSE;
      lds[L_STRIP + idx] *= scl[NPOSE + 9 * psb + a] * scl[cc];
    }
  }
#else
  if (matrix)
  // 16x16 tiles of the packed lower triangle dealt to the wavefronts, 4 entries per lane and tile (the same lane <-> entry
  // map as the accumulators of the factorization): every lane has the same amount of work; three tiles per round with
  // all their loads in flight before the first store, the tile index arithmetic on the scalar unit, and entries outside
  // the matrix go to the lane's dump slot instead of a predicated store
  {
    const int lane = t & 63, lr = lane & 15, lk = lane >> 4;
    const int wvu = __builtin_amdgcn_readfirstlane(t >> 6);
    constexpr int NTR = (NF + 15) / 16, NTILE = NTR * (NTR + 1) / 2, NW = NT / 64, UN = 3;
#pragma unroll 1
    for (int base = wvu; base < NTILE; base += UN * NW) {
      int off[UN][4];
      double v[UN][4], f[UN][4];
#pragma unroll
      for (int u = 0; u < UN; u++) {
        const int tile = base + u * NW;
        const bool tv = tile < NTILE;
        const int tl = min(tile, NTILE - 1);
        int ti = 0;
        while ((ti + 1) * (ti + 2) / 2 <= tl) ti++;
        const int tj = tl - ti * (ti + 1) / 2;
        const int gj = 16 * tj + lr;
        const double sj = scl[min(gj, NF - 1)];
#pragma unroll
        for (int r = 0; r < 4; r++) {
          const int gi = 16 * ti + lk + 4 * r;
          const bool ok = tv && gi < NF && gj <= gi;
          off[u][r] = ok ? L_S + roff(gi) + gj : L_DUMP + lane;
          f[u][r] = scl[min(gi, NF - 1)] * sj;
          v[u][r] = lds[off[u][r]];
        }
      }
#pragma unroll
      for (int u = 0; u < UN; u++)
#pragma unroll
        for (int r = 0; r < 4; r++) lds[off[u][r]] = v[u][r] * f[u][r];
    }
  }
#endif
  if (t < c.nf) lds[L_HEE + t] *= scl[NF + t] * scl[NF + t];
  for (int i = t; i < NF + c.nf; i += NT) lds[L_G + i] *= scl[i];
  __syncthreads();
}

// Evaluator::Plus : xc = x (+) (step * scale)
AVM_DEV void state_plus() {
  double* lds = LDS();
  const int t = threadIdx.x;
  const double* x = lds + L_X;
  double* xc = lds + L_XC;
  const double* st = lds + L_ST;
  const double* scl = lds + L_SC;
  if (t < NFR) {
    const int o = t * 6;
    for (int k = 0; k < 3; k++) xc[t * 7 + k] = x[t * 7 + k] + st[o + k] * scl[o + k];
    quat q{x[t * 7 + 6], x[t * 7 + 3], x[t * 7 + 4], x[t * 7 + 5]};
    quat r = qnormalized(qmul(q, deltaQ(mk3(st[o + 3] * scl[o + 3], st[o + 4] * scl[o + 4], st[o + 5] * scl[o + 5]))));
    xc[t * 7 + 3] = r.x, xc[t * 7 + 4] = r.y, xc[t * 7 + 5] = r.z, xc[t * 7 + 6] = r.w;
  }
  if (t >= 64 && t < 64 + 99) {
    const int k = t - 64;
    xc[XSB + k] = x[XSB + k] + st[SB0 + k] * scl[SB0 + k];
  }
#ifdef AVM_TP
  for (int e = t; e < MAXE; e += NT) xc[XLAM + e] = x[XLAM + e] + st[NF + e] * scl[NF + e];
#else
  if (t >= 192 && t < 192 + MAXE) {
    const int e = t - 192;
    xc[XLAM + e] = x[XLAM + e] + st[NF + e] * scl[NF + e];
  }
#endif
#ifdef AVM_X
  // relo_Pose (frame 11) / ex_pose: PoseLocalParameterization::Plus when they are variables, else carried over untouched
  const WinCtx& c = lds_ctx();
  if (t >= 384 && t < 386) {
    const bool ex = t == 385;
    const int xo = ex ? XEX : 7 * NFR, o = ex ? XC_EX : 6 * NFR;
    if (ex ? c.est_ex != 0 : c.relo_n > 0) {
      for (int k = 0; k < 3; k++) xc[xo + k] = x[xo + k] + st[o + k] * scl[o + k];
      quat q{x[xo + 6], x[xo + 3], x[xo + 4], x[xo + 5]};
      quat r = qnormalized(qmul(q, deltaQ(mk3(st[o + 3] * scl[o + 3], st[o + 4] * scl[o + 4], st[o + 5] * scl[o + 5]))));
      xc[xo + 3] = r.x, xc[xo + 4] = r.y, xc[xo + 5] = r.z, xc[xo + 6] = r.w;
    } else {
      for (int k = 0; k < 7; k++) xc[xo + k] = x[xo + k];
    }
  }
  if (t == 386) xc[XTD] = c.est_td ? x[XTD] + st[XC_TD] * scl[XC_TD] : x[XTD];
#endif
}
