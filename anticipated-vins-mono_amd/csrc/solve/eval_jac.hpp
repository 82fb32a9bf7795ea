// solve/eval_jac.hpp - eval_jac: the full evaluation (phases A to E) that fills S, W, hee and g
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// Full evaluation at lds[L_X]: fills S (unscaled H_ff), W, hee, g (unscaled) and returns the cost.
AVM_NOINL double eval_jac(const WinCtx&, const avm_options&) {
  const WinCtx& c = lds_ctx();
  const avm_options& o = lds_opt();
  double* lds = LDS();
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  (void)ids;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const double* xs = lds + L_X;
  constexpr int xs_off = L_X;
  PROF_T0();
  build_frames(L_X, 0);
  for (int i = t; i < SPP; i += NT) lds[L_S + i] = 0.0;
  for (int i = t; i < VEC; i += NT) lds[L_G + i] = 0.0;
#ifdef AVM_TP
  for (int i = t; i < 6 * ACCW; i += NT) lds[L_ACC + i] = 0.0;  // the frame tasks' E^T E / E^T r accumulators (wavefront 0's are lds[L_HEE], lds[L_G + NF])
  for (int i = t; i < 152; i += NT) lds[L_HEE + i] = 0.0;
#endif
  if (t < NFRP) ids[I_PMASK + t] = 0;
  double* IJR = c.sc + Scratch::IJRAW;  // (zeroed once per window: imu_raw rewrites the same entries every time)
  __syncthreads();
  Frames fr{lds + L_FR, lds + L_FR + 9 * NFRP};
  double acc = 0;
  // ---- phase A: projection factors (wavefronts 0..ASM_WAVES-1) || raw IMU Jacobians (the next wavefront) || the prior
  const long long pa__ = c.prof ? clock64() : 0;
  if (wv < ASM_WAVES) {
#ifdef AVM_X
    for (int b = 1; b < NFRP; b++)
      if (ids[I_FRW + b] == wv) acc += frame_task(c, o, b, L_S + SPP + wv * XSTG);
#else
    AVM_PRIO_BULK();
    acc += frame_task(c, o, wv, L_S + SPP + wv * XSTG);  // all the frames of this wavefront as one list
    AVM_PRIO_LIGHT();
#endif
  }
#ifdef AVM_TP
  if (wv == IMUW && lane < 10) {
#else
  else if (wv == ASM_WAVES && lane < 10) {
#endif
    const int i = lane;
    if (c.psum[i] <= o.max_sum_dt)
      imu_raw<true>(xs, fr.R, o, c.pdelta + i * 10, c.pjac + i * 225, c.psum[i], c.lba + i * 3, c.lbg + i * 3, i, IJR + i * IJBLK);
  }
  // ... || the prior (dx, residual, cost, J0^T r_p) on the last wavefront, which has the lightest load of phase A
#ifdef AVM_X
  if (wv == NT / 64 - 1 && c.pn > 0) {
    const double pc = prior_wave<true>(xs_off, 0, c.pn, L_DXP);
    if (lane == 0) acc += pc;
  }
#else
  // (the raw-IMU wavefront takes the last two fifths of the prior's rows once it is done: each of the two reads J0 along its
  //  own rows only)
  if (wv >= IMUW && c.pn > 0) {
    const int h = (3 * c.pn + 2) / 5;
    const double pc = wv == IMUW ? prior_wave<true>(xs_off, h, c.pn, L_DX2) : prior_wave<true>(xs_off, 0, h, L_DXP);
    if (lane == 0) acc += pc;
  }
#endif
  if (c.prof && lane == 0) c.prof[48 + wv] += clock64() - pa__;  // this wavefront's busy time in phase A
  __syncthreads();
  PROF(c, 0);
  // ---- phase B: per-feature sums over the start pose, diagonal blocks, pose gradient
  {
    double* W = c.sc + Scratch::W;
    const double* PF = c.sc + Scratch::PF;
    // sums over the feature's own factors: one thread per (quantity, feature), features along the lanes
    // (the W blocks of frames that do not observe a feature were zeroed once, at window load)
    // (every round's loads are requested before the first sum: one trip to the slot's memory instead of one per round)
    constexpr int NRND = (MAXE * NQB + NT - 1) / NT;
    double pv[NRND][NFR - 1];
#ifdef AVM_X
    double prl[NRND];
#endif
#pragma unroll
    for (int u = 0; u < NRND; u++) {
      const int idx = min(t + u * NT, max(c.nf * NQB - 1, 0));
      const int q = idx / max(c.nf, 1), e = idx - q * c.nf;
      // (a window without features has no table entry to read: the clamped loads then stay at the start of the region)
      const int a = c.nf > 0 ? ids[I_FSTART + e] : 0, no = c.nf > 0 ? ids[I_FNOBS + e] : 0;
      // + k * stride : the factor observed in frame a + k.  q < 3 (Ji_t^T Je): minus the observing frame's E^T F entry, read out of W (frame_task)
      const double* P = q < 3 ? W + (6 * a + q) * WLE + e : PF + (q * NFRP + a) * WLE + e;
      const int pst = q < 3 ? 6 * WLE : WLE;
      // all (<= 10) loads in flight, clamped to the feature's last observation and masked; same pairing of the
      // partial sums as a sequential two-accumulator loop
#pragma unroll
      for (int k = 1; k < NFR; k++) pv[u][k - 1] = P[min(k, max(no - 1, 0)) * pst];
#ifdef AVM_X
      prl[u] = q < 3 ? W[(6 * (NFRP - 1) + q) * WLE + e] : PF[(q * NFRP + (NFRP - 1)) * WLE + e];
#endif
    }
#ifndef AVM_X
    // the partial (a,a) blocks of the frame tasks, summed further down, are requested now as well
#ifdef AVM_TP
    constexpr int NPR = (NFR * SPARTW + NT - 1) / NT;  // 297 sums on 256 threads: two rounds
    double pp[NPR][NFR - 1];
#pragma unroll
    for (int u = 0; u < NPR; u++) {
      const int tt = min(t + u * NT, NFR * SPARTW - 1);
      const int f = tt / SPARTW, q = tt % SPARTW;
#pragma unroll
      for (int b = 1; b < NFR; b++) pp[u][b - 1] = (c.sc + Scratch::PART)[((size_t)b * NFR + f) * SPARTW + q];  // unconditional, masked below
    }
#else
    double pp[NFR - 1];
    if (t < NFR * SPARTW) {
      const int f = t / SPARTW, q = t % SPARTW;
#pragma unroll
      for (int b = 1; b < NFR; b++) pp[b - 1] = (c.sc + Scratch::PART)[((size_t)b * NFR + f) * SPARTW + q];  // unconditional, masked below
    }
#endif
#endif
#pragma unroll
    for (int u = 0; u < NRND; u++) {
      const int idx = t + u * NT;
      if (idx >= c.nf * NQB) break;
      const int q = idx / c.nf, e = idx - q * c.nf;
      const int a = ids[I_FSTART + e], no = ids[I_FNOBS + e];
      double s0a = 0, s1a = 0;
#pragma unroll
      for (int k = 1; k < NFR; k++) {
        const double v = k < no ? pv[u][k - 1] : 0.0;
        if (k & 1) s0a += v; else s1a += v;
      }
#ifdef AVM_X
      // + the feature's relocalization factor (frame 11; its slots were zeroed at window load for unmatched features)
      const double sraw = (s0a + s1a) + (c.relo_n > 0 ? prl[u] : 0.0);
      const double sacc = q < 3 ? -sraw : sraw;  // (the W entries are minus the products summed here: exact)
      if (q < 6)
        W[(6 * a + q) * WLE + e] = sacc;
      else if (q == PQ_HEE)
        lds[L_HEE + e] = sacc;
      else if (q == PQ_GE)
        lds[L_G + NF + e] = sacc;
      else
        W[(XC_EX + (q - PQ_JEX)) * WLE + e] = sacc;  // E^T F of the ex_pose (6) and td (1) columns
#else
      const double sacc = q < 3 ? -(s0a + s1a) : s0a + s1a;  // (the W entries are minus the products summed here: exact)
      if (q < 6)
        W[(6 * a + q) * WLE + e] = sacc;
      else if (q == PQ_HEE)
        lds[L_HEE + e] = sacc;
      else
        lds[L_G + NF + e] = sacc;
#endif
    }
#ifdef AVM_TP
    for (int e = t; e < c.nf; e += NT) {  // the four wavefronts' accumulators, in a fixed order
      const double* ac = lds + L_ACC + e;
      lds[L_HEE + e] = (lds[L_HEE + e] + ac[0]) + (ac[2 * ACCW] + ac[4 * ACCW]);
      lds[L_G + NF + e] = (lds[L_G + NF + e] + ac[ACCW]) + (ac[3 * ACCW] + ac[5 * ACCW]);
    }
#endif
    const double* PART = c.sc + Scratch::PART;
#ifdef AVM_X
    __syncthreads();  // (the sums below add to blocks other frames' tasks have written: all of phase A is behind the barrier above)
    for (int tt = t; tt < NFR * SPARTW + PARTX; tt += NT) {
      if (tt < NFR * SPARTW) {
        const int f = tt / SPARTW, q = tt % SPARTW;
        double sacc = 0;
        double pp[NFRP - 1];
#pragma unroll
        for (int b = 1; b < NFRP; b++) pp[b - 1] = PART[((size_t)b * NFR + f) * SPARTW + q];
#pragma unroll
        for (int b = 1; b < NFRP; b++)
          if (b > f && (ids[I_PMASK + b] & (1 << f))) sacc += pp[b - 1];
        if (q < SP_GA) {
          int i = 0;
          while ((i + 1) * (i + 2) / 2 <= q) i++;
          const int j = q - i * (i + 1) / 2;
          lds[L_S + roff(6 * f + i) + 6 * f + j] += sacc * (lds[L_SC + 6 * f + i] * lds[L_SC + 6 * f + j]);
        } else if (q < SP_XA) {
          lds[L_G + 6 * f + (q - SP_GA)] += sacc;
        } else {
          lds[L_S + roff(XC_EX + (q - SP_XA) / 6) + 6 * f + (q - SP_XA) % 6] += sacc * (lds[L_SC + XC_EX + (q - SP_XA) / 6] * lds[L_SC + 6 * f + (q - SP_XA) % 6]);  // ([ex td], start pose f)
        }
      } else {
        const int q = tt - NFR * SPARTW;
        double sacc = 0;
        for (int b = 1; b < NFRP; b++) sacc += PART[PARTX0 + (size_t)b * PARTX + q];  // (a frame without factors wrote zeros)
        if (q < 28) {
          int i = 0;
          while ((i + 1) * (i + 2) / 2 <= q) i++;
          lds[L_S + roff(XC_EX + i) + XC_EX + (q - i * (i + 1) / 2)] = sacc * (lds[L_SC + XC_EX + i] * lds[L_SC + XC_EX + (q - i * (i + 1) / 2)]);
        } else {
          lds[L_G + XC_EX + (q - 28)] = sacc;
        }
      }
    }
    __syncthreads();
    // members that are switched off: unit diagonal, nothing else (their rows / columns stay zero), so their step is exactly 0
    if (t < 13) {
      const int col = NFR * 6 + t;  // relo 66..71 | ex 72..77 | td 78
      const bool on = t < 6 ? c.relo_n > 0 : (t < 12 ? c.est_ex != 0 : c.est_td != 0);
      if (!on) lds[L_S + roff(col) + col] = lds[L_SC + col] * lds[L_SC + col];  // (1.0, Jacobi-scaled like every other entry)
    }
#elif defined(AVM_TP)
#pragma unroll
    for (int u = 0; u < NPR; u++) {
      const int tt = t + u * NT;
      if (tt >= NFR * SPARTW) break;
      const int f = tt / SPARTW, q = tt % SPARTW;
      double sacc = 0;
#pragma unroll
      for (int b = 1; b < NFR; b++)
        if (b > f && (ids[I_PMASK + b] & (1 << f))) sacc += pp[u][b - 1];
      if (q < SP_GA) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= q) i++;
        const int j = q - i * (i + 1) / 2;
        lds[L_S + roff(6 * f + i) + 6 * f + j] += sacc * (lds[L_SC + 6 * f + i] * lds[L_SC + 6 * f + j]);
      } else {
        lds[L_G + 6 * f + (q - SP_GA)] += sacc;
      }
    }
#else
    if (t < NFR * SPARTW) {
      const int f = t / SPARTW, q = t % SPARTW;
      double sacc = 0;
#pragma unroll
      for (int b = 1; b < NFR; b++)
        if (b > f && (ids[I_PMASK + b] & (1 << f))) sacc += pp[b - 1];
      if (q < SP_GA) {
        int i = 0;
        while ((i + 1) * (i + 2) / 2 <= q) i++;
        const int j = q - i * (i + 1) / 2;
        lds[L_S + roff(6 * f + i) + 6 * f + j] += sacc * (lds[L_SC + 6 * f + i] * lds[L_SC + 6 * f + j]);
      } else {
        lds[L_G + 6 * f + (q - SP_GA)] += sacc;
      }
    }
#endif
  }
  PROF(c, 1);
  // phase D's operands (sqrt_info, the raw Jacobians wave ASM_WAVES left in the slot during phase A) and phase E's packed
  // prior are fetched now: their trip to the slot's memory overlaps the zeroing and the barriers in between
#ifdef AVM_TP
  // ten factors on four wavefronts: three rounds of factors that share no frame - {0 2 4 6}, {8 1 3 5}, {7 9}
  constexpr int NIMR = 3;
  auto imu_of = [&](int rd) { return rd == 0 ? 2 * wv : (rd == 1 ? (wv == 0 ? 8 : 2 * wv - 1) : (wv == 0 ? 7 : (wv == 1 ? 9 : -1))); };
  ImuOperands io[NIMR];
#pragma unroll
  for (int rd = 0; rd < NIMR; rd++)
    if (imu_of(rd) >= 0) imu_factor_load(imu_of(rd), io[rd]);
  constexpr int NIT = 12;  // rounds fetched ahead: they cover a prior of up to 77 rows (the tail of a larger one is added straight from the slot)
#else
  ImuOperands io[2];
  if (wv < 5) imu_factor_load(2 * wv, io[0]), imu_factor_load(2 * wv + 1, io[1]);
  constexpr int NIT = (HPK_MAX + NT - 1) / NT;  // 10 rounds cover the largest prior
#endif
  const int npk = c.pn * (c.pn + 1) / 2;
  int dd[NIT];
  double hv[NIT];
  if (c.pn > 0) {
    gcdouble* HPk = c.sc + Scratch::HP;
    const gint* dst = reinterpret_cast<const gint*>(c.sc + Scratch::HP + HPK_MAX);
#pragma unroll
    for (int u = 0; u < NIT; u++) {
      const int idx = min(t + u * NT, npk - 1);
      dd[u] = dst[idx], hv[u] = HPk[idx];
    }
  }
  // rows 66.. of S (the staging area is dead now)
#ifdef AVM_TP
  for (int i = t; i < 99 * SBW + 9 * NPOSE; i += NT) lds[L_SBC + i] = 0.0;  // the speed-bias rows in structural form + the prior's strip
#else
  for (int i = SPP + t; i < SROWS; i += NT) lds[L_S + i] = 0.0;
#endif
  __syncthreads();
  PROF(c, 3);
  // ---- phase D: IMU factors on MFMA, one wavefront per factor; even factors then odd ones (neighbours share a frame)
  {
#ifdef AVM_TP
#pragma unroll
    for (int rd = 0; rd < NIMR; rd++) {
      const int i = imu_of(rd);
      if (i >= 0 && c.psum[max(i, 0)] <= o.max_sum_dt) acc += imu_factor_mfma(c, i, io[rd]);
      __syncthreads();
    }
#else
#pragma unroll
    for (int par = 0; par < 2; par++) {
      if (wv < 5) {
        const int i = 2 * wv + par;
        if (c.psum[i] <= o.max_sum_dt) acc += imu_factor_mfma(c, i, io[par]);
      }
      __syncthreads();
    }
#endif
  }
  PROF(c, 7);
  // ---- phase E: prior  H += Hp (packed values + destinations prepared once per solve), g += J0^T r_p
  if (c.pn > 0) {
    // H += Hp (packed values + destinations, fetched above), g += J0^T r_p (phase A left it in lds[L_DXP])
    {
#pragma unroll
      for (int u = 0; u < NIT; u++)
        if (t + u * NT < npk && dd[u] >= 0) lds[L_S + dd[u]] += hv[u];
#ifdef AVM_TP
      for (int idx = t + NIT * NT; idx < npk; idx += NT) {
        const int d = reinterpret_cast<const gint*>(c.sc + Scratch::HP + HPK_MAX)[idx];
        if (d >= 0) lds[L_S + d] += (c.sc + Scratch::HP)[idx];
      }
#endif
    }
    {
      const int* pidx = ids + I_PIDX;
#ifdef AVM_X
      if (t < c.pn && pidx[t] >= 0) lds[L_G + pidx[t]] += lds[L_DXP + t];
#else
      if (t < c.pn && pidx[t] >= 0) lds[L_G + pidx[t]] += lds[L_DXP + t] + lds[L_DX2 + t];
#endif
    }
  }
  const double cost = block_sum1(acc);
  __syncthreads();
  PROF(c, 8);
  return cost;
}
