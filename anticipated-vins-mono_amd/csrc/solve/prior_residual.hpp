// solve/prior_residual.hpp - the prior's residual, cost and J0^T r_p: prior_residual_dev (a workgroup), prior_wave (one wavefront)
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

#ifndef AVM_TP
// prior residual r_p = r0 + J0 * dx(xs) into lds[L_RP]; returns (to all threads) nothing; needs syncs by caller
AVM_NOINL void prior_residual_dev(const WinCtx&, int xs_off) {
  const WinCtx& c = lds_ctx();
  double* lds = LDS();
  const double* xs = lds + xs_off;
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  (void)ids;
  const int t = threadIdx.x;
  // r_p[i] = r0[i] + sum_k J0[i][k] dx[k] : 4 lanes per row (k = part, part + 4, ...).  The row's entries do not depend on
  // dx: their loads are issued first, so the trip to the slot's memory overlaps the dx computation and the barrier
  const int row = t >> 2, part = t & 3;
  static_assert(NT >= 4 * MAXPRIOR, "one pass over the rows");
  double v[MAXPRIOR / 4], r0 = 0.0;
  {
    gcdouble* Jr = c.pJ + (size_t)min(row, max(c.pn - 1, 0)) * c.ldp;
#pragma unroll
    for (int j = 0; j < MAXPRIOR / 4; j++) v[j] = Jr[min(part + 4 * j, max(c.pn - 1, 0))];  // clamped, masked below
    r0 = c.pr[min(row, max(c.pn - 1, 0))];
  }
  if (t < c.pnblk) {
    const int kind = ids[I_PBLK + t * 3], fr = ids[I_PBLK + t * 3 + 1], off = ids[I_PBLK + t * 3 + 2];
#ifdef AVM_X
    const double* xb = kind == AVM_BLK_POSE ? xs + fr * 7 : (kind == AVM_BLK_SPEEDBIAS ? xs + XSB + fr * 9 : (kind == AVM_BLK_TD ? xs + XTD : xs + XEX));
#else
    // ex_pose is constant in the solve; its current value sits behind ric/tic
    const double* xb = kind == AVM_BLK_POSE ? xs + fr * 7 : (kind == AVM_BLK_SPEEDBIAS ? xs + XSB + fr * 9 : lds + L_RIC + (kind == AVM_BLK_TD ? 19 : 12));
#endif
    double dx[9];
    prior_block_dx(kind, xb, c.px0 + t * 9, dx);
    const int n = kind == AVM_BLK_SPEEDBIAS ? 9 : (kind == AVM_BLK_TD ? 1 : 6);
    for (int k = 0; k < n; k++) lds[L_DXP + off + k] = dx[k];
  }
  __syncthreads();
  {
    double s = 0;
#pragma unroll
    for (int j = 0; j < MAXPRIOR / 4; j++) s += (part + 4 * j < c.pn ? v[j] : 0.0) * lds[L_DXP + part + 4 * j];
    s += lane_xor<1>(s);
    s += lane_xor<2>(s);
    if (row < c.pn && part == 0) lds[L_RP + row] = r0 + s;
  }
  __syncthreads();
}

#endif  // !AVM_TP

// The prior's share of an evaluation on ONE wavefront, with wave-level synchronisation only, so that it runs beside the
// projection factors (whose wavefronts do not touch these LDS ranges) instead of in a phase of its own:
//   dx -> lds[L_DXP],  r_p = r0 + J0 dx -> lds[L_RP],  and (WANT_G) g_p = J0^T r_p -> lds[L_DXP], over dx;
// returns 1/2 |r_p|^2 on every lane.  J0 is read along its rows both times (16 lanes per row for r_p, a lane per column
// for g_p), several rows in flight; every sum has a fixed order.
// Rows [rb, re) of the prior only, dx / g_p in the buffer at buf_off: two wavefronts can share the prior, each with its own buffer;
// their costs and their g_p add up (r_p rows are disjoint).
template <bool WANT_G>
AVM_DEV double prior_wave(int xs_off, int rb, int re, int buf_off) {
  const WinCtx& c = lds_ctx();
  double* lds = LDS();
  const double* xs = lds + xs_off;
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  (void)ids;
  const int lane = threadIdx.x & 63, lr = lane & 15, lg = lane >> 4;
  const int pn = c.pn, pn1 = max(pn - 1, 0);
  if (lane < c.pnblk) {
    const int kind = ids[I_PBLK + lane * 3], fr = ids[I_PBLK + lane * 3 + 1], off = ids[I_PBLK + lane * 3 + 2];
#ifdef AVM_X
    const double* xb = kind == AVM_BLK_POSE ? xs + fr * 7 : (kind == AVM_BLK_SPEEDBIAS ? xs + XSB + fr * 9 : (kind == AVM_BLK_TD ? xs + XTD : xs + XEX));
#else
    // ex_pose is constant in the solve; its current value sits behind ric/tic
    const double* xb = kind == AVM_BLK_POSE ? xs + fr * 7 : (kind == AVM_BLK_SPEEDBIAS ? xs + XSB + fr * 9 : lds + L_RIC + (kind == AVM_BLK_TD ? 19 : 12));
#endif
    double dx[9];
    prior_block_dx(kind, xb, c.px0 + lane * 9, dx);
    const int n = kind == AVM_BLK_SPEEDBIAS ? 9 : (kind == AVM_BLK_TD ? 1 : 6);
    for (int k = 0; k < n; k++) lds[buf_off + off + k] = dx[k];
  }
  wave_lds_sync();
  constexpr int NK = MAXPRIOR / 16, RU = 7;  // 6 column groups of 16; 7 x 4 rows in flight (three trips to the slot's memory for 75 rows)
  double dxv[NK];
#pragma unroll
  for (int j = 0; j < NK; j++) dxv[j] = lr + 16 * j < pn ? lds[buf_off + lr + 16 * j] : 0.0;
  double cost = 0;
  for (int r0 = rb; r0 < re; r0 += 4 * RU) {
    double v[RU][NK], rr[RU];
#pragma unroll
    for (int u = 0; u < RU; u++) {
      const int rc = min(r0 + 4 * u + lg, pn1);
      gcdouble* Jr = c.pJ + (size_t)rc * c.ldp;
#pragma unroll
      for (int j = 0; j < NK; j++) v[u][j] = Jr[min(lr + 16 * j, pn1)];  // clamped; the padding columns meet dx = 0
      rr[u] = c.pr[rc];
    }
#pragma unroll
    for (int u = 0; u < RU; u++) {
      double sacc = 0;
#pragma unroll
      for (int j = 0; j < NK; j++) sacc += v[u][j] * dxv[j];
      sacc += lane_xor<8>(sacc);
      sacc += lane_xor<4>(sacc);
      sacc += lane_xor<2>(sacc);
      sacc += lane_xor<1>(sacc);
      const int row = r0 + 4 * u + lg;
      const double rp = rr[u] + sacc;
      if (lr == 0 && row < re) {
        lds[L_RP + row] = rp;
        cost += 0.5 * rp * rp;
      }
    }
  }
  cost = wave_sum(cost);
  if (WANT_G) {
    wave_lds_sync();
    // g_p[k] = sum_i J0[i][k] r_p[i]: lane = column (k = lane, lane + 64), rows in ascending order, 19 rows in flight
    constexpr int GU = 19;  // (four trips for 75 rows)
    const int k0 = min(lane, pn1), k1 = min(lane + 64, pn1);
    double g0 = 0, g1 = 0;
    for (int i0 = rb; i0 < re; i0 += GU) {
      double a0[GU], a1[GU];
#pragma unroll
      for (int u = 0; u < GU; u++) {
        gcdouble* Jr = c.pJ + (size_t)min(i0 + u, pn1) * c.ldp;
        a0[u] = Jr[k0], a1[u] = Jr[k1];
      }
#pragma unroll
      for (int u = 0; u < GU; u++) {
        const double r = i0 + u < re ? lds[L_RP + min(i0 + u, MAXPRIOR - 1)] : 0.0;
        g0 += a0[u] * r, g1 += a1[u] * r;
      }
    }
    lds[buf_off + lane] = lane < pn ? g0 : 0.0;  // (dx lives in dxv by now)
    if (lane + 64 < MAXPRIOR) lds[buf_off + lane + 64] = lane + 64 < pn ? g1 : 0.0;
  }
  return cost;
}
