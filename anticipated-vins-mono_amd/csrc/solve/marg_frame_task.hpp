// solve/marg_frame_task.hpp - marginalization, phase A: a wavefront's projection factors of the start-0 features (marg_frame_task)
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
AVM_NOINL void marg_frame_task(const WinCtx&, const avm_options&, int b0, int b1, int stage_off) {
  // The wavefront's (at most two) frames b0 < b1 as ONE list of factors, 64 at a time: a chunk may straddle the two frames (5
  // chunks for two frames of 150 factors instead of 3 + 3), the MFMA accumulation is cut at the frame boundary.
  const WinCtx& c = lds_ctx();
  const avm_options& o = lds_opt();
  using namespace mg;
  double* lds = LDS();
  double* stage = lds + stage_off;
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  (void)ids;
  const int lane = threadIdx.x & 63;
  const int n0 = ids[I_NCOV + b0], n1 = b1 < NFR ? ids[I_NCOV + b1] : 0, ntot = n0 + n1;
  Frames fr{lds + L_FR, lds + L_FR + 99};
  const double* xs = lds + L_X;
  const double sqi = o.focal_length / 1.5;
  // FEATURE-MAJOR like the solve's slot (round 3): the lanes of a chunk are consecutive features of one frame, so W / PF / PF2 are
  // written as whole cache lines (they were [feature][column] and [quantity][observation slot]: 8-byte stores 640 and 88 bytes
  // apart, 80 K of this phase's 181 K cycles per window)
  double* W = c.sc + Scratch::W;       // Wt[MNW][WLE]: E^T F, column-major over the features
  double* PF = c.sc + Scratch::PF;     // [PQ_JEX][NFR][WLE] Ji^T Je (6), Je^T Je, Je^T r of the factor (feature e, frame b)
  double* PF2 = c.sc + Scratch::PF + MPF2;  // [7][NFR][WLE] Jex^T Je (6), Jtd^T Je
  const double td = lds[L_RIC + 19];   // para_Td (0 unless estimate_td)
  d4 D00 = {0, 0, 0, 0}, D10 = {0, 0, 0, 0}, D11 = {0, 0, 0, 0}, E00 = {0, 0, 0, 0}, E10 = {0, 0, 0, 0}, E11 = {0, 0, 0, 0};
  const int drow = lane >> 4, dcol = lane & 15;
  // COMPACT (no time offset in the problem: the reference's default): Jj's translation columns are minus Ji's (projection_factor.cpp:
  // 81-95: both are +-reduce ric^T Rj^T), so the staged row is [Jj_r 0-2 | Ji_t 3-5 | Ji_r 6-8 | r 9 | Jex 10-15] - ONE 16-column tile
  // and ONE X^T X product per k-step instead of three; the three Gram tiles the scatter below works on are read back out of it
  // (entries of other lanes through ds_bpermute, signs for the columns that stand for Jj_t) when a frame ends.
  const bool cp = !c.est_td;
  auto gram_get = [&](const d4& G, int Rs, int Cs) {  // entry (Rs, Cs) of a 16 x 16 accumulator tile, for every lane its own
    const int src = (Rs & 3) * 16 + Cs, q = Rs >> 2;
    const double v0 = __shfl(G[0], src, 64), v1 = __shfl(G[1], src, 64), v2 = __shfl(G[2], src, 64), v3 = __shfl(G[3], src, 64);
    return q == 0 ? v0 : (q == 1 ? v1 : (q == 2 ? v2 : v3));
  };
  auto cmap = [](int p, double& sg) {  // column p of [Jj | Ji | r] -> its column in the compact row, and its sign
    sg = p < 3 ? -1.0 : 1.0;
    return p < 3 ? 3 + p : (p < 6 ? p - 3 : (p < 9 ? p - 3 : (p < 12 ? p - 3 : 9)));
  };
  auto end_frame = [&](int b) {  // the blocks frame b owns, from the accumulators
    double* PART = c.sc + Scratch::PART + (size_t)b * PARTW;
    D00 += E00, D10 += E10, D11 += E11;
    if (cp) {
      const d4 G = D00 + D10;  // (all four chains of the one tile)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = drow + 4 * r;
        double sr, sc2;
        const int mr = cmap(min(row, 12), sr), mc = cmap(min(dcol, 12), sc2);
        const double g00 = gram_get(G, mr, mc), g10 = gram_get(G, 10 + min(row, 5), mc), g11 = gram_get(G, 10 + min(row, 5), 10 + min(dcol, 5));
        D00[r] = (row < 13 && dcol < 13) ? sr * sc2 * g00 : 0.0;
        D10[r] = (row < 6 && dcol < 13) ? sc2 * g10 : 0.0;
        D11[r] = (row < 6 && dcol < 6) ? g11 : 0.0;
      }
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = drow + 4 * r;
      // D00: rows/cols over [Jj | Ji | r]
      if (row < 6 && dcol <= row) lds[L_S + roff(6 * b + row) + 6 * b + dcol] = D00[r];                   // (b,b)
      if (row < 6 && dcol >= 6 && dcol < 12) lds[L_S + roff(6 * b + row) + (dcol - 6)] = D00[r];          // (b,0)
      if (row < 6 && dcol == 12) lds[M_G + 6 * b + row] = D00[r];                                         // g_b
      if (row >= 6 && row < 12) {
        const int i = row - 6;
        if (dcol >= 6 && dcol < 12 && dcol - 6 <= i) PART[MP_AA + i * (i + 1) / 2 + (dcol - 6)] = D00[r]; // (0,0)
        if (dcol == 12) PART[MP_GA + i] = D00[r];                                                          // g_0
      }
      // D10: rows = [Jex | Jtd] (7), cols = [Jj | Ji | r]
      if (row < 7) {
        if (dcol < 6) PART[MP_XB + row * 6 + dcol] = D10[r];                    // ([ex td], pose b)
        if (dcol >= 6 && dcol < 12) PART[MP_XA + row * 6 + (dcol - 6)] = D10[r]; // ([ex td], pose 0)
        if (dcol == 12) PART[MP_GX + row] = D10[r];                             // g_[ex td]
        if (dcol <= row) PART[MP_XX + row * (row + 1) / 2 + dcol] = D11[r];     // ([ex td], [ex td])
      }
    }
    D00 = D10 = D11 = E00 = E10 = E11 = d4{0, 0, 0, 0};
  };
  // inputs of a chunk (feature id, its two observations) are fetched one chunk ahead, as in the solve's frame task (round 5: the
  // id and then the observations were two dependent trips to memory at the top of every chunk)
  int e_nx = 0, b_nx = b0, s0_nx = 0;
  double ob_nx[4] = {0, 0, 0, 0};
  auto fetch = [&](int chunk0) {
    const int ic = min(chunk0 + lane, max(ntot - 1, 0));
    b_nx = ic < n0 ? b0 : b1;
    e_nx = c.cov[b_nx * MAXE + (ic < n0 ? ic : ic - n0)];  // (inactive lanes repeat the last factor: valid, never stored)
    s0_nx = ids[I_FOBS + e_nx];
    const int s = s0_nx + b_nx;
    ob_nx[0] = c.obs[2 * s0_nx], ob_nx[1] = c.obs[2 * s0_nx + 1], ob_nx[2] = c.obs[2 * s], ob_nx[3] = c.obs[2 * s + 1];
  };
  if (ntot > 0) fetch(0);
  for (int chunk0 = 0; chunk0 < ntot; chunk0 += 64) {
    const int idx = chunk0 + lane;
    const bool act = idx < ntot;
    const int b = b_nx, e = e_nx, s0 = s0_nx, s = s0 + b;
    const double ob0 = ob_nx[0], ob1 = ob_nx[1], ob2 = ob_nx[2], ob3 = ob_nx[3];
    if (chunk0 + 64 < ntot) fetch(chunk0 + 64);
    double r[2] = {0, 0}, Ji[12], Jj[12], Je[2] = {0, 0}, Jx[12], Jt[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 12; k++) Ji[k] = 0, Jj[k] = 0, Jx[k] = 0;
    if (act) {
      double ob[4] = {ob0, ob1, ob2, ob3}, ai[4] = {0, 0, 0, 0}, aj[4] = {0, 0, 0, 0};
      if (c.est_td) {  // ProjectionTdFactor (estimator.cpp:874-885)
#pragma unroll
        for (int k = 0; k < 4; k++) ai[k] = c.aux[4 * s0 + k], aj[k] = c.aux[4 * s + k];
        td_shift(ob, ai, aj, td, o.tr, o.row);
      }
      proj_eval<true>(xs, fr, lds + L_RIC, lds + L_RIC + 9, ob[0], ob[1], ob[2], ob[3], xs[XLAM + e], 0, b, sqi, o.cauchy_a, true, r, Ji, Jj,
                      Je, Jx, Jt, ai[0], ai[1], aj[0], aj[1]);
      if (!c.est_td) Jt[0] = Jt[1] = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) {
        W[(size_t)(6 * b + k) * WLE + e] = Jj[k] * Je[0] + Jj[6 + k] * Je[1];
        if (k >= 3) PF[(size_t)((PQ_JI + k) * NFR + b) * WLE + e] = Ji[k] * Je[0] + Ji[6 + k] * Je[1];  // (k < 3: minus W's entry, as in the solve's frame task)
        PF2[(size_t)(k * NFR + b) * WLE + e] = Jx[k] * Je[0] + Jx[6 + k] * Je[1];
      }
      PF[(size_t)(PQ_HEE * NFR + b) * WLE + e] = Je[0] * Je[0] + Je[1] * Je[1];
      PF[(size_t)(PQ_GE * NFR + b) * WLE + e] = Je[0] * r[0] + Je[1] * r[1];
      if (c.est_td) PF2[(size_t)((PQ_JTD - PQ_JEX) * NFR + b) * WLE + e] = Jt[0] * Je[0] + Jt[1] * Je[1];  // (without a time offset the per-feature sums take a zero instead)
    }
    // staged column-major like the solve kernel's frame tasks (Jj 0-5 | Ji 6-11 | r 12 | Jex 13-18): one 16-byte store
    // per column, contiguous across the lanes; inactive lanes stage zeros, so no row needs masking.  The tile holds half
    // a chunk: lanes 0-31 stage and the wavefront multiplies, then lanes 32-63.
    const int nact = min(64, ntot - chunk0);
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
      const int nh = min(max(nact - 32 * half, 0), 32);
      if (nh == 0) break;  // (uniform)
      if ((lane >> 5) == half) {
        dv2* st = reinterpret_cast<dv2*>(stage) + (lane & 31);
        if (cp) {
#pragma unroll
          for (int k = 0; k < 3; k++) {
            st[k * (MXRS / 2)] = dv2{Jj[3 + k], Jj[9 + k]};
            st[(3 + k) * (MXRS / 2)] = dv2{Ji[k], Ji[6 + k]};
            st[(6 + k) * (MXRS / 2)] = dv2{Ji[3 + k], Ji[9 + k]};
          }
          st[9 * (MXRS / 2)] = dv2{r[0], r[1]};
#pragma unroll
          for (int k = 0; k < 6; k++) st[(10 + k) * (MXRS / 2)] = dv2{Jx[k], Jx[6 + k]};
        } else {
#pragma unroll
          for (int k = 0; k < 6; k++) {
            st[k * (MXRS / 2)] = dv2{Jj[k], Jj[6 + k]};
            st[(6 + k) * (MXRS / 2)] = dv2{Ji[k], Ji[6 + k]};
            st[(13 + k) * (MXRS / 2)] = dv2{Jx[k], Jx[6 + k]};
          }
          st[12 * (MXRS / 2)] = dv2{r[0], r[1]};
          st[19 * (MXRS / 2)] = dv2{Jt[0], Jt[1]};
        }
      }
      wave_lds_sync();
      // the factors of frame b0 in this half, then those of b1 (either may be empty)
      const int g0 = chunk0 + 32 * half;                      // list position of the half's first factor
      const int nb0 = min(max(n0 - g0, 0), nh);               // factors of b0 in the half
#pragma unroll 1
      for (int run = 0; run < 2; run++) {
        const int l = run == 0 ? 0 : nb0, l_end = run == 0 ? nb0 : nh;
        if (l_end <= l) continue;  // (uniform)
        if (run == 1 && g0 + l == n0 && n0 > 0) end_frame(b0);  // frame b1 begins exactly here: frame b0 is complete
        // lane group drow takes the two rows of factor 4 j + drow (one 16-byte read per tile), four j at a time: 24 MFMAs on
        // six independent chains; factors outside the run are masked out by their index
        const int j_end = (l_end + 3) >> 2;
        if (cp) {  // one tile: two MFMAs (the two residual rows) per k-step, eight in flight
#pragma unroll 1
          for (int j0 = l >> 2; j0 < j_end; j0 += 4) {
            dv2 u0[4];
#pragma unroll
            for (int u = 0; u < 4; u++) u0[u] = *reinterpret_cast<const dv2*>(stage + dcol * MXRS + 8 * min(j0 + u, 7) + 2 * drow);
#pragma unroll
            for (int u = 0; u < 4; u++) {
              const int f = 4 * (j0 + u) + drow;
              const bool on = f >= l && f < l_end;
              const double a0 = on ? u0[u][0] : 0.0, a1 = on ? u0[u][1] : 0.0;
              if (u & 1) {
                D10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, D10, 0, 0, 0);  // (D10 / E10: the second pair of chains of the
                E10 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, E10, 0, 0, 0);  //  same tile, folded into D00 below)
              } else {
                D00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, D00, 0, 0, 0);
                E00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, E00, 0, 0, 0);
              }
            }
          }
          continue;
        }
#pragma unroll 1
        for (int j0 = l >> 2; j0 < j_end; j0 += 4) {
          dv2 u0[4], u1[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int ro = 8 * min(j0 + u, 7) + 2 * drow;
            u0[u] = *reinterpret_cast<const dv2*>(stage + min(dcol, 12) * MXRS + ro);
            u1[u] = *reinterpret_cast<const dv2*>(stage + (13 + min(dcol, 6)) * MXRS + ro);
          }
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int f = 4 * (j0 + u) + drow;
            const bool on = f >= l && f < l_end;
            const double a0 = (on && dcol < 13) ? u0[u][0] : 0.0, a1 = (on && dcol < 13) ? u0[u][1] : 0.0;
            const double x0 = (on && dcol < 7) ? u1[u][0] : 0.0, x1 = (on && dcol < 7) ? u1[u][1] : 0.0;
            D00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, D00, 0, 0, 0);
            D10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, a0, D10, 0, 0, 0);
            D11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, x0, D11, 0, 0, 0);
            E00 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, E00, 0, 0, 0);
            E10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, a1, E10, 0, 0, 0);
            E11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, x1, E11, 0, 0, 0);
          }
        }
      }
      wave_lds_sync();
    }
  }
  // what is still in the accumulators belongs to the last frame with factors; a frame without factors owns zeros
  if (n1 > 0) {
    end_frame(b1);
    if (n0 == 0) end_frame(b0);
  } else {
    end_frame(b0);
    if (b1 < NFR) end_frame(b1);
  }
}
