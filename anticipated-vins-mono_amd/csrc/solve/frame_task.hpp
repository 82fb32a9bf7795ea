// solve/frame_task.hpp - the frame task of the latency and throughput builds: projection factors -> X^T X on the matrix cores
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// All projection factors observed in frame b, by one wavefront (lane = factor, 64 at a time).
// Each lane evaluates its factor, then the 2 x 13 rows [Jj | Ji | r] of the 64 factors are staged in LDS
// and X^T X is accumulated with v_mfma_f64_16x16x4: one 16x16 product gives Jj^T Jj (block b,b),
// Jj^T Ji (block b,a), Ji^T Ji (goes to block a,a), Jj^T r and Ji^T r at once — the cross-lane reduction
// is done by the matrix core.  Features are sorted by start frame, so factors with the same start frame a
// are consecutive; the B operand is masked per a-run to keep the (b,a)/(a,a) blocks separate.
// Blocks (b,b), (b,a) and g_b belong to this frame only and are written straight into LDS; the (a,a)
// contributions go to PART[b][a] in the scratch slot and are summed in a fixed order afterwards.
// One wavefront takes ALL the frames assigned to it as one list of factors (frames in ascending order, each frame's factors
// in feature order), 64 at a time: a chunk may straddle two frames, so a wavefront with two frames of 150 factors runs 5
// chunks instead of 3 + 3.  The runs of the MFMA accumulation are keyed by (frame b, start frame a).
AVM_DEV double frame_task(const WinCtx&, const avm_options&, int wvi, int stage_off) {
  const WinCtx& c = lds_ctx();
  const avm_options& o = lds_opt();
  double* lds = LDS();
  double* stage = lds + stage_off;
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  (void)ids;
  const int lane = threadIdx.x & 63;
  Frames fr{lds + L_FR, lds + L_FR + 99};
  const double* xs = lds + L_X;
  const double sqi = o.focal_length / 1.5;
  double* W = c.sc + Scratch::W;
  double* PF = c.sc + Scratch::PF;
  double* PART0 = c.sc + Scratch::PART;
  const double* scl = lds + L_SC;
  d4 Dtot = {0, 0, 0, 0}, Drun = {0, 0, 0, 0}, Drun1 = {0, 0, 0, 0}, Drun2 = {0, 0, 0, 0}, Drun3 = {0, 0, 0, 0};
  int a_run = -1, b_run = -1, pmask = 0;
  double cost = 0;
  const int drow = lane >> 4, dcol = lane & 15;
  // end offsets of the frames in this wavefront's list (a frame of another wavefront has zero width); wave-uniform values
  // kept in scalar registers, so that locating a factor costs a few compares and no LDS traffic
  int endo[NFR];
  endo[0] = 0;
  {
    int off = 0;
#pragma unroll
    for (int bb = 1; bb < NFR; bb++) {
      off += ids[I_FRW + bb] == wvi ? ids[I_NCOV + bb] : 0;
      endo[bb] = __builtin_amdgcn_readfirstlane(off);
    }
  }
  const int ntot = endo[NFR - 1];  // factors of this wavefront's frames
  // position in the wavefront's list -> (frame, index in the frame's list); past the end: the last factor (masked by `act`)
  auto locate = [&](int idx, int& bl, int& pos) {
    const int ic = min(idx, ntot - 1);
    int start = 0;
    bl = 1;
#pragma unroll
    for (int bb = 1; bb < NFR - 1; bb++) {
      const bool past = ic >= endo[bb];
      bl += past ? 1 : 0;
      start = past ? endo[bb] : start;
    }
    pos = ic - start;
  };
  auto flush = [&]() {  // ends the run (b_run, a_run)
    if (a_run < 0) return;
    Drun = (Drun + Drun1) + (Drun2 + Drun3);
    Drun1 = Drun2 = Drun3 = d4{0, 0, 0, 0};
    double* PART = PART0 + (size_t)b_run * NFR * SPARTW;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = drow + 4 * r;
      const double v = Drun[r];
      // (entries of S are written Jacobi-scaled: s_i s_j H_ij, with s = 1 until the first evaluation has fixed it)
      if (row < 6 && dcol >= 6 && dcol < 12)
        lds[L_S + roff(6 * b_run + row) + 6 * a_run + (dcol - 6)] = v * (scl[6 * b_run + row] * scl[6 * a_run + (dcol - 6)]);  // Jj^T Ji
      if (row >= 6 && row < 12) {
        const int i = row - 6;
        if (dcol >= 6 && dcol < 12 && dcol - 6 <= i) PART[a_run * SPARTW + SP_AA + i * (i + 1) / 2 + (dcol - 6)] = v;  // Ji^T Ji (lower)
        if (dcol == 12) PART[a_run * SPARTW + SP_GA + i] = v;                                                    // Ji^T r
      }
    }
    pmask |= 1 << a_run;
    Dtot += Drun;
    Drun = d4{0, 0, 0, 0};
    a_run = -1;
  };
  auto end_frame = [&]() {  // block (b,b) lower triangle and g_b of the frame that just ended
    flush();
    if (b_run < 0) return;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int row = drow + 4 * r;
      if (row < 6 && dcol <= row) lds[L_S + roff(6 * b_run + row) + 6 * b_run + dcol] = Dtot[r] * (scl[6 * b_run + row] * scl[6 * b_run + dcol]);
      if (row < 6 && dcol == 12) lds[L_G + 6 * b_run + row] = Dtot[r];
    }
    if (lane == 0) ids[I_PMASK + b_run] = pmask;
    Dtot = d4{0, 0, 0, 0};
    pmask = 0;
  };
  // inputs of a chunk (feature id, its two observations) are fetched one chunk ahead: their HBM / L2 latency hides
  // behind the stores, the staging and the MFMA chain of the chunk before
  int e_nx = 0, fa_nx = 0, b_nx = 1;
  double ob_nx[4] = {0, 0, 0, 0};
  auto fetch = [&](int chunk0) {
    int pos;
    locate(chunk0 + lane, b_nx, pos);
    e_nx = c.cov[b_nx * MAXE + pos];
    fa_nx = ids[I_FSTART + e_nx];
    const int s0 = ids[I_FOBS + e_nx], s = s0 + (b_nx - fa_nx);
    ob_nx[0] = c.obs[2 * s0], ob_nx[1] = c.obs[2 * s0 + 1], ob_nx[2] = c.obs[2 * s], ob_nx[3] = c.obs[2 * s + 1];
  };
  if (ntot > 0) fetch(0);
  for (int chunk0 = 0; chunk0 < ntot; chunk0 += 64) {
    const int idx = chunk0 + lane;
    const bool act = idx < ntot;
    const int e = e_nx, fa = fa_nx, b = b_nx;  // (inactive lanes repeat the wavefront's last factor: valid, never stored)
    const double ob0 = ob_nx[0], ob1 = ob_nx[1], ob2 = ob_nx[2], ob3 = ob_nx[3];
    if (chunk0 + 64 < ntot) fetch(chunk0 + 64);
    double r[2] = {0, 0}, Ji[12], Jj[12], Je[2] = {0, 0};
#pragma unroll
    for (int k = 0; k < 12; k++) Ji[k] = 0, Jj[k] = 0;
    if (act) {
      cost += proj_eval<true>(xs, fr, lds + L_RIC, lds + L_RIC + 9, ob0, ob1, ob2, ob3,
                              xs[XLAM + e], fa, b, sqi, o.cauchy_a, true, r, Ji, Jj, Je);
      // (round 5: Ji's translation columns are minus Jj's - set so in proj_eval -, so Ji_t^T Je is exactly -W[6 b + k][e], k < 3: those three products
      //  are not stored a second time, the per-feature sums read them out of W.  Every 8 bytes per factor written here cost 0.1 ms per 4096 windows:
      //  profiles/r05e_experiments.md section 10.)
#pragma unroll
      for (int k = 0; k < 6; k++) {
        W[(6 * b + k) * WLE + e] = Jj[k] * Je[0] + Jj[6 + k] * Je[1];
        if (k >= 3) PF[((PQ_JI + k) * NFR + b) * WLE + e] = Ji[k] * Je[0] + Ji[6 + k] * Je[1];
      }
#ifndef AVM_TP
      PF[(PQ_HEE * NFR + b) * WLE + e] = Je[0] * Je[0] + Je[1] * Je[1];
      PF[(PQ_GE * NFR + b) * WLE + e] = Je[0] * r[0] + Je[1] * r[1];
#endif
    }
#ifdef AVM_TP
    {
      // E^T E and E^T r of the chunk's factors into this wavefront's accumulators (L_ACC, solve/layout.hpp), frame by frame: the frames of a list are in ascending
      // order along the lanes, and a feature occurs once per frame - so the lanes of one frame never meet in an address, and a feature's terms are
      // added in the order of this wavefront's frames, always the same
      const double he = Je[0] * Je[0] + Je[1] * Je[1], ge = Je[0] * r[0] + Je[1] * r[1];
      double* a0 = wvi == 0 ? lds + L_HEE : lds + L_ACC + (2 * (wvi - 1)) * ACCW;
      double* a1 = wvi == 0 ? lds + L_G + NF : lds + L_ACC + (2 * (wvi - 1) + 1) * ACCW;
      int bb = __builtin_amdgcn_readfirstlane(b);
      for (;;) {
        if (act && b == bb) a0[e] += he, a1[e] += ge;
        wave_lds_sync();
        const unsigned long long rest = __ballot(act && b > bb);
        if (!rest) break;
        bb = __builtin_amdgcn_readlane(b, (int)__ffsll((long long)rest) - 1);
      }
    }
    // Throughput build: the staging tile holds HALF a chunk (lanes 0-31 stage and the wavefront multiplies, then lanes 32-63; the
    // scheme of marg_frame_task).  A run that straddles the two halves simply continues: the switches below only act on a new key.
    const int nact = min(64, ntot - chunk0);
    const int key = (b << 4) | fa;  // frames ascending, start frames ascending inside a frame: equal keys are consecutive
#pragma unroll 1
    for (int half = 0; half < 2; half++) {
      const int h0 = 32 * half, lim = min(nact, h0 + 32);
      if (h0 >= nact) break;  // (uniform)
      if ((lane >> 5) == half) {
        dv2* st = reinterpret_cast<dv2*>(stage) + (lane & 31);
#pragma unroll
        for (int k = 0; k < 6; k++) st[k * (XRS_H / 2)] = dv2{Jj[k], Jj[6 + k]}, st[(6 + k) * (XRS_H / 2)] = dv2{Ji[k], Ji[6 + k]};
        st[12 * (XRS_H / 2)] = dv2{r[0], r[1]};
      }
      wave_lds_sync();
      int l = h0;
      while (l < lim) {
        const int k_cur = __shfl(key, l, 64);
        const int l_end = min(l + __popcll(__ballot(act && key == k_cur && lane >= l)), lim);
        if ((k_cur >> 4) != b_run) {
          end_frame();
          b_run = k_cur >> 4;
        }
        if ((k_cur & 15) != a_run) {
          flush();
          a_run = k_cur & 15;
        }
        const int j_end = (l_end - h0 + 3) >> 2;
#pragma unroll 1
        for (int j0 = (l - h0) >> 2; j0 < j_end; j0 += 4) {
          dv2 v[4];
#pragma unroll
          for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const dv2*>(stage + min(dcol, 12) * XRS_H + 8 * min(j0 + u, 7) + 2 * drow);
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int f = h0 + 4 * (j0 + u) + drow;
            const bool in = dcol < 13 && f >= l && f < l_end;
            const double a0 = in ? v[u][0] : 0.0, a1 = in ? v[u][1] : 0.0;
            if (u & 1) {
              Drun2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, Drun2, 0, 0, 0);
              Drun3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, Drun3, 0, 0, 0);
            } else {
              Drun = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, Drun, 0, 0, 0);
              Drun1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, Drun1, 0, 0, 0);
            }
          }
        }
        l = l_end;
      }
      wave_lds_sync();
    }
  }
#else
    // staged column-major, X^T[col][row], row = 2 lane + residual row: one 16-byte store per column, contiguous
    // across the lanes (a row-major [row][14] tile puts the 64 lanes of a store on 8 banks)
    {
      dv2* st = reinterpret_cast<dv2*>(stage) + lane;
#pragma unroll
      for (int k = 0; k < 6; k++) st[k * (XRS / 2)] = dv2{Jj[k], Jj[6 + k]}, st[(6 + k) * (XRS / 2)] = dv2{Ji[k], Ji[6 + k]};
      st[12 * (XRS / 2)] = dv2{r[0], r[1]};
    }
    wave_lds_sync();
    const int nact = min(64, ntot - chunk0);
    const int key = (b << 4) | fa;  // frames ascending, start frames ascending inside a frame: equal keys are consecutive
    int l = 0;
    while (l < nact) {
      const int k_cur = __shfl(key, l, 64);
      const int cnt = __popcll(__ballot(act && key == k_cur));
      const int l_end = l + cnt;
      if ((k_cur >> 4) != b_run) {
        end_frame();
        b_run = k_cur >> 4;
      }
      if ((k_cur & 15) != a_run) {
        flush();
        a_run = k_cur & 15;
      }
      // The k index of X^T X is a summation index: lane group drow takes the two rows of factor 4 j + drow for the
      // k-step pair j (one 16-byte read, conflict-free with the 132-row column stride), four pairs = eight MFMAs at a
      // time with the reads issued together, on four independent chains (an MFMA issues every 16 cycles but completes
      // after 64).  Factors outside the run are masked out by their index, so they add exact zeros.
      const int j_end = (l_end + 3) >> 2;
#pragma unroll 1
      for (int j0 = l >> 2; j0 < j_end; j0 += 4) {
        dv2 v[4];
#pragma unroll
        for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const dv2*>(stage + min(dcol, 12) * XRS + 8 * min(j0 + u, 15) + 2 * drow);
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const int f = 4 * (j0 + u) + drow;
          const bool in = dcol < 13 && f >= l && f < l_end;
          const double a0 = in ? v[u][0] : 0.0, a1 = in ? v[u][1] : 0.0;
          if (u & 1) {
            Drun2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, Drun2, 0, 0, 0);
            Drun3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, Drun3, 0, 0, 0);
          } else {
            Drun = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, a0, Drun, 0, 0, 0);
            Drun1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, a1, Drun1, 0, 0, 0);
          }
        }
      }
      l = l_end;
    }
    wave_lds_sync();
  }
#endif
  end_frame();
  return cost;
}
