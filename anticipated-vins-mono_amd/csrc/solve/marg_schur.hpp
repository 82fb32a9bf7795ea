// solve/marg_schur.hpp - marginalization, phase F: elimination of the start-0 inverse depths (marg_schur_macro_tile, marg_schur_phase)
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// One wavefront's share of the elimination of the start-0 inverse depths (marginalization): the tiles (R, C),
// R in {R0, R1}, C in {C0, C1}, C <= R, of  W^T diag(1 / E^T E) W  over the MNW = 73 (padded 80) columns of W = E^T F
// (66 pose + 6 ex_pose + 1 td column, feature-major Wt[MNW][WLE]: solve/slot.hpp).  Padded row 73 carries g_e / (E^T E) in place of a W column,
// so tile row 4 also delivers the right-hand-side update.  Operands straight from the scratch slot, 8 k-steps of
// loads in flight, no staging, no barriers.
template <int R0, int R1, int C0, int C1>
AVM_DEV void marg_schur_macro_tile(int nf0) {
  using namespace mg;
  const WinCtx& c = lds_ctx();
  double* lds = LDS();
  gcdouble* W = c.sc + Scratch::W;
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  constexpr int NR = R1 >= 0 ? 2 : 1, NC = C1 >= 0 ? 2 : 1;
  constexpr int RB[2] = {R0, R1}, CB[2] = {C0, C1};
  constexpr bool SAME = R0 == C0 && R1 == C1;
  constexpr int KB = 8, NW = MNW;
  d4 D[2][2] = {{{0, 0, 0, 0}, {0, 0, 0, 0}}, {{0, 0, 0, 0}, {0, 0, 0, 0}}};
  for (int e0 = 0; e0 < nf0; e0 += 4 * KB) {
    double vr[2][KB], vc[2][KB], fe[KB], xe[KB];
    // (the k index is a summation index: lane group lk takes the 8 consecutive features e0 + 8 lk .. + 7 = 64 contiguous bytes of a
    //  column of Wt, as in schur_macro_tile; rows clamped, masked afterwards; the features beyond nf0 read stale but finite entries of
    //  the region - WLE leaves room for the 8-feature granularity - and are masked out by `on`)
#pragma unroll
    for (int a = 0; a < NR; a++) {
      gcdv2* src = reinterpret_cast<gcdv2*>(W + (size_t)min(16 * RB[a] + li, NW - 1) * WLE + e0 + 8 * lk);
#pragma unroll
      for (int m2 = 0; m2 < KB / 2; m2++) {
        const dv2 v = src[m2];
        vr[a][2 * m2] = v.x, vr[a][2 * m2 + 1] = v.y;
      }
    }
    if (!SAME) {
#pragma unroll
      for (int b = 0; b < NC; b++) {
        gcdv2* src = reinterpret_cast<gcdv2*>(W + (size_t)min(16 * CB[b] + li, NW - 1) * WLE + e0 + 8 * lk);
#pragma unroll
        for (int m2 = 0; m2 < KB / 2; m2++) {
          const dv2 v = src[m2];
          vc[b][2 * m2] = v.x, vc[b][2 * m2 + 1] = v.y;
        }
      }
    }
#pragma unroll
    for (int m = 0; m < KB; m++) {
      const int ec = min(e0 + 8 * lk + m, nf0 - 1);
      fe[m] = lds[L_HEE + ec], xe[m] = lds[L_HEE + ec] * lds[M_GE + ec];
    }
#pragma unroll
    for (int m = 0; m < KB; m++) {
      const bool on = e0 + 8 * lk + m < nf0;
      double aop[2], bop[2];
#pragma unroll
      for (int a = 0; a < NR; a++) {
        const int col = 16 * RB[a] + li;
        const double w = (on && col < NW) ? vr[a][m] : 0.0;
        aop[a] = col == NW ? (on ? xe[m] : 0.0) : w * fe[m];
        if (SAME) bop[a] = w;
      }
      if (!SAME) {
#pragma unroll
        for (int b = 0; b < NC; b++) bop[b] = (on && 16 * CB[b] + li < NW) ? vc[b][m] : 0.0;
      }
#pragma unroll
      for (int a = 0; a < NR; a++)
#pragma unroll
        for (int b = 0; b < NC; b++)
          if (CB[b] <= RB[a]) D[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[a], bop[b], D[a][b], 0, 0, 0);
    }
  }
#pragma unroll
  for (int a = 0; a < NR; a++)
#pragma unroll
    for (int b = 0; b < NC; b++) {
      if (CB[b] > RB[a]) continue;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int gi = 16 * RB[a] + lk + 4 * r, gj = 16 * CB[b] + li;
        if (gi < NW && gj <= gi) {
          const int si = mg_col(gi), sj = mg_col(gj);
          lds[L_S + roff(max(si, sj)) + min(si, sj)] -= D[a][b][r];
        }
        if (gi == NW && gj < NW) lds[M_G + mg_col(gj)] -= D[a][b][r];
      }
    }
}

// Phase F of the marginalization as a function of its own (round 6): inlined, its accumulators and operands pushed the kernel body's
// allocation so far that the registers holding SPILLED SGPRs were spilled themselves - every thread-range predicate of the kernel then began
// with a trip to scratch memory (106 sites, 32 of them in this phase's scatter).
AVM_NOINL void marg_schur_phase(int nf0) {
#ifdef AVM_TP
  AVM_PRIO_BULK();
  switch (threadIdx.x >> 6) {  // four wavefronts, one per SIMD: 4 | 3 + 1 | 3 | 2 + 2 tiles (as schur_reduce)
    case 0: marg_schur_macro_tile<2, 3, 0, 1>(nf0); break;
    case 1: marg_schur_macro_tile<0, 1, 0, 1>(nf0), marg_schur_macro_tile<4, -1, 4, -1>(nf0); break;
    case 2: marg_schur_macro_tile<2, 3, 2, 3>(nf0); break;
    default: marg_schur_macro_tile<4, -1, 0, 1>(nf0), marg_schur_macro_tile<4, -1, 2, 3>(nf0); break;
  }
  AVM_PRIO_LIGHT();
#else
  switch (threadIdx.x >> 6) {
    case 0: marg_schur_macro_tile<2, 3, 0, 1>(nf0); break;
    case 1: marg_schur_macro_tile<0, 1, 0, 1>(nf0); break;
    case 2: marg_schur_macro_tile<2, 3, 2, 3>(nf0); break;
    case 3: marg_schur_macro_tile<4, -1, 0, 1>(nf0); break;
    case 7: marg_schur_macro_tile<4, -1, 2, 3>(nf0); break;
    case 5: marg_schur_macro_tile<4, -1, 4, -1>(nf0); break;
    default: break;
  }
#endif
}
