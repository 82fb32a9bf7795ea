// solve/marg_feature_sums.hpp - marginalization, phase B: the per-feature sums (marg_feature_sums)
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// Phase B of the marginalization (the per-feature sums) as a function of its own, like marg_schur_phase: its ten-deep load arrays are 140 registers
AVM_NOINL void marg_feature_sums(int nf0) {
  const WinCtx& c = lds_ctx();
  using namespace mg;
  double* lds = LDS();
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  const int t = threadIdx.x;
  double* W = c.sc + Scratch::W;
  const double* PF = c.sc + Scratch::PF;
  const double* PF2 = c.sc + Scratch::PF + MPF2;
  // (the factor of feature e observed in frame k - these features start in frame 0 - sits at [quantity][k][e])
  // the two heavy items of a feature (f == 0: its own pose block, hee, g_e;  f == 11: the ex_pose / td columns) are dealt
  // densely to the threads; the structural zeros of the frames that do not observe it follow in a loop of their own
  for (int idx = t; idx < nf0 * 2; idx += NT) {
    const int e = idx >> 1, f = (idx & 1) ? 11 : 0;
    const int no = ids[I_FNOBS + e];
    {
      const double* P = f == 0 ? PF : PF2;
      // all loads of the feature's (<= 10) factors in flight at once, clamped to its last observation and masked
      // (f == 11: the six ex_pose columns and the td column, W columns 66..72)
      double pv[7][NFR - 1];
#pragma unroll
      for (int k = 1; k < NFR; k++)
#pragma unroll
        for (int q = 0; q < 7; q++) {  // (f == 0, q < 3: Ji_t^T Je is minus the observing frame's W entry - marg_frame_task does not store it twice)
          const int kk = min(k, max(no - 1, 0));
          pv[q][k - 1] = (f == 0 && q < 3) ? W[(size_t)(6 * kk + q) * WLE + e] : P[(size_t)(min(q, (f == 0 || !c.est_td) ? 5 : 6) * NFR + kk) * WLE + e];
        }
      double sacc[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int k = 1; k < NFR; k++)
#pragma unroll
        for (int q = 0; q < 7; q++) sacc[q] += k < no ? pv[q][k - 1] : 0.0;
#pragma unroll
      for (int q = 0; q < 6; q++) W[(size_t)(6 * f + q) * WLE + e] = (f == 0 && q < 3) ? -sacc[q] : sacc[q];
      if (f == 11) W[(size_t)(MNW - 1) * WLE + e] = c.est_td ? sacc[6] : 0.0;
      if (f == 0) {
        double hv[2][NFR - 1];
#pragma unroll
        for (int k = 1; k < NFR; k++) {
          const int kk = min(k, max(no - 1, 0));
          hv[0][k - 1] = PF[(size_t)(PQ_HEE * NFR + kk) * WLE + e], hv[1][k - 1] = PF[(size_t)(PQ_GE * NFR + kk) * WLE + e];
        }
        double he = 0, ge = 0;
#pragma unroll
        for (int k = 1; k < NFR; k++) he += k < no ? hv[0][k - 1] : 0.0, ge += k < no ? hv[1][k - 1] : 0.0;
        lds[L_HEE + e] = he;
        lds[M_GE + e] = ge;
      }
    }
  }
  for (int idx = t; idx < nf0 * (NFR - 1); idx += NT) {
    const int e = idx / (NFR - 1), f = 1 + idx % (NFR - 1);
    if (f >= ids[I_FNOBS + e]) {
#pragma unroll
      for (int q = 0; q < 6; q++) W[(size_t)(6 * f + q) * WLE + e] = 0.0;
    }
  }
}
