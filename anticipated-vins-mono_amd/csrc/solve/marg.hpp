// solve/marg.hpp - marginalization: layout (namespace mg), assembly, elimination, eigen-decomposition, pseudo-inverse
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// =====================================================================================
// Post-solve marginalization: MarginalizationInfo::addResidualBlockInfo / preMarginalize /
// marginalize / getParameterBlocks (vins_estimator/src/factor/marginalization_factor.cpp:89-319)
// as driven by Estimator::optimization() (estimator.cpp:817-990), one workgroup per window.
//
// Variable layout of the joint system: poses 0..65 | speed-bias 66..164 | ex_pose 165..170 (171 dims,
// packed lower triangle in LDS).  Factors: old prior, IMU factor 0, every projection factor of the
// features that start in frame 0 (with their ex_pose Jacobians) — assembled with the same MFMA X^T X
// scheme as the solve (X row = Jj | Ji | r | Jex).  The inverse depths of those features are
// eliminated first as scalar pivots (they are mutually independent; identical to the reference's joint
// eigen-pseudo-inverse of Amm whenever no eigenvalue is clamped), then pose0/speedbias0 through the
// eigen-decomposition of their 15x15 block with the reference's 1e-8 clamp, and the kept block is
// square-rooted through a second eigen-decomposition (parallel cyclic Jacobi in LDS).
// Deterministic block order (the reference's is address-hash order): kept = poses by frame,
// speed-bias by frame, ex_pose.
namespace mg {
constexpr int MXRS = 68;                              // rows per staged column: HALF a chunk (32 factors x 2 residual rows) + 4 (bank spread)
constexpr int MXSTG = 20 * MXRS;                      // column-major staging tile: Jj 0-5 | Ji 6-11 | r 12 | Jex 13-18 | Jtd 19
#ifdef AVM_TP
// THROUGHPUT form of the marginalization (marginalize_tp_kernel in window_solve_tp.o, round 5): the same phases as a 256-thread
// workgroup inside the throughput build's 80 KB of LDS, so that TWO windows are resident per CU - the kernel is a sequence of short
// latency-bound phases (62 % of its wavefront cycles waiting), and a second window fills them.  What makes it fit: the joint system
// only holds the variables a marginalization can touch - poses | speed-bias 0, 1 | ex_pose | td = 91 instead of 172 (packed 33 KB
// instead of 117): IMU factor 0 reaches speed-biases 0 and 1, the projection factors the poses and ex_pose / td, and the old prior
// whatever it kept last time, which for a prior the reference can build is a subset of these (estimator.cpp:904-916 keeps
// para_SpeedBias[1], shifted to frame 0).  A prior with a speed-bias block of a later frame takes the other kernel (the host checks:
// window_prior_fits_marg_tp).  Speed-biases 0 and 1 keep their indices (66 .. 83), so imu_col() and SB0 + 9 fr hold unchanged.
constexpr int MEX0 = 84, MTD = 90, MVARS = 91;
constexpr int MASM = 4;                               // every wavefront assembles (frames 1 8 9 | 2 7 10 | 3 6 + raw IMU, prior | 4 5 + prior)
#else
constexpr int MEX0 = 165, MTD = 171, MVARS = 172;     // 172 variables: poses | speed-biases | ex_pose | td
constexpr int MASM = 7;                               // assembling wavefronts (staging must stay below row 165: half tiles let seven fit)
#endif
constexpr int MROWS = croff(MVARS);
#ifdef AVM_TP
// LDS of the throughput form: S (4232) | EA EV EB / IMU factor rows (2048) | T (1536) | g_e (152) ... b in the scaling vector's place;
// the staging tiles of phase A lie over everything from row 66 of S to 7684, all of it written after phase A only
constexpr int M_WCH = MROWS;                          // Amm, its eigenvectors / inverse factor, Arm (n x 16); before: the IMU factor's rows
constexpr int M_GT = M_WCH + 2048;                    // T = Arm Amm^+ (n x 16)
constexpr int M_GE = M_GT + 96 * 16;                  // g_e (152)
constexpr int M_G = L_SC;                             // b over the 91 variables (the Jacobi scaling is the solve's)
static_assert(M_GE + 152 <= M_G && MVARS <= VEC && M_G + VEC <= L_X, "marg layout (throughput form)");
static_assert(L_S + SPP + MASM * MXSTG <= M_G, "marg staging must not reach b");
#else
constexpr int M_G = MROWS;                            // b over the 171 variables (176)
constexpr int M_GE = M_G + 176;                       // g_e (152)
constexpr int M_WCH = M_GE + 152;                     // [24][80] Schur staging / IMU factor rows
constexpr int M_GT = L_G;                             // T = Arm Amm^+ in the range of the solve's gradient / scaling vectors (unused here)
constexpr int MWCH = 24;
static_assert(M_WCH + MWCH * WLD <= L_G, "marg layout");
static_assert(SPP + MASM * MXSTG <= 13778, "marg staging must not reach the ex_pose rows (roff(165))");
#endif
constexpr int PARTW = 146;  // aa 21 | g_a 6 | [ex td].pose0 42 | [ex td]^2 28 | g_[ex td] 7 | [ex td].pose_b 42
constexpr int MNW = 73;     // columns of W = E^T F here: 66 pose | 6 ex_pose | 1 td
}  // namespace mg

// column of the joint system for W column c (0..71): poses, then ex_pose
AVM_DEV int mg_col(int c) { return c < NPOSE ? c : mg::MEX0 + (c - NPOSE); }  // (td: W column 72 -> variable 171)

// One wavefront's share of the elimination of the start-0 inverse depths (marginalization): the tiles (R, C),
// R in {R0, R1}, C in {C0, C1}, C <= R, of  W^T diag(1 / E^T E) W  over the 72 (padded 80) columns of W = E^T F
// (66 pose + 6 ex_pose columns, row-major [e][72] here).  Padded row 72 carries g_e / (E^T E) in place of a W column,
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

// ... and the two single-wavefront jobs beside the frame tasks (IMU factor 0's raw Jacobians on one lane, the old prior's residual and gradient)
AVM_NOINL void marg_imu0_raw() {
  const WinCtx& c = lds_ctx();
  double* lds = LDS();
  imu_raw<true>(lds + L_X, lds + L_FR, lds_opt(), c.pdelta, c.pjac, c.psum[0], c.lba, c.lbg, 0, c.sc + Scratch::IJRAW);
}
AVM_NOINL void marg_prior_wave(int rb, int re, int buf_off) { (void)prior_wave<true>(L_X, rb, re, buf_off); }
// Phase D of the marginalization (IMU factor 0: J = sqrt_info [r | J_raw], then J^T J and J^T r into the system) as a function of its own
AVM_NOINL void marg_imu0_gram() {
  const WinCtx& c = lds_ctx();
  using namespace mg;
  double* lds = LDS();
  const int t = threadIdx.x;
  const double* IJR = c.sc + Scratch::IJRAW;
  double* IJ = lds + M_WCH;
  for (int idx = t; idx < 465; idx += NT) {
    const int r = idx / 31, cc = idx % 31;
    // (sqrt_info is stored with zeros below its diagonal: all fifteen products, their thirty loads in flight at once - as a loop
    //  from k = r every step was a trip to the slot of its own)
    double ps[15], ij[15];
#pragma unroll
    for (int k = 0; k < 15; k++) ps[k] = c.psqrt[r * 15 + k], ij[k] = IJR[k * 31 + cc];
    double sacc = 0;
#pragma unroll
    for (int k = 0; k < 15; k++) sacc += k >= r ? ps[k] * ij[k] : 0.0;
    IJ[idx] = sacc;
  }
  __syncthreads();
  for (int q = t; q < 495; q += NT) {
    if (q < 465) {
      int p = 0;
      while ((p + 1) * (p + 2) / 2 <= q) p++;
      const int qq = q - p * (p + 1) / 2;
      double sacc = 0;
      for (int r = 0; r < 15; r++) sacc += IJ[r * 31 + 1 + p] * IJ[r * 31 + 1 + qq];
      const int ip = imu_col(0, p), iq = imu_col(0, qq);
      lds[L_S + roff(max(ip, iq)) + min(ip, iq)] += sacc;
    } else {
      const int p = q - 465;
      double sacc = 0;
      for (int r = 0; r < 15; r++) sacc += IJ[r * 31 + 1 + p] * IJ[r * 31];
      lds[M_G + imu_col(0, p)] += sacc;
    }
  }
  __syncthreads();
}
// Phase B of the marginalization (the per-feature sums) as a function of its own, like marg_schur_phase: its ten-deep load arrays are 140 registers
AVM_NOINL void marg_feature_sums(int nf0) {
  const WinCtx& c = lds_ctx();
  using namespace mg;
  double* lds = LDS();
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  const int t = threadIdx.x;
  double* W = c.sc + Scratch::W;
  const double* PF = c.sc + Scratch::PF;
  const double* PF2 = c.sc + Scratch::PF + 8 * (size_t)NFR * WLE;
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
      if (f == 11) W[(size_t)72 * WLE + e] = c.est_td ? sacc[6] : 0.0;
      if (f == 0) {
        double hv[2][NFR - 1];
#pragma unroll
        for (int k = 1; k < NFR; k++) {
          const int kk = min(k, max(no - 1, 0));
          hv[0][k - 1] = PF[(size_t)(6 * NFR + kk) * WLE + e], hv[1][k - 1] = PF[(size_t)(7 * NFR + kk) * WLE + e];
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
  double* PF = c.sc + Scratch::PF;     // [8][NFR][WLE] Ji^T Je (6), Je^T Je, Je^T r of the factor (feature e, frame b)
  double* PF2 = c.sc + Scratch::PF + 8 * (size_t)NFR * WLE;  // [7][NFR][WLE] Jex^T Je (6), Jtd^T Je
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
        if (dcol >= 6 && dcol < 12 && dcol - 6 <= i) PART[i * (i + 1) / 2 + (dcol - 6)] = D00[r];         // (0,0)
        if (dcol == 12) PART[21 + i] = D00[r];                                                            // g_0
      }
      // D10: rows = [Jex | Jtd] (7), cols = [Jj | Ji | r]
      if (row < 7) {
        if (dcol < 6) PART[104 + row * 6 + dcol] = D10[r];                      // ([ex td], pose b)
        if (dcol >= 6 && dcol < 12) PART[27 + row * 6 + (dcol - 6)] = D10[r];   // ([ex td], pose 0)
        if (dcol == 12) PART[97 + row] = D10[r];                                // g_[ex td]
        if (dcol <= row) PART[69 + row * (row + 1) / 2 + dcol] = D11[r];        // ([ex td], [ex td])
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
        if (k >= 3) PF[(size_t)(k * NFR + b) * WLE + e] = Ji[k] * Je[0] + Ji[6 + k] * Je[1];  // (k < 3: minus W's entry, as in the solve's frame task)
        PF2[(size_t)(k * NFR + b) * WLE + e] = Jx[k] * Je[0] + Jx[6 + k] * Je[1];
      }
      PF[(size_t)(6 * NFR + b) * WLE + e] = Je[0] * Je[0] + Je[1] * Je[1];
      PF[(size_t)(7 * NFR + b) * WLE + e] = Je[0] * r[0] + Je[1] * r[1];
      if (c.est_td) PF2[(size_t)(6 * NFR + b) * WLE + e] = Jt[0] * Je[0] + Jt[1] * Je[1];  // (without a time offset the per-feature sums take a zero instead)
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

// Cyclic Jacobi eigen-decomposition of the symmetric n x n matrix A (row-major, leading dimension ld) in LDS.
// Only the LOWER triangle of A is read and written.  On return the diagonal of A holds the eigenvalues and
// the columns of V the eigenvectors (A0 = V diag V^T).
// Round-robin pairing: n/2 disjoint rotations per step.  A <- J^T A J is applied as independent 2x2 blocks
// (rows of pair k1, columns of pair k2, k1 >= k2); V <- V J with threads grouped by pair so the rotation is
// loaded once for several rows.  The step is LDS-instruction bound, so every access is kept to the minimum:
// rotation table read as double2 / int2, no mirrored writes.  Two barriers per step.
template <int NTH>
AVM_NOINL int jacobi_eig_lds(int A_off, int V_off, int n, int ld, int rot_off) {
  double* A = LDS() + A_off;
  double* V = LDS() + V_off;
  double2* rcs = reinterpret_cast<double2*>(LDS() + rot_off);        // [np] (c, s)
  int2* rpq = reinterpret_cast<int2*>(LDS() + rot_off + 2 * 64);     // [np] (p, q), p < q
  double* red = LDS() + L_RED;
  constexpr bool WAVE = NTH == 64;  // a single wavefront: wave-level ordering of its LDS traffic is enough
  auto sync = [&]() {
    if (WAVE)
      wave_lds_sync();
    else
      __syncthreads();
  };
  const int t = WAVE ? (threadIdx.x & 63) : threadIdx.x;
  const int ne = (n + 1) & ~1, np = ne >> 1;
  for (int i = t; i < n * n; i += NTH) V[(i / n) * ld + i % n] = (i / n == i % n) ? 1.0 : 0.0;
  // static work assignment
  //  - blocks (k1 >= k2): up to MAXB per thread
  //  - V: thread -> pair kv = t / tpp, rows (t % tpp) + tpp * m
  constexpr int MAXB = 3, MAXR = 8;
  const int nblk = np * (np + 1) / 2;
  short bk1[MAXB], bk2[MAXB];
#pragma unroll
  for (int u = 0; u < MAXB; u++) {
    const int idx = t + u * NTH;
    bk1[u] = -1, bk2[u] = 0;
    if (idx < nblk) {
      int k1 = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
      while ((k1 + 1) * (k1 + 2) / 2 <= idx) k1++;
      while (k1 * (k1 + 1) / 2 > idx) k1--;
      bk1[u] = (short)k1, bk2[u] = (short)(idx - k1 * (k1 + 1) / 2);
    }
  }
  const int tpp = max(1, NTH / np);          // threads per pair for the V update
  const int kv = t / tpp, rv0 = t % tpp;     // pair and first row of this thread (kv >= np: idle)
  sync();
  auto Lw = [&](int i, int j) -> double& { return A[max(i, j) * ld + min(i, j)]; };
  int sweeps = 0;
  for (int sweep = 0; sweep < 20; sweep++) {
    // converged when every |a_pq| <= tol sqrt(a_pp a_qq) (relative criterion: keeps the small eigenvalues
    // accurate, which matters for the 1e-8 clamp next to eigenvalues of 1e12)
    double off = 0;
    for (int i = t; i < n * n; i += NTH) {
      const int r = i / n, q = i % n;
      if (r <= q) continue;
      const double v = fabs(A[r * ld + q]);
      const double sc = sqrt(fabs(A[r * ld + r]) * fabs(A[q * ld + q]));
      off = fmax(off, sc > 0.0 ? v / sc : (v > 0.0 ? 1.0 : 0.0));
    }
    if (WAVE) {
      off = wave_max(off);
    } else {
      off = block_max<NTH>(off, red);
    }
    if (off <= 1e-15) break;
    sweeps++;
    for (int step = 0; step < ne - 1; step++) {
      if (t < np) {
        const int a = t == 0 ? ne - 1 : (step + t) % (ne - 1);
        const int b = t == 0 ? step : (step - t + (ne - 1)) % (ne - 1);
        const int pI = min(a, b), qI = max(a, b);
        double cs = 1.0, sn = 0.0;
        if (qI < n) {
          const double apq = A[qI * ld + pI];
          if (fabs(apq) > 1e-300) {
            const double tau = (A[qI * ld + qI] - A[pI * ld + pI]) / (2.0 * apq);
            const double tt = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            cs = fast_rsqrt(1.0 + tt * tt);
            sn = tt * cs;
          }
        }
        rcs[t] = double2{cs, sn};
        rpq[t] = int2{pI, qI};
      }
      sync();
#pragma unroll
      for (int u = 0; u < MAXB; u++) {
        if (bk1[u] < 0) continue;
        const int k1 = bk1[u], k2 = bk2[u];
        const int2 pq1 = rpq[k1], pq2 = rpq[k2];
        const double2 r1v = rcs[k1], r2v = rcs[k2];
        const int p1 = pq1.x, q1 = pq1.y, p2 = pq2.x, q2 = pq2.y;
        const double c1 = r1v.x, s1 = r1v.y, c2 = r2v.x, s2 = r2v.y;
        const bool r1 = q1 < n, r2 = q2 < n;  // a dummy partner (odd n) leaves its line untouched (c = 1, s = 0)
        if (k1 != k2) {
          double& e00 = Lw(p1, p2);
          const double a00 = e00, a01 = r2 ? Lw(p1, q2) : 0.0, a10 = r1 ? Lw(q1, p2) : 0.0, a11 = (r1 && r2) ? Lw(q1, q2) : 0.0;
          const double b00 = c1 * a00 - s1 * a10, b01 = c1 * a01 - s1 * a11;
          const double b10 = s1 * a00 + c1 * a10, b11 = s1 * a01 + c1 * a11;
          e00 = c2 * b00 - s2 * b01;
          if (r2) Lw(p1, q2) = s2 * b00 + c2 * b01;
          if (r1) Lw(q1, p2) = c2 * b10 - s2 * b11;
          if (r1 && r2) Lw(q1, q2) = s2 * b10 + c2 * b11;
        } else {
          // diagonal block of the pair itself: [app apq; apq aqq] -> diag(app - t apq, aqq + t apq)
          const double app = A[p1 * ld + p1];
          if (r1) {
            const double aqq = A[q1 * ld + q1], apq = A[q1 * ld + p1];
            A[p1 * ld + p1] = c1 * c1 * app - 2.0 * c1 * s1 * apq + s1 * s1 * aqq;
            A[q1 * ld + q1] = s1 * s1 * app + 2.0 * c1 * s1 * apq + c1 * c1 * aqq;
            A[q1 * ld + p1] = (c1 * c1 - s1 * s1) * apq + c1 * s1 * (app - aqq);
          }
        }
      }
      if (kv < np) {
        const int2 pq = rpq[kv];
        if (pq.y < n) {
          const double2 cs2 = rcs[kv];
#pragma unroll
          for (int m = 0; m < MAXR; m++) {
            const int i = rv0 + tpp * m;
            if (i < n) {
              const double x = V[i * ld + pq.x], y = V[i * ld + pq.y];
              V[i * ld + pq.x] = cs2.x * x - cs2.y * y;
              V[i * ld + pq.y] = cs2.y * x + cs2.x * y;
            }
          }
        }
      }
      sync();
    }
  }
  return sweeps;
}

// Fast path of the 16 x 16 pseudo-inverse of the marginalization (Amm^+ = V diag(lambda > eps ? 1 / lambda : 0) V^T,
// marginalization_factor.cpp:283-286) for the usual case that NO eigenvalue is clamped: then Amm^+ is the plain inverse,
// which one wavefront gets from the same register-resident square-root-free Cholesky as the solve's diagonal blocks
// (lanes 0..15 = rows, lanes 16..31 = rows of the identity -> L^-T), ~3K cycles instead of ~135K for the Jacobi sweeps.
// The condition is checked rigorously: lambda_min >= 1 / trace(Amm^-1), so "trace(Amm^-1) < 1 / eps" (and positive
// pivots) proves that every eigenvalue is above eps; otherwise the caller falls back to the eigen-decomposition.
// On success the result is handed over in the eigen-solver's output format: EV[i][c] = (L D^1/2)^-T rows, diag(EA) = the
// pivots d_c, so that EV diag(1 / d) EV^T = Amm^-1.  EA is left untouched on failure.  Call with one full wavefront.
AVM_NOINL bool pinv16_cholesky(double* EA, double* EV, int m, double eps) {  // (outlined: its sixteen-register row was spilled inside the kernel body)
  constexpr int NB = 16;
  const int r = threadIdx.x & 63;
  const bool idl = (r & 48) == 16;
  double a[NB];
  {
    const int rc = r & 15;
#pragma unroll
    for (int k = 0; k < NB; k++) a[k] = idl ? (rc == k ? 1.0 : 0.0) : EA[rc * NB + min(k, rc)];
  }
  double uprev = 0.0, dvec = 1.0;
#pragma unroll
  for (int j = 0; j < NB; j++) {
    if (j > 0) a[j] = fma(-uprev, readlane_d(a[j - 1], j), a[j]);
    const double djj = readlane_d(a[j], j);
    dvec = (r & 15) == j ? djj : dvec;
    double y = __builtin_amdgcn_rcp(djj), e = 0;
    AVM_PIVOT_TAIL(0, false)
    e = fma(-djj, y, 1.0);
    AVM_PIVOT_TAIL(1, false)
    y = fma(y, e, y);
    AVM_PIVOT_TAIL(2, false)
    e = fma(-djj, y, 1.0);
    AVM_PIVOT_TAIL(3, false)
    y = fma(y, e, y);
    AVM_PIVOT_TAIL(4, false)
    uprev = a[j] * y;
  }
  // trace(Amm^-1) = sum_i sum_c x_i[c]^2 / d_c over the real indices; pivots must be positive
  double tr = 0.0;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < NB; c++) {
    const double dc = readlane_d(dvec, c);
    if (c < m) {
      bad |= !(dc > 0.0);
      tr = fma(a[c] * a[c], 1.0 / dc, tr);
    }
  }
  tr = (idl && (r & 15) < m) ? tr : 0.0;
  tr = wave_sum(tr);
  const bool fast = !bad && tr * eps < 1.0;  // (NaN compares false)
  if (fast) {
    if (idl) {
#pragma unroll
      for (int c = 0; c < NB; c++) EV[(r & 15) * NB + c] = a[c];
    }
    wave_lds_sync();
    if (r < NB) EA[r * NB + r] = dvec;  // pad indices (>= m) carry pivot 1 and are masked by the consumer
  }
  return fast;
}
