// solve/marg_kernel.hpp - the marginalization kernel
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// -DAVM_MARG_MIXED (window_solve_mm.o, window_solve_tp_mm.o: this kernel and nothing else): the marginalization flag PER WINDOW,
// A.marg_flags[w] read inside the window loop, for avm_window_solve_batch_flags.  The flag is still the same for every thread of a
// workgroup, like the `continue` of "MARGIN_SECOND_NEW had nothing to drop", and AVM_MARGIN_NONE is that same report: the caller keeps
// the prior it had.  A build of its own and not a null test in the one kernel: these bodies use the whole register file, and with a flag
// that varies from window to window the latency form makes three more trips to spill memory per window (scripts/isa_spill_trips.py: 22
// against 19).  The launch with one flag for the batch keeps the code it had.
#ifdef AVM_TP
#ifdef AVM_MARG_MIXED
#define AVM_MARG_KERNEL marginalize_tp_mixed_kernel
#else
#define AVM_MARG_KERNEL marginalize_tp_kernel
#endif
#define AVM_MARG_OCC __attribute__((amdgpu_waves_per_eu(2, 2)))  // two four-wavefront workgroups per CU, like the solve beside it
#else
#ifdef AVM_MARG_MIXED
#define AVM_MARG_KERNEL marginalize_mixed_kernel
#else
#define AVM_MARG_KERNEL marginalize_kernel
#endif
#define AVM_MARG_OCC
#endif
__global__ __launch_bounds__(NT) AVM_MARG_OCC void AVM_MARG_KERNEL(SolveArgs A, avm_prior_out PO, int* err, double* scale_out) {
  lds_base_check();
  AVM_PRIO_LIGHT();
  using namespace mg;
  double* lds = LDS();
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const avm_options& o = lds_opt();
  const avm_window_batch& B = A.b;
#ifndef AVM_MARG_MIXED
  const int flag = A.opt.marginalization_flag;
#endif
  for (int w = blockIdx.x; w < B.n_windows; w += gridDim.x) {
#ifdef AVM_MARG_MIXED
    const int flag = A.marg_flags[w];
    const bool not_marginalized = flag == AVM_MARGIN_NONE;
#else
    constexpr bool not_marginalized = false;
#endif
    WinCtx cl;
    cl.prof = A.prof ? as_global(A.prof + (size_t)blockIdx.x * PROF_SLOTS) : nullptr;
    cl.sc = as_global(A.scratch + (size_t)blockIdx.x * Scratch::TOTAL);
    cl.osf = as_global(A.iscratch + (size_t)blockIdx.x * ISCRATCH);
    cl.cov = cl.osf + MAXOBS;
    cl.w = w;
    cl.nf = B.n_feat[w];
    cl.obs = as_global(B.obs_xy + (size_t)w * B.max_obs * 2);
    cl.pdelta = as_global(A.pre_delta + (size_t)w * 100), cl.pjac = as_global(A.pre_jac + (size_t)w * 2250), cl.psqrt = as_global(A.pre_sqrt + (size_t)w * 2250);
    cl.psum = as_global(A.pre_sum_dt + (size_t)w * 10);
    cl.lba = as_global(B.imu_lin_ba + (size_t)w * 30), cl.lbg = as_global(B.imu_lin_bg + (size_t)w * 30);
    cl.pn = B.prior_n ? B.prior_n[w] : 0;
    cl.pnblk = cl.pn > 0 ? B.prior_nblk[w] : 0;
    cl.ldp = B.max_prior;
    cl.pJ = as_global(B.prior_J + (size_t)w * B.max_prior * B.max_prior);
    cl.pr = as_global(B.prior_r + (size_t)w * B.max_prior);
    cl.px0 = as_global(B.prior_x0 + (size_t)w * B.max_pblk * 9);
    cl.nobs_tot = 0;
    cl.est_ex = 0, cl.est_td = (A.opt.estimate_td != 0 && B.obs_vel_td && B.td) ? 1 : 0;
    cl.aux = cl.est_td ? as_global(B.obs_vel_td + (size_t)w * B.max_obs * 4) : nullptr;
    cl.relo_n = 0, cl.has_relo = 0, cl.relo_xy = nullptr;  // (the relocalization factors take no part in the marginalization)
    __syncthreads();  // the previous window's readers of the LDS context are done
    lds_store_ctx(cl, A.opt);
    const WinCtx& c = lds_ctx();
    __syncthreads();
    PROF_T0();
    // ---- load the post-solve state and tables.  Every table entry of this thread is requested before the first one is stored (round 5:
    // written as one loop per table, each load waited for its own store - eight dependent trips to memory per window, half of this phase)
    static_assert(NT >= 160 && 99 <= NT && MAXE <= NT, "one entry of every table per thread");
    {
      const int nfl = c.nf, npb = c.pnblk;
      constexpr int PBT0 = NT >= 512 ? 256 : 160;
      const bool in_f = t < nfl, in_pb = t >= PBT0 && t < PBT0 + npb;
      const int kpb = in_pb ? t - PBT0 : 0;
      const double v_pose = B.pose[(size_t)w * 77 + min(t, 76)], v_sb = B.speedbias[(size_t)w * 99 + min(t, 98)];
      const double v_lam = in_f ? B.inv_depth[(size_t)w * B.max_feat + t] : 1.0;
      const size_t kf = (size_t)w * B.max_feat + (in_f ? t : 0);
      const int v_fs = B.feat_start[kf], v_fn = B.feat_nobs[kf], v_fo = B.feat_obs_begin[kf];
      const double v_ex = B.ex_pose[(size_t)w * 7 + min(t, 6)];
      const double v_td = (t == 7 && c.est_td) ? B.td[w] : 0.0;
      const int v_pk = in_pb ? B.prior_blk_kind[(size_t)w * B.max_pblk + kpb] : 0, v_pf = in_pb ? B.prior_blk_frame[(size_t)w * B.max_pblk + kpb] : 0;
      double ex[7] = {0, 0, 0, 0, 0, 0, 1};
      if (t == 0) {
#pragma unroll
        for (int k = 0; k < 7; k++) ex[k] = B.ex_pose[(size_t)w * 7 + k];
      }
      __builtin_amdgcn_sched_barrier(0);
      for (int i = t; i < MAXPRIOR; i += NT) lds[L_DXP + i] = 0.0, lds[L_RP + i] = 0.0;
#ifdef AVM_TP
      for (int i = t; i < MROWS; i += NT) lds[L_S + i] = 0.0;
      for (int i = t; i < VEC; i += NT) lds[M_G + i] = 0.0;
      for (int i = t; i < 152; i += NT) lds[M_GE + i] = 0.0;
#else
      for (int i = t; i < MROWS + 176 + 152; i += NT) lds[i] = 0.0;  // S, b, g_e
#endif
      for (int i = t; i < 152; i += NT) lds[L_HEE + i] = 0.0;
      if (t < 77) lds[L_X + t] = v_pose;
      if (t < 99) lds[L_X + XSB + t] = v_sb;
      if (t < MAXE) lds[L_X + XLAM + t] = v_lam;
      if (in_f) ids[I_FSTART + t] = v_fs, ids[I_FNOBS + t] = v_fn, ids[I_FOBS + t] = v_fo;
      if (t < 7) lds[L_RIC + 12 + t] = v_ex;
      if (t == 7) lds[L_RIC + 19] = v_td;  // para_Td
      if (in_pb) ids[I_PBLK + kpb * 3] = v_pk, ids[I_PBLK + kpb * 3 + 1] = v_pf;  // the prior's block table
      if (t == 0) {
        double R[9];
        q2R(quat{ex[6], ex[3], ex[4], ex[5]}, R);
        for (int k = 0; k < 9; k++) lds[L_RIC + k] = R[k];
        for (int k = 0; k < 3; k++) lds[L_RIC + 9 + k] = ex[k];
      }
    }
    __syncthreads();
    if (t == 0) {  // offsets and state columns of the prior's blocks (read after the barrier that precedes phase A)
      int off = 0;
      for (int k = 0; k < c.pnblk; k++) {
        const int kind = ids[I_PBLK + k * 3], fr = ids[I_PBLK + k * 3 + 1];
        ids[I_PBLK + k * 3 + 2] = off;
        const int n = kind == AVM_BLK_SPEEDBIAS ? 9 : (kind == AVM_BLK_TD ? 1 : 6);
        for (int q = 0; q < n; q++)
          ids[I_PIDX + off + q] = kind == AVM_BLK_POSE ? fr * 6 + q : (kind == AVM_BLK_SPEEDBIAS ? SB0 + fr * 9 + q : (kind == AVM_BLK_TD ? MTD : MEX0 + q));
        off += n;
      }
    }
    // does the prior take part?  MARGIN_SECOND_NEW needs pose[WINDOW_SIZE-1] in it (estimator.cpp:926-927)
    bool use_prior = c.pn > 0;
    bool has9 = false;
    for (int k = 0; k < c.pnblk; k++)
      if (ids[I_PBLK + k * 3] == AVM_BLK_POSE && ids[I_PBLK + k * 3 + 1] == AVM_WINDOW_SIZE - 1) has9 = true;
    if (not_marginalized || (flag == AVM_MARGIN_SECOND_NEW && !(use_prior && has9))) {
      if (t == 0) PO.n[w] = -1, PO.nblk[w] = 0;  // nothing to do: the caller keeps the old prior
      continue;
    }
    const bool imu0 = flag == AVM_MARGIN_OLD && c.psum[0] < o.max_sum_dt;  // estimator.cpp:841
    if (flag == AVM_MARGIN_OLD) {
      for (int f = 1 + wv; f < NFR; f += NT / 64) {  // start-frame-0 features observed in frame f (ballot compaction, see the solve)
        int n = 0;
        for (int e0 = 0; e0 < c.nf; e0 += 64) {
          const int e = min(e0 + lane, MAXE - 1);
          const bool in = e0 + lane < c.nf && ids[I_FSTART + e] == 0 && f < ids[I_FNOBS + e];
          const unsigned long long m = __ballot(in);
          if (in) c.cov[f * MAXE + n + __popcll(m & ((1ull << lane) - 1ull))] = e;
          n += __popcll(m);
        }
        if (lane == 0) ids[I_NCOV + f] = n;
      }
    } else if (t < NFR) {
      ids[I_NCOV + t] = 0;
    }
    if (t == 0) ids[I_NCOV] = 0;
    build_frames(L_X, 0);
    double* IJR = c.sc + Scratch::IJRAW;
    for (int i = t; i < IJBLK; i += NT) IJR[i] = 0.0;
    __syncthreads();
    int nf0 = 0;  // features starting at frame 0 (they come first)
    for (int e0 = 0; e0 < c.nf; e0 += 64) nf0 += __popcll(__ballot(e0 + lane < c.nf && ids[I_FSTART + min(e0 + lane, MAXE - 1)] == 0));
    PROF(c, 16);
    // ---- phase A: projection factors of the start-0 features || IMU factor 0
#ifdef AVM_TP
    {
      // four wavefronts, one per SIMD: frames {1 8 9} {2 7 10} {3 6} {4 5} (a start-0 feature's track ends early or late: the factor
      // counts fall with the frame, and this deal keeps the sums level), a pair as one list of factors, the third frame after it;
      // wavefront 2 then takes IMU factor 0 and two fifths of the old prior's rows, wavefront 3 the other three fifths (each reads J0
      // along its own rows only; the partial gradients are added in phase E, as in the solve)
      static_assert(NFR == 11 && MASM == 4, "the deal below");
      const int stage = L_S + SPP + wv * MXSTG;
      AVM_PRIO_BULK();
      switch (wv) {
        case 0: marg_frame_task(c, o, 1, 8, stage), marg_frame_task(c, o, 9, NFR, stage); break;
        case 1: marg_frame_task(c, o, 2, 7, stage), marg_frame_task(c, o, 10, NFR, stage); break;
        case 2: marg_frame_task(c, o, 3, 6, stage); break;
        default: marg_frame_task(c, o, 4, 5, stage); break;
      }
      AVM_PRIO_LIGHT();
      if (wv == 2 && lane == 0 && imu0) marg_imu0_raw();
      if (wv >= 2 && use_prior) {
        const int h = (3 * c.pn + 2) / 5;
        if (wv == 2)
          marg_prior_wave(h, c.pn, L_DX2);
        else
          marg_prior_wave(0, h, L_DXP);
      }
    }
#else
    if (wv < MASM) {
      marg_frame_task(c, o, 1 + wv, 1 + wv + MASM, L_S + SPP + wv * MXSTG);  // this wavefront's (at most two) frames
      static_assert(1 + 2 * MASM >= NFR, "two frames per wavefront cover all frames");
    } else if (wv == 7) {
      if (lane == 0 && imu0) marg_imu0_raw();
      // ... and the old prior's residual and gradient (MarginalizationFactor at the current state): dx, r_p, J0^T r_p
      if (use_prior) marg_prior_wave(0, c.pn, L_DXP);
    }
#endif
    __syncthreads();
    PROF(c, 17);
    // ---- phase B: per-feature sums, PART gather
    marg_feature_sums(nf0);
    __syncthreads();  // staging dead: rows >= 66 can be cleared, then the PART sums land (incl. the ex_pose rows)
    for (int i = SPP + t; i < MROWS; i += NT) lds[L_S + i] = 0.0;
    __syncthreads();
    if (flag == AVM_MARGIN_OLD && t < PARTW) {
      const double* PART = c.sc + Scratch::PART;
      const int q = t;  // (rows MEX0 .. MEX0 + 6 = the six ex_pose variables and td)
      // (every frame's PART row was written by its frame task - zeros for a frame without factors -, so all ten loads go out at once:
      //  behind the `I_NCOV > 0` test they were ten dependent trips to the slot)
      double pv[NFR - 1];
#pragma unroll
      for (int b = 1; b < NFR; b++) pv[b - 1] = PART[(size_t)b * PARTW + q];
      if (q < MP_XB) {
        double sacc = 0;
#pragma unroll
        for (int b = 1; b < NFR; b++) sacc += ids[I_NCOV + b] > 0 ? pv[b - 1] : 0.0;
        if (q < MP_GA) {
          int i = 0;
          while ((i + 1) * (i + 2) / 2 <= q) i++;
          lds[L_S + roff(i) + (q - i * (i + 1) / 2)] = sacc;
        } else if (q < MP_XA) {
          lds[M_G + (q - MP_GA)] = sacc;
        } else if (q < MP_XX) {
          lds[L_S + roff(MEX0 + (q - MP_XA) / 6) + (q - MP_XA) % 6] = sacc;
        } else if (q < MP_GX) {
          const int k = q - MP_XX;
          int i = 0;
          while ((i + 1) * (i + 2) / 2 <= k) i++;
          lds[L_S + roff(MEX0 + i) + MEX0 + (k - i * (i + 1) / 2)] = sacc;
        } else {
          lds[M_G + MEX0 + (q - MP_GX)] = sacc;
        }
      } else {
        const int k = q - MP_XB;
#pragma unroll
        for (int b = 1; b < NFR; b++)
          if (ids[I_NCOV + b] > 0) lds[L_S + roff(MEX0 + k / 6) + 6 * b + k % 6] = pv[b - 1];
      }
    }
    __syncthreads();
    PROF(c, 18);
    // ---- phase D: IMU factor 0
    if (imu0) marg_imu0_gram();
    PROF(c, 19);
    // ---- phase E: old prior (MarginalizationFactor at the current state)
    if (use_prior) {
      const int* pidx = ids + I_PIDX;
      prior_jtj_add_lds(c.pJ, c.ldp, c.pn, L_S);
#ifdef AVM_TP
      if (t < c.pn) lds[M_G + pidx[t]] += lds[L_DXP + t] + lds[L_DX2 + t];  // g += J0^T r_p (the two shares of phase A)
#else
      if (t < c.pn) lds[M_G + pidx[t]] += lds[L_DXP + t];  // g += J0^T r_p (left in lds[L_DXP] by phase A)
#endif
    }
    __syncthreads();
    PROF(c, 20);
    // ---- phase F: eliminate the start-0 inverse depths (scalar pivots)
    if (flag == AVM_MARGIN_OLD && nf0 > 0) {
      if (t < MAXE) lds[L_HEE + t] = (t < nf0 && lds[L_HEE + t] > o.marg_eps) ? 1.0 / lds[L_HEE + t] : 0.0;  // 1 / E^T E in place
      __syncthreads();
      marg_schur_phase(nf0);
    }
    __syncthreads();
    PROF(c, 21);
    // ---- phase G: dropped / kept variable lists (ints at I_FSTART.. are dead now)
    int* midx = ids + 0;       // [<=16]
    int* kidx = ids + 16;      // [<=96]
    int* kblk = ids + 120;     // [<=16] id of kept block k : pose f -> f, speedbias f -> 11+f, ex -> 22, td -> 23
    int* cnts = ids + 140;     // m, n, nblk
    __syncthreads();
    if (t == 0) {
      int present = 0;  // bit id
      for (int k = 0; k < c.pnblk; k++) {
        const int kind = ids[I_PBLK + k * 3], fr = ids[I_PBLK + k * 3 + 1];
        present |= 1 << (kind == AVM_BLK_POSE ? fr : (kind == AVM_BLK_SPEEDBIAS ? 11 + fr : (kind == AVM_BLK_TD ? 23 : 22)));
      }
      if (!use_prior) present = 0;
      int m = 0, n = 0, nb = 0;
      if (flag == AVM_MARGIN_OLD) {
        if (imu0) present |= (1 << 0) | (1 << 11) | (1 << 1) | (1 << 12);
        if (nf0 > 0) present |= (1 << 0) | (1 << 22) | (c.est_td ? 1 << 23 : 0);  // ProjectionTdFactor keeps para_Td (estimator.cpp:880-883)
        for (int b = 1; b < NFR; b++)
          if (ids[I_NCOV + b] > 0) present |= 1 << b;
        for (int q = 0; q < 6; q++) midx[m++] = q;
        for (int q = 0; q < 9; q++) midx[m++] = SB0 + q;
        present &= ~((1 << 0) | (1 << 11));
      } else {
        for (int q = 0; q < 6; q++) midx[m++] = 6 * (AVM_WINDOW_SIZE - 1) + q;
        present &= ~(1 << (AVM_WINDOW_SIZE - 1));
      }
      for (int id = 0; id < 24; id++) {
        if (!(present & (1 << id))) continue;
        const int base = id < 11 ? 6 * id : (id < 22 ? SB0 + 9 * (id - 11) : (id == 23 ? MTD : MEX0));
        const int sz = (id >= 11 && id < 22) ? 9 : (id == 23 ? 1 : 6);
        if (n + sz > MAXKEEP || n + sz > PO.max_prior || nb >= MAXPBLK || nb >= PO.max_pblk) {
          atomicMin(err, w);  // (lowest failing window) the host turns this into AVM_ERR_CAPACITY: a truncated kept set would silently lose information
          break;
        }
        kblk[nb++] = id;
        for (int q = 0; q < sz; q++) kidx[n++] = base + q;
      }
      cnts[0] = m, cnts[1] = n, cnts[2] = nb;
    }
    __syncthreads();
    const int m = cnts[0], n = cnts[1], nblk = cnts[2];
    // extract Amm (16x16 at EA), Arm (n x 16 at EB), Arr (n x n), b before the packed matrix is overwritten
    auto Sget = [&](int i, int j) { return lds[L_S + roff(max(i, j)) + min(i, j)]; };
    double* EA = lds + M_WCH;            // Amm 16 x 16, then its eigenvectors next to it
    double* EV = EA + 256;               // 16 x 16
    double* EB = EV + 256;               // Arm : n x 16   (n <= 96 -> 1536)  (M_WCH region holds 1920+; spills into the dead L_G.. vectors)
    // (the 16x16 eigen-solver keeps its rotation records at L_HEE: hee / dxp / rp are dead by now)
    double* BV = lds + L_FR + 198;       // b_m (16), b_r (96): the candidate-state frame slot is unused here
    for (int idx = t; idx < 16 * 16; idx += NT) {
      const int i = idx / 16, j = idx % 16;
      EA[idx] = (i < m && j < m) ? 0.5 * (Sget(midx[i], midx[j]) + Sget(midx[j], midx[i])) : (i == j ? 1.0 : 0.0);
    }
    for (int idx = t; idx < n * 16; idx += NT) {
      const int i = idx / 16, j = idx % 16;
      EB[idx] = j < m ? Sget(kidx[i], midx[j]) : 0.0;
    }
    if (t < 16) BV[t] = t < m ? lds[M_G + midx[t]] : 0.0;
    if (t >= 64 && t < 64 + n) BV[16 + t - 64] = lds[M_G + kidx[t - 64]];
    __syncthreads();
    PROF(c, 22);
    // pseudo-inverse of Amm: Cholesky fast path when provably no eigenvalue is clamped, else the eigen-decomposition
    if (t < 64) {
      const bool fast = pinv16_cholesky(EA, EV, m, o.marg_eps);
      if (t == 0) cnts[3] = fast ? 1 : 0;
    }
    __syncthreads();
    if (!cnts[3]) {
      if (t < 64) jacobi_eig_lds<64>(M_WCH, M_WCH + 256, 16, 16, L_HEE);  // 16 x 16: one wavefront, no block barriers
      __syncthreads();
    }
    PROF(c, 23);
    // Amm^+ = V diag(1/lambda > eps) V^T  -> EA (reuse) ; T = Arm Amm^+ ; A' = Arr - T Amr ; b' = br - T bm
    {
      // (1 / lambda once, by sixteen threads, through LDS - g_e's array is dead since phase F: every thread used to divide sixteen times)
      double* lam_inv = lds + M_GE;
      if (t < 16) lam_inv[t] = (t < m && EA[t * 16 + t] > o.marg_eps) ? 1.0 / EA[t * 16 + t] : 0.0;
      __syncthreads();
      if (t < 256) {
        const int i = t / 16, j = t % 16;
        double sacc = 0;
        for (int k = 0; k < 16; k++) sacc += EV[i * 16 + k] * lam_inv[k] * EV[j * 16 + k];
        EA[t] = (i < m && j < m) ? sacc : 0.0;
      }
      __syncthreads();
    }
    // T = Arm Amm^+ : n x 16, in the LDS range of the solve's gradient / scaling vectors (unused here; it was in the scratch slot:
    // every entry of A' then waited for 16 trips to its memory)
#ifndef AVM_TP
    static_assert(MAXKEEP * 16 <= L_X - L_G, "T fits the dead vectors");
#endif
    static_assert(MAXKEEP <= 96, "T / Arm: 96 rows");
    double* GT = lds + M_GT;
    for (int idx = t; idx < n * 16; idx += NT) {
      const int i = idx / 16, j = idx % 16;
      double sacc = 0;
      for (int k = 0; k < 16; k++) sacc += EB[i * 16 + k] * EA[k * 16 + j];
      GT[idx] = sacc;
    }
    __syncthreads();
    // A' and b' go to the output slots PO.J / PO.r; prior_eig_kernel (prior_eig.hip) turns them into
    // linearized_jacobians / linearized_residuals in place
    {
      double* oJ = PO.J + (size_t)w * PO.max_prior * PO.max_prior;
      double* orr = PO.r + (size_t)w * PO.max_prior;
      // T Amr by 16 x 16 tiles on the matrix cores (K = the 16 dropped columns): lower tiles only - the eigen-solver reads the lower
      // triangle only, as Eigen's SelfAdjointEigenSolver does - dealt to the wavefronts; operands straight from LDS (the scalar form
      // read 32 LDS words per entry: 11 K cycles per window)
      {
        const int lr = lane & 15, lk = lane >> 4, ntl = (n + 15) >> 4;
        for (int tile = wv; tile < ntl * (ntl + 1) / 2; tile += NT / 64) {
          int ti = 0;
          while ((ti + 1) * (ti + 2) / 2 <= tile) ti++;
          const int tj = tile - ti * (ti + 1) / 2;
          const int ra = min(16 * ti + lr, n - 1), rb = min(16 * tj + lr, n - 1);
          d4 D = {0, 0, 0, 0};
#pragma unroll
          for (int mq = 0; mq < 4; mq++) D = __builtin_amdgcn_mfma_f64_16x16x4f64(GT[ra * 16 + lk + 4 * mq], EB[rb * 16 + lk + 4 * mq], D, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const int i = 16 * ti + lk + 4 * r, j = 16 * tj + lr;
            if (i < n && j <= i) {
              const double arr = Sget(kidx[i], kidx[j]), sacc = D[r];
              oJ[(size_t)i * PO.max_prior + j] = arr - sacc;
              // The magnitude the diagonal entry was formed at (|Arr_ii| + |(Arm Amm^+ Amr)_ii|: the bias rows of the kept
              // speed-bias block are differences of two numbers of size 1e10 .. 1e12) goes to the ctx's scale array:
              // prior_eig_kernel's clamp measures an eigenvalue against the rounding noise of ITS variables (prior_eig.hip).
              if (i == j) scale_out[(size_t)w * PO.max_prior + i] = fabs(arr) + fabs(sacc);
            }
          }
        }
      }
      if (t < n) {
        double sacc = 0;
        for (int k = 0; k < 16; k++) sacc += GT[t * 16 + k] * BV[k];
        orr[t] = BV[16 + t] - sacc;
      }
      PROF(c, 24);
      if (t < nblk) {
        const int id = kblk[t];
        const int kind = id < 11 ? AVM_BLK_POSE : (id < 22 ? AVM_BLK_SPEEDBIAS : (id == 23 ? AVM_BLK_TD : AVM_BLK_EXPOSE));
        int fr = id < 11 ? id : (id < 22 ? id - 11 : 0);
        if (kind == AVM_BLK_POSE || kind == AVM_BLK_SPEEDBIAS) {
          if (flag == AVM_MARGIN_OLD)
            fr -= 1;  // addr_shift, estimator.cpp:904-909
          else if (fr == AVM_WINDOW_SIZE)
            fr -= 1;  // estimator.cpp:965-969
        }
        PO.blk_kind[(size_t)w * PO.max_pblk + t] = kind;
        PO.blk_frame[(size_t)w * PO.max_pblk + t] = fr;
        double* x0 = PO.x0 + ((size_t)w * PO.max_pblk + t) * 9;
        const double* src = kind == AVM_BLK_POSE ? lds + L_X + id * 7
                            : (kind == AVM_BLK_SPEEDBIAS ? lds + L_X + XSB + (id - 11) * 9 : lds + L_RIC + (kind == AVM_BLK_TD ? 19 : 12));
        const int gs = kind == AVM_BLK_SPEEDBIAS ? 9 : (kind == AVM_BLK_TD ? 1 : 7);
        for (int q = 0; q < 9; q++) x0[q] = q < gs ? src[q] : 0.0;
      }
      if (t == 0) PO.n[w] = n, PO.nblk[w] = nblk;
    }
    __syncthreads();
    PROF(c, 26);
    if (c.prof && t == 0) c.prof[30] += 1;
  }
}
