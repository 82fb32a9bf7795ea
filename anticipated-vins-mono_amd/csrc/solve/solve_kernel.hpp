// solve/solve_kernel.hpp - the solve kernel: window load, frame deal, TrustRegionMinimizer, gauge fix, summary
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// -DAVM_WIN_LIST: the same kernel over a list of windows, A.win_list[0 .. A.n_list) (avm_window_solve_batch_relo: the plain and the
// relocalizing windows of one batch take different builds).  Scratch slot, iscratch and prof stay the workgroup's; every table is the window's.
#ifdef AVM_WIN_LIST
#define AVM_SOLVE_NAME(k) k##_list_kernel
#define AVM_SOLVE_ARGS SolveListArgs
#else
#define AVM_SOLVE_NAME(k) k##_kernel
#define AVM_SOLVE_ARGS SolveArgs
#endif
#ifdef AVM_X
#define AVM_SOLVE_KERNEL AVM_SOLVE_NAME(window_solve_x)
#define AVM_SOLVE_OCC
#elif defined(AVM_TP)
#define AVM_SOLVE_KERNEL AVM_SOLVE_NAME(window_solve_tp)
#define AVM_SOLVE_OCC __attribute__((amdgpu_waves_per_eu(2, 2)))  // two four-wavefront workgroups per CU: 256 registers each
#else
#define AVM_SOLVE_KERNEL AVM_SOLVE_NAME(window_solve)
#define AVM_SOLVE_OCC
#endif
__global__ __launch_bounds__(NT) AVM_SOLVE_OCC void AVM_SOLVE_KERNEL(AVM_SOLVE_ARGS A) {
  lds_base_check();
  red_init();
  AVM_PRIO_LIGHT();
  double* lds = LDS();
  int* ids = reinterpret_cast<int*>(lds + L_INT);
  // (no thread index of the kernel's own: every segment below takes a fresh one - fresh_tid(), solve/lds.hpp)
  const avm_options& o = lds_opt();
  // The same options from the kernel arguments (scalar registers), for the trust-region loop's own decisions.  A comparison with a value
  // read from LDS is a per-lane branch to the compiler, and every loop scalar that is assigned on one side of such a branch only is merged
  // behind it in a vector register (which is spilled and reloaded), whatever uni() did to the assignment.  With the branches of the loop
  // decided in scalar registers (these options; uni() on what an outlined phase returns or LDS holds) the scalars stay scalar.
  const avm_options& ou = A.opt;
  const avm_window_batch& B = A.b;

#ifdef AVM_WIN_LIST
  for (int li = blockIdx.x; li < A.n_list; li += gridDim.x) {
    const int w = A.win_list ? A.win_list[li] : li;  // (the same for every thread of the workgroup)
#else
  for (int w = blockIdx.x; w < B.n_windows; w += gridDim.x) {
#endif
    WinCtx cl;
    cl.sc = as_global(A.scratch + (size_t)blockIdx.x * Scratch::TOTAL);
    cl.osf = as_global(A.iscratch + (size_t)blockIdx.x * ISCRATCH);
    cl.cov = cl.osf + MAXOBS;
    cl.w = w;
    cl.prof = A.prof ? as_global(A.prof + (size_t)blockIdx.x * PROF_SLOTS) : nullptr;
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
    {
      int tot = 0;
      if (cl.nf > 0) tot = B.feat_obs_begin[(size_t)w * B.max_feat + cl.nf - 1] + B.feat_nobs[(size_t)w * B.max_feat + cl.nf - 1];
      cl.nobs_tot = tot;
    }
#ifdef AVM_X
    cl.est_ex = A.opt.estimate_extrinsic != 0, cl.est_td = A.opt.estimate_td != 0;
    cl.aux = (cl.est_td && B.obs_vel_td) ? as_global(B.obs_vel_td + (size_t)w * B.max_obs * 4) : nullptr;
    if (!cl.aux) cl.est_td = 0;  // (the host refuses estimate_td without the per-observation data)
    cl.has_relo = B.relo_n && B.relo_feat && B.relo_xy && B.relo_pose;
#ifdef AVM_WIN_LIST
    if (A.relo_active && A.relo_active[w] == 0) cl.has_relo = 0;  // (none of the window's relo_* rows is read, relo_pose is not written)
#endif
    cl.relo_n = cl.has_relo ? min(max(B.relo_n[w], 0), cl.nf) : 0;
    cl.relo_xy = cl.relo_n > 0 ? as_global(B.relo_xy + (size_t)w * B.max_feat * 2) : nullptr;
#endif
    __syncthreads();  // the previous window's readers of the LDS context are done
    lds_store_ctx(cl, A.opt);
    const WinCtx& c = lds_ctx();
    __syncthreads();
    PROF_T0();
    long long pq__ = 0;
    (void)pq__;
    PROFQ_T0();
    const long long pw__ = clock64();
    const long long wall0 = A.time_cap_ticks > 0 ? wall_clock64() : 0;  // (only thread 0's copy is ever compared)
    // ---------------- load ----------------
    {  // states
      const int t = fresh_tid();
      for (int i = t; i < 77; i += NT) lds[L_X + i] = B.pose[(size_t)w * 77 + i];
      for (int i = t; i < 99; i += NT) lds[L_X + XSB + i] = B.speedbias[(size_t)w * 99 + i];
      for (int i = t; i < MAXE; i += NT) lds[L_X + XLAM + i] = i < c.nf ? B.inv_depth[(size_t)w * B.max_feat + i] : 1.0;
    }
    {  // the solve's vectors
      const int t = fresh_tid();
#ifdef AVM_X
      for (int i = t; i < VEC; i += NT) lds[L_SC + i] = 1.0, lds[L_ST + i] = 0.0, lds[L_Y + i] = 0.0, lds[L_DD + i] = 1.0;
      if (t < 7) {
        lds[L_X + XEX + t] = B.ex_pose[(size_t)w * 7 + t];
        // relo_Pose is frame 11 of the state; without a relocalization frame it mirrors pose 0 (never read by a factor)
        lds[L_X + 7 * NFR + t] = c.has_relo ? B.relo_pose[(size_t)w * 7 + t] : B.pose[(size_t)w * 77 + t];
      }
      if (t == 7) lds[L_X + XTD] = (c.est_td && B.td) ? B.td[w] : 0.0;
      if (t == 8) lds[L_X + XTD + 1] = 0.0;
#elif defined(AVM_TP)
      for (int i = t; i < VEC; i += NT) lds[L_SC + i] = 1.0, lds[L_ST + i] = 0.0, lds[L_Y + i] = 0.0, lds[L_DD + i] = 1.0;
#else
      for (int i = t; i < VEC; i += NT) lds[L_SC + i] = 1.0, lds[L_ST + i] = 0.0, lds[L_Y + i] = 0.0, lds[L_DG + i] = 0.0, lds[L_DD + i] = 1.0;
#endif
      for (int i = t; i < MAXPRIOR; i += NT) lds[L_DXP + i] = 0.0, lds[L_RP + i] = 0.0;
    }
    {  // tables: the features' track tables, the prior's block table, ric / tic
      const int t = fresh_tid();
      if (t < c.nf) {
        ids[I_FSTART + t] = B.feat_start[(size_t)w * B.max_feat + t];
        ids[I_FNOBS + t] = B.feat_nobs[(size_t)w * B.max_feat + t];
        ids[I_FOBS + t] = B.feat_obs_begin[(size_t)w * B.max_feat + t];
      }
      if (t >= PBT0 && t < PBT0 + c.pnblk) {  // the prior's block table (one round trip instead of one per block)
        const int k = t - PBT0;
        ids[I_PBLK + k * 3] = B.prior_blk_kind[(size_t)w * B.max_pblk + k], ids[I_PBLK + k * 3 + 1] = B.prior_blk_frame[(size_t)w * B.max_pblk + k];
      }
#ifndef AVM_X
      if (t == 0) {
        const double* ex = B.ex_pose + (size_t)w * 7;
        double R[9];
        q2R(quat{ex[6], ex[3], ex[4], ex[5]}, R);
        for (int k = 0; k < 9; k++) lds[L_RIC + k] = R[k];
        for (int k = 0; k < 3; k++) lds[L_RIC + 9 + k] = ex[k];
      }
#endif
    }
    __syncthreads();
    PROFQ(c, 38);
    {  // observation slot -> feature
      const int t = fresh_tid();
#ifndef AVM_X
      if (t < 7) lds[L_RIC + 12 + t] = B.ex_pose[(size_t)w * 7 + t];  // current ex_pose for the prior's dx
      if (t == 7) lds[L_RIC + 19] = B.td ? B.td[w] : 0.0;             // ... and para_Td (a constant here)
#endif
      if (t < c.nf) {
        const int s0 = ids[I_FOBS + t], no = ids[I_FNOBS + t];
        for (int k = 0; k < no; k++) c.osf[s0 + k] = t;
      }
    }
    {
      // fs[a] = first feature with start >= a, and per frame the features observed in it (as imu_j) in feature order:
      // one wavefront per list, features along the lanes, positions from a ballot's prefix population count
      const int t = fresh_tid(), ln = t & 63;
      for (int q = t >> 6; q <= NFR; q += NT / 64) {
        int cnt = 0;
        for (int e0 = 0; e0 < c.nf; e0 += 64) cnt += __popcll(__ballot(e0 + ln < c.nf && ids[I_FSTART + min(e0 + ln, MAXE - 1)] < q));
        if (ln == 0) ids[I_FS + q] = cnt;
      }
    }
    if (fresh_tid() == 0) {  // the prior's index lists
      int off = 0;
#ifdef AVM_TP
      int psb_ = 0;
#else
      int nsb_ = 0, sbfr_ = 0;
#endif
      for (int k = 0; k < c.pnblk; k++) {
        const int kind = ids[I_PBLK + k * 3], fr = ids[I_PBLK + k * 3 + 1];  // (loaded by 16 lanes at once above)
        ids[I_PBLK + k * 3 + 2] = off;
        const int n = kind == AVM_BLK_SPEEDBIAS ? 9 : (kind == AVM_BLK_TD ? 1 : 6);
#ifdef AVM_X
        for (int q = 0; q < n; q++)
          ids[I_PIDX + off + q] = kind == AVM_BLK_POSE ? fr * 6 + q
                                  : (kind == AVM_BLK_SPEEDBIAS ? SB0 + fr * 9 + q
                                     : (kind == AVM_BLK_TD ? (c.est_td ? XC_TD : -1) : (c.est_ex ? XC_EX + q : -1)));
#else
        for (int q = 0; q < n; q++) ids[I_PIDX + off + q] = kind == AVM_BLK_POSE ? fr * 6 + q : (kind == AVM_BLK_SPEEDBIAS ? SB0 + fr * 9 + q : -1);
#endif
#ifdef AVM_TP
        if (kind == AVM_BLK_SPEEDBIAS) psb_ = fr;  // (at most one such block: the host checks it before it chooses this kernel)
#else
        if (kind == AVM_BLK_SPEEDBIAS) nsb_++, sbfr_ |= fr;
#endif
        off += n;
      }
#ifdef AVM_TP
      ids[I_PSB] = psb_;
#else
      // the rule of window_prior_tp_misfit (kernels.hpp): chol_regs' elimination order takes a prior whose only speed-bias block is frame 0's
      ids[I_CRFIT] = (nsb_ <= 1 && sbfr_ == 0) ? 1 : 0;
#endif
    }
    for (int f = 1 + fresh_wave(); f < NFR; f += NT / 64) {  // features observed in frame f (as imu_j), in feature order
      const int ln = fresh_lane();
      int n = 0;
      unsigned am = 0;  // start frames that occur among the frame's factors (one accumulation run of the frame task each)
      for (int e0 = 0; e0 < c.nf; e0 += 64) {
        const int e = min(e0 + ln, MAXE - 1), a = ids[I_FSTART + e];
        const bool in = e0 + ln < c.nf && a < f && f < a + ids[I_FNOBS + e];
        const unsigned long long m = __ballot(in);
        if (in) c.cov[f * MAXE + n + __popcll(m & ((1ull << ln) - 1ull))] = e;
        n += __popcll(m);
#pragma unroll
        for (int aa = 0; aa < NFR - 1; aa++) am |= __any(in && a == aa) ? 1u << aa : 0u;
      }
      if (ln == 0) ids[I_NCOV + f] = n, ids[I_NRUN + f] = __popc(am);
    }
    {
      const int t = fresh_tid();
      if (t == 0) ids[I_NCOV] = 0;
#ifdef AVM_X
      // frame 11: the features matched in the relocalization frame (the host's list, in its order)
      for (int k = t; k < c.relo_n; k += NT) c.cov[(NFRP - 1) * MAXE + k] = min(max(B.relo_feat[(size_t)w * B.max_feat + k], 0), max(c.nf - 1, 0));
      if (t == 64) ids[I_NCOV + NFRP - 1] = c.relo_n;
#endif
    }
    __syncthreads();
    PROFQ(c, 39);
    // frame deal (each form takes its fresh thread index at its head)
#ifdef AVM_X
    if (fresh_tid() == 0) {  // longest-processing-time assignment of the frames to the assembling wavefronts
      int done = 0;
      ids[I_FRW] = -1;
      // (the loads in registers - constant indices only: indexed by a run-time value the array lived in private memory, 53 scratch instructions
      //  in a one-thread loop of 130 steps per window)
      int load[ASM_WAVES];
#pragma unroll
      for (int k = 0; k < ASM_WAVES; k++) load[k] = 0;
      for (int k = 1; k < NFRP; k++) {
        int bb = -1, bn = -1;
        for (int f = 1; f < NFRP; f++)
          if (!(done & (1 << f)) && ids[I_NCOV + f] > bn) bn = ids[I_NCOV + f], bb = f;
        int bw = 0, lb = load[0];
#pragma unroll
        for (int q = 1; q < ASM_WAVES; q++)
          if (load[q] < lb) lb = load[q], bw = q;
        ids[I_FRW + bb] = bw;
        const int inc = ((bn + 63) / 64) * 64 + 8;
#pragma unroll
        for (int q = 0; q < ASM_WAVES; q++) load[q] += q == bw ? inc : 0;
        done |= 1 << bb;
      }
    }
#elif defined(AVM_TP)
    if (const int t = fresh_tid(); t < 64) {
      // Longest-processing-time assignment of the frames to the four wavefronts (lane q keeps the load of wavefront q, in factors).
      // Every wavefront has a SIMD to itself within the workgroup; wavefront 2 also evaluates the raw IMU Jacobians (about two
      // chunks' worth) and two fifths of the prior's rows, wavefront 3 the other three fifths: they start with that load.
      // (Round 5: with the issue priorities those two run at the light level and weigh less than they did: 60 / 300 factors' worth,
      //  re-measured - were 88 / 380: ragged tracks 11.82 -> 11.74 ms, dense 12.54 -> 12.49.)
      int fc = t == 2 ? TP_WIMU + (c.pn > 0 ? 2 * TP_WPRI / 5 : 0) : (t == 3 && c.pn > 0 ? 3 * TP_WPRI / 5 : 0), done = 0;
      if (t == 0) ids[I_FRW] = -1;
      for (int k = 1; k < NFRP; k++) {
        int bb = -1, bn = -1;
        for (int f = 1; f < NFRP; f++) {
          const int n = ids[I_NCOV + f] + LPT_RUNW * max(ids[I_NRUN + f] - 1, 0);
          if (!(done & (1 << f)) && n > bn) bn = n, bb = f;
        }
        const int own = (fc + 63) >> 6, with = (fc + bn + 63) >> 6;
        int key = (with << 16) | (own << 8) | t;
        if (t >= ASM_WAVES) key = 0x7fffffff;
        key = min(key, lane_xor<2>(key)), key = min(key, lane_xor<1>(key));
        const int bw = __builtin_amdgcn_readfirstlane(key) & 255;
        if (t == bw) fc += bn;
        if (t == 0) ids[I_FRW + bb] = bw;
        done |= 1 << bb;
      }
    }
#else
    if (const int t = fresh_tid(); t < 64) {
      // Longest-processing-time assignment of the frames to the assembling wavefronts, by the lanes of wavefront 0 (lane q
      // keeps the factor count of wavefront q).  A wavefront's cost is its number of 64-factor chunks over ALL its frames;
      // wavefronts w and w + 4 share a SIMD, so the quantity to keep level is the chunk count per SIMD (the raw-IMU
      // wavefront 6 weighs about two chunks on SIMD 2, the prior's wavefront 7 about one on SIMD 3).  Largest frame first,
      // to the wavefront that leaves its SIMD lowest (ties: the one with fewer chunks of its own, then the lower index).
      int fc = 0, done = 0;
      if (t == 0) ids[I_FRW] = -1;
      for (int k = 1; k < NFRP; k++) {
        // (a frame weighs its factors plus LPT_RUNW factors' worth for every accumulation run beyond the first - a run costs a flush of
        //  the partial blocks and a group of eight MFMAs however short it is: with ragged tracks a frame has up to ten runs of a
        //  handful of factors each, and by factor counts alone two wavefronts ended up with twice the others' time)
        int bb = -1, bn = -1;
        for (int f = 1; f < NFRP; f++) {
          const int n = ids[I_NCOV + f] + LPT_RUNW * max(ids[I_NRUN + f] - 1, 0);
          if (!(done & (1 << f)) && n > bn) bn = n, bb = f;
        }
        const int own = (fc + 63) >> 6, with = (fc + bn + 63) >> 6;
        const int partner = lane_xor<4>(own);
        int key = ((with + partner + ((t & 3) == 2 ? 2 : ((t & 3) == 3 ? 1 : 0))) << 16) | (own << 8) | t;
        if (t >= ASM_WAVES) key = 0x7fffffff;
        key = min(key, lane_xor<4>(key)), key = min(key, lane_xor<2>(key)), key = min(key, lane_xor<1>(key));
        const int bw = __builtin_amdgcn_readfirstlane(key) & 255;
        if (t == bw) fc += bn;
        if (t == 0) ids[I_FRW + bb] = bw;
        done |= 1 << bb;
      }
    }
#endif
    __syncthreads();
    // once per window: the structural zeros of the scratch slot (raw IMU Jacobians outside their blocks, E^T F of
    // the frames that do not observe a feature) - the evaluations only ever rewrite the same nonzero entries
    {
      const int t = fresh_tid();
      gdouble* IJR = c.sc + Scratch::IJRAW;
      for (int i = t; i < (NFR - 1) * IJBLK; i += NT) IJR[i] = 0.0;
      gdouble* Wt = c.sc + Scratch::W;
      for (int idx = t; idx < c.nf * NFR; idx += NT) {
        const int f = idx / c.nf, e = idx - f * c.nf;
        const int a = ids[I_FSTART + e], no = ids[I_FNOBS + e];
        if (f < a || f >= a + no) {
#pragma unroll
          for (int q = 0; q < 6; q++) Wt[(6 * f + q) * WLE + e] = 0.0;
        }
      }
#ifdef AVM_X
      // relocalization frame: E^T F rows 66..71 and the per-factor products of frame 11 are zero except for the matched
      // features, whose entries frame task 11 rewrites at every evaluation
      gdouble* PF = c.sc + Scratch::PF;
      for (int idx = t; idx < MAXE * 6; idx += NT) Wt[(6 * NFR + idx / MAXE) * WLE + idx % MAXE] = 0.0;
      for (int idx = t; idx < MAXE * NQ; idx += NT) PF[((idx / MAXE) * NFRP + (NFRP - 1)) * WLE + idx % MAXE] = 0.0;
#endif
    }
    PROFQ(c, 40);
    // Hp = J0^T J0 (constant during the solve: hoisted out of the per-iteration J^T J)
    if (c.pn > 0) prior_jtj_packed(c.pJ, c.ldp, c.pn, c.sc + Scratch::HP, reinterpret_cast<gint*>(c.sc + Scratch::HP + HPK_MAX));
    __syncthreads();
    PROFQ(c, 41);

    PROF(c, 9);
    // ---------------- TrustRegionMinimizer ----------------
    if (const int t = fresh_tid(); t < 32) lds[L_SUM + t] = 0.0;
    int n_successful = 0, accept_mask = 0;
    unid initial_cost = 0;
    unid radius = ou.initial_trust_region_radius, mu = 1e-8;
    const double min_mu = 1e-8, max_mu = 1.0, mu_inc = 10.0;
    bool reuse = false, first = true, have_alpha = false;
#if defined(AVM_X) || defined(AVM_TP)
    auto DG = [&](int i) { return lds[L_G + i] / lds[L_DD + i]; };  // g / D, recomputed (the same division every time)
#else
    auto DG = [&](int i) { return lds[L_DG + i]; };
#endif
    unid alpha = 0, dogleg_step_norm = 0;
    unid gnorm = 0, gn_norm = 0, ytg = 0, jusq = 0;  // |g/D|, |D y|, y^T g, |J u|^2
    unid k1 = 0, k2 = 0;                             // step = -(k1 * g/D^2 + k2 * y)
    unid x_cost = 0, x_norm = 0, gradient_max_norm = 0;
    int iteration = 0, num_invalid = 0, termination = AVM_TERM_NO_CONVERGENCE;
    bool step_ok = true;

    // squared ambient norm over the variable parameter blocks (Ceres' reduced program: constant blocks are not in it)
#ifdef AVM_X
    auto amb_sq = [&](const double* xa, const double* xb) {  // |xa - xb|^2, xb == nullptr: |xa|^2
      const int t = fresh_tid();
      double s = 0;
      auto term = [&](int i) {
        const double d = xb ? xa[i] - xb[i] : xa[i];
        s += d * d;
      };
      for (int i = t; i < 7 * NFR; i += NT) term(i);                                 // poses
      if (c.relo_n > 0 && t >= 128 && t < 135) term(7 * NFR + t - 128);             // relo_Pose
      for (int i = t; i < 99 + c.nf; i += NT) term(XSB + i);                          // speed-biases, inverse depths
      if (c.est_ex && t >= 192 && t < 199) term(XEX + t - 192);
      if (c.est_td && t == 200) term(XTD);
      return block_sum1(s);
    };
    auto amb_norm = [&](const double* xs) { return sqrt(amb_sq(xs, nullptr)); };
#else
    auto amb_norm = [&](const double* xs) {
      double s = 0;
      for (int i = fresh_tid(); i < 176 + c.nf; i += NT) s += xs[i] * xs[i];
      return sqrt(block_sum1(s));
    };
#endif
    // evaluate + scaling + gradient max norm at lds[L_X]
    // what follows a Jacobian evaluation at lds[L_X]: scaling, gradient max norm
    auto post_evaluate = [&]() {
      PROF_T0();
      // Jacobi scaling from the column norms of the first Jacobian (diag of unscaled H)
      const bool was_first = first;
      (void)was_first;
      if (first) {
        if (ou.jacobi_scaling) {
          const int t = fresh_tid();
#ifdef AVM_TP
          if (t < NF) lds[L_SC + t] = 1.0 / (1.0 + sqrt(lds[s_off(t, t)]));
          for (int e = t; e < c.nf; e += NT) lds[L_SC + NF + e] = 1.0 / (1.0 + sqrt(lds[L_HEE + e]));
#else
          if (t < NF) lds[L_SC + t] = 1.0 / (1.0 + sqrt(lds[L_S + roff(t) + t]));
          if (t >= 192 && t < 192 + c.nf) lds[L_SC + NF + t - 192] = 1.0 / (1.0 + sqrt(lds[L_HEE + t - 192]));
#endif
        }
        first = false;
      }
      // gradient_max_norm = |x - Plus(x, -g)|_inf with the unscaled gradient
      double gm = 0;
      {
        const int t = fresh_tid();
        const double* x = lds + L_X;
        const double* g = lds + L_G;
        if (t < NFR) {
          for (int k = 0; k < 3; k++) gm = fmax(gm, fabs(g[t * 6 + k]));
          quat q{x[t * 7 + 6], x[t * 7 + 3], x[t * 7 + 4], x[t * 7 + 5]};
          quat r = qnormalized(qmul(q, deltaQ(mk3(-g[t * 6 + 3], -g[t * 6 + 4], -g[t * 6 + 5]))));
          gm = fmax(gm, fmax(fmax(fabs(q.x - r.x), fabs(q.y - r.y)), fmax(fabs(q.z - r.z), fabs(q.w - r.w))));
        }
        if (t >= 64 && t < 64 + 99) gm = fmax(gm, fabs(g[SB0 + t - 64]));
#ifdef AVM_TP
        for (int e = t; e < c.nf; e += NT) gm = fmax(gm, fabs(g[NF + e]));
#else
        if (t >= 192 && t < 192 + c.nf) gm = fmax(gm, fabs(g[NF + t - 192]));
#endif
#ifdef AVM_X
        if ((t == 400 && c.relo_n > 0) || (t == 401 && c.est_ex)) {  // relo_Pose / ex_pose: pose blocks like the others
          const int xo = t == 401 ? XEX : 7 * NFR, go = t == 401 ? XC_EX : 6 * NFR;
          for (int k = 0; k < 3; k++) gm = fmax(gm, fabs(g[go + k]));
          quat q{x[xo + 6], x[xo + 3], x[xo + 4], x[xo + 5]};
          quat r = qnormalized(qmul(q, deltaQ(mk3(-g[go + 3], -g[go + 4], -g[go + 5]))));
          gm = fmax(gm, fmax(fmax(fabs(q.x - r.x), fabs(q.y - r.y)), fmax(fabs(q.z - r.z), fabs(q.w - r.w))));
        }
        if (t == 402 && c.est_td) gm = fmax(gm, fabs(g[XC_TD]));
#endif
      }
      gradient_max_norm = uni(block_max1(gm));
      __syncthreads();
      if (c.prof && fresh_tid() == 0) c.prof[43] += clock64() - pt__;
      scale_system(c, was_first);
      PROF(c, 10);
    };
    auto evaluate_x = [&]() {
      x_cost = uni(eval_jac(c, o));
      post_evaluate();
    };
    // eval_jac() stages the frame tasks' rows in the LDS range that also holds the Gauss-Newton step, the dogleg step
    // and the candidate state, so a speculative evaluation parks what a rejection needs (current point, GN step)
    // in the spare tail of the slot's prior region (its address from the LDS context at every use: kept for the window it was one more
    // spilled register pair, and an LDS read is cheaper than a trip to scratch memory)
    auto spec_save = [&]() { return c.sc + Scratch::HP + HP_SPEC; };
    auto spec_enter = [&]() {  // x -> backup, x <- candidate
      __syncthreads();
      const int t = fresh_tid();
      gdouble* save = spec_save();
      for (int i = t; i < XN; i += NT) save[i] = lds[L_X + i], lds[L_X + i] = lds[L_XC + i];
      for (int i = t; i < VEC; i += NT) save[XN + i] = lds[L_Y + i];
      __syncthreads();
    };
    auto spec_restore = [&]() {  // x <- backup, candidate <- x
      __syncthreads();
      gdouble* save = spec_save();
      for (int i = fresh_tid(); i < XN; i += NT) {
        const double cand = lds[L_X + i];
        lds[L_X + i] = save[i];
        lds[L_XC + i] = cand;
      }
      __syncthreads();
    };
    auto spec_restore_gn_step = [&]() {  // after the system at x has been rebuilt (eval_jac stages over it again)
      gdouble* save = spec_save();
      for (int i = fresh_tid(); i < VEC; i += NT) lds[L_Y + i] = save[XN + i];
      __syncthreads();
    };
    // Speculation (exact: the same evaluations, fewer of them).  Ceres evaluates the cost at the candidate and, if
    // the step is accepted, evaluates residuals AND Jacobians at that same point again.  While steps keep being
    // accepted with a good model fit, the Jacobian is evaluated at the candidate right away (its cost decides the
    // step) and nothing is recomputed on acceptance; a rejected speculation pays one extra evaluation to restore
    // the system at x, and switches speculation off until a step with rho > 0.75 comes by.
    bool speculate = A.speculate != 0;

    x_norm = uni(amb_norm(lds + L_X));
    evaluate_x();
    initial_cost = x_cost;
    unid ref_cost = x_cost;

    while (true) {
      PROFQ_T0();
      // FinalizeIterationAndCheckIfMinimizerCanContinue
      if (iteration > 0) {
        if (step_ok) n_successful++;
        if (iteration <= AVM_MAX_ITER_TRACE) {
          if (fresh_tid() == 0) lds[L_SUM + iteration - 1] = x_cost, lds[L_SUM + 16 + iteration - 1] = radius;
          if (step_ok) accept_mask |= 1 << (iteration - 1);
        }
      }
      if (A.time_cap_ticks > 0) {
        // MaxSolverTimeReached (checked before the iteration limit, like Ceres): options.max_solver_time_in_seconds of
        // estimator.cpp:803-806.  One thread reads the clock, the verdict goes through LDS so that it is workgroup-uniform.
        if (fresh_tid() == 0) ids[I_TIMEUP] = wall_clock64() - wall0 >= A.time_cap_ticks;
        __syncthreads();
        if (uni(ids[I_TIMEUP])) {
          termination = AVM_TERM_NO_CONVERGENCE;
          break;
        }
      }
      if (iteration >= ou.max_num_iterations) {
        termination = AVM_TERM_NO_CONVERGENCE;
        break;
      }
      if (step_ok && gradient_max_norm <= ou.gradient_tolerance) {
        termination = AVM_TERM_GRADIENT_TOL;
        break;
      }
      if (radius <= ou.min_trust_region_radius) {
        termination = AVM_TERM_MIN_RADIUS;
        break;
      }
      iteration++;
      step_ok = false;
      bool solver_ok = true;
      if (!reuse) {
        reuse = true;
        have_alpha = false;
        // D = sqrt(clamp(diag(J'^T J'))), g/D
        {
          const int t = fresh_tid();
#ifdef AVM_TP
          if (t < NF) lds[L_DD + t] = sqrt(fmin(fmax(lds[s_off(t, t)], o.min_lm_diagonal), o.max_lm_diagonal));
          for (int e = t; e < c.nf; e += NT) lds[L_DD + NF + e] = sqrt(fmin(fmax(lds[L_HEE + e], o.min_lm_diagonal), o.max_lm_diagonal));
#else
          if (t < NF) lds[L_DD + t] = sqrt(fmin(fmax(lds[L_S + roff(t) + t], o.min_lm_diagonal), o.max_lm_diagonal));
          if (t >= 192 && t < 192 + c.nf) lds[L_DD + NF + t - 192] = sqrt(fmin(fmax(lds[L_HEE + t - 192], o.min_lm_diagonal), o.max_lm_diagonal));
#endif
        }
        __syncthreads();
        double g2 = 0;
        for (int i = fresh_tid(); i < NF + c.nf; i += NT) {
          const double v = lds[L_G + i] / lds[L_DD + i];
#if !defined(AVM_X) && !defined(AVM_TP)
          lds[L_DG + i] = v;
#endif
          g2 += v * v;
        }
        gnorm = uni(sqrt(block_sum1(g2)));
        // Gauss-Newton step with mu retry (DoglegStrategy::ComputeGaussNewtonStep)
        solver_ok = false;
        bool rebuilt = true;
        PROFQ(c, 32);
        while (mu < max_mu) {
          if (!rebuilt) {  // S was destroyed by a failed factorisation: rebuild the normal equations
            evaluate_x();
            rebuilt = true;
          }
          PROF_T0();
          schur_reduce(c, mu);
          PROF(c, 11);
#ifdef AVM_TP
          // factorization + both triangular solves on the register tiles of the four wavefronts (y -> lds[L_Y])
          bool ok;
          AVM_PRIO_BULK_CHOL();  // (its pivot chains raise themselves to 3)
          switch (__builtin_amdgcn_readfirstlane(fresh_wave())) {
            case 0: ok = uni(chol_regs<0>()); break;
            case 1: ok = uni(chol_regs<1>()); break;
            case 2: ok = uni(chol_regs<2>()); break;
            default: ok = uni(chol_regs<3>()); break;
          }
          AVM_PRIO_LIGHT();
          PROF(c, 12);
          if (!ok) {
            mu = uni(mu * mu_inc);
            rebuilt = false;
            continue;
          }
#else
          bool ok;
          if (uni(ids[I_CRFIT])) {  // (uniform: the window's prior has the structure chol_regs' pattern is closed for)
            switch (__builtin_amdgcn_readfirstlane(fresh_wave())) {
              case 0: ok = uni(chol_regs<0>()); break;
              case 1: ok = uni(chol_regs<1>()); break;
              case 2: ok = uni(chol_regs<2>()); break;
              case 3: ok = uni(chol_regs<3>()); break;
#ifdef AVM_X
              case 4: ok = uni(chol_regs<4>()); break;
              case 5: ok = uni(chol_regs<5>()); break;
              case 6: ok = uni(chol_regs<6>()); break;
              default: ok = uni(chol_regs<7>()); break;
#else
              default: ok = uni(chol_regs<4>()); break;  // (wavefronts 4..7: no tiles)
#endif
            }
            PROF(c, 12);
          } else {
            ok = uni(cholesky_lds(c.prof));
            PROF(c, 12);
            if (ok) chol_solve_lds(L_Y);
            PROF(c, 13);
          }
          if (!ok) {
            mu = uni(mu * mu_inc);
            rebuilt = false;
            continue;
          }
#endif
          const double bad_y = uni(back_substitute(c, mu));
          PROF(c, 14);
          if (bad_y > 0) {
            mu = uni(mu * mu_inc);
            rebuilt = false;
            continue;
          }
          solver_ok = true;
          break;
        }
        PROFQ_T0();
        if (solver_ok) {
          double a1 = 0, a2 = 0;
          for (int i = fresh_tid(); i < NF + c.nf; i += NT) {
            const double yv = lds[L_Y + i], dv = lds[L_DD + i] * yv;
            a1 += dv * dv;
            a2 += yv * lds[L_G + i];
          }
          block_sum1x2(a1, a2);
          gn_norm = uni(sqrt(a1));
          ytg = uni(a2);
        }
      }
      bool step_is_valid = false;
      double model_cost_change = 0;
      if (solver_ok) {
        // ComputeTraditionalDoglegStep
        if (gn_norm <= radius) {
          k1 = 0, k2 = 1;
          dogleg_step_norm = gn_norm;
        } else {
          if (!have_alpha) {  // Cauchy point, needed only when the GN step leaves the trust region
            for (int i = fresh_tid(); i < VEC; i += NT) lds[L_ST + i] = i < NF + c.nf ? DG(i) / lds[L_DD + i] : 0.0;
            __syncthreads();
            PROFQ(c, 33);
            jusq = uni(jac_times_vec_sq(c, o));
            alpha = uni(gnorm * gnorm / jusq);
            have_alpha = true;
            __syncthreads();
            PROFQ(c, 34);
          }
          if (gnorm * alpha >= radius) {
            k1 = uni(radius / gnorm), k2 = 0;
            dogleg_step_norm = radius;
          } else {
            // a = -alpha g/D, b = -D y
            const double b_dot_a = alpha * ytg;  // (-alpha g/D).(-D y) = alpha g^T y
            const double a2n = (alpha * gnorm) * (alpha * gnorm);
            const double bma = a2n - 2 * b_dot_a + gn_norm * gn_norm;
            const double cc = b_dot_a - a2n;
            const double dd = sqrt(cc * cc + bma * (radius * radius - a2n));
            const double beta = (cc <= 0) ? (dd - cc) / bma : (radius * radius - a2n) / (dd + cc);
            k1 = uni(alpha * (1.0 - beta)), k2 = uni(beta);
            double s2 = 0;
            for (int i = fresh_tid(); i < NF + c.nf; i += NT) {
              const double v = -k1 * DG(i) - k2 * lds[L_DD + i] * lds[L_Y + i];
              s2 += v * v;
            }
            dogleg_step_norm = uni(sqrt(block_sum1(s2)));
          }
        }
        for (int i = fresh_tid(); i < VEC; i += NT)
          lds[L_ST + i] = i < NF + c.nf ? -(k1 * DG(i) / lds[L_DD + i] + k2 * lds[L_Y + i]) : 0.0;
        // model_cost_change = -step^T g - 1/2 step^T H step, with H y = g - mu D^2 y
        {
          const double utg = gnorm * gnorm;                     // u^T g, u = g/D^2
          const double yDy = gn_norm * gn_norm;                 // y^T D^2 y
          const double uHy = utg - mu * ytg;                    // u^T (g - mu D^2 y)
          const double yHy = ytg - mu * yDy;
          const double sHs = k1 * k1 * (k1 != 0 ? (double)jusq : 0.0) + 2 * k1 * k2 * uHy + k2 * k2 * yHy;
          model_cost_change = uni((k1 * utg + k2 * ytg) - 0.5 * sHs);
        }
        step_is_valid = model_cost_change > 0.0;
        if (step_is_valid) num_invalid = 0;
        __syncthreads();
      }
      if (!step_is_valid) {
        if (++num_invalid >= ou.max_num_consecutive_invalid_steps) {
          termination = AVM_TERM_FAILURE;
          break;
        }
        mu = uni(mu * mu_inc);  // StepIsInvalid
        reuse = false;
        evaluate_x();  // S holds a Cholesky factor: rebuild the normal equations for the retry
        continue;
      }
      // candidate
      PROFQ(c, 33);
      PROF_T0();
      state_plus();
      __syncthreads();
#ifdef AVM_X
      const double step_norm = uni(sqrt(amb_sq(lds + L_X, lds + L_XC)));
#else
      double d2 = 0;
      for (int i = fresh_tid(); i < 176 + c.nf; i += NT) {
        const double d = lds[L_X + i] - lds[L_XC + i];
        d2 += d * d;
      }
      const double step_norm = uni(sqrt(block_sum1(d2)));
#endif
      // the last iteration the options allow: the minimizer stops right after it (the iteration limit is checked before
      // the gradient tolerance, trust_region_minimizer.cc FinalizeIterationAndCheckIfMinimizerCanContinue), so the
      // Jacobian Ceres evaluates at the accepted point is never used: only the cost is computed there
      const bool last_iteration = iteration >= ou.max_num_iterations;
      const bool spec = speculate && !last_iteration;
      double cand_cost;
      PROFQ(c, 35);
      if (spec) {
        spec_enter();  // x <- candidate; the current point and the GN step are parked in the slot
        cand_cost = uni(eval_jac(c, o));
        PROF(c, 15);
      } else {
        build_frames(L_XC, 1);
        __syncthreads();
        cand_cost = uni(eval_cost(c, o, L_XC, 1));
        PROF(c, 15);
      }
      PROFQ_T0();
      if (step_norm <= ou.parameter_tolerance * (x_norm + ou.parameter_tolerance)) {
        if (spec) spec_restore();  // the minimizer stops at the current point, not at the candidate
        termination = AVM_TERM_PARAMETER_TOL;
        break;
      }
      const double cost_change = x_cost - cand_cost;
      if (fabs(cost_change) <= ou.function_tolerance * x_cost) {
        if (spec) spec_restore();
        termination = AVM_TERM_FUNCTION_TOL;
        break;
      }
      const double rel = uni((ref_cost - cand_cost) / model_cost_change);
      if (rel > ou.min_relative_decrease) {
        if (spec) {
          // the system at the accepted point is already assembled
          x_norm = uni(amb_norm(lds + L_X));
          x_cost = cand_cost;
          post_evaluate();
        } else {
          __syncthreads();
          for (int i = fresh_tid(); i < XN; i += NT) lds[L_X + i] = lds[L_XC + i];
          __syncthreads();
          x_norm = uni(amb_norm(lds + L_X));
          if (last_iteration)
            x_cost = cand_cost;
          else
            evaluate_x();
        }
        speculate = A.speculate != 0 && rel > 0.75;
        step_ok = true;
        if (rel < 0.25) radius = uni(radius * 0.5);
        if (rel > 0.75) radius = uni(fmax(radius, 3.0 * dogleg_step_norm));
        mu = uni(fmax(min_mu, 2.0 * mu / mu_inc));
        reuse = false;
        ref_cost = cand_cost;
      } else {
        if (spec) {
          // back to the current point: rebuild its system (g, E^T F, raw IMU Jacobians) for the retried step
          spec_restore();
          evaluate_x();
          spec_restore_gn_step();
        }
        speculate = false;
        radius = uni(radius * 0.5);
        reuse = true;
      }
      PROFQ(c, 36);
    }
    __syncthreads();
    PROFQ_T0();
    // ---------------- double2vector + vector2double (estimator.cpp:521-587, 477-519) ----------------
    {
      // rot_diff from yaw of frame 0 before / after ; stored in lds[L_GF..+9], origin_P0 in +9..12
      gauge_rot_diff(B.pose + (size_t)w * 77, (B.failure_occur && B.last_pose0 && B.failure_occur[w]) ? B.last_pose0 + (size_t)w * 7 : nullptr, L_GF);
      __syncthreads();
      if (const int t = fresh_tid(); t < NFRP) {
        const double* rd = lds + L_GF;
        const double* x = lds + L_X;
        quat q = qnormalized(quat{x[t * 7 + 6], x[t * 7 + 3], x[t * 7 + 4], x[t * 7 + 5]});
        double Rq[9], Rs[9];
        q2R(q, Rq);
        mat3mul(rd, Rq, Rs);
        const v3 P = Rmul(rd, mk3(x[t * 7] - lds[L_GF + 12], x[t * 7 + 1] - lds[L_GF + 13], x[t * 7 + 2] - lds[L_GF + 14])) +
                     mk3(lds[L_GF + 9], lds[L_GF + 10], lds[L_GF + 11]);
        const quat qo = R2q(Rs);
        if (t < NFR) {
          const v3 V = Rmul(rd, mk3(x[XSB + t * 9], x[XSB + t * 9 + 1], x[XSB + t * 9 + 2]));
          double* po = B.pose + (size_t)w * 77 + t * 7;
          po[0] = P.x, po[1] = P.y, po[2] = P.z, po[3] = qo.x, po[4] = qo.y, po[5] = qo.z, po[6] = qo.w;
          double* so = B.speedbias + (size_t)w * 99 + t * 9;
          so[0] = V.x, so[1] = V.y, so[2] = V.z;
          for (int k = 3; k < 9; k++) so[k] = x[XSB + t * 9 + k];
        }
#ifdef AVM_X
        else if (c.has_relo) {  // relo_t / relo_r of estimator.cpp:590-596 (frame 11 went through the same transformation; with
                                // no matched feature it did not move in the solve, the gauge fix applies all the same)
          double* po = B.relo_pose + (size_t)w * 7;
          po[0] = P.x, po[1] = P.y, po[2] = P.z, po[3] = qo.x, po[4] = qo.y, po[5] = qo.z, po[6] = qo.w;
        }
#endif
      }
      if (fresh_tid() == 64) {
        double* ex = B.ex_pose + (size_t)w * 7;
        double R[9];
#ifdef AVM_X
        const double* exs = lds + L_X + XEX;  // tic / ric come back from para_Ex_Pose (estimator.cpp:569-579)
        for (int k = 0; k < 3; k++) ex[k] = exs[k];
        q2R(quat{exs[6], exs[3], exs[4], exs[5]}, R);
#else
        q2R(quat{ex[6], ex[3], ex[4], ex[5]}, R);
#endif
        const quat qo = R2q(R);
        ex[3] = qo.x, ex[4] = qo.y, ex[5] = qo.z, ex[6] = qo.w;
      }
#ifdef AVM_X
      if (fresh_tid() == 65 && c.est_td && B.td) B.td[w] = lds[L_X + XTD];
#endif
#ifdef AVM_TP
      for (int e = fresh_tid(); e < c.nf; e += NT) B.inv_depth[(size_t)w * B.max_feat + e] = 1.0 / (1.0 / lds[L_X + XLAM + e]);
#else
      if (const int t = fresh_tid(); t >= 128 && t < 128 + c.nf) {
        const int e = t - 128;
        B.inv_depth[(size_t)w * B.max_feat + e] = 1.0 / (1.0 / lds[L_X + XLAM + e]);
      }
#endif
    }
    PROFQ(c, 37);
    if (c.prof && fresh_tid() == 0) c.prof[31] += 1, c.prof[42] += clock64() - pw__;
    if (fresh_tid() == 0 && A.summary) {
      avm_solve_summary* so = A.summary + w;
      so->termination = termination;
      so->num_iterations = iteration;
      so->num_successful = n_successful;
      so->accept_mask = accept_mask;
      so->initial_cost = initial_cost;
      so->final_cost = x_cost;
      for (int k = 0; k < AVM_MAX_ITER_TRACE; k++) so->cost_trace[k] = lds[L_SUM + k], so->radius_trace[k] = lds[L_SUM + 16 + k];
    }
    __syncthreads();
  }
}
