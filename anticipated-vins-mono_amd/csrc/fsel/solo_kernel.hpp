// fsel/solo_kernel.hpp - fsel_solo_kernel: one workgroup per frame, lazy evaluation
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

// ---- SOLO: one workgroup per frame, lazy evaluation (batches of many frames) -------------------------------------------------------
// The frame kernel (frame_kernel.hpp) spreads ONE frame's 425 evaluations per round over a team of workgroups and pays an exchange of records per
// round; a batch larger than the number of teams queues.  Here a frame belongs to one workgroup from its first round to its last -
// no records, no waiting for anybody, hundreds of frames side by side - which only pays because a round does not have to score every
// candidate: the objective is submodular (every p Delta is positive semidefinite), so a candidate's gain f_l(S) - logdet C(S) can only
// shrink as features are added, and the gain it had when it was last scored, g_l, bounds its value now: f_l <= logdet C + g_l (Minoux'
// accelerated greedy; logdet C is the last winner's value).  Per round:
//   1. every live candidate's Hadamard bound (the std::map equal-key rule and the order of the pick need all of them);
//   2. the candidates with g_l >= lazy_tau x (the last winner's gain) are scored, four per wavefront, Delta straight from memory;
//   3. the pick among the scored ones, and its check: a candidate that was NOT scored and whose bound logdet C + g_l + margin reaches
//      the winner's value is scored after all and the pick repeated, until nobody is left.  A candidate that is never scored in a
//      round is therefore PROVEN to lose it (strictly, beyond the margin: it can neither win nor tie), which is all the reference's
//      loop (feature_selector.cpp:669-683) needs of it: ids and fValues are those of the full evaluation.  lazy_tau trades second
//      passes against scored candidates and cannot change a result.
// Measured on the bench frames (500 candidates, 150 selected, H = 10): ~40 candidates scored per round instead of 425.
constexpr int FS_SOLO_NT = 512;
static_assert(FS_SOLO_NT == FS_FRAME_MAXC, "one candidate per thread");

template <int T, int BS, int NB>
__global__ __launch_bounds__(FS_SOLO_NT) void fsel_solo_kernel(FselDev A, int32_t* sync) {
  FS_TABLES_GUARD(A);
  constexpr int NW = FS_SOLO_NT / 64, MAXC = FS_FRAME_MAXC;
  __shared__ double sC[T * T], sdpp[T];
  __shared__ double s_f[MAXC], s_u[MAXC], s_ua[MAXC], s_ue[MAXC], s_bound[MAXC], s_pr[MAXC], s_inv[T];
  __shared__ unsigned char s_alive[MAXC], s_scored[MAXC];
  __shared__ short s_list[MAXC];
  __shared__ double s_g0;
  __shared__ double s_wf[2][NW], s_wu[2][NW];
  __shared__ int s_wi[2][NW];
  // [T][MAXC]: every candidate's Delta diagonal, candidates along the lanes - what the bound estimates of every round read.  3 H = 39: 160 KB in
  // double precision, so the LDS copy is SINGLE precision there (the estimates' error bars account for it) and the exact bounds - rare - read
  // the double-precision diagonals from A.ddiag.
  using dd_t = std::conditional_t<(T > 30), float, double>;
  extern __shared__ double s_dd_raw[];
  dd_t* s_dd = reinterpret_cast<dd_t*>(s_dd_raw);
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6, g = lane >> 4;
  __shared__ int s_or[2][NW];
  int orc = 0;
  // "does any thread of the workgroup say yes": one barrier (two slots: a slot is written again only after the barrier of the call between)
  auto wg_or = [&](bool v) {
    const int sl = orc++ & 1;
    const bool a = __any(v);
    if (lane == 0) s_or[sl][wv] = a ? 1 : 0;
    __syncthreads();
    int r = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) r |= s_or[sl][w];
    return r != 0;
  };
  const bool rec_lane = (lane & 15) == 0;
  const avm_fsel_batch& b = A.b;
  const int mc = b.max_cand;
  // the candidates whose thread says `mark` -> s_list (ascending) with their gain bounds beside them in s_lb; returns how many
  __shared__ int s_cnt[NW];
  __shared__ double s_lb[MAXC];
  auto build_list = [&](bool mark) {
    const unsigned long long bal = __ballot(mark);
    if (lane == 0) s_cnt[wv] = __popcll(bal);
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      const int cnt = s_cnt[w];
      base += w < wv ? cnt : 0, tot += cnt;
    }
    if (mark) {
      const int pos = base + __popcll(bal & ((1ull << lane) - 1ull));
      s_list[pos] = (short)t, s_lb[pos] = s_bound[t];
    }
    __syncthreads();
    return tot;
  };
  for (int p = blockIdx.x; p < b.n_problems; p += gridDim.x) {
    __syncthreads();
    const int nc = b.n_cand[p];
    const int kappa = max(0, b.max_features - (b.n_used ? b.n_used[p] : 0));
    const size_t pc = (size_t)p * mc;
    const double* Dp = A.delta + pc * T * T;
    const double* Dk = A.delta_pk + pc * (T * (T + 1) / 2);
    for (int idx = t; idx < T * T; idx += FS_SOLO_NT) sC[idx] = A.C[(size_t)p * T * T + idx];
    for (int idx = t; idx < T; idx += FS_SOLO_NT) sdpp[idx] = A.dpp[(size_t)p * T + idx];
    const int c = t;  // this thread's candidate
    {
      const bool ok = c < nc && A.valid[pc + min(c, mc - 1)] != 0;
      s_alive[c] = ok ? 1 : 0, s_bound[c] = HUGE_VAL, s_scored[c] = 0;
      s_pr[c] = ok ? b.cand_prob[pc + c] : 0.0;
    }
    for (int idx = t; idx < nc * T; idx += FS_SOLO_NT) {  // (one strided pass over the frame's Deltas)
      const int cc = idx / T, d = idx % T;
      const double dv = Dp[(size_t)cc * T * T + d * T + d];
      s_dd[d * MAXC + cc] = (dd_t)dv;
      if constexpr (T > 30) A.ddiag[pc * T + idx] = dv;
    }
    const double ld_nn = A.consts[(size_t)p * 4], ub_nn = A.consts[(size_t)p * 4 + 1];
    __syncthreads();
    if (wv == 0) {  // logdet of the frame's first C: the same evaluation with p = 0 - on the Delta of the first VALID candidate (the setup
                    // kernel writes delta_pk for those only: 0 x stale memory could be 0 x NaN)
      int first = -1;
      for (int c0 = 0; c0 < MAXC && first < 0; c0 += 64) {
        const unsigned long long m = __ballot(s_alive[c0 + lane] != 0);
        if (m) first = c0 + __ffsll((long long)m) - 1;
      }
      double ld0, ub0;
      const bool ok0 = fsel_logdet4<T, BS, NB, false, 2>(sC, sdpp, Dk + (size_t)max(first, 0) * (T * (T + 1) / 2), 0.0, &ld0, &ub0);
      if (lane == 0) s_g0 = ok0 ? (ld_nn + 2.0 * ld0) : __builtin_nan("");
    }
    __syncthreads();
    double G = s_g0, gprev = HUGE_VAL;
    // the EXACT Hadamard bounds of the candidates of s_list (fsel_ub4: the one function every compared bound comes from)
    auto bound_list = [&](int n) {
      for (int i0 = 0; i0 < n; i0 += NW * 4) {
        if (i0 + wv * 4 >= n) break;  // (uniform per wavefront)
        const int i = i0 + wv * 4 + g;
        const int cc = s_list[min(i, n - 1)];
        double ubt;
        if constexpr (T > 30) ubt = fsel_ub4<T, BS, NB>(sdpp, A.ddiag + (pc + cc) * T, 1, s_pr[cc]);
        else ubt = fsel_ub4<T, BS, NB>(sdpp, reinterpret_cast<const double*>(s_dd) + cc, MAXC, s_pr[cc]);
        if (i < n && rec_lane) s_u[cc] = ub_nn + ubt;
      }
    };
    // scores the candidates of s_list, four per wavefront, Delta straight from memory
    auto score_list = [&](int n) {
      for (int i0 = 0; i0 < n; i0 += NW * 4) {
        if (i0 + wv * 4 >= n) break;  // (uniform per wavefront)
        const int i = i0 + wv * 4 + g;
        const int cc = s_list[min(i, n - 1)];  // (a row without a candidate scores the list's last one again and drops the result)
        double ld, ubt;
        const bool ok = fsel_logdet4<T, BS, NB, false, 2>(sC, sdpp, Dk + (size_t)cc * (T * (T + 1) / 2), s_pr[cc], &ld, &ubt);
        if (i < n && rec_lane) {
          const double f = ok ? (ld_nn + 2.0 * ld) : __builtin_nan("");
          s_f[cc] = f, s_scored[cc] = 1;
          s_bound[cc] = ok ? f - G : HUGE_VAL;  // (a failed factorization: scored again every round)
        }
      }
      bound_list(n);
    };
    int nsel = 0;
    long long tk[6] = {0, 0, 0, 0, 0, 0}, tq[5] = {0, 0, 0, 0, 0}, tqp = 0, tkp = 0, n_scored = 0, n_second = 0, n_flag = 0, n_pass = 0;
    const bool stats = A.lazy_stats != 0 && p == 0;
#define FS_SOLO_Q(i) if (stats) { const long long n__ = clock64(); tq[i] += n__ - tqp; tqp = n__; }
    // The round's winner among the scored candidates: the lexicographic maximum of (fValue, bound, id) - feature_selector.cpp:669-683 with
    // the std::map equal-key rule of sortedlogDetUB (see fsel_pick_local): a live candidate with a higher id and a BIT-IDENTICAL bound
    // shadows the winner, scored or not.  The bounds of the unscored candidates are not computed every round.  What is: an estimate ua of
    // every live candidate's bound MINUS the part all candidates share, sum_d log1p(p Delta_dd / dpp_d), with a rigorous error bar ue
    // (a term below 0.01 by its series, remainder < x^4 / 4; above, by the single-precision logarithm, 4e-7 of the term).  Two bounds can
    // only be BIT-equal when the estimates are closer than the two error bars plus the rounding of the exact evaluation (64 T ulps of
    // the bound: 1.3e-10 on values of a few hundred at T = 30); only then the unscored candidate gets its exact bound, by the same function, to be compared.
    auto pick = [&](bool live, bool scored, double* fwin) -> int {
      constexpr int MAXSH = 8;
      int sh[MAXSH], nsh = 0;
#pragma unroll
      for (int qq = 0; qq < MAXSH; qq++) sh[qq] = -1;
      const double cf = scored ? s_f[c] : __builtin_nan("");
      if (stats) tqp = clock64();
      for (int pass = 0;; pass++) {
        const int sl = pass & 1;
        const double cu = s_u[c];  // (exact for the scored candidates and for those a previous pass has flagged)
        bool out = !scored;
#pragma unroll
        for (int qq = 0; qq < MAXSH; qq++) out |= sh[qq] == c;
        const bool in = !out && cf > -1.0;  // (NaN never wins)
        {  // the wavefront's best: three maxima in a row, each over the lanes that tie in the previous ones
          const double wf = fs_wave_max(in ? cf : -1.0);
          const bool tf = in && cf == wf;
          const double wu = fs_wave_max(tf ? cu : -DBL_MAX);
          const bool tu = tf && cu == wu;
          const int wi = fs_wave_max(tu ? c : -1);
          if (lane == 0) s_wf[sl][wv] = wf, s_wu[sl][wv] = wu, s_wi[sl][wv] = wi;
        }
        __syncthreads();
        double bf = s_wf[sl][0], bu = s_wu[sl][0];
        int bi = s_wi[sl][0];
#pragma unroll
        for (int w = 1; w < NW; w++) {
          const double f2 = s_wf[sl][w], u2 = s_wu[sl][w];
          const int i2 = s_wi[sl][w];
          if (i2 >= 0 && (bi < 0 || f2 > bf || (f2 == bf && (u2 > bu || (u2 == bu && i2 > bi))))) bf = f2, bu = u2, bi = i2;
        }
        *fwin = bf;
        FS_SOLO_Q(0)
        if (bi < 0 || A.no_key_rule || nsh >= MAXSH) return bi;  // (more than MAXSH chained collisions in one round: keep the last winner)
        const double slack = 64.0 * DBL_EPSILON * T * fmax(fabs(s_u[bi]), 1.0);  // (rounding of the two exact bounds: it grows with their size)
        const bool flag = live && !scored && c > bi && !(fabs(s_ua[c] - s_ua[bi]) > s_ue[c] + s_ue[bi] + slack);  // (an estimate that is not finite: compare the exact bounds)
        n_pass++;
        if (wg_or(flag)) {
          n_flag++;
          bound_list(build_list(flag));
          __syncthreads();
        }
        FS_SOLO_Q(1)
        const bool hit = live && c > bi && (scored || flag) && s_u[c] == bu;
        const bool anyhit = wg_or(hit);
        FS_SOLO_Q(2)
        if (!anyhit) return bi;
#pragma unroll
        for (int qq = 0; qq < MAXSH; qq++)
          if (qq == nsh) sh[qq] = bi;
        nsh++;
      }
    };
#define FS_SOLO_SEG(i) if (stats) { const long long n__ = clock64(); tk[i] += n__ - tkp; tkp = n__; }
    for (int k = 0; k < kappa; k++) {
      if (stats) tkp = clock64();
      // ---- 1. who is scored in the first pass; the estimate of every live candidate's bound
      const double th = A.lazy_tau * gprev;
      const bool live = c < nc && s_alive[c] != 0;
      if (t < T) s_inv[t] = 1.0 / sdpp[t];
      __syncthreads();
      bool mark = live && !(s_bound[c] < th);
      s_scored[c] = 0;
      int n = build_list(mark);
      // A first pass holds NW * 4 = 32 candidates (two wavefronts per SIMD: the CU's FP64 pipe is full); a 33rd costs half a pass more.  When
      // more are marked, only the 32 with the largest gain bounds are scored now - the others are exactly the ones the check of the pick
      // looks at again, and it rarely needs them (their bounds are the lowest of the marked).  Like lazy_tau: a choice of WHEN a candidate
      // is scored, never of the result.
      constexpr int CAP = NW * 4;
      if (n > CAP && gprev < HUGE_VAL) {
        const double bc = s_bound[c];
        int rank = 0;
        if (mark) {
#pragma unroll 4
          for (int j = 0; j < n; j++) {
            const int cj = s_list[j];
            const double bj = s_lb[j];
            rank += (bj > bc || (bj == bc && cj < c)) ? 1 : 0;
          }
        }
        mark = mark && rank < CAP;
        __syncthreads();  // (every reader of the first list is done)
        n = build_list(mark);
      }
      // The listed candidates' Deltas are asked for NOW (one 8-byte read per 128-byte line, a candidate per instruction: 29 lanes) and the
      // values are looked at only after the estimates below: the evaluations then find their operands in the L2 instead of waiting
      // for memory with all eight wavefronts (a scoring pass: 31 K cycles, 19 K with the operands in cache).
      constexpr int PKN = T * (T + 1) / 2, PFQ = (CAP + NW - 1) / NW, PFL = (PKN + 15) / 16;
      double pf[PFQ];
#pragma unroll
      for (int q = 0; q < PFQ; q++) {
        const int i = wv + q * NW;
        pf[q] = 0.0;
        if (n <= CAP && i < n && lane < PFL) pf[q] = Dk[(size_t)s_list[i] * PKN + min(lane * 16, PKN - 1)];
      }
      FS_SOLO_SEG(0)
      {
        double ua = 0.0, ue = 0.0;
        if (live) {
          const double prc = s_pr[c];
          const dd_t* dd = s_dd + c;
#pragma unroll
          for (int d = 0; d < T; d++) {
            const double x = (prc * dd[d * MAXC]) * s_inv[d];
            const bool small = fabs(x) <= 0.01;  // (NaN: the other branch, and the estimate is NaN - compared exactly)
            const double x2 = x * x, lg = (double)__log2f((float)(1.0 + x)) * 0.6931471805599453;
            ua += small ? x * (1.0 + x * (-0.5 + x * (1.0 / 3.0))) : lg;
            // the series' remainder is below x^4 / 4 / (1 - |x|); the other branch: 1 + x rounded to single precision (6e-8 of it) and a
            // logarithm good to two units in its last place (2.4e-7 of the result)
            ue += (small ? 0.26 * x2 * x2 + 1e-15 * fabs(x) : 1e-7 + 3e-7 * fabs(lg)) + (T > 30 ? 1.2e-7 * fabs(x) : 0.0);  // (a single-precision diagonal: 6e-8 of x)
          }
        }
        s_ua[c] = ua, s_ue[c] = ue;
      }
#pragma unroll
      for (int q = 0; q < PFQ; q++) asm volatile("" ::"v"(pf[q]));
      FS_SOLO_SEG(1)
      n_scored += n;
      // ---- 2. the scores (and the exact bounds of the scored)
      score_list(n);
      FS_SOLO_SEG(2)
      // ---- 3. the pick and its check
      int win;
      double fwin;
      for (;;) {
        __syncthreads();
        const bool scored = live && s_scored[c] != 0;
        win = pick(live, scored, &fwin);
        const double V = win >= 0 ? fwin : -1.0;  // (the reference's fMax = -1.0 when nobody has won)
        const double margin = 1e-8 * fmax(1.0, fabs(V));
        const bool need = live && !scored && !(G + s_bound[c] + margin < V);
        if (stats) tqp = clock64();
        const bool anyneed = wg_or(need);
        FS_SOLO_Q(3)
        if (!anyneed) break;
        n = build_list(need);
        FS_SOLO_SEG(3)
        n_scored += n, n_second++;
        score_list(n);
        FS_SOLO_SEG(4)
      }
      FS_SOLO_SEG(3)
      if (win < 0) break;  // lMax == -1: nothing is added; later rounds would repeat the same state
      double frun = -HUGE_VAL;
      if (A.out.min_gap) {
        // avm_fsel_out::min_gap: the winner's value minus the largest value any OTHER live candidate can have this round - its score if it
        // was scored, else its bound G + g_l, which the check above has put more than 1e-8 (relative) below the winner: exact whenever
        // the gap is smaller than that, a lower bound otherwise
        const bool scd = live && s_scored[c] != 0;
        double r2 = (live && c != win) ? (scd ? s_f[c] : G + s_bound[c]) : -HUGE_VAL;
        if (!(r2 > -1.0)) r2 = -HUGE_VAL;  // (NaN / a failed factorization never wins)
        r2 = fs_wave_max(r2);
        __syncthreads();
        if (lane == 0) s_wf[0][wv] = r2;
        __syncthreads();
        frun = s_wf[0][0];
#pragma unroll
        for (int w = 1; w < NW; w++) frun = fmax(frun, s_wf[0][w]);
        __syncthreads();
      }
      if (t == 0) {
        A.out.selected_ids[(size_t)p * b.max_features + nsel] = b.cand_id[pc + win];
        if (A.out.fvalues) A.out.fvalues[(size_t)p * b.max_features + nsel] = fwin;
        if (A.out.min_gap) A.out.min_gap[(size_t)p * b.max_features + nsel] = fwin - frun;
        A.out.n_selected[p] = nsel + 1;
        A.black[pc + win] = 1;
      }
      nsel++;
      gprev = fwin - G, G = fwin;  // the winner's value IS logdet of the next C
      const double prw = s_pr[win];
      const double* Dw = Dp + (size_t)win * T * T;
      constexpr int NFOLD = (T * T + FS_SOLO_NT - 1) / FS_SOLO_NT;  // (the thread's entries of the winner's Delta in one trip to memory)
      double dwv[NFOLD];
#pragma unroll
      for (int q = 0; q < NFOLD; q++) dwv[q] = Dw[min(t + q * FS_SOLO_NT, T * T - 1)];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int q = 0; q < NFOLD; q++) {
        const int idx = t + q * FS_SOLO_NT;
        if (idx < T * T) {
          sC[idx] = sC[idx] + prw * dwv[q];
          if (idx / T == idx % T) sdpp[idx / T] = sdpp[idx / T] + prw * dwv[q];
        }
      }
      if (t == 0) s_alive[win] = 0;
      __syncthreads();
      FS_SOLO_SEG(5)
    }
#undef FS_SOLO_SEG
#undef FS_SOLO_Q
    if (stats && t == 0) {  // (cycles: marks + estimates, list, first-pass scores, pick + check, second-pass scores, fold; then the counters)
      long long* o = reinterpret_cast<long long*>(sync + 32);
      for (int i = 0; i < 6; i++) o[i] = tk[i];
      o[6] = n_scored, o[7] = n_second, o[8] = nsel, o[9] = n_flag, o[10] = n_pass;
      for (int i = 0; i < 4; i++) o[11 + i] = tq[i];
    }
    if (t == 0) {
      A.nsel[p] = nsel;
      __hip_atomic_fetch_add(&sync[4], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // frames finished
      // candidate evaluations this frame executed (what bench.py prices the solo form's roofline on): a 64-bit count at sync[16..17]
      __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(sync + 16), (unsigned long long)n_scored, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
}
