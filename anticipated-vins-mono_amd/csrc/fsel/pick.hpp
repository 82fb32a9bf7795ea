// fsel/pick.hpp - the double-buffered round state (FselPar) and the round's winner: fsel_pick_local, fsel_pick_frame
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

constexpr int FS_CPWG = (FS_NT / 64) * 4;  // candidates per workgroup of the round and frame kernels

// State that changes from round to round exists twice (C, dpp, the live list and its inverse, nlive, fval, ub: buffer `par` at
// offset par * size): launch k reads the buffers k & 1 and writes the others, so that no workgroup of a launch reads what another
// one writes.  That lets ONE launch per round do both halves of a greedy step:
//   1. every workgroup picks the winner of the previous round for itself from the values the previous launch left (a few KB,
//      the same deterministic argmax everywhere; workgroup 0 of the problem also records it and writes the next buffers:
//      C + p Delta_winner, the live list with the winner swap-removed);
//   2. it evaluates its candidates against that next state, which it patches in on the fly (the same expressions workgroup 0
//      stores, so the values are bit-identical to the stored ones).
// Round 1 and the first half of round 2 launched a pick kernel between two evaluations: 300 dependent launches per select, and the
// gaps between them were 40 % of the time.  Now 151.
struct FselPar {
  const double *C, *dpp, *fval, *ub;
  const int32_t *live, *pos;
  double *Cn, *dppn, *fvaln, *ubn;
  int32_t *liven, *posn, *nliven;
  int nl;
};
AVM_DEV FselPar fsel_par(const FselDev& A, int p, int k) {
  const avm_fsel_batch& b = A.b;
  const int T = 3 * b.horizon, cur = k & 1, nxt = cur ^ 1;
  const size_t P = b.n_problems, mc = b.max_cand, TT = (size_t)T * T;
  FselPar r;
  r.C = A.C + (cur * P + p) * TT, r.Cn = A.C + (nxt * P + p) * TT;
  r.dpp = A.dpp + (cur * P + p) * T, r.dppn = A.dpp + (nxt * P + p) * T;
  r.fval = A.fval + (cur * P + p) * mc, r.fvaln = A.fval + (nxt * P + p) * mc;
  r.ub = A.ub + (cur * P + p) * mc, r.ubn = A.ub + (nxt * P + p) * mc;
  r.live = A.live + (cur * P + p) * mc, r.liven = A.live + (nxt * P + p) * mc;
  r.pos = A.pos + (cur * P + p) * mc, r.posn = A.pos + (nxt * P + p) * mc;
  r.nl = A.nlive[cur * P + p], r.nliven = A.nlive + nxt * P + p;
  return r;
}

// ---- the round's winner (feature_selector.cpp:669-683), computed by every workgroup of the problem for itself ---------------
// returns the winner's candidate index (-1: none) to all threads; *fwin its value; *frun (when the caller asked for avm_fsel_out::min_gap)
// the largest value among the OTHER candidates of the round (-HUGE_VAL: nobody else took part)
AVM_DEV int fsel_pick_local(const FselDev& A, const FselPar& S, double* fwin, double* frun) {
  __shared__ double s_f[FS_NT / 64], s_u[FS_NT / 64];
  __shared__ int s_i[FS_NT / 64];
  __shared__ int s_win;
  const int t = threadIdx.x;
  const int32_t* live = S.live;
  const int nl = S.nl;
  auto better = [](double f, double u, int i, double f2, double u2, int i2) {
    if (i2 < 0) return false;
    if (i < 0) return true;
    return f2 > f || (f2 == f && (u2 > u || (u2 == u && i2 > i)));
  };
  // sortedlogDetUB keeps the upper bounds in a std::map<double, int> (feature_selector.cpp:724): of two live candidates
  // with BIT-IDENTICAL upper bounds only the later (higher) id survives the round, the other one is never scored.  The
  // argmax below therefore runs until its winner is not shadowed by a higher id with the same key; `shadowed` holds the
  // (at most a handful of) candidates that were ruled out this way.  One extra pass over the bounds in the usual case.
  constexpr int MAXSH = 8;
  __shared__ int s_shadow[MAXSH];
  __shared__ int s_nsh, s_hit;
  __syncthreads();  // (the shared variables may still be read by a slower wavefront of this workgroup's previous use)
  if (t == 0) s_nsh = 0;
  __syncthreads();
  // this thread's candidates (at most FS_PC of them) stay in registers for every pass of the loop below
  constexpr int FS_PC = 4;  // (candidates beyond FS_PC * FS_NT = 1024 are re-read in every pass)
  int cl[FS_PC];
  double cf[FS_PC], cu[FS_PC];
  // (values are stored by SLOT of the live list they were computed for - the list of these buffers - so the three loads are
  //  independent: one trip to memory)
#pragma unroll
  for (int q = 0; q < FS_PC; q++) {
    const int sq = min(t + q * FS_NT, max(nl - 1, 0));
    cl[q] = live[sq], cf[q] = S.fval[sq], cu[q] = S.ub[sq];
    if (t + q * FS_NT >= nl) cl[q] = -1;
  }
  double bf;
  int bi;
  for (;;) {
    // lexicographic max of (fValue, ub, id) over live candidates with fValue > fMax0 = -1.0 (NaN never wins)
    bf = -1.0;
    double bu = -DBL_MAX;
    bi = -1;
    const int nsh = s_nsh;
#pragma unroll
    for (int q = 0; q < FS_PC; q++) {
      const int l = cl[q];
      bool sh = l < 0;
      for (int qq = 0; qq < nsh; qq++) sh |= s_shadow[qq] == l;
      const double f = cf[q], u = cu[q];
      if (sh || !(f > -1.0)) continue;
      if (bi < 0 || f > bf || (f == bf && (u > bu || (u == bu && l > bi)))) bf = f, bu = u, bi = l;
    }
    for (int s = t + FS_PC * FS_NT; s < nl; s += FS_NT) {
      const int l = live[s];
      bool sh = false;
      for (int qq = 0; qq < nsh; qq++) sh |= s_shadow[qq] == l;
      const double f = S.fval[s], u = S.ub[s];
      if (sh || !(f > -1.0)) continue;
      if (bi < 0 || f > bf || (f == bf && (u > bu || (u == bu && l > bi)))) bf = f, bu = u, bi = l;
    }
    {  // the wavefront's best: three maxima in a row, each over the lanes that tie in the previous ones
      const double wf = fs_wave_max(bi >= 0 ? bf : -1.0);
      const bool tf = bi >= 0 && bf == wf;
      const double wu = fs_wave_max(tf ? bu : -DBL_MAX);
      const bool tu = tf && bu == wu;
      bi = fs_wave_max(tu ? bi : -1), bf = wf, bu = wu;
    }
    if ((t & 63) == 0) s_f[t >> 6] = bf, s_u[t >> 6] = bu, s_i[t >> 6] = bi;
    __syncthreads();
    if (t == 0) {
      for (int w = 1; w < FS_NT / 64; w++)
        if (better(bf, bu, bi, s_f[w], s_u[w], s_i[w])) bf = s_f[w], bu = s_u[w], bi = s_i[w];
      s_win = bi, s_f[0] = bf, s_u[0] = bu, s_hit = 0;
    }
    __syncthreads();
    const int cand = s_win;
    if (cand < 0) break;
    const double cuw = s_u[0];
    int hit = 0;
#pragma unroll
    for (int q = 0; q < FS_PC; q++)  // a live candidate with a higher id and the same key?
      if (cl[q] > cand && cu[q] == cuw) hit = 1;
    for (int s = t + FS_PC * FS_NT; s < nl; s += FS_NT)
      if (live[s] > cand && S.ub[s] == cuw) hit = 1;
    if (hit) s_hit = 1;
    __syncthreads();
    if (!s_hit || s_nsh >= MAXSH || A.no_key_rule) break;  // (more than MAXSH chained collisions in one round: keep the last winner)
    __syncthreads();
    if (t == 0) s_shadow[s_nsh++] = cand;
    __syncthreads();
  }
  *fwin = s_f[0];
  if (A.out.min_gap) {  // the runner-up: the best value among the others that took part (the candidates the std::map rule ruled out above did not)
    const int wl = s_win, nsh = s_nsh;
    double r2 = -HUGE_VAL;
#pragma unroll
    for (int q = 0; q < FS_PC; q++) {
      const int l = cl[q];
      bool sh = l < 0 || l == wl;
      for (int qq = 0; qq < nsh; qq++) sh |= s_shadow[qq] == l;
      if (!sh && cf[q] > -1.0) r2 = fmax(r2, cf[q]);
    }
    for (int sq = t + FS_PC * FS_NT; sq < nl; sq += FS_NT) {
      const int l = live[sq];
      bool sh = l == wl;
      for (int qq = 0; qq < nsh; qq++) sh |= s_shadow[qq] == l;
      const double f = S.fval[sq];
      if (!sh && f > -1.0) r2 = fmax(r2, f);
    }
    r2 = fs_wave_max(r2);
    __syncthreads();  // (s_u is free: every thread has read the winner's bound)
    if ((t & 63) == 0) s_u[t >> 6] = r2;
    __syncthreads();
    double rr = s_u[0];
#pragma unroll
    for (int w = 1; w < FS_NT / 64; w++) rr = fmax(rr, s_u[w]);
    *frun = rr;
  }
  return s_win;
}

// The same pick for the single-frame kernel (slot s IS candidate s; the caller hands in this thread's two candidates - index -1 =
// not in the race - with the values it has read): two workgroup barriers per pass, the shadow list in registers, and the
// lexicographic maximum of (fValue, ub, id) as three maxima in a row, each over the lanes that tie in the previous ones.
AVM_DEV int fsel_pick_frame(const FselDev& A, const int* cl, const double* cf, const double* cu, double* fwin, double* frun) {
  __shared__ double s_f[2][FS_NT / 64], s_u[2][FS_NT / 64];
  __shared__ int s_i[2][FS_NT / 64], s_h[2][FS_NT / 64];
  const int t = threadIdx.x, wv = t >> 6;
  constexpr int MAXSH = 8;
  int sh[MAXSH], nsh = 0;
#pragma unroll
  for (int qq = 0; qq < MAXSH; qq++) sh[qq] = -1;
  for (int pass = 0;; pass++) {
    const int sl = pass & 1;
    double bf = -1.0, bu = -DBL_MAX;
    int bi = -1;
#pragma unroll
    for (int q = 0; q < 2; q++) {
      const int l = cl[q];
      bool out = l < 0;
#pragma unroll
      for (int qq = 0; qq < MAXSH; qq++) out |= sh[qq] == l;
      const double f = cf[q], u = cu[q];
      if (out || !(f > -1.0)) continue;
      if (bi < 0 || f > bf || (f == bf && (u > bu || (u == bu && l > bi)))) bf = f, bu = u, bi = l;
    }
    {  // the wavefront's best (a lane without a candidate carries f = -1, which no candidate in the race has)
      const double wf = fs_wave_max(bi >= 0 ? bf : -1.0);
      const bool tf = bi >= 0 && bf == wf;
      const double wu = fs_wave_max(tf ? bu : -DBL_MAX);
      const bool tu = tf && bu == wu;
      const int wi = fs_wave_max(tu ? bi : -1);
      if ((t & 63) == 0) s_f[sl][wv] = wf, s_u[sl][wv] = wu, s_i[sl][wv] = wi;
    }
    __syncthreads();
    bf = s_f[sl][0], bu = s_u[sl][0], bi = s_i[sl][0];
#pragma unroll
    for (int w = 1; w < FS_NT / 64; w++) {
      const double f2 = s_f[sl][w], u2 = s_u[sl][w];
      const int i2 = s_i[sl][w];
      if (i2 >= 0 && (bi < 0 || f2 > bf || (f2 == bf && (u2 > bu || (u2 == bu && i2 > bi))))) bf = f2, bu = u2, bi = i2;
    }
    *fwin = bf;
    // the runner-up for avm_fsel_out::min_gap (see fsel_pick_local): one more maximum, only when it was asked for
    auto runner_up = [&](int wl) {
      if (!A.out.min_gap) return;
      double r2 = -HUGE_VAL;
#pragma unroll
      for (int q = 0; q < 2; q++) {
        const int l = cl[q];
        bool out = l < 0 || l == wl;
#pragma unroll
        for (int qq = 0; qq < MAXSH; qq++) out |= sh[qq] == l;
        if (!out && cf[q] > -1.0) r2 = fmax(r2, cf[q]);
      }
      r2 = fs_wave_max(r2);
      __syncthreads();  // (every thread has read slot sl of s_u)
      if ((t & 63) == 0) s_u[sl][wv] = r2;
      __syncthreads();
      double rr = s_u[sl][0];
#pragma unroll
      for (int w = 1; w < FS_NT / 64; w++) rr = fmax(rr, s_u[sl][w]);
      *frun = rr;
    };
    if (bi < 0 || A.no_key_rule || nsh >= MAXSH) {  // (more than MAXSH chained collisions in one round: keep the last winner)
      runner_up(bi);
      return bi;
    }
    // std::map rule (see fsel_pick_local): a live candidate with a higher id and the same key shadows the winner
    const bool hit = (cl[0] > bi && cu[0] == bu) || (cl[1] > bi && cu[1] == bu);
    const bool wh = __any(hit);
    if ((t & 63) == 0) s_h[sl][wv] = wh ? 1 : 0;
    __syncthreads();
    int any = 0;
#pragma unroll
    for (int w = 0; w < FS_NT / 64; w++) any |= s_h[sl][w];
    if (!any) {
      runner_up(bi);
      return bi;
    }
#pragma unroll
    for (int qq = 0; qq < MAXSH; qq++)
      if (qq == nsh) sh[qq] = bi;
    nsh++;
  }
}
