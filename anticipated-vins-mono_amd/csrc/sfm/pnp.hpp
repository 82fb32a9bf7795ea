// sfm/pnp.hpp - cv::solvePnP(useExtrinsicGuess, ITERATIVE) with K = I in the CvLevMarq reading of the statement, for a team of
// threads (a 256-thread workgroup in the chain, one wavefront per non-key frame).  Team: NT, tid(), sync(), sum<N>(v) - the fixed-order
// reduction of N values, the result in every thread - and max1(v).  Every decision is taken from reduced values, which are the same
// bits in every thread: the team never diverges, and the 6 x 6 Cholesky runs redundantly in every lane (no broadcast, no barrier).
// Points: a functor pts(i, M, m) -> bool over i in [0, n); thread t takes i = t, t + NT, ...: the summation order depends on nothing
// but the point's index.
#pragma once
#include "math.hpp"

namespace avm {
namespace sfm {

// one pass over the points: err2, and with want_j the symmetric 6 x 6 (21 sums) and J^T e (6): 28 sums, one reduction
template <class Team, class Pts>
SFM_HD double pnp_evaluate(Team& tm, const Pts& pts, int n, const double* p, bool want_j, double* JtJ, double* Jte) {
  double R[9], dR[27];
  rodrigues_mat(p, R, want_j ? dR : nullptr);
  double acc[28];
  for (int i = 0; i < 28; i++) acc[i] = 0;
  for (int i = tm.tid(); i < n; i += Team::NT) {
    double M[3], m[2], X[3];
    if (!pts(i, M, m)) continue;
    mulv(R, M, X);
    X[0] += p[3], X[1] += p[4], X[2] += p[5];
    const double iz = 1 / X[2];
    const double e[2] = {X[0] * iz - m[0], X[1] * iz - m[1]};
    acc[27] += e[0] * e[0] + e[1] * e[1];
    if (!want_j) continue;
    const double dp[2][3] = {{iz, 0, -X[0] * iz * iz}, {0, iz, -X[1] * iz * iz}};
    double J[2][6];
    for (int c = 0; c < 3; c++) {
      double dX[3];
      mulv(dR + 9 * c, M, dX);
      for (int a = 0; a < 2; a++) J[a][c] = dp[a][0] * dX[0] + dp[a][1] * dX[1] + dp[a][2] * dX[2], J[a][3 + c] = dp[a][c];
    }
    int s = 0;
    for (int a = 0; a < 6; a++)
      for (int b = a; b < 6; b++) acc[s++] += J[0][a] * J[0][b] + J[1][a] * J[1][b];
    for (int a = 0; a < 6; a++) acc[21 + a] += J[0][a] * e[0] + J[1][a] * e[1];
  }
  if (want_j) {
    tm.template sum<28>(acc);
    int s = 0;
    for (int a = 0; a < 6; a++)
      for (int b = a; b < 6; b++) JtJ[a * 6 + b] = JtJ[b * 6 + a] = acc[s++];
    for (int a = 0; a < 6; a++) Jte[a] = acc[21 + a];
  } else {
    tm.template sum<1>(acc + 27);
  }
  return acc[27];
}

// R0, t0: the guess; on success R (row-major) and t.  false: theta = pi, a pivot that is not positive, a non-finite step
template <class Team, class Pts>
SFM_HD bool solve_pnp(Team& tm, const Pts& pts, int n, const double* R0, const double* t0, double* R, double* t) {
  // the powers of ten of lambda as the decimal literals they are (correctly rounded)
  const double P10[33] = {1e-16, 1e-15, 1e-14, 1e-13, 1e-12, 1e-11, 1e-10, 1e-9, 1e-8, 1e-7, 1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1e-1, 1e0,
                          1e1,   1e2,   1e3,   1e4,   1e5,   1e6,   1e7,   1e8,  1e9,  1e10, 1e11, 1e12, 1e13, 1e14, 1e15, 1e16};
  double param[6], prev[6], JtJ[36], Jte[6];
  if (!rodrigues_vec(R0, prev)) return false;
  for (int i = 0; i < 3; i++) prev[3 + i] = t0[i];
  for (int i = 0; i < 6; i++) param[i] = prev[i];
  int lg = -3, iters = 0;
  double prev_err2 = pnp_evaluate(tm, pts, n, prev, true, JtJ, Jte);
  // (every pass through the loop either keeps a step - at most 20 - or raises lg - at most 33 times in a row)
  for (int guard = 0; guard < 20 * 40; guard++) {
    double A[36], d[6];
    for (int i = 0; i < 36; i++) A[i] = JtJ[i];
    const double lam = P10[lg + 16];
    for (int i = 0; i < 6; i++) A[i * 7] = A[i * 7] * (1 + lam);
    if (!cholesky_solve<6>(A, Jte, d)) return false;
    for (int i = 0; i < 6; i++) param[i] = prev[i] - d[i];
    const double err2 = pnp_evaluate(tm, pts, n, param, false, nullptr, nullptr);
    bool ok = fin(err2);
    for (int i = 0; i < 6; i++) ok = ok && fin(param[i]);
    if (!ok) return false;
    double dn = 0, pn = 0;
    for (int i = 0; i < 6; i++) dn += (param[i] - prev[i]) * (param[i] - prev[i]), pn += prev[i] * prev[i];
    dn = sqrt(dn), pn = sqrt(pn);
    const double change = pn > 0 ? dn / pn : INFINITY;
    if (err2 > prev_err2) {
      lg += 1;
      if (lg <= 16) continue;
    }
    lg = lg - 1 > -16 ? lg - 1 : -16;
    iters += 1;
    if (iters >= 20 || !(change > (double)FLT_EPSILON)) break;
    for (int i = 0; i < 6; i++) prev[i] = param[i];
    prev_err2 = pnp_evaluate(tm, pts, n, prev, true, JtJ, Jte);
  }
  rodrigues_mat(param, R, nullptr);
  t[0] = param[3], t[1] = param[4], t[2] = param[5];
  return true;
}

}  // namespace sfm
}  // namespace avm
