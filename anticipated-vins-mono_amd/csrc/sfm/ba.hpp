// sfm/ba.hpp - the full BA of GlobalSFM::construct (initial_sfm.cpp:232-289) in the statement's reading of Ceres' TrustRegionMinimizer
// (LEVENBERG_MARQUARDT, DENSE_SCHUR, defaults) for one stream and one team.
//   residual rows   are never stored (4 224 x 20 doubles): obs_row() recomputes a row from the state wherever it is needed - the same
//                   function on the same bits gives the same row in the linearization, the elimination and the model cost.
//   linearize       per frame one pass over the points and ONE reduction of 28 sums (the 21 entries of sum Jc^T Jc, Jc^T r, r^T r); a
//                   point's own sums (gradient, V) are its thread's.
//   lm_step         S = sum U - sum_j E_j V_j^-1 E_j^T: the points are eliminated one 3 x 3 block at a time, chunks of 16 points of E and
//                   E V^-1 (64 rows x 48 columns each) stand in LDS and the team's schur_chunk() multiplies them (v_mfma_f64_16x16x4 on
//                   the device: wavefront w holds row tile w of the 64 x 64 system in 4 accumulators across all chunks).  Row 63 of E
//                   carries the points' gradients, so column 63 of the product is the right-hand side's correction.  Then the Cholesky
//                   factorization of the 57 x 57 system in LDS, left-looking, the right-hand side as row 57.
// Summation orders are fixed by the indices alone: no atomics, the result does not depend on the batch.
#pragma once
#include "chain.hpp"

namespace avm {
namespace sfm {

enum { TERM_NO_CONVERGENCE = 0, TERM_GRADIENT = 1, TERM_PARAMETER = 2, TERM_FUNCTION = 3, TERM_MIN_RADIUS = 4, TERM_FAILURE = 5 };
struct BaSummary {
  double initial_cost, final_cost;
  int iterations, successful, termination;
};

struct ObsRow {
  double r[2], Jc[2][6], Jp[2][3];
};
SFM_HD void obs_res(const double* Rn, const double* ct, const double* X, const double* uv, double* r, double* p, double* pr) {
  mulv(Rn, X, pr);
  for (int c = 0; c < 3; c++) p[c] = pr[c] + ct[c];
  r[0] = p[0] / p[2] - uv[0], r[1] = p[1] / p[2] - uv[1];
}
// the row of one observation; scc / scp: the Jacobi scales (null: the unscaled row); a constant camera column is zero
SFM_HD void obs_row(const double* Rn, const double* ct, const double* X, const double* uv, const int* cidx, const double* scc, const double* scp,
                    ObsRow& o) {
  double p[3], pr[3];
  obs_res(Rn, ct, X, uv, o.r, p, pr);
  const double iz = 1 / p[2];
  const double dp[2][3] = {{iz, 0, -p[0] * iz * iz}, {0, iz, -p[1] * iz * iz}};
  double K[9];
  skew33(pr, K);
  for (int a = 0; a < 2; a++)
    for (int c = 0; c < 3; c++) {
      o.Jc[a][c] = dp[a][0] * (K[c] * -2) + dp[a][1] * (K[3 + c] * -2) + dp[a][2] * (K[6 + c] * -2);
      o.Jc[a][3 + c] = dp[a][c];
      o.Jp[a][c] = dp[a][0] * Rn[c] + dp[a][1] * Rn[3 + c] + dp[a][2] * Rn[6 + c];
    }
  for (int c = 0; c < 6; c++) {
    const double s = cidx[c] < 0 ? 0.0 : scc ? scc[cidx[c]] : 1.0;
    o.Jc[0][c] *= s, o.Jc[1][c] *= s;
  }
  if (scp)
    for (int c = 0; c < 3; c++) o.Jp[0][c] *= scp[c], o.Jp[1][c] *= scp[c];
}

template <class Team>
SFM_HD void set_rotations(Team& tm, const double* q, double* Rn) {
  for (int f = tm.tid(); f < NK; f += Team::NT) {
    const double* c = q + 4 * f;
    const double s = 1 / sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2] + c[3] * c[3]);
    const double n[4] = {c[0] * s, c[1] * s, c[2] * s, c[3] * s};
    q2R9(n, Rn + 9 * f);
  }
  tm.sync();
}

// sum of squares of the ambient vector: quaternions of the free rotations, free translations, points (b: subtracted first, or null)
template <class Team>
SFM_HD double ambient_norm(Team& tm, const StreamIn& in, ChainLds& sh, bool diff) {
  double s = 0;
  for (int f = tm.tid(); f < NK; f += Team::NT) {
    if (sh.cidx[6 * f] >= 0)
      for (int c = 0; c < 4; c++) {
        const double d = diff ? sh.cq[4 * f + c] - sh.nq[4 * f + c] : sh.cq[4 * f + c];
        s += d * d;
      }
    if (sh.cidx[6 * f + 3] >= 0)
      for (int c = 0; c < 3; c++) {
        const double d = diff ? sh.ct[3 * f + c] - sh.nt[3 * f + c] : sh.ct[3 * f + c];
        s += d * d;
      }
  }
  for (int j = tm.tid(); j < in.nf; j += Team::NT) {
    if (!sh.state[j]) continue;
    for (int c = 0; c < 3; c++) {
      const double x = sh.X[3 * j + c];
      const double d = diff ? x - (x + sh.sp[3 * j + c] * sh.scp[3 * j + c]) : x;
      s += d * d;
    }
  }
  tm.template sum<1>(&s);
  return sqrt(s);
}

// cost of (q, t given through Rn / ct, X or the candidate X + sp scp)
template <class Team>
SFM_HD double ba_cost(Team& tm, const StreamIn& in, ChainLds& sh, const double* Rn, const double* ct, bool cand) {
  double s = 0;
  for (int j = tm.tid(); j < in.nf; j += Team::NT) {
    if (!sh.state[j]) continue;
    double X[3], r[2], p[3], pr[3];
    for (int c = 0; c < 3; c++) X[c] = cand ? sh.X[3 * j + c] + sh.sp[3 * j + c] * sh.scp[3 * j + c] : sh.X[3 * j + c];
    for (int f = in.start[j]; f < in.start[j] + in.nobs[j]; f++) {
      obs_res(Rn + 9 * f, ct + 3 * f, X, obs_of(in, j, f), r, p, pr);
      s += r[0] * r[0] + r[1] * r[1];
    }
  }
  tm.template sum<1>(&s);
  return s / 2;
}

// cost; U, gc, gp into LDS; the unscaled gradient's max norm to *gmax.  first: the Jacobi scales are taken here
template <class Team>
SFM_HD double linearize(Team& tm, const StreamIn& in, ChainLds& sh, bool first, double* gmax) {
  set_rotations(tm, sh.cq, sh.Rn);
  ObsRow o;
  if (first) {
    for (int f = 0; f < NK; f++) {
      double a[6] = {0, 0, 0, 0, 0, 0};
      for (int j = tm.tid(); j < in.nf; j += Team::NT) {
        if (!sh.state[j] || !sees(in, j, f)) continue;
        obs_row(sh.Rn + 9 * f, sh.ct + 3 * f, sh.X + 3 * j, obs_of(in, j, f), sh.cidx + 6 * f, nullptr, nullptr, o);
        for (int c = 0; c < 6; c++) a[c] += o.Jc[0][c] * o.Jc[0][c] + o.Jc[1][c] * o.Jc[1][c];
      }
      tm.template sum<6>(a);
      if (tm.tid() == 0)
        for (int c = 0; c < 6; c++)
          if (sh.cidx[6 * f + c] >= 0) sh.scc[sh.cidx[6 * f + c]] = 1 / (1 + sqrt(a[c]));
    }
    for (int j = tm.tid(); j < in.nf; j += Team::NT) {
      if (!sh.state[j]) continue;
      double n2[3] = {0, 0, 0};
      for (int f = in.start[j]; f < in.start[j] + in.nobs[j]; f++) {
        obs_row(sh.Rn + 9 * f, sh.ct + 3 * f, sh.X + 3 * j, obs_of(in, j, f), sh.cidx + 6 * f, nullptr, nullptr, o);
        for (int c = 0; c < 3; c++) n2[c] += o.Jp[0][c] * o.Jp[0][c] + o.Jp[1][c] * o.Jp[1][c];
      }
      for (int c = 0; c < 3; c++) sh.scp[3 * j + c] = 1 / (1 + sqrt(n2[c]));
    }
    tm.sync();
  }
  for (int j = tm.tid(); j < in.nf; j += Team::NT) sh.gp[3 * j] = sh.gp[3 * j + 1] = sh.gp[3 * j + 2] = 0;
  double cost = 0;
  for (int f = 0; f < NK; f++) {
    double a[28];
    for (int i = 0; i < 28; i++) a[i] = 0;
    for (int j = tm.tid(); j < in.nf; j += Team::NT) {
      if (!sh.state[j] || !sees(in, j, f)) continue;
      obs_row(sh.Rn + 9 * f, sh.ct + 3 * f, sh.X + 3 * j, obs_of(in, j, f), sh.cidx + 6 * f, sh.scc, sh.scp + 3 * j, o);
      int s = 0;
      for (int p = 0; p < 6; p++)
        for (int q = p; q < 6; q++) a[s++] += o.Jc[0][p] * o.Jc[0][q] + o.Jc[1][p] * o.Jc[1][q];
      for (int c = 0; c < 6; c++) a[21 + c] += o.Jc[0][c] * o.r[0] + o.Jc[1][c] * o.r[1];
      a[27] += o.r[0] * o.r[0] + o.r[1] * o.r[1];
      for (int c = 0; c < 3; c++) sh.gp[3 * j + c] += o.Jp[0][c] * o.r[0] + o.Jp[1][c] * o.r[1];  // (the point's own thread, frames ascending)
    }
    tm.template sum<28>(a);
    cost += a[27];
    if (tm.tid() == 0) {
      for (int i = 0; i < 21; i++) sh.U[21 * f + i] = a[i];
      for (int c = 0; c < 6; c++)
        if (sh.cidx[6 * f + c] >= 0) sh.gc[sh.cidx[6 * f + c]] = a[21 + c];
    }
  }
  tm.sync();
  // max norm of x - Plus(x, -gradient), the gradient unscaled
  double g = 0;
  for (int f = tm.tid(); f < NK; f += Team::NT) {
    const int* ci = sh.cidx + 6 * f;
    if (ci[0] >= 0) {
      double d[3], qp[4];
      for (int c = 0; c < 3; c++) d[c] = -sh.gc[ci[c]] / sh.scc[ci[c]];
      quat_plus(sh.cq + 4 * f, d, qp);
      for (int c = 0; c < 4; c++) g = fmax(g, fabs(sh.cq[4 * f + c] - qp[c]));
    }
    if (ci[3] >= 0)
      for (int c = 3; c < 6; c++) g = fmax(g, fabs(sh.gc[ci[c]] / sh.scc[ci[c]]));
  }
  for (int j = tm.tid(); j < in.nf; j += Team::NT)
    if (sh.state[j])
      for (int c = 0; c < 3; c++) g = fmax(g, fabs(sh.gp[3 * j + c] / sh.scp[3 * j + c]));
  *gmax = tm.max1(g);
  return cost / 2;
}

SFM_HD double clamp_diag(double v) { return fmin(fmax(v, 1e-6), 1e32); }
SFM_HD int sym6(int a, int b) {  // index of (a, b) in the 21 upper entries, row by row
  if (a > b) {
    const int t = a;
    a = b, b = t;
  }
  return a * 6 - a * (a - 1) / 2 + (b - a);
}

// the step of (JtJ + D^2) y = Jt r by elimination of the points: -y of the cameras into sh.yc, of the points into sh.sp; *mcc: the
// model cost change.  false: a pivot of the reduced system is not positive
template <class Team>
SFM_HD bool lm_step(Team& tm, const StreamIn& in, ChainLds& sh, double radius, double* mcc) {
  ObsRow o;
  for (int i = tm.tid(); i < 64 * LDS_S; i += Team::NT) sh.S[i] = 0;
  for (int i = tm.tid(); i < 64 * LDW; i += Team::NT) sh.Y[i] = 0, sh.W[i] = 0;
  // V^-1 per point
  for (int j = tm.tid(); j < in.nf; j += Team::NT) {
    if (!sh.state[j]) continue;
    double V[6] = {0, 0, 0, 0, 0, 0};
    for (int f = in.start[j]; f < in.start[j] + in.nobs[j]; f++) {
      obs_row(sh.Rn + 9 * f, sh.ct + 3 * f, sh.X + 3 * j, obs_of(in, j, f), sh.cidx + 6 * f, sh.scc, sh.scp + 3 * j, o);
      int s = 0;
      for (int p = 0; p < 3; p++)
        for (int q = p; q < 3; q++) V[s++] += o.Jp[0][p] * o.Jp[0][q] + o.Jp[1][p] * o.Jp[1][q];
    }
    V[0] += clamp_diag(V[0]) / radius, V[3] += clamp_diag(V[3]) / radius, V[5] += clamp_diag(V[5]) / radius;
    inv3sym(V, sh.Vi + 6 * j);
  }
  tm.sync();
  for (int i = tm.tid(); i < NK * 36; i += Team::NT) {
    const int f = i / 36, a = (i % 36) / 6, b = i % 6;
    const int ia = sh.cidx[6 * f + a], ib = sh.cidx[6 * f + b];
    if (ia < 0 || ib < 0) continue;
    sh.S[ia * LDS_S + ib] = sh.U[21 * f + sym6(a, b)];
    if (a == b) sh.dc[ia] = sh.U[21 * f + sym6(a, a)];
  }
  tm.schur_zero();
  for (int j0 = 0; j0 < in.nf; j0 += CHUNK) {
    tm.sync();  // (the product of the chunk before has read Y and W)
    for (int w = tm.tid(); w < CHUNK * 16; w += Team::NT) {
      const int pl = w / 16, f = w % 16, j = j0 + pl;
      const bool pt = j < in.nf && sh.state[j];
      if (f == NK)
        for (int c = 0; c < 3; c++) sh.W[63 * LDW + 3 * pl + c] = pt ? sh.gp[3 * j + c] : 0.0;
      if (f >= NK) continue;
      double Wf[6][3], Yf[6][3];
      const bool on = pt && sees(in, j, f);
      if (on) {
        obs_row(sh.Rn + 9 * f, sh.ct + 3 * f, sh.X + 3 * j, obs_of(in, j, f), sh.cidx + 6 * f, sh.scc, sh.scp + 3 * j, o);
        for (int a = 0; a < 6; a++) {
          for (int c = 0; c < 3; c++) Wf[a][c] = o.Jc[0][a] * o.Jp[0][c] + o.Jc[1][a] * o.Jp[1][c];
          sym3mulv(sh.Vi + 6 * j, Wf[a], Yf[a]);
        }
      }
      for (int a = 0; a < 6; a++) {
        const int row = sh.cidx[6 * f + a];
        if (row < 0) continue;
        for (int c = 0; c < 3; c++) sh.W[row * LDW + 3 * pl + c] = on ? Wf[a][c] : 0.0, sh.Y[row * LDW + 3 * pl + c] = on ? Yf[a][c] : 0.0;
      }
    }
    tm.sync();
    tm.schur_chunk(sh.Y, sh.W);
  }
  tm.sync();
  tm.schur_store(sh.S);  // S -= sum of the chunks' Y W^T
  tm.sync();
  for (int i = tm.tid(); i < NCAM; i += Team::NT) {
    sh.S[NCAM * LDS_S + i] = sh.gc[i] + sh.S[i * LDS_S + 63];  // rhs = gc - sum_j Y_j gp_j
    sh.S[i * LDS_S + i] += clamp_diag(sh.dc[i]) / radius;
  }
  tm.sync();
  // L L^T = S in the lower triangle, row 57 becomes y = L^-1 rhs
  for (int j = 0; j < NCAM; j++) {
    double d = sh.S[j * LDS_S + j];
    for (int k = 0; k < j; k++) d -= sh.S[j * LDS_S + k] * sh.S[j * LDS_S + k];
    if (!(d > 0)) return false;
    const double ljj = sqrt(d);
    tm.sync();
    for (int i = j + tm.tid(); i <= NCAM; i += Team::NT) {
      if (i == j) {
        sh.S[j * LDS_S + j] = ljj;
        continue;
      }
      double s = sh.S[i * LDS_S + j];
      for (int k = 0; k < j; k++) s -= sh.S[i * LDS_S + k] * sh.S[j * LDS_S + k];
      sh.S[i * LDS_S + j] = s / ljj;
    }
    tm.sync();
  }
  for (int i = tm.tid(); i < NCAM; i += Team::NT) sh.yc[i] = sh.S[NCAM * LDS_S + i];
  tm.sync();
  for (int i = NCAM - 1; i >= 0; i--) {
    const double xi = sh.yc[i] / sh.S[i * LDS_S + i];
    tm.sync();
    for (int k = tm.tid(); k <= i; k += Team::NT) sh.yc[k] = k == i ? xi : sh.yc[k] - sh.S[i * LDS_S + k] * xi;
    tm.sync();
  }
  for (int i = tm.tid(); i < NCAM; i += Team::NT) sh.yc[i] = -sh.yc[i];
  tm.sync();
  // the points' steps and the model cost change
  double m = 0;
  for (int j = tm.tid(); j < in.nf; j += Team::NT) {
    if (!sh.state[j]) continue;
    double t[3] = {sh.gp[3 * j], sh.gp[3 * j + 1], sh.gp[3 * j + 2]};
    for (int f = in.start[j]; f < in.start[j] + in.nobs[j]; f++) {
      obs_row(sh.Rn + 9 * f, sh.ct + 3 * f, sh.X + 3 * j, obs_of(in, j, f), sh.cidx + 6 * f, sh.scc, sh.scp + 3 * j, o);
      for (int a = 0; a < 6; a++) {
        const int row = sh.cidx[6 * f + a];
        if (row < 0) continue;
        for (int c = 0; c < 3; c++) t[c] += (o.Jc[0][a] * o.Jp[0][c] + o.Jc[1][a] * o.Jp[1][c]) * sh.yc[row];
      }
    }
    double sp[3];
    sym3mulv(sh.Vi + 6 * j, t, sp);
    for (int c = 0; c < 3; c++) sp[c] = -sp[c], sh.sp[3 * j + c] = sp[c];
    for (int f = in.start[j]; f < in.start[j] + in.nobs[j]; f++) {
      obs_row(sh.Rn + 9 * f, sh.ct + 3 * f, sh.X + 3 * j, obs_of(in, j, f), sh.cidx + 6 * f, sh.scc, sh.scp + 3 * j, o);
      double mm[2];
      for (int a = 0; a < 2; a++) {
        mm[a] = o.Jp[a][0] * sp[0] + o.Jp[a][1] * sp[1] + o.Jp[a][2] * sp[2];
        for (int c = 0; c < 6; c++)
          if (sh.cidx[6 * f + c] >= 0) mm[a] += o.Jc[a][c] * sh.yc[sh.cidx[6 * f + c]];
      }
      m -= mm[0] * (o.r[0] + mm[0] / 2) + mm[1] * (o.r[1] + mm[1] / 2);
    }
  }
  tm.template sum<1>(&m);
  *mcc = m;
  return true;
}

// sh.cq, sh.ct, sh.X (the features with state) are adjusted in place
template <class Team>
SFM_HD BaSummary bundle_adjust(Team& tm, const StreamIn& in, ChainLds& sh) {
  if (tm.tid() == 0) {
    int n = 0;
    for (int f = 0; f < NK; f++)
      for (int c = 0; c < 6; c++) {
        const bool cst = (c < 3 && f == in.l) || (c >= 3 && (f == in.l || f == NK - 1));
        sh.cidx[6 * f + c] = cst ? -1 : n++;
      }
  }
  for (int i = tm.tid(); i < 64; i += Team::NT) sh.gc[i] = sh.dc[i] = sh.yc[i] = 0, sh.scc[i] = 1;
  tm.sync();
  BaSummary su;
  double gmax, x_norm = ambient_norm(tm, in, sh, false);
  double x_cost = linearize(tm, in, sh, true, &gmax);
  su.initial_cost = x_cost;
  double radius = 1e4, decrease = 2;
  int it = 0, n_ok = 0, invalid = 0, term = -1;
  bool ok_step = true;
  for (;;) {
    if (it >= in.max_it)
      term = TERM_NO_CONVERGENCE;
    else if (ok_step && !(gmax > 1e-10))
      term = TERM_GRADIENT;
    else if (radius <= 1e-32)
      term = TERM_MIN_RADIUS;
    if (term >= 0) break;
    it++;
    ok_step = false;
    double mcc = 0;
    const bool solved = lm_step(tm, in, sh, radius, &mcc);
    if (!(solved && mcc > 0)) {
      if (++invalid >= 5) {
        term = TERM_FAILURE;
        break;
      }
      radius = radius / decrease, decrease = decrease * 2;
      continue;
    }
    invalid = 0;
    for (int f = tm.tid(); f < NK; f += Team::NT) {
      const int* ci = sh.cidx + 6 * f;
      if (ci[0] >= 0) {
        const double d[3] = {sh.yc[ci[0]] * sh.scc[ci[0]], sh.yc[ci[1]] * sh.scc[ci[1]], sh.yc[ci[2]] * sh.scc[ci[2]]};
        quat_plus(sh.cq + 4 * f, d, sh.nq + 4 * f);
      } else {
        for (int c = 0; c < 4; c++) sh.nq[4 * f + c] = sh.cq[4 * f + c];
      }
      for (int c = 0; c < 3; c++) sh.nt[3 * f + c] = ci[3] >= 0 ? sh.ct[3 * f + c] + sh.yc[ci[3 + c]] * sh.scc[ci[3 + c]] : sh.ct[3 * f + c];
    }
    tm.sync();
    set_rotations(tm, sh.nq, sh.Rn2);
    const double cand_cost = ba_cost(tm, in, sh, sh.Rn2, sh.nt, true);
    const double step_norm = ambient_norm(tm, in, sh, true);
    if (!(step_norm > 1e-8 * (x_norm + 1e-8))) {
      term = TERM_PARAMETER;
      break;
    }
    if (!(fabs(x_cost - cand_cost) > 1e-6 * x_cost)) {
      term = TERM_FUNCTION;
      break;
    }
    const double rho = (x_cost - cand_cost) / mcc;
    if (rho > 1e-3) {
      tm.sync();
      for (int i = tm.tid(); i < NK * 4; i += Team::NT) sh.cq[i] = sh.nq[i];
      for (int i = tm.tid(); i < NK * 3; i += Team::NT) sh.ct[i] = sh.nt[i];
      for (int j = tm.tid(); j < in.nf; j += Team::NT)
        if (sh.state[j])
          for (int c = 0; c < 3; c++) sh.X[3 * j + c] = sh.X[3 * j + c] + sh.sp[3 * j + c] * sh.scp[3 * j + c];
      tm.sync();
      x_norm = ambient_norm(tm, in, sh, false);
      x_cost = linearize(tm, in, sh, false, &gmax);
      ok_step = true, n_ok++;
      const double t = 2 * rho - 1;
      radius = fmin(radius / fmax(1.0 / 3.0, 1 - t * t * t), 1e16);
      decrease = 2;
    } else {
      radius = radius / decrease, decrease = decrease * 2;
    }
  }
  su.final_cost = x_cost;
  su.iterations = it, su.successful = n_ok, su.termination = term;
  return su;
}

}  // namespace sfm
}  // namespace avm
