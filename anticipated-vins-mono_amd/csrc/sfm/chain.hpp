// sfm/chain.hpp - GlobalSFM::construct up to the BA (initial_sfm.cpp:117-217) for one stream and one team: sfm_f from the track tables,
// the poses of l and 10 from relativePose's result, the forward chain (PnP, triangulateTwoFrames), the l - i triangulations, the backward
// chain, the leftovers.  "state already true => skip" and the order of the pairs are the statement's run().
#pragma once
#include "pnp.hpp"

namespace avm {
namespace sfm {

constexpr int MAXF = 384;  // AVM_MAX_FEAT_WIDE: features of a stream
constexpr int LDW = 49;    // row stride of a chunk of E (48 columns: 16 points): odd, so the 16 rows of an MFMA operand fall into 16 different bank pairs
constexpr int CHUNK = 16;  // points per chunk

// one stream's inputs (pointers at the stream's own rows)
struct StreamIn {
  int l, nf, n_frames, max_it, max_pts;
  const int32_t *start, *nobs, *obeg, *key, *frame_n_pts, *frame_pt_id, *feat_id;
  const double *obs, *relR, *relT, *ex_pose, *frame_pt_xy;
};
SFM_HD bool sees(const StreamIn& in, int j, int f) { return f >= in.start[j] && f < in.start[j] + in.nobs[j]; }
SFM_HD const double* obs_of(const StreamIn& in, int j, int f) { return in.obs + 2 * (size_t)(in.obeg[j] + f - in.start[j]); }

// the workgroup's LDS (the host build: a plain struct).  145 KiB: one workgroup per CU.
struct ChainLds {
  double S[64 * LDS_S];                  // the reduced camera system, row 57 the right-hand side
  double Y[64 * LDW], W[64 * LDW];       // a chunk of E V^-1 and of E (row 63 of W: the points' gradients)
  double X[MAXF * 3], scp[MAXF * 3], gp[MAXF * 3], Vi[MAXF * 6], sp[MAXF * 3];  // per point: position, Jacobi scale, gradient, V^-1, step
  double U[NK * 21], gc[64], dc[64], scc[64], yc[64];  // per frame sum of Jc^T Jc; camera gradient, diagonal, Jacobi scale, step
  double cq[NK * 4], ct[NK * 3], nq[NK * 4], nt[NK * 3], Rn[NK * 9], Rn2[NK * 9];  // cameras, the candidate, their rotations
  double cR[NK * 9], Pose[NK * 12];      // the chain's rotations and [R | t]
  double red[4 * 28];
  int state[MAXF];
  int cidx[NK * 6];
};

template <class Team>
SFM_HD void tri_two(Team& tm, const StreamIn& in, ChainLds& sh, int f0, int f1) {
  for (int j = tm.tid(); j < in.nf; j += Team::NT) {
    if (sh.state[j] || !sees(in, j, f0) || !sees(in, j, f1)) continue;
    const double *a = obs_of(in, j, f0), *b = obs_of(in, j, f1);
    triangulate_point(sh.Pose + 12 * f0, sh.Pose + 12 * f1, a[0], a[1], b[0], b[1], sh.X + 3 * j);
    sh.state[j] = 1;
  }
  tm.sync();
}

// cR[i], ct[i] (all threads hold the same R, t) -> LDS, with cq[i] and Pose[i]
template <class Team>
SFM_HD void set_camera(Team& tm, ChainLds& sh, int i, const double* R, const double* t, const double* q) {
  if (tm.tid() == 0) {
    for (int k = 0; k < 9; k++) sh.cR[9 * i + k] = R[k];
    for (int k = 0; k < 3; k++) sh.ct[3 * i + k] = t[k];
    if (q) {
      for (int k = 0; k < 4; k++) sh.cq[4 * i + k] = q[k];
    } else {
      R2q4(R, sh.cq + 4 * i);
    }
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) sh.Pose[12 * i + 4 * r + c] = R[3 * r + c];
      sh.Pose[12 * i + 4 * r + 3] = t[r];
    }
  }
  tm.sync();
}

template <class Team>
SFM_HD bool chain_step(Team& tm, const StreamIn& in, ChainLds& sh, int i, int src) {
  double cnt = 0;
  for (int j = tm.tid(); j < in.nf; j += Team::NT) cnt += (sh.state[j] && sees(in, j, i)) ? 1.0 : 0.0;
  tm.template sum<1>(&cnt);
  if (cnt < 10) return false;
  auto pts = [&](int j, double* M, double* m) {
    if (!sh.state[j] || !sees(in, j, i)) return false;
    const double* o = obs_of(in, j, i);
    m[0] = f32r(o[0]), m[1] = f32r(o[1]);
    for (int c = 0; c < 3; c++) M[c] = f32r(sh.X[3 * j + c]);
    return true;
  };
  double R0[9], t0[3], R[9], t[3];
  for (int k = 0; k < 9; k++) R0[k] = sh.cR[9 * src + k];
  for (int k = 0; k < 3; k++) t0[k] = sh.ct[3 * src + k];
  if (!solve_pnp(tm, pts, in.nf, R0, t0, R, t)) return false;
  set_camera(tm, sh, i, R, t, nullptr);
  return true;
}

// false: a chain frame has fewer than 10 points or its PnP fails (ok = 1)
template <class Team>
SFM_HD bool run_chain(Team& tm, const StreamIn& in, ChainLds& sh) {
  const int l = in.l;
  for (int j = tm.tid(); j < MAXF; j += Team::NT) sh.state[j] = 0, sh.X[3 * j] = sh.X[3 * j + 1] = sh.X[3 * j + 2] = 0;
  tm.sync();
  {  // q[l] = 1, T[l] = 0; q[10] = q[l] * Quaterniond(relative_R), T[10] = relative_T; c_* = their inverses
    const double ql[4] = {1, 0, 0, 0}, Tl[3] = {0, 0, 0};
    double qr[4], q10[4];
    R2q4(in.relR, qr);
    qmul4(ql, qr, q10);
    for (int s = 0; s < 2; s++) {
      const double* q = s ? q10 : ql;
      const double* T = s ? in.relT : Tl;
      double cq[4], R[9], t[3];
      qinv4(q, cq);
      q2R9(cq, R);
      mulv(R, T, t);
      for (int k = 0; k < 3; k++) t[k] = -t[k];
      set_camera(tm, sh, s ? NK - 1 : l, R, t, cq);
    }
  }
  for (int i = l; i < NK - 1; i++) {
    if (i > l && !chain_step(tm, in, sh, i, i - 1)) return false;
    tri_two(tm, in, sh, i, NK - 1);
  }
  for (int i = l + 1; i < NK - 1; i++) tri_two(tm, in, sh, l, i);
  for (int i = l - 1; i >= 0; i--) {
    if (!chain_step(tm, in, sh, i, i + 1)) return false;
    tri_two(tm, in, sh, i, l);
  }
  for (int j = tm.tid(); j < in.nf; j += Team::NT) {
    if (sh.state[j] || in.nobs[j] < 2) continue;
    const int f0 = in.start[j], f1 = f0 + in.nobs[j] - 1;
    const double *a = obs_of(in, j, f0), *b = obs_of(in, j, f1);
    triangulate_point(sh.Pose + 12 * f0, sh.Pose + 12 * f1, a[0], a[1], b[0], b[1], sh.X + 3 * j);
    sh.state[j] = 1;
  }
  tm.sync();
  return true;
}

}  // namespace sfm
}  // namespace avm
