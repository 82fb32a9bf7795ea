// sfm/frame_pnp.hpp - what follows the BA: q = bq^-1, T = -(q bt) and the key frames' poses (initial_sfm.cpp:290-304,
// estimator.cpp:290-297), and "solve pnp for all frame" (estimator.cpp:298-344) for one non-key frame and one team.
#pragma once
#include "ba.hpp"

namespace avm {
namespace sfm {

SFM_HD void ric_of(const double* ex_pose, double* ric) {
  const double qic[4] = {ex_pose[6], ex_pose[3], ex_pose[4], ex_pose[5]};
  q2R9(qic, ric);
}

// key frame i after the BA: q [4], T [3], frame_R = R(q) ric^T [9] (frame_T = T)
SFM_HD void key_frame_pose(const double* bq, const double* bt, const double* ex_pose, double* q, double* T, double* FR) {
  double Rq[9], ric[9];
  qinv4(bq, q);
  qrot3(q, bt, T);
  for (int c = 0; c < 3; c++) T[c] = -T[c];
  ric_of(ex_pose, ric);
  q2R9(q, Rq);
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) FR[3 * r + c] = Rq[3 * r] * ric[3 * c] + Rq[3 * r + 1] * ric[3 * c + 1] + Rq[3 * r + 2] * ric[3 * c + 2];
}

// Non-key frame k with i key frames in front of it.  q, T: the stream's [11][4] / [11][3] after the BA; point, pstate: its points and
// their states; jidx: max_pts ints of the team's LDS.  Returns 0 and FR / FT (written by thread 0), or 3: fewer than 6 known points,
// or the PnP fails.
template <class Team>
SFM_HD int frame_pnp(Team& tm, const StreamIn& in, int k, int i, int* jidx, const double* q, const double* T, const double* point,
                     const int32_t* pstate, double* FR, double* FT) {
  const int np = in.frame_n_pts[k] < 0 ? 0 : in.frame_n_pts[k] < in.max_pts ? in.frame_n_pts[k] : in.max_pts;
  const int32_t* ids = in.frame_pt_id + (size_t)k * in.max_pts;
  const double* xy = in.frame_pt_xy + (size_t)k * in.max_pts * 2;
  double cnt = 0;
  for (int n = tm.tid(); n < np; n += Team::NT) {
    int j = -1;
    for (int e = 0; e < in.nf; e++)
      if (in.feat_id[e] == ids[n]) {  // the first row with the id wins
        j = e;
        break;
      }
    if (j >= 0 && !pstate[j]) j = -1;
    jidx[n] = j;
    cnt += j >= 0 ? 1.0 : 0.0;
  }
  tm.sync();
  tm.template sum<1>(&cnt);
  if (cnt < 6) return 3;
  const int g = i < NK - 1 ? i : NK - 1;
  double qg[4], Ri[9], Pi[3], R[9], t[3];
  qinv4(q + 4 * g, qg);
  q2R9(qg, Ri);
  mulv(Ri, T + 3 * g, Pi);
  for (int c = 0; c < 3; c++) Pi[c] = -Pi[c];
  auto pts = [&](int n, double* M, double* m) {
    const int j = jidx[n];
    if (j < 0) return false;
    for (int c = 0; c < 3; c++) M[c] = f32r(point[3 * j + c]);
    m[0] = f32r(xy[2 * n]), m[1] = f32r(xy[2 * n + 1]);
    return true;
  };
  if (!solve_pnp(tm, pts, np, Ri, Pi, R, t)) return 3;
  if (tm.tid() == 0) {  // R_pnp = R^T, frame_R = R_pnp ric^T, frame_T = R_pnp (-t)
    double ric[9];
    ric_of(in.ex_pose, ric);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) FR[3 * r + c] = R[r] * ric[3 * c] + R[3 + r] * ric[3 * c + 1] + R[6 + r] * ric[3 * c + 2];
      FT[r] = R[r] * -t[0] + R[3 + r] * -t[1] + R[6 + r] * -t[2];
    }
  }
  return 0;
}

}  // namespace sfm
}  // namespace avm
