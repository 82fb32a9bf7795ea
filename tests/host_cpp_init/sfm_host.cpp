// TEST INFRASTRUCTURE.  The text of csrc/sfm/*.hpp compiled for the host with a team of ONE thread: the same chain, PnP, BA and
// frame PnP as the device kernels, minus what only a device has (the wave reductions, the MFMA product: written out here).  It lets the
// CPU tier check the algorithm's text against the statement's fixture; it is no fallback and the package never loads it.
//   g++ -std=c++17 -O2 -shared -fPIC -DSFM_HD=inline sfm_host.cpp -o libsfm_host.so
#include <cstring>
#include <memory>
#include <vector>

#include "../../anticipated-vins-mono_amd/csrc/sfm/frame_pnp.hpp"
#include "../../anticipated-vins-mono_amd/csrc/sfm/rules.hpp"

using namespace avm;
using namespace avm::sfm;

namespace {
struct HostTeam {
  static constexpr int NT = 1;
  std::vector<double> acc = std::vector<double>(64 * 64);
  int tid() const { return 0; }
  void sync() {}
  template <int N>
  void sum(double*) {}
  double max1(double v) { return v; }
  void schur_zero() { std::fill(acc.begin(), acc.end(), 0.0); }
  void schur_chunk(const double* Y, const double* W) {
    for (int i = 0; i < 64; i++)
      for (int j = 0; j < 64; j++)
        for (int k = 0; k < 3 * CHUNK; k++) acc[i * 64 + j] += Y[i * LDW + k] * W[j * LDW + k];
  }
  void schur_store(double* S) {
    for (int i = 0; i < 64; i++)
      for (int j = 0; j < 64; j++) S[i * LDS_S + j] -= acc[i * 64 + j];
  }
};
}  // namespace

// the table check and one stream after the other, with the commit rules of avm_init.h; returns 0, or 8 * stream + rule of a refused batch
extern "C" int sfm_host_run(const avm_sfm_batch* s, const avm_window_batch* w, const int32_t* feat_id, avm_sfm_out* out) {
  for (int b = 0; b < s->n_windows; b++)
    if (const int rule = check_sfm_tables(*s, b)) return 8 * b + rule;
  auto sh = std::make_unique<ChainLds>();
  const size_t MF = s->max_frames, MFE = w->max_feat;
  std::vector<int> jidx(s->max_pts + 1);
  for (int b = 0; b < s->n_windows; b++) {
    StreamIn in;
    in.l = s->l[b], in.nf = w->n_feat[b], in.n_frames = s->n_frames[b], in.max_it = s->ba_max_num_iterations, in.max_pts = s->max_pts;
    in.start = w->feat_start + b * MFE, in.nobs = w->feat_nobs + b * MFE, in.obeg = w->feat_obs_begin + b * MFE;
    in.obs = w->obs_xy + (size_t)b * w->max_obs * 2;
    in.key = s->key_index + b * NK, in.frame_n_pts = s->frame_n_pts + b * MF;
    in.frame_pt_id = s->frame_pt_id + b * MF * s->max_pts, in.frame_pt_xy = s->frame_pt_xy + b * MF * s->max_pts * 2;
    in.feat_id = feat_id + b * MFE;
    in.relR = s->relative_R + b * 9, in.relT = s->relative_T + b * 3, in.ex_pose = w->ex_pose + b * 7;
    HostTeam tm;
    bool finite = true;
    for (int i = 0; i < 9; i++) finite = finite && fin(in.relR[i]);
    for (int i = 0; i < 3; i++) finite = finite && fin(in.relT[i]);
    if (!finite) {
      out->ok[b] = 4;
      continue;
    }
    if (!run_chain(tm, in, *sh)) {
      out->ok[b] = 1;
      continue;
    }
    if (out->pnp_q) std::memcpy(out->pnp_q + b * NK * 4, sh->cq, sizeof(double) * NK * 4);
    if (out->pnp_t) std::memcpy(out->pnp_t + b * NK * 3, sh->ct, sizeof(double) * NK * 3);
    const BaSummary su = bundle_adjust(tm, in, *sh);
    out->ba_cost[2 * b] = su.initial_cost, out->ba_cost[2 * b + 1] = su.final_cost;
    out->ba_counts[3 * b] = su.iterations, out->ba_counts[3 * b + 1] = su.successful, out->ba_counts[3 * b + 2] = su.termination;
    if (!(su.termination >= TERM_GRADIENT && su.termination <= TERM_MIN_RADIUS) && !(5e-3 > su.final_cost)) {
      out->ok[b] = 2;
      continue;
    }
    std::vector<double> q(NK * 4), T(NK * 3), FR(in.n_frames * 9), FT(in.n_frames * 3), point(in.nf * 3 + 3);
    std::vector<int32_t> state(in.nf + 1);
    for (int i = 0; i < NK; i++) {
      key_frame_pose(sh->cq + 4 * i, sh->ct + 3 * i, in.ex_pose, &q[4 * i], &T[3 * i], &FR[9 * in.key[i]]);
      for (int c = 0; c < 3; c++) FT[3 * in.key[i] + c] = T[3 * i + c];
    }
    for (int j = 0; j < in.nf; j++) {
      state[j] = sh->state[j];
      for (int c = 0; c < 3; c++) point[3 * j + c] = sh->state[j] ? sh->X[3 * j + c] : 0.0;
    }
    int ok = 0;
    for (int k = 0, i = 0; k < in.n_frames; k++) {
      if (i < NK && in.key[i] == k) {
        i++;
        continue;
      }
      if (frame_pnp(tm, in, k, i, jidx.data(), q.data(), T.data(), point.data(), state.data(), &FR[9 * k], &FT[3 * k])) ok = 3;
    }
    if (ok == 0) {
      for (double v : FR) ok = fin(v) ? ok : 4;
      for (double v : FT) ok = fin(v) ? ok : 4;
    }
    out->ok[b] = ok;
    if (ok == 0 || ok == 3) {
      std::memcpy(out->q + b * NK * 4, q.data(), sizeof(double) * NK * 4);
      std::memcpy(out->T + b * NK * 3, T.data(), sizeof(double) * NK * 3);
      std::memcpy(out->point + b * MFE * 3, point.data(), sizeof(double) * in.nf * 3);
      std::memcpy(out->point_state + b * MFE, state.data(), sizeof(int32_t) * in.nf);
    }
    if (ok == 0) {
      std::memcpy(out->frame_R + b * MF * 9, FR.data(), sizeof(double) * in.n_frames * 9);
      std::memcpy(out->frame_T + b * MF * 3, FT.data(), sizeof(double) * in.n_frames * 3);
    }
  }
  return 0;
}
