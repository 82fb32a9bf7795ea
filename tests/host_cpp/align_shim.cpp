// Test hooks around avm_host::Estimator::visualInitialAlign (include/avm_host.hpp): pytest fills all_image_frame, Headers and the
// window members from one window of an avm_align_batch / avm_window_batch, runs the marshalling or the call, and reads the members
// back.  Test infrastructure only - the product is the header.  Compiled by the test modules themselves into a temporary directory.
#include <cstring>
#include <string>

#include "avm_host.hpp"

using namespace avm_host;

namespace {
thread_local std::string g_err;

struct Host {
  Context ctx;
  Estimator est;
  explicit Host(int device) : ctx(device, 1, 1), est(ctx) {}
};

template <class F>
int guarded(F f) {
  try {
    f();
    return 0;
  } catch (const Error& e) {
    g_err = e.what();
    return e.status;
  } catch (const std::exception& e) {
    g_err = e.what();
    return -100;
  }
}
Vector3d v3(const double* p) { return Vector3d{p[0], p[1], p[2]}; }
}  // namespace

extern "C" {

const char* as_last_error() { return g_err.c_str(); }
void* as_create(int device) { return new Host(device); }
void as_destroy(void* h) { delete static_cast<Host*>(h); }
double as_stamp(int k) { return 100.0 + 0.05 * k; }  // the stamp the shim gives frame k of all_image_frame

// window w of the two batches into the Estimator's members; drop_header >= 0: Headers[drop_header] gets a stamp no frame has
int as_load(void* hp, const avm_align_batch* a, const avm_window_batch* b, int w, int drop_header) {
  Host& H = *static_cast<Host*>(hp);
  return guarded([&] {
    Estimator& E = H.est;
    E.clearState();
    const int MF = a->max_frames, F = a->n_frames[w];
    const size_t S = a->max_samp;
    E.tic[0] = v3(a->tic + (size_t)w * 3);
    for (int k = 0; k < F; k++) {
      ImageFrame f;
      std::copy(a->frame_R + ((size_t)w * MF + k) * 9, a->frame_R + ((size_t)w * MF + k) * 9 + 9, f.R.begin());
      f.T = v3(a->frame_T + ((size_t)w * MF + k) * 3);
      if (k > 0) {
        const size_t iv = (size_t)w * (MF - 1) + (k - 1), row0 = iv * (S + 1);
        IntegrationBase p(v3(a->imu_acc + row0 * 3), v3(a->imu_gyr + row0 * 3), v3(a->imu_lin_ba + iv * 3), v3(a->imu_lin_bg + iv * 3));
        for (int s = 0; s < a->imu_n[iv]; s++) p.push_back(a->imu_dt[iv * S + s], v3(a->imu_acc + (row0 + s + 1) * 3), v3(a->imu_gyr + (row0 + s + 1) * 3));
        f.pre_integration = p;
      }
      E.all_image_frame[as_stamp(k)] = f;
    }
    for (int i = 0; i < AVM_NFRAMES; i++) E.Headers[i] = i == drop_header ? 1.0 : as_stamp(a->key_index[(size_t)w * AVM_NFRAMES + i]);
    if (!b) return;
    const double* pose = b->pose + (size_t)w * 77;
    const double* sb = b->speedbias + (size_t)w * 99;
    for (int i = 0; i < AVM_NFRAMES; i++) {
      E.Ps[i] = v3(pose + 7 * i);
      E.Rs[i] = Quaterniond{pose[7 * i + 3], pose[7 * i + 4], pose[7 * i + 5], pose[7 * i + 6]};
      E.Vs[i] = v3(sb + 9 * i), E.Bas[i] = v3(sb + 9 * i + 3), E.Bgs[i] = v3(sb + 9 * i + 6);
    }
    const double* ex = b->ex_pose + (size_t)w * 7;
    E.ric[0] = Quaterniond{ex[3], ex[4], ex[5], ex[6]};
    for (int e = 0; e < b->n_feat[w]; e++) {
      const size_t fe = (size_t)w * b->max_feat + e;
      FeaturePerId f(e, b->feat_start[fe]);
      f.estimated_depth = 1.0 / b->inv_depth[fe];
      for (int t = 0; t < b->feat_nobs[fe]; t++) {
        const double* o = b->obs_xy + ((size_t)w * b->max_obs + b->feat_obs_begin[fe] + t) * 2;
        FeaturePerFrame pf;
        pf.point = {o[0], o[1], 1.0};
        f.feature_per_frame.push_back(pf);
      }
      E.f_manager.feature.push_back(f);
    }
    const size_t WS = b->max_samp;
    for (int j = 0; j < AVM_WINDOW_SIZE; j++) {
      const size_t iv = (size_t)w * AVM_WINDOW_SIZE + j, row0 = iv * (WS + 1);
      IntegrationBase p(v3(b->imu_acc + row0 * 3), v3(b->imu_gyr + row0 * 3), v3(b->imu_lin_ba + iv * 3), v3(b->imu_lin_bg + iv * 3));
      for (int s = 0; s < b->imu_n[iv]; s++) p.push_back(b->imu_dt[iv * WS + s], v3(b->imu_acc + (row0 + s + 1) * 3), v3(b->imu_gyr + (row0 + s + 1) * 3));
      E.pre_integrations[j + 1] = p;
    }
  });
}

// Estimator::marshalAlign into the caller's one-window tables, which have the strides dims[0] = max_frames, dims[1] = max_samp;
// dims[2] receives n_frames
int as_marshal(void* hp, int32_t* dims, double* frame_R, double* frame_T, double* tic, int32_t* imu_n, double* imu_dt, double* imu_acc,
               double* imu_gyr, double* imu_lin_ba, double* imu_lin_bg, int32_t* key_index) {
  Host& H = *static_cast<Host*>(hp);
  return guarded([&] {
    AlignTables t;
    H.est.marshalAlign(t);
    const int MF = dims[0], MS = dims[1], F = t.n_frames, S = t.max_samp;
    if (F > MF || S > MS) throw Error(AVM_ERR_CAPACITY, "the caller's strides are too small");
    dims[2] = F;
    std::copy(t.frame_R.begin(), t.frame_R.end(), frame_R);
    std::copy(t.frame_T.begin(), t.frame_T.end(), frame_T);
    std::copy(t.tic.begin(), t.tic.end(), tic);
    std::copy(t.key_index.begin(), t.key_index.end(), key_index);
    for (int j = 0; j < F - 1; j++) {
      imu_n[j] = t.imu_n[j];
      for (int s = 0; s < S; s++) imu_dt[(size_t)j * MS + s] = t.imu_dt[(size_t)j * S + s];
      for (int s = 0; s < (S + 1) * 3; s++)
        imu_acc[(size_t)j * (MS + 1) * 3 + s] = t.imu_acc[(size_t)j * (S + 1) * 3 + s], imu_gyr[(size_t)j * (MS + 1) * 3 + s] = t.imu_gyr[(size_t)j * (S + 1) * 3 + s];
      for (int c = 0; c < 3; c++) imu_lin_ba[j * 3 + c] = t.imu_lin_ba[j * 3 + c], imu_lin_bg[j * 3 + c] = t.imu_lin_bg[j * 3 + c];
    }
  });
}

// bool Estimator::visualInitialAlign(); *result receives it
int as_align(void* hp, int32_t* result) {
  Host& H = *static_cast<Host*>(hp);
  return guarded([&] { *result = H.est.visualInitialAlign() ? 1 : 0; });
}

// the members the call leaves: pose [11][7], speedbias [11][9], inverse depths of the features of the problem in list order [n],
// g [3], delta_bg [3], x [3 F + 1], the linearization biases of pre_integrations[1..10] [10][6] (ba | bg) and of
// all_image_frame's [F - 1][6], is_key_frame [F]; returns solver_flag (0 INITIAL, 1 NON_LINEAR)
int as_state(void* hp, double* pose, double* speedbias, double* inv_depth, double* g, double* delta_bg, double* x, double* lin, double* lin_all,
             int32_t* is_key) {
  Host& H = *static_cast<Host*>(hp);
  Estimator& E = H.est;
  for (int i = 0; i < AVM_NFRAMES; i++) {
    const double p[7] = {E.Ps[i][0], E.Ps[i][1], E.Ps[i][2], E.Rs[i].x, E.Rs[i].y, E.Rs[i].z, E.Rs[i].w};
    std::copy(p, p + 7, pose + 7 * i);
    for (int k = 0; k < 3; k++) speedbias[9 * i + k] = E.Vs[i][k], speedbias[9 * i + 3 + k] = E.Bas[i][k], speedbias[9 * i + 6 + k] = E.Bgs[i][k];
  }
  int n = 0;
  for (auto& f : E.f_manager.feature)
    if (in_problem(f)) inv_depth[n++] = 1.0 / f.estimated_depth;
  for (int k = 0; k < 3; k++) g[k] = E.g[k], delta_bg[k] = E.align_delta_bg[k];
  std::copy(E.align_x.begin(), E.align_x.end(), x);
  for (int j = 0; j < AVM_WINDOW_SIZE; j++)
    for (int k = 0; k < 3; k++) lin[6 * j + k] = E.pre_integrations[j + 1].linearized_ba[k], lin[6 * j + 3 + k] = E.pre_integrations[j + 1].linearized_bg[k];
  int k = 0;
  for (auto it = E.all_image_frame.begin(); it != E.all_image_frame.end(); ++it, ++k) {
    is_key[k] = it->second.is_key_frame ? 1 : 0;
    if (k == 0) continue;
    for (int c = 0; c < 3; c++)
      lin_all[6 * (k - 1) + c] = it->second.pre_integration.linearized_ba[c], lin_all[6 * (k - 1) + 3 + c] = it->second.pre_integration.linearized_bg[c];
  }
  return E.solver_flag == Estimator::NON_LINEAR ? 1 : 0;
}
}
