// fsel/aux_kernels.hpp - the horizon from the IMU, the depth cloud, findNNDepth as a parity surface; fsel_kd_doubles, fsel_horizon_supported
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

// ---- B4: HorizonGenerator::imu (utility/horizon_generator.cpp:25-69), one thread per frame ------------------------
__global__ __launch_bounds__(64) void fsel_horizon_imu_kernel(avm_fsel_horizon_in in, double* hor_pos, double* hor_quat) {
  const int p = blockIdx.x * 64 + threadIdx.x;
  if (p >= in.n_problems) return;
  const int H = in.horizon;
  double* pos = hor_pos + (size_t)p * (H + 1) * 3;
  double* qo = hor_quat + (size_t)p * (H + 1) * 4;
  const v3 gravity = mk3(0, 0, -9.80665);  // state_defs.h:37-41
  const v3 Ba = mk3(in.k_ba[3 * p], in.k_ba[3 * p + 1], in.k_ba[3 * p + 2]);
  const v3 a = mk3(in.acc[3 * p], in.acc[3 * p + 1], in.acc[3 * p + 2]), w = mk3(in.gyr[3 * p], in.gyr[3 * p + 1], in.gyr[3 * p + 2]);
  for (int k = 0; k < 3; k++) pos[k] = in.k_pos[3 * p + k], pos[3 + k] = in.k1_pos[3 * p + k];
  for (int k = 0; k < 4; k++) qo[k] = in.k_quat[4 * p + k], qo[4 + k] = in.k1_quat[4 * p + k];
  const double dI = in.delta_imu[p];
  const int nr = in.nr_imu[p];
  const quat Qimu = deltaQ(dI * w);  // unnormalized, and the attitude is never renormalized in the loop
  v3 pp = mk3(in.k1_pos[3 * p], in.k1_pos[3 * p + 1], in.k1_pos[3 * p + 2]), vv = mk3(in.k1_vel[3 * p], in.k1_vel[3 * p + 1], in.k1_vel[3 * p + 2]);
  quat q{in.k1_quat[4 * p + 3], in.k1_quat[4 * p], in.k1_quat[4 * p + 1], in.k1_quat[4 * p + 2]};
  for (int h = 2; h <= H; h++) {
    for (int i = 0; i < nr; i++) {
      q = qmul(q, Qimu);
      const v3 qa = qrot(q, a - Ba);
      vv = vv + dI * (gravity + qa);
      pp = pp + dI * vv + dI * (dI * (0.5 * gravity)) + dI * (dI * (0.5 * qa));
    }
    pos[3 * h] = pp.x, pos[3 * h + 1] = pp.y, pos[3 * h + 2] = pp.z;
    qo[4 * h] = q.x, qo[4 * h + 1] = q.y, qo[4 * h + 2] = q.z, qo[4 * h + 3] = q.w;
  }
}

hipError_t launch_fsel_horizon_imu(const avm_fsel_horizon_in& in, double* hor_pos, double* hor_quat, hipStream_t stream) {
  if (in.n_problems == 0) return hipSuccess;
  hipLaunchKernelGGL(fsel_horizon_imu_kernel, dim3((in.n_problems + 63) / 64), dim3(64), 0, stream, in, hor_pos, hor_quat);
  return hipGetLastError();
}

// ---- B8 (first half): the depth cloud of initKDTree() (feature_selector.cpp:396-419), one thread per window ---------
__global__ __launch_bounds__(64) void fsel_build_cloud_kernel(avm_window_batch B, const double* k1_pos, const double* k1_quat, int max_cloud,
                                                              int32_t* n_cloud, double* cloud_xy, double* cloud_depth) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= B.n_windows) return;
  const double* ex = B.ex_pose + (size_t)w * 7;
  const v3 tic = mk3(ex[0], ex[1], ex[2]);
  const quat qic{ex[6], ex[3], ex[4], ex[5]};
  double ric[9];
  q2R(qic, ric);
  const quat qk1{k1_quat[4 * w + 3], k1_quat[4 * w], k1_quat[4 * w + 1], k1_quat[4 * w + 2]};
  const v3 pk1 = mk3(k1_pos[3 * w], k1_pos[3 * w + 1], k1_pos[3 * w + 2]);
  const double* pose = B.pose + (size_t)w * NFR * 7;
  double* xy = cloud_xy + (size_t)w * max_cloud * 2;
  double* dep = cloud_depth + (size_t)w * max_cloud;
  int n = 0;
  for (int e = 0; e < B.n_feat[w] && n < max_cloud; e++) {
    const int f = B.feat_start[(size_t)w * B.max_feat + e];
    if (f > (NFR - 1) * 3.0 / 4.0) continue;
    const double est_depth = 1.0 / B.inv_depth[(size_t)w * B.max_feat + e];
    if (!(est_depth >= 0)) continue;
    double Rs[9];
    q2R(quat{pose[f * 7 + 6], pose[f * 7 + 3], pose[f * 7 + 4], pose[f * 7 + 5]}, Rs);
    const double* o = B.obs_xy + ((size_t)w * B.max_obs + B.feat_obs_begin[(size_t)w * B.max_feat + e]) * 2;
    const v3 pts_i = est_depth * mk3(o[0], o[1], 1.0);
    const v3 w_pts = Rmul(Rs, Rmul(ric, pts_i) + tic) + mk3(pose[f * 7], pose[f * 7 + 1], pose[f * 7 + 2]);
    const v3 p_IL = qrot(qinv(qk1), w_pts - pk1);
    const v3 p_CL = qrot(qinv(qic), p_IL - tic);
    xy[2 * n] = p_CL.x / p_CL.z, xy[2 * n + 1] = p_CL.y / p_CL.z, dep[n] = est_depth;
    n++;
  }
  n_cloud[w] = n;
}

// B8, second half as a parity surface: findNNDepth of every candidate, one wavefront per (frame, candidate) - the search the setup
// kernel runs inside calcInfoFromFeatures - in all three of its forms: by a whole wavefront, by a 16-lane row (the candidates' slices:
// feature_front4) and by one thread (the used features: feature_delta).  They must agree bit for bit; a disagreement is reported as NaN.
__global__ __launch_bounds__(256) void fsel_nn_depth_kernel(avm_fsel_batch b, const double* kd, double* depth_out) {
  const int p = blockIdx.y, cnd = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (cnd >= b.n_cand[p]) return;  // (wave-uniform)
  const double* xy = b.cand_xy + ((size_t)p * b.max_cand + cnd) * 2;
  const double d = kd_depth<64>(b, kd, p, xy[0], xy[1]);
  const double d16 = kd_depth<16>(b, kd, p, xy[0], xy[1]), d1 = kd_depth<1>(b, kd, p, xy[0], xy[1]);
  const bool same = __double_as_longlong(d16) == __double_as_longlong(d) && __double_as_longlong(d1) == __double_as_longlong(d);
  if ((threadIdx.x & 63) == 0) depth_out[(size_t)p * b.max_cand + cnd] = __all(same) ? d : __longlong_as_double(0x7ff8000000000000ll);
}

hipError_t launch_fsel_nn_depth(const avm_fsel_batch& b, double* kd, double* depth_out, hipStream_t stream) {
  if (b.n_problems == 0 || b.max_cand == 0) return hipSuccess;
  FselDev d{};
  d.b = b, d.kd = kd, d.vflag = nullptr;
  hipError_t e = launch_fsel_kdtree(d, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(fsel_nn_depth_kernel, dim3((b.max_cand + 3) / 4, b.n_problems), dim3(256), 0, stream, b, kd, depth_out);
  return hipGetLastError();
}
size_t fsel_kd_doubles(const avm_fsel_batch& b) { return (size_t)b.n_problems * kd_stride(b.max_cloud > 0 ? b.max_cloud : 0) + 8; }

hipError_t launch_fsel_build_cloud(const avm_window_batch& b, const double* k1_pos, const double* k1_quat, int max_cloud, int32_t* n_cloud,
                                   double* cloud_xy, double* cloud_depth, hipStream_t stream) {
  if (b.n_windows == 0) return hipSuccess;
  hipLaunchKernelGGL(fsel_build_cloud_kernel, dim3((b.n_windows + 63) / 64), dim3(64), 0, stream, b, k1_pos, k1_quat, max_cloud, n_cloud, cloud_xy,
                     cloud_depth);
  return hipGetLastError();
}

bool fsel_horizon_supported(int H) { return H == 2 || H == 3 || H == 5 || H == 10 || H == FS_MAX_H; }
