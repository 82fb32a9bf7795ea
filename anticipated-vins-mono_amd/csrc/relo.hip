// relo.hip — relocalization in the stream loop, on device-resident tables (include/avm.h, "relocalization and the prior hand-over in the
// stream loop"): the frame stamps beside the batch (Headers[i].stamp of slideWindow and processImage, estimator.cpp:126,1015,1021,1064),
// Estimator::setReloFrame (:1109-1127), the match loop of optimization() on the solve's view (:765-790) and the outputs of
// double2vector() (:588-604).  One 256-thread workgroup per window in the kernels that walk a list, one thread per window in the others;
// every call has a check kernel that runs first, on its own, and writes nothing but the verdict (kernels.hpp).
#include "devmath.hpp"
#include "kernels.hpp"
#include "track_prims.hpp"

namespace avm {
namespace {

typedef double d2 __attribute__((ext_vector_type(2)));  // one match_xy row
static_assert(AVM_MAX_FEAT <= 64 * TRK_MAX_CHUNKS, "block_compact's chunk totals hold the view's rows");

// ---- avm_headers_step_batch ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void headers_step_check_kernel(int n_windows, const int32_t* flags, int* first_bad) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= n_windows) return;
  if (flags[w] != AVM_MARGIN_OLD && flags[w] != AVM_MARGIN_SECOND_NEW) report(first_bad, w, HDR_BAD_FLAG);
}

__global__ __launch_bounds__(64) void headers_step_kernel(int n_windows, double* stamp, const int32_t* flags, const double* new_stamp) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= n_windows) return;
  double* s = stamp + (size_t)w * AVM_NFRAMES;
  if (flags) {
    if (flags[w] == AVM_MARGIN_OLD) {
      for (int i = 0; i < AVM_WINDOW_SIZE; i++) s[i] = s[i + 1];
      s[AVM_WINDOW_SIZE] = s[AVM_WINDOW_SIZE - 1];
    } else {
      s[AVM_WINDOW_SIZE - 1] = s[AVM_WINDOW_SIZE];
    }
  }
  if (new_stamp) s[AVM_WINDOW_SIZE] = new_stamp[w];
}

// ---- avm_set_relo_frame_batch -----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRK_NT) void set_relo_frame_check_kernel(avm_relo_msg_batch M, int* first_bad) {
  __shared__ int s_bad;
  const int w = blockIdx.x, tid = threadIdx.x;
  if (M.has_msg[w] == 0) return;  // (uniform over the workgroup, like every early return below)
  const int nm = M.n_match[w];
  if (nm < 0 || nm > M.max_match) {
    if (tid == 0) report(first_bad, w, SETRELO_BAD_NMATCH);
    return;
  }
  if (tid == 0) s_bad = 0;
  __syncthreads();
  const int32_t* ids = M.match_id + (size_t)w * M.max_match;
  bool bad = false;
  for (int i = tid + 1; i < nm; i += TRK_NT) bad = bad || ids[i] <= ids[i - 1];
  if (bad) s_bad = 1;
  __syncthreads();
  if (tid == 0 && s_bad) report(first_bad, w, SETRELO_BAD_IDS);
}

__global__ __launch_bounds__(TRK_NT) void set_relo_frame_kernel(avm_window_batch B, const double* stamp, avm_relo_msg_batch M, avm_relo_state S) {
  const int w = blockIdx.x, tid = threadIdx.x;
  if (M.has_msg[w] == 0) return;
  const int nm = M.n_match[w];
  const size_t mi = (size_t)w * M.max_match, si = (size_t)w * S.max_match;
  for (int i = tid; i < nm; i += TRK_NT) {
    S.match_id[si + i] = M.match_id[mi + i];
    *reinterpret_cast<d2*>(S.match_xy + 2 * (si + i)) = *reinterpret_cast<const d2*>(M.match_xy + 2 * (mi + i));
  }
  if (tid != 0) return;
  const double fs = M.frame_stamp[w];
  S.relo_stamp[w] = fs, S.n_match[w] = nm;
  for (int j = 0; j < 3; j++) S.prev_relo_t[(size_t)w * 3 + j] = M.prev_relo_t[(size_t)w * 3 + j];
  for (int j = 0; j < 4; j++) S.prev_relo_q[(size_t)w * 4 + j] = M.prev_relo_q[(size_t)w * 4 + j];
  for (int i = 0; i < AVM_WINDOW_SIZE; i++)  // (no break: the last frame with this stamp wins)
    if (fs == stamp[(size_t)w * AVM_NFRAMES + i]) {
      S.relo_frame[w] = i, S.relocalization_info[w] = 1;
      for (int j = 0; j < AVM_SIZE_POSE; j++) S.relo_pose[(size_t)w * AVM_SIZE_POSE + j] = B.pose[((size_t)w * AVM_NFRAMES + i) * AVM_SIZE_POSE + j];
    }
}

// ---- avm_relo_resolve_batch -------------------------------------------------------------------------------------------------------------
// view.n_feat is inside [0, view.max_feat] and view.max_feat <= AVM_MAX_FEAT, state.max_match <= AVM_MAX_IMAGE_PTS (the host has checked)
__global__ __launch_bounds__(TRK_NT) void relo_resolve_check_kernel(ReloResolveArgs a, int* first_bad) {
  __shared__ int s_bad;
  const int w = blockIdx.x, tid = threadIdx.x;
  const int nv = a.view.n_feat[w], F = a.full_max_feat;
  if (tid == 0) s_bad = 1 << 30;
  __syncthreads();
  const int32_t* row = a.view_row + (size_t)w * a.view.max_feat;
  const int32_t* fid = a.feat_id + (size_t)w * F;
  const bool active = a.state.relocalization_info[w] != 0;
  int bad = 1 << 30;
  for (int k = tid; k < nv; k += TRK_NT) {
    const int r = row[k], p = k > 0 ? row[k - 1] : -1;
    if (r < 0 || r >= F || r <= p) bad = min(bad, (int)RESOLVE_BAD_ROW);
    else if (active && p >= 0 && fid[r] <= fid[p]) bad = min(bad, (int)RESOLVE_BAD_VIEW_IDS);  // (p < r < F: both inside the table)
  }
  if (active) {
    const int rf = a.state.relo_frame[w], nm = a.state.n_match[w];
    if (rf < 0 || rf >= AVM_WINDOW_SIZE) bad = min(bad, (int)RESOLVE_BAD_FRAME);
    if (nm < 0 || nm > a.state.max_match) bad = min(bad, (int)RESOLVE_BAD_NMATCH);
    else {
      const int32_t* mid = a.state.match_id + (size_t)w * a.state.max_match;
      for (int i = tid + 1; i < nm; i += TRK_NT)
        if (mid[i] <= mid[i - 1]) bad = min(bad, (int)RESOLVE_BAD_MATCH_IDS);
    }
  }
  if (bad != 1 << 30) atomicMin(&s_bad, bad);
  __syncthreads();
  if (tid == 0 && s_bad != 1 << 30) report(first_bad, w, s_bad);
}

// Both id lists ascend (checked), so the reference's two-pointer walk emits exactly the eligible rows whose id is among the matches, in
// row order: every row looks its id up, the ballot ranks the hits.
__global__ __launch_bounds__(TRK_NT) void relo_resolve_kernel(ReloResolveArgs a) {
  __shared__ int s_mid[AVM_MAX_IMAGE_PTS], s_vid[AVM_MAX_FEAT], s_tot[TRK_MAX_CHUNKS];
  const int w = blockIdx.x, tid = threadIdx.x;
  if (a.state.relocalization_info[w] == 0) {  // (uniform)
    if (tid == 0) a.relo_n[w] = 0, a.relo_frame[w] = 0;
    return;
  }
  const int nv = a.view.n_feat[w], nm = a.state.n_match[w], rf = a.state.relo_frame[w];
  const int32_t* row = a.view_row + (size_t)w * a.view.max_feat;
  const int32_t* fid = a.feat_id + (size_t)w * a.full_max_feat;
  const int32_t* start = a.view.feat_start + (size_t)w * a.view.max_feat;
  const int32_t* mid = a.state.match_id + (size_t)w * a.state.max_match;
  const double* mxy = a.state.match_xy + (size_t)w * a.state.max_match * 2;
  int32_t* feat = a.relo_feat + (size_t)w * a.view.max_feat;
  double* xy = a.relo_xy + (size_t)w * a.view.max_feat * 2;
  for (int i = tid; i < nm; i += TRK_NT) s_mid[i] = mid[i];
  for (int k = tid; k < nv; k += TRK_NT) s_vid[k] = fid[row[k]];
  __syncthreads();
  const int n = block_compact(nv, s_tot, [&](int k) { return start[k] <= rf && find_id(s_mid, nm, s_vid[k]) >= 0; },
                              [&](int k, int rank) {
                                feat[rank] = k;
                                *reinterpret_cast<d2*>(xy + 2 * (size_t)rank) = *reinterpret_cast<const d2*>(mxy + 2 * (size_t)find_id(s_mid, nm, s_vid[k]));
                              });
  if (tid != 0) return;
  a.relo_n[w] = n, a.relo_frame[w] = rf;
  atomicAdd(a.n_active, 1);
}

// ---- avm_relo_finish_batch --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void relo_finish_check_kernel(int n_windows, avm_relo_state S, int* first_bad) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= n_windows || S.relocalization_info[w] == 0) return;
  if (S.relo_frame[w] < 0 || S.relo_frame[w] >= AVM_WINDOW_SIZE) report(first_bad, w, FINISH_BAD_FRAME);
}

AVM_DEV double yaw_deg(const double* R) { return atan2(R[3], R[0]) / M_PI * 180.0; }  // Utility::R2ypr(R).x(), utility.h:73,80
AVM_DEV double normalize_angle(double a) {                                             // Utility::normalizeAngle, utility.h:130-139
  const double two_pi = 2.0 * 180;
  return a > 0 ? a - two_pi * floor((a + 180.0) / two_pi) : a + two_pi * floor((-a + 180.0) / two_pi);
}

__global__ __launch_bounds__(64) void relo_finish_kernel(avm_window_batch B, avm_relo_state S) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= B.n_windows || S.relocalization_info[w] == 0) return;
  const double* rp = S.relo_pose + (size_t)w * AVM_SIZE_POSE;
  const double* fp = B.pose + ((size_t)w * AVM_NFRAMES + S.relo_frame[w]) * AVM_SIZE_POSE;
  const double* pt = S.prev_relo_t + (size_t)w * 3;
  const double* pq = S.prev_relo_q + (size_t)w * 4;
  double relo_r[9], Rs[9], prev_r[9], rel[9];
  q2R(qnormalized(quat{rp[6], rp[3], rp[4], rp[5]}), relo_r);
  q2R(qnormalized(quat{fp[6], fp[3], fp[4], fp[5]}), Rs);
  q2R(quat{pq[3], pq[0], pq[1], pq[2]}, prev_r);
  const v3 relo_t = mk3(rp[0], rp[1], rp[2]), Ps = mk3(fp[0], fp[1], fp[2]);
  const double yaw_relo = yaw_deg(relo_r);
  const double dyaw = yaw_deg(prev_r) - yaw_relo;
  const double y = dyaw / 180.0 * M_PI, cy = cos(y), sy = sin(y);  // ypr2R(dyaw, 0, 0) = Rz: the other two factors are the identity
  const double Rz[9] = {cy, -sy, 0, sy, cy, 0, 0, 0, 1};
  const v3 dt = mk3(pt[0], pt[1], pt[2]) - Rmul(Rz, relo_t);
  const v3 rt = RTmul(relo_r, Ps - relo_t);
  double relo_rT[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) relo_rT[i * 3 + j] = relo_r[j * 3 + i];
  mat3mul(relo_rT, Rs, rel);
  const quat rq = R2q(rel);
  S.drift_correct_yaw[w] = dyaw;
  double* o = S.drift_correct_t + (size_t)w * 3;
  o[0] = dt.x, o[1] = dt.y, o[2] = dt.z;
  o = S.relo_relative_t + (size_t)w * 3;
  o[0] = rt.x, o[1] = rt.y, o[2] = rt.z;
  o = S.relo_relative_q + (size_t)w * 4;
  o[0] = rq.x, o[1] = rq.y, o[2] = rq.z, o[3] = rq.w;
  S.relo_relative_yaw[w] = normalize_angle(yaw_deg(Rs) - yaw_relo);
  S.relocalization_info[w] = 0;
}

}  // namespace

hipError_t launch_headers_step_check(int n_windows, const int32_t* flags, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(headers_step_check_kernel, dim3((n_windows + 63) / 64), dim3(64), 0, stream, n_windows, flags, first_bad);
  return hipGetLastError();
}

hipError_t launch_headers_step(int n_windows, double* stamp, const int32_t* flags, const double* new_stamp, hipStream_t stream) {
  hipLaunchKernelGGL(headers_step_kernel, dim3((n_windows + 63) / 64), dim3(64), 0, stream, n_windows, stamp, flags, new_stamp);
  return hipGetLastError();
}

hipError_t launch_set_relo_frame_check(const avm_relo_msg_batch& msg, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(set_relo_frame_check_kernel, dim3(msg.n_windows), dim3(TRK_NT), 0, stream, msg, first_bad);
  return hipGetLastError();
}

hipError_t launch_set_relo_frame(const avm_window_batch& b, const double* stamp, const avm_relo_msg_batch& msg, const avm_relo_state& state,
                                 hipStream_t stream) {
  hipLaunchKernelGGL(set_relo_frame_kernel, dim3(msg.n_windows), dim3(TRK_NT), 0, stream, b, stamp, msg, state);
  return hipGetLastError();
}

hipError_t launch_relo_resolve_check(const ReloResolveArgs& a, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(relo_resolve_check_kernel, dim3(a.view.n_windows), dim3(TRK_NT), 0, stream, a, first_bad);
  return hipGetLastError();
}

hipError_t launch_relo_resolve(const ReloResolveArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(relo_resolve_kernel, dim3(a.view.n_windows), dim3(TRK_NT), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_relo_finish_check(int n_windows, const avm_relo_state& state, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(relo_finish_check_kernel, dim3((n_windows + 63) / 64), dim3(64), 0, stream, n_windows, state, first_bad);
  return hipGetLastError();
}

hipError_t launch_relo_finish(const avm_window_batch& b, const avm_relo_state& state, hipStream_t stream) {
  hipLaunchKernelGGL(relo_finish_kernel, dim3((b.n_windows + 63) / 64), dim3(64), 0, stream, b, state);
  return hipGetLastError();
}

}  // namespace avm
