// global_sfm.hip — the deterministic half of Estimator::initialStructure on gfx950: GlobalSFM::construct (initial/initial_sfm.cpp:117-312)
// and "solve pnp for all frame" (estimator.cpp:277-344), against the statement tests/golden/gen_global_sfm.py.  A list of parts:
//   sfm/math.hpp   the scalar pieces (Rodrigues, the 4 x 4 triangulation, the small Cholesky), host and device
//   sfm/pnp.hpp    cv::solvePnP in the CvLevMarq reading, for a team
//   sfm/chain.hpp  sfm_f, the chain of PnP and triangulateTwoFrames, the workgroup's LDS map
//   sfm/ba.hpp     the full BA in the Ceres reading
//   sfm/frame_pnp.hpp  q, T and the key frames' poses after the BA; the PnP of one non-key frame
//   sfm/team.hpp   the teams: 256-thread workgroup (reductions, the MFMA product of the elimination), one wavefront
//   sfm/rules.hpp  the table check
// Kernels:
//   validate_sfm_kernel    one thread per (stream, frame) and one per stream: the rules of sfm/rules.hpp
//   sfm_chain_ba_kernel    one 256-thread workgroup per stream: chain, BA, q / T, the key frames' frame_R / frame_T
//   sfm_frame_pnp_kernel   one wavefront per (stream, non-key frame)
//   sfm_commit_kernel      one wavefront per stream: folds the frames' outcomes into ok and commits what the contract says is written
// The two middle kernels write stages (SfmArgs) only, apart from pnp_q / pnp_t, ba_counts / ba_cost; the commit decides per stream.
#include "devmath.hpp"
#include "kernels.hpp"
#include "sfm/team.hpp"
#include "sfm/frame_pnp.hpp"

namespace avm {
using namespace sfm;

namespace {
__device__ StreamIn stream_in(const SfmArgs& A, int b) {
  const avm_sfm_batch& s = A.s;
  const avm_window_batch& w = A.w;
  StreamIn in;
  in.l = min(max(s.l[b], 0), 9);
  in.nf = min(max(w.n_feat[b], 0), min(w.max_feat, MAXF));
  in.n_frames = min(max(s.n_frames[b], NK), s.max_frames);
  in.max_it = s.ba_max_num_iterations;
  in.max_pts = s.max_pts;
  in.start = w.feat_start + (size_t)b * w.max_feat, in.nobs = w.feat_nobs + (size_t)b * w.max_feat;
  in.obeg = w.feat_obs_begin + (size_t)b * w.max_feat, in.obs = w.obs_xy + (size_t)b * w.max_obs * 2;
  in.key = s.key_index + (size_t)b * NK;
  in.frame_n_pts = s.frame_n_pts + (size_t)b * s.max_frames;
  in.frame_pt_id = s.frame_pt_id + (size_t)b * s.max_frames * s.max_pts;
  in.frame_pt_xy = s.frame_pt_xy + (size_t)b * s.max_frames * s.max_pts * 2;
  in.feat_id = A.feat_id + (size_t)b * w.max_feat;
  in.relR = s.relative_R + (size_t)b * 9, in.relT = s.relative_T + (size_t)b * 3, in.ex_pose = w.ex_pose + (size_t)b * 7;
  return in;
}
}  // namespace

__global__ __launch_bounds__(64) void validate_sfm_kernel(avm_sfm_batch s, int* first_bad) {
  const long t = (long)blockIdx.x * 64 + threadIdx.x;
  const int units = s.max_frames + 1;
  const int b = (int)(t / units), k = (int)(t % units);
  if (b >= s.n_windows) return;
  const int rule = k == s.max_frames ? check_sfm_stream(s, b) : check_sfm_frame(s, b, k);
  if (rule) atomicMin(first_bad, b * 8 + rule);
}

hipError_t launch_validate_sfm(const avm_sfm_batch& s, int* first_bad, hipStream_t stream) {
  const long n = (long)s.n_windows * (s.max_frames + 1);
  hipLaunchKernelGGL(validate_sfm_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, stream, s, first_bad);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void sfm_chain_ba_kernel(SfmArgs A) {
  extern __shared__ double lds_raw[];
  ChainLds& sh = *reinterpret_cast<ChainLds*>(lds_raw);
  const int b = blockIdx.x, tid = threadIdx.x;
  const StreamIn in = stream_in(A, b);
  Block256 tm;
  tm.red = sh.red;
  bool finite = true;
  for (int i = 0; i < 9; i++) finite = finite && fin(in.relR[i]);
  for (int i = 0; i < 3; i++) finite = finite && fin(in.relT[i]);
  if (!finite) {
    if (tid == 0) A.st[b] = 4;
    return;
  }
  if (!run_chain(tm, in, sh)) {
    if (tid == 0) A.st[b] = 1;
    return;
  }
  if (A.out.pnp_q && tid < NK * 4) A.out.pnp_q[(size_t)b * NK * 4 + tid] = sh.cq[tid];
  if (A.out.pnp_t && tid < NK * 3) A.out.pnp_t[(size_t)b * NK * 3 + tid] = sh.ct[tid];
  const BaSummary su = bundle_adjust(tm, in, sh);
  if (tid == 0) {
    A.out.ba_cost[2 * b] = su.initial_cost, A.out.ba_cost[2 * b + 1] = su.final_cost;
    A.out.ba_counts[3 * b] = su.iterations, A.out.ba_counts[3 * b + 1] = su.successful, A.out.ba_counts[3 * b + 2] = su.termination;
  }
  const bool converged = su.termination >= TERM_GRADIENT && su.termination <= TERM_MIN_RADIUS;
  if (!converged && !(5e-3 > su.final_cost)) {
    if (tid == 0) A.st[b] = 2;
    return;
  }
  // q = bq^-1, T = -(q * bt); the key frames' frame_R = R(q) ric^T, frame_T = T
  if (tid < NK) {
    double q[4], T[3], FR[9];
    key_frame_pose(sh.cq + 4 * tid, sh.ct + 3 * tid, in.ex_pose, q, T, FR);
    const int k = min(max(in.key[tid], 0), A.s.max_frames - 1);
    for (int i = 0; i < 4; i++) A.sq[((size_t)b * NK + tid) * 4 + i] = q[i];
    for (int i = 0; i < 3; i++) A.sT[((size_t)b * NK + tid) * 3 + i] = T[i], A.sfT[((size_t)b * A.s.max_frames + k) * 3 + i] = T[i];
    for (int i = 0; i < 9; i++) A.sR[((size_t)b * A.s.max_frames + k) * 9 + i] = FR[i];
    A.fst[(size_t)b * A.s.max_frames + k] = 0;
  }
  for (int j = tid; j < in.nf; j += 256) {
    for (int c = 0; c < 3; c++) A.spoint[((size_t)b * A.w.max_feat + j) * 3 + c] = sh.state[j] ? sh.X[3 * j + c] : 0.0;
    A.sstate[(size_t)b * A.w.max_feat + j] = sh.state[j];
  }
  if (tid == 0) A.st[b] = 0;
}

__global__ __launch_bounds__(64) void sfm_frame_pnp_kernel(SfmArgs A) {
  __shared__ int jidx[AVM_MAX_IMAGE_PTS];
  const int MF = A.s.max_frames;
  const int b = blockIdx.x / MF, k = blockIdx.x % MF, lane = threadIdx.x;
  if (A.st[b] != 0) return;
  const StreamIn in = stream_in(A, b);
  if (k >= in.n_frames) return;
  int i = 0;  // key frames in front of k; a key frame itself is the chain kernel's
  for (int c = 0; c < NK; c++) {
    if (in.key[c] == k) return;
    i += in.key[c] < k ? 1 : 0;
  }
  Wave64 tm;
  const int st = frame_pnp(tm, in, k, i, jidx, A.sq + (size_t)b * NK * 4, A.sT + (size_t)b * NK * 3, A.spoint + (size_t)b * A.w.max_feat * 3,
                           A.sstate + (size_t)b * A.w.max_feat, A.sR + ((size_t)b * MF + k) * 9, A.sfT + ((size_t)b * MF + k) * 3);
  if (lane == 0) A.fst[(size_t)b * MF + k] = st;
}

__global__ __launch_bounds__(64) void sfm_commit_kernel(SfmArgs A) {
  const int b = blockIdx.x, lane = threadIdx.x, MF = A.s.max_frames;
  int ok = A.st[b];
  const int F = min(max(A.s.n_frames[b], NK), MF), nf = min(max(A.w.n_feat[b], 0), A.w.max_feat);
  if (ok == 0) {
    double bad3 = 0, badf = 0;
    for (int k = lane; k < F; k += 64) bad3 = fmax(bad3, A.fst[(size_t)b * MF + k] == 3 ? 1.0 : 0.0);
    bad3 = wave_max(bad3);
    if (bad3 > 0) {
      ok = 3;
    } else {
      for (int i = lane; i < F * 9; i += 64) badf = fmax(badf, fin(A.sR[(size_t)b * MF * 9 + i]) ? 0.0 : 1.0);
      for (int i = lane; i < F * 3; i += 64) badf = fmax(badf, fin(A.sfT[(size_t)b * MF * 3 + i]) ? 0.0 : 1.0);
      if (wave_max(badf) > 0) ok = 4;
    }
  }
  if (lane == 0) A.out.ok[b] = ok;
  if (ok == 0 || ok == 3) {
    for (int i = lane; i < NK * 4; i += 64) A.out.q[(size_t)b * NK * 4 + i] = A.sq[(size_t)b * NK * 4 + i];
    for (int i = lane; i < NK * 3; i += 64) A.out.T[(size_t)b * NK * 3 + i] = A.sT[(size_t)b * NK * 3 + i];
    for (int i = lane; i < nf * 3; i += 64) A.out.point[(size_t)b * A.w.max_feat * 3 + i] = A.spoint[(size_t)b * A.w.max_feat * 3 + i];
    for (int i = lane; i < nf; i += 64) A.out.point_state[(size_t)b * A.w.max_feat + i] = A.sstate[(size_t)b * A.w.max_feat + i];
  }
  if (ok == 0) {
    for (int i = lane; i < F * 9; i += 64) A.out.frame_R[(size_t)b * MF * 9 + i] = A.sR[(size_t)b * MF * 9 + i];
    for (int i = lane; i < F * 3; i += 64) A.out.frame_T[(size_t)b * MF * 3 + i] = A.sfT[(size_t)b * MF * 3 + i];
  }
}

hipError_t launch_sfm_chain_ba(const SfmArgs& a, hipStream_t stream) {
  return launch_lds<sfm_chain_ba_kernel>(dim3(a.s.n_windows), dim3(256), (int)sizeof(ChainLds), stream, a);
}
hipError_t launch_sfm_frame_pnp(const SfmArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(sfm_frame_pnp_kernel, dim3((unsigned)a.s.n_windows * a.s.max_frames), dim3(64), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_sfm_commit(const SfmArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(sfm_commit_kernel, dim3(a.s.n_windows), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace avm
