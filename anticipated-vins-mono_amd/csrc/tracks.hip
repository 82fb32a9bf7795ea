// tracks.hip — the feature manager's per-image bookkeeping on device-resident tables (include/avm.h, "the feature manager on
// device-resident tables"): FeatureManager::addFeatureCheckParallax's append by feature id (feature_manager.cpp:45-72), the buffer half of
// Estimator::processIMU (estimator.cpp:92-98), the solve's filtered view of the whole list (estimator.cpp:715) and setDepth's copy back
// (feature_manager.cpp:141-159); and FeatureSelector::select()'s bookkeeping around the selection on the tracker's image
// (feature_selector.cpp:98-120, 156-196, 208-219; select_image.hpp); and the prior a window keeps when its marginalization dropped nothing
// (estimator.cpp:926-927; avm_prior_keep_batch).  Integer bookkeeping and copies only: no floating-point operation in this file.
// One 256-thread workgroup per window in the kernels that walk a list; every call has a check kernel of the same shape that runs first,
// on its own, and writes nothing but the verdict (kernels.hpp), so that a refused batch leaves every table of every window as it was.
#include "devmath.hpp"
#include "kernels.hpp"
#include "select_image.hpp"
#include "track_prims.hpp"  // TRK_NT, block_compact, find_id, report

namespace avm {
namespace {

constexpr int TRK_SLOTS = (AVM_MAX_OBS_WIDE + TRK_NT - 1) / TRK_NT;  // 17 observation slots per thread
static_assert(AVM_MAX_IMAGE_PTS % 64 == 0 && AVM_MAX_FEAT_WIDE <= AVM_MAX_IMAGE_PTS, "chunk totals are sized by the image");

// inclusive prefix sum over the wavefront, every lane active: the shift ladder of wave_sum_shr with each lane keeping its partial sum
AVM_DEV int wave_scan_incl(int v) {
  v += dpp_mov<0x111>(v);       // row_shr:1
  v += dpp_mov<0x112>(v);       // row_shr:2
  v += dpp_mov<0x114>(v);       // row_shr:4
  v += dpp_mov<0x118>(v);       // row_shr:8   -> every lane holds the sum of its row up to itself
  v += dpp_mov<0x142, 0xa>(v);  // row_bcast:15 -> rows 1 and 3 add the row in front of them
  v += dpp_mov<0x143, 0xc>(v);  // row_bcast:31 -> rows 2 and 3 add rows 0 + 1
  return v;
}

// out[i] = in[0] + ... + in[i - 1] for i <= n (out[n]: the total); tot: TRK_MAX_CHUNKS ints of LDS.  Ends with a workgroup barrier.
AVM_DEV void block_scan_excl(const int* in, int* out, int n, int* tot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c * 64 < n; c += TRK_WAVES) {  // (wave-uniform bounds: the DPP ladder runs with every lane active)
    const int i = c * 64 + lane, v = i < n ? in[i] : 0;
    const int s = wave_scan_incl(v);
    if (i < n) out[i] = s - v;
    if (lane == 63) tot[c] = s;
  }
  __syncthreads();
  for (int i = threadIdx.x; i <= n; i += TRK_NT) {
    const int chunks = i < n ? i >> 6 : (n + 63) >> 6;  // the chunks in front of item i; all of them for the total
    int base = 0;
    for (int c = 0; c < chunks; c++) base += tot[c];
    out[i] = (i < n ? out[i] : 0) + base;
  }
  __syncthreads();
}

// the row e < n_rows with begin[e] <= d < begin[e + 1] (begin strictly ascending from 0: every row has an observation)
AVM_DEV int row_of_slot(const int* begin, int n_rows, int d) {
  int lo = 0, hi = n_rows;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (begin[mid] <= d) lo = mid;
    else hi = mid;
  }
  return lo;
}

typedef double d2 __attribute__((ext_vector_type(2)));  // one observation (d4, devmath.hpp: its obs_vel_td row)

// The barrier between "every thread has read its sources" and "the first destination is written" of a move that overlaps itself.  A
// workgroup barrier alone lets a wavefront's global loads still be in flight when another wavefront's stores issue: wait until the values
// are in the registers first (s_waitcnt vmcnt(0), expcnt and lgkmcnt left alone).
AVM_DEV void sources_read_barrier() {
  __builtin_amdgcn_s_waitcnt(0x0F70);
  __syncthreads();
}

// ---- avm_add_image_batch ------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TRK_NT) void add_image_check_kernel(avm_window_batch B, const int32_t* feat_id, avm_image_batch I, int* first_bad) {
  __shared__ int s_id[AVM_MAX_IMAGE_PTS], s_fid[AVM_MAX_FEAT_WIDE], s_bad, s_matched, s_obs;
  const int w = blockIdx.x, tid = threadIdx.x;
  const int np = I.n_pts[w], nf = B.n_feat[w];
  if (np < 0 || np > I.max_pts) {  // (uniform over the workgroup: nothing below indexes with it)
    if (tid == 0) report(first_bad, w, TRK_BAD_NPTS);
    return;
  }
  if (tid == 0) s_bad = 1 << 30, s_matched = 0, s_obs = 0;
  const int32_t* ids = I.feature_id + (size_t)w * I.max_pts;
  const int32_t* fid = feat_id + (size_t)w * B.max_feat;
  const int32_t* fstart = B.feat_start + (size_t)w * B.max_feat;
  const int32_t* fnobs = B.feat_nobs + (size_t)w * B.max_feat;
  int bad = 1 << 30;
  for (int i = tid; i < np; i += TRK_NT) {
    s_id[i] = ids[i];
    if (i > 0 && ids[i] <= ids[i - 1]) bad = min(bad, (int)TRK_BAD_IDS);
  }
  for (int e = tid; e < nf; e += TRK_NT) s_fid[e] = fid[e];
  __syncthreads();
  int matched = 0, obs = 0;
  for (int e = tid; e < nf; e += TRK_NT) {
    const int st = fstart[e], no = fnobs[e], id = s_fid[e];
    obs += no;
    if (st + no > AVM_WINDOW_SIZE) bad = min(bad, (int)TRK_BAD_FULL);
    for (int j = 0; j < e; j++)
      if (s_fid[j] == id) bad = min(bad, (int)TRK_BAD_DUP);
    if (find_id(s_id, np, id) >= 0) {
      matched++;
      if (st + no < AVM_WINDOW_SIZE) bad = min(bad, (int)TRK_BAD_LOST);
    }
  }
  atomicAdd(&s_matched, matched), atomicAdd(&s_obs, obs);
  if (bad != 1 << 30) atomicMin(&s_bad, bad);
  __syncthreads();
  if (tid != 0) return;
  bad = s_bad;
  if (nf + (np - s_matched) > B.max_feat) bad = min(bad, (int)TRK_CAP_FEAT);
  if (s_obs + np > B.max_obs) bad = min(bad, (int)TRK_CAP_OBS);
  if (bad != 1 << 30) report(first_bad, w, bad);
}

// The append and the dense rewrite of one window's observation table.  The move overlaps itself in both directions (rows move left over
// the roll's holes and right past the appended observations), so every source is read into registers before the barrier behind which the
// first destination is written: TRK_SLOTS slots per thread, obs_xy and obs_vel_td each in a pass of their own.
__global__ __launch_bounds__(TRK_NT) void add_image_kernel(avm_window_batch B, int32_t* feat_id, avm_image_batch I) {
  __shared__ int s_id[AVM_MAX_IMAGE_PTS], s_mark[AVM_MAX_IMAGE_PTS];  // the image's ids; 1: the point extended a track of the list
  // per row of the NEW list: the image point it takes (-1: none), its old feat_obs_begin, its new feat_nobs, its new feat_obs_begin
  __shared__ int s_pt[AVM_MAX_FEAT_WIDE], s_ob[AVM_MAX_FEAT_WIDE], s_no[AVM_MAX_FEAT_WIDE], s_begin[AVM_MAX_FEAT_WIDE + 1];
  __shared__ int s_tot[TRK_MAX_CHUNKS];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int np = I.n_pts[w], nf = B.n_feat[w];
  const int32_t* ids = I.feature_id + (size_t)w * I.max_pts;
  const double* ixy = I.xy + (size_t)w * I.max_pts * 2;
  int32_t* fid = feat_id + (size_t)w * B.max_feat;
  int32_t* fstart = const_cast<int32_t*>(B.feat_start) + (size_t)w * B.max_feat;
  int32_t* fnobs = const_cast<int32_t*>(B.feat_nobs) + (size_t)w * B.max_feat;
  int32_t* fobs = const_cast<int32_t*>(B.feat_obs_begin) + (size_t)w * B.max_feat;
  double* obs = const_cast<double*>(B.obs_xy) + (size_t)w * B.max_obs * 2;
  double* lam = B.inv_depth + (size_t)w * B.max_feat;
  for (int i = tid; i < np; i += TRK_NT) s_id[i] = ids[i], s_mark[i] = 0;
  __syncthreads();
  // every row of the list looks its id up in the image (find_if over the list per point, the other way round)
  for (int e = tid; e < nf; e += TRK_NT) {
    const int p = find_id(s_id, np, fid[e]);
    if (p >= 0) s_mark[p] = 1;
    s_pt[e] = p, s_ob[e] = fobs[e], s_no[e] = fnobs[e] + (p >= 0 ? 1 : 0);
  }
  __syncthreads();
  // the new tracks: the unmarked points in image order (ascending id), behind the list
  const int n_new = block_compact(np, s_tot, [&](int i) { return s_mark[i] == 0; },
                                  [&](int i, int rank) {
                                    const int e = nf + rank;
                                    s_pt[e] = i, s_ob[e] = 0, s_no[e] = 1;
                                    fid[e] = s_id[i], fstart[e] = AVM_WINDOW_SIZE, lam[e] = -1.0;
                                  });
  const int nf2 = nf + n_new;
  block_scan_excl(s_no, s_begin, nf2, s_tot);
  const int total = s_begin[nf2];
  // where every slot of the new table comes from: >= 0 a slot of the old table, < 0 the image point ~src
  // (sfor: the slot index is a constant in the source, so that src and v are registers and never an array in scratch memory)
  int src[TRK_SLOTS];
  sfor<TRK_SLOTS>([&](auto K) {
    constexpr int k = K;
    const int d = tid + k * TRK_NT;
    src[k] = 0;
    if (d < total) {
      const int e = row_of_slot(s_begin, nf2, d), j = d - s_begin[e];
      const int old_no = s_no[e] - (s_pt[e] >= 0 ? 1 : 0);
      src[k] = j < old_no ? s_ob[e] + j : ~s_pt[e];
    }
  });
  {
    d2 v[TRK_SLOTS];
    sfor<TRK_SLOTS>([&](auto K) {
      constexpr int k = K;
      if (tid + k * TRK_NT < total) v[k] = *reinterpret_cast<const d2*>(src[k] >= 0 ? obs + 2 * (size_t)src[k] : ixy + 2 * (size_t)(~src[k]));
    });
    sources_read_barrier();
    sfor<TRK_SLOTS>([&](auto K) {
      constexpr int k = K;
      if (tid + k * TRK_NT < total) *reinterpret_cast<d2*>(obs + 2 * (size_t)(tid + k * TRK_NT)) = v[k];
    });
  }
  if (B.obs_vel_td) {
    double* vtd = const_cast<double*>(B.obs_vel_td) + (size_t)w * B.max_obs * 4;
    const double* itd = I.vel_td + (size_t)w * I.max_pts * 4;
    d4 v[TRK_SLOTS];
    sfor<TRK_SLOTS>([&](auto K) {
      constexpr int k = K;
      if (tid + k * TRK_NT < total) v[k] = *reinterpret_cast<const d4*>(src[k] >= 0 ? vtd + 4 * (size_t)src[k] : itd + 4 * (size_t)(~src[k]));
    });
    sources_read_barrier();
    sfor<TRK_SLOTS>([&](auto K) {
      constexpr int k = K;
      if (tid + k * TRK_NT < total) *reinterpret_cast<d4*>(vtd + 4 * (size_t)(tid + k * TRK_NT)) = v[k];
    });
  }
  for (int e = tid; e < nf2; e += TRK_NT) fnobs[e] = s_no[e], fobs[e] = s_begin[e];
  if (tid == 0) const_cast<int32_t*>(B.n_feat)[w] = nf2;
}

// ---- avm_imu_push_batch --------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void imu_push_check_kernel(avm_window_batch B, const int32_t* n, int max_in, int* first_bad) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= B.n_windows) return;
  if (n[w] < 0 || n[w] > max_in) report(first_bad, w, PUSH_BAD_N);
  else if (B.imu_n[(size_t)w * 10 + 9] + n[w] > B.max_samp) report(first_bad, w, PUSH_CAP);
}

__global__ __launch_bounds__(64) void imu_push_kernel(avm_window_batch B, const int32_t* n, int max_in, const double* dt, const double* acc,
                                                      const double* gyr) {
  const int w = blockIdx.x, lane = threadIdx.x;
  const int SD = B.max_samp, SA = (B.max_samp + 1) * 3;
  int32_t* imu_n = const_cast<int32_t*>(B.imu_n) + (size_t)w * 10;
  double* wdt = const_cast<double*>(B.imu_dt) + ((size_t)w * 10 + 9) * SD;
  double* wacc = const_cast<double*>(B.imu_acc) + ((size_t)w * 10 + 9) * SA;
  double* wgyr = const_cast<double*>(B.imu_gyr) + ((size_t)w * 10 + 9) * SA;
  const int n9 = imu_n[9], m = n[w];
  for (int k = lane; k < m; k += 64) wdt[n9 + k] = dt[(size_t)w * max_in + k];
  for (int k = lane; k < 3 * m; k += 64)  // (row 0 is the sample the interval was constructed with)
    wacc[(n9 + 1) * 3 + k] = acc[(size_t)w * max_in * 3 + k], wgyr[(n9 + 1) * 3 + k] = gyr[(size_t)w * max_in * 3 + k];
  __syncthreads();  // (every lane has read imu_n[9])
  if (lane == 0) imu_n[9] = n9 + m;
}

// ---- avm_solve_view_batch / avm_solve_view_store_depths ---------------------------------------------------------------------------------
AVM_DEV bool in_view(int st, int no) { return no >= 2 && st < AVM_WINDOW_SIZE - 2; }  // estimator.cpp:715

__global__ __launch_bounds__(TRK_NT) void solve_view_check_kernel(avm_window_batch F, avm_window_batch V, int* first_bad) {
  __shared__ int s_rows, s_obs;
  const int w = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) s_rows = 0, s_obs = 0;
  __syncthreads();
  const int nf = F.n_feat[w];
  int rows = 0, obs = 0;
  for (int e = tid; e < nf; e += TRK_NT) {
    const int st = F.feat_start[(size_t)w * F.max_feat + e], no = F.feat_nobs[(size_t)w * F.max_feat + e];
    if (in_view(st, no)) rows++, obs += no;
  }
  atomicAdd(&s_rows, rows), atomicAdd(&s_obs, obs);
  __syncthreads();
  if (tid != 0) return;
  if (s_rows > V.max_feat) report(first_bad, w, VIEW_CAP_FEAT);
  else if (s_obs > V.max_obs) report(first_bad, w, VIEW_CAP_OBS);
}

__global__ __launch_bounds__(TRK_NT) void solve_view_kernel(avm_window_batch F, avm_window_batch V, int32_t* view_row) {
  __shared__ int s_row[AVM_MAX_FEAT], s_no[AVM_MAX_FEAT], s_begin[AVM_MAX_FEAT + 1], s_tot[TRK_MAX_CHUNKS];
  const int w = blockIdx.x, tid = threadIdx.x;
  const int nf = F.n_feat[w];
  const int32_t* fstart = F.feat_start + (size_t)w * F.max_feat;
  const int32_t* fnobs = F.feat_nobs + (size_t)w * F.max_feat;
  const int32_t* fobs = F.feat_obs_begin + (size_t)w * F.max_feat;
  const size_t vf = (size_t)w * V.max_feat, vo = (size_t)w * V.max_obs;
  int32_t* vstart = const_cast<int32_t*>(V.feat_start) + vf;
  int32_t* vnobs = const_cast<int32_t*>(V.feat_nobs) + vf;
  int32_t* vobs = const_cast<int32_t*>(V.feat_obs_begin) + vf;
  const int nv = block_compact(nf, s_tot, [&](int e) { return in_view(fstart[e], fnobs[e]); },
                               [&](int e, int k) {
                                 s_row[k] = e, s_no[k] = fnobs[e];
                                 view_row[vf + k] = e, vstart[k] = fstart[e], vnobs[k] = fnobs[e];
                                 V.inv_depth[vf + k] = F.inv_depth[(size_t)w * F.max_feat + e];
                               });
  block_scan_excl(s_no, s_begin, nv, s_tot);
  const int total = s_begin[nv];
  for (int k = tid; k < nv; k += TRK_NT) vobs[k] = s_begin[k];
  if (tid == 0) const_cast<int32_t*>(V.n_feat)[w] = nv;
  const double* fxy = F.obs_xy + (size_t)w * F.max_obs * 2;
  double* vxy = const_cast<double*>(V.obs_xy) + vo * 2;
  const double* ftd = V.obs_vel_td ? F.obs_vel_td + (size_t)w * F.max_obs * 4 : nullptr;
  double* vtd = V.obs_vel_td ? const_cast<double*>(V.obs_vel_td) + vo * 4 : nullptr;
  for (int d = tid; d < total; d += TRK_NT) {
    const int k = row_of_slot(s_begin, nv, d);
    const size_t s = (size_t)fobs[s_row[k]] + (d - s_begin[k]);
    *reinterpret_cast<d2*>(vxy + 2 * (size_t)d) = *reinterpret_cast<const d2*>(fxy + 2 * s);
    if (vtd) *reinterpret_cast<d4*>(vtd + 4 * (size_t)d) = *reinterpret_cast<const d4*>(ftd + 4 * s);
  }
}

__global__ __launch_bounds__(64) void store_depths_check_kernel(avm_window_batch F, avm_window_batch V, const int32_t* view_row, int* first_bad) {
  const int w = blockIdx.x, lane = threadIdx.x;
  const int nf = F.n_feat[w], nv = V.n_feat[w];
  if (nf < 0 || nf > F.max_feat || nv < 0 || nv > V.max_feat) {
    if (lane == 0) report(first_bad, w, DEPTH_BAD_NFEAT);
    return;
  }
  const int32_t* row = view_row + (size_t)w * V.max_feat;
  bool bad = false;
  for (int k = lane; k < nv; k += 64) bad = bad || row[k] < 0 || row[k] >= nf || (k > 0 && row[k] <= row[k - 1]);
  if (bad) report(first_bad, w, DEPTH_BAD_ROW);
}

__global__ __launch_bounds__(TRK_NT) void store_depths_kernel(avm_window_batch F, avm_window_batch V, const int32_t* view_row) {
  const int w = blockIdx.x;
  const int nv = V.n_feat[w];
  for (int k = threadIdx.x; k < nv; k += TRK_NT)
    F.inv_depth[(size_t)w * F.max_feat + view_row[(size_t)w * V.max_feat + k]] = V.inv_depth[(size_t)w * V.max_feat + k];
}

// ---- avm_prior_keep_batch ---------------------------------------------------------------------------------------------------------------
// estimator.cpp:926-927: a window whose marginalization reported n < 0 keeps the prior it was solved with (B's prior tables: CHK_PRIOR passed)
__global__ __launch_bounds__(64) void prior_keep_check_kernel(avm_window_batch B, avm_prior_out P, int* first_bad) {
  const int w = blockIdx.x * 64 + threadIdx.x;
  if (w >= B.n_windows || P.n[w] >= 0) return;
  const int n = B.prior_n[w], nb = B.prior_nblk[w];
  if (nb < 0 || nb > B.max_pblk) report(first_bad, w, KEEP_BAD_NBLK);
  else if (n > P.max_prior || nb > P.max_pblk) report(first_bad, w, KEEP_CAP);
}

__global__ __launch_bounds__(TRK_NT) void prior_keep_kernel(avm_window_batch B, avm_prior_out P) {
  const int w = blockIdx.x, tid = threadIdx.x;
  if (P.n[w] >= 0) return;  // (uniform; thread 0 writes P.n behind the barrier, after every thread has read it)
  const int n = B.prior_n[w], nb = B.prior_nblk[w];
  const size_t bs = B.max_prior, ps = P.max_prior;
  const double* J = B.prior_J + (size_t)w * bs * bs;
  double* Jo = P.J + (size_t)w * ps * ps;
  for (int k = tid; k < n * n; k += TRK_NT) Jo[(size_t)(k / n) * ps + k % n] = J[(size_t)(k / n) * bs + k % n];
  for (int k = tid; k < n; k += TRK_NT) P.r[(size_t)w * ps + k] = B.prior_r[(size_t)w * bs + k];
  for (int k = tid; k < nb; k += TRK_NT) {
    P.blk_kind[(size_t)w * P.max_pblk + k] = B.prior_blk_kind[(size_t)w * B.max_pblk + k];
    P.blk_frame[(size_t)w * P.max_pblk + k] = B.prior_blk_frame[(size_t)w * B.max_pblk + k];
  }
  for (int k = tid; k < nb * 9; k += TRK_NT) P.x0[(size_t)w * P.max_pblk * 9 + k] = B.prior_x0[(size_t)w * B.max_pblk * 9 + k];
  __syncthreads();
  if (tid == 0) P.n[w] = n, P.nblk[w] = nb;
}

// ---- avm_fsel_select_image_batch -----------------------------------------------------------------------------------------------------
// FeatureSelector::select()'s bookkeeping (feature_selector.cpp:98-120, 156-196) around the selection: check, split (image -> the
// selector problem), merge (selection -> image_out and the selector's state).  The three kernels see a window the same way, through
// SelWindow: counts clamped to the strides, so that every index below is inside its table whatever the tables hold.
struct SelWindow {
  int np, nt, s;  // image points, tracked ids, old points: ids[0 .. s) <= last_feature_id < ids[s .. np)  (splitOnFeatureId, :208-219)
  bool init, first;
};

// number of ids[0 .. n) that are <= k: std::map::upper_bound (memory-safe on any input)
AVM_DEV int upper_bound_id(const int* ids, int n, int k) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] <= k) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// Stages the window's ids in s_id, clears s_mark and splits; ends with a workgroup barrier.  Every member is uniform over the workgroup.
AVM_DEV SelWindow sel_stage(const SelectImageArgs& a, int w, int* s_id, int* s_mark) {
  SelWindow q;
  q.np = min(max(a.image.n_pts[w], 0), min(a.image.max_pts, AVM_MAX_IMAGE_PTS));
  q.nt = min(max(a.state.n_tracked[w], 0), a.state.max_tracked);
  q.init = a.initialized ? a.initialized[w] != 0 : true;
  q.first = a.state.first_image[w] != 0;
  const int last = a.state.last_feature_id[w];
  const int32_t* ids = a.image.feature_id + (size_t)w * a.image.max_pts;
  for (int i = threadIdx.x; i < q.np; i += TRK_NT) s_id[i] = ids[i], s_mark[i] = 0;
  __syncthreads();
  q.s = upper_bound_id(s_id, q.np, last);
  return q;
}

// s_mark[p] = 1 for the old points whose id is in the tracked list: one thread per TRACKED id looks it up in the image (the list is in
// append order, unsorted).  No barrier.
AVM_DEV void sel_mark_tracked(const SelWindow& q, const int32_t* tracked, const int* s_id, int* s_mark) {
  for (int t = threadIdx.x; t < q.nt; t += TRK_NT) {
    const int p = find_id(s_id, q.s, tracked[t]);
    if (p >= 0) s_mark[p] = 1;
  }
}

// The same walk TRK_NT entries at a time in list order, with the entries that stay in the list ranked (all of them, or with `prune` the
// ones found in the image): emit(id, rank) for each, their number returned to every thread.  Item i of a chunk is ranked by thread i, so
// `id` is the thread's own register, read behind sources_read_barrier() before the chunk's first emit: emit may write the list in place.
// s_keep: TRK_NT ints of LDS.  Ends with a workgroup barrier unless the list is empty.
template <class Emit>
AVM_DEV int sel_walk_tracked(const SelWindow& q, const int32_t* tracked, int prune, const int* s_id, int* s_mark, int* s_keep, int* s_tot,
                             Emit emit) {
  int kept = 0;
  for (int base = 0; base < q.nt; base += TRK_NT) {  // (uniform bounds)
    const int t = base + threadIdx.x;
    int id = 0, keep = 0;
    if (t < q.nt) {
      id = tracked[t];
      const int p = find_id(s_id, q.s, id);
      if (p >= 0) s_mark[p] = 1;
      keep = p >= 0 || !prune;
    }
    s_keep[threadIdx.x] = keep;
    sources_read_barrier();
    const int n = block_compact(min(TRK_NT, q.nt - base), s_tot, [&](int i) { return s_keep[i] != 0; }, [&](int, int rank) { emit(id, kept + rank); });
    kept += n;
  }
  return kept;
}

__global__ __launch_bounds__(TRK_NT) void select_image_check_kernel(SelectImageArgs a, int* first_bad) {
  __shared__ int s_id[AVM_MAX_IMAGE_PTS], s_mark[AVM_MAX_IMAGE_PTS], s_tot[TRK_MAX_CHUNKS], s_keep[TRK_NT], s_bad;
  const int w = blockIdx.x, tid = threadIdx.x;
  const int np = a.image.n_pts[w], nt = a.state.n_tracked[w];
  if (np < 0 || np > a.image.max_pts || nt < 0 || nt > a.state.max_tracked) {  // (uniform over the workgroup)
    if (tid == 0) report(first_bad, w, np < 0 || np > a.image.max_pts ? SEL_BAD_NPTS : SEL_BAD_NTRACKED);
    return;
  }
  if (tid == 0) s_bad = 0;
  const SelWindow q = sel_stage(a, w, s_id, s_mark);
  bool bad = false;
  for (int i = tid + 1; i < q.np; i += TRK_NT) bad = bad || s_id[i] <= s_id[i - 1];
  if (bad) s_bad = 1;
  __syncthreads();
  if (s_bad) {  // (uniform; the lookups below want ascending ids)
    if (tid == 0) report(first_bad, w, SEL_BAD_IDS);
    return;
  }
  const int kept = sel_walk_tracked(q, a.state.tracked_id + (size_t)w * a.state.max_tracked, a.prune_lost, s_id, s_mark, s_keep, s_tot, [](int, int) {});
  const int n_used = block_compact(q.s, s_tot, [&](int i) { return s_mark[i] != 0; }, [](int, int) {});
  if (tid != 0) return;
  const int n_new = q.np - q.s, n_old = q.s;
  const int picks = min(max(0, a.problem.max_features - n_used), n_new);  // min(kappa, n_new): the most the selection can return
  int n_out, n_app;
  if (q.init) n_out = n_used + picks, n_app = picks;
  else {
    n_out = q.first ? n_new : n_used, n_app = q.first ? n_new : 0;
    if (n_out < a.init_thresh) n_out = q.first ? q.np : n_old;
  }
  int rule = 1 << 30;
  if (q.init && n_new > a.problem.max_cand) rule = min(rule, (int)SEL_CAP_CAND);
  if (n_used > a.problem.max_used) rule = min(rule, (int)SEL_CAP_USED);
  if (n_out > a.image_out.max_pts) rule = min(rule, (int)SEL_CAP_IMAGE);
  if (kept + n_app > a.state.max_tracked) rule = min(rule, (int)SEL_CAP_TRACKED);
  if (rule != 1 << 30) report(first_bad, w, rule);
}

// Writes problem.n_used / used_* (every window) and n_cand / cand_* (initialized windows; the others get n_cand = 0): nothing else.
__global__ __launch_bounds__(TRK_NT) void select_split_kernel(SelectImageArgs a) {
  __shared__ int s_id[AVM_MAX_IMAGE_PTS], s_mark[AVM_MAX_IMAGE_PTS], s_tot[TRK_MAX_CHUNKS];
  const int w = blockIdx.x, tid = threadIdx.x;
  const SelWindow q = sel_stage(a, w, s_id, s_mark);
  sel_mark_tracked(q, a.state.tracked_id + (size_t)w * a.state.max_tracked, s_id, s_mark);
  __syncthreads();
  const avm_fsel_batch& F = a.problem;
  const double* ixy = a.image.xy + (size_t)w * a.image.max_pts * 2;
  int32_t* used_id = const_cast<int32_t*>(F.used_id) + (size_t)w * F.max_used;
  double* used_xy = const_cast<double*>(F.used_xy) + (size_t)w * F.max_used * 2;
  const int n_used = block_compact(q.s, s_tot, [&](int i) { return s_mark[i] != 0; },
                                   [&](int i, int rank) {
                                     if (rank >= F.max_used) return;
                                     used_id[rank] = s_id[i];
                                     *reinterpret_cast<d2*>(used_xy + 2 * (size_t)rank) = *reinterpret_cast<const d2*>(ixy + 2 * (size_t)i);
                                   });
  // the new points are the tail of the image: their rank in index order is i - s
  const int n_cand = q.init ? min(q.np - q.s, F.max_cand) : 0;
  int32_t* cand_id = const_cast<int32_t*>(F.cand_id) + (size_t)w * F.max_cand;
  double* cand_xy = const_cast<double*>(F.cand_xy) + (size_t)w * F.max_cand * 2;
  double* cand_prob = const_cast<double*>(F.cand_prob) + (size_t)w * F.max_cand;
  const double* prob = a.prob + (size_t)w * a.image.max_pts;
  for (int j = tid; j < n_cand; j += TRK_NT) {
    const int i = q.s + j;
    cand_id[j] = s_id[i];
    *reinterpret_cast<d2*>(cand_xy + 2 * (size_t)j) = *reinterpret_cast<const d2*>(ixy + 2 * (size_t)i);
    cand_prob[j] = prob[i];
  }
  if (tid == 0) const_cast<int32_t*>(F.n_used)[w] = min(n_used, F.max_used), const_cast<int32_t*>(F.n_cand)[w] = n_cand;
}

// The selection is in a.out: image_out and the selector's state.  The tracked list is compacted in place, TRK_NT entries at a time in
// list order: a kept entry moves left or stays, so a chunk's destinations are entries of this chunk or of earlier ones, all of which
// have been read - this chunk's into registers, behind sources_read_barrier().
__global__ __launch_bounds__(TRK_NT) void select_merge_kernel(SelectImageArgs a) {
  __shared__ int s_id[AVM_MAX_IMAGE_PTS], s_mark[AVM_MAX_IMAGE_PTS], s_tot[TRK_MAX_CHUNKS], s_keep[TRK_NT];
  const int w = blockIdx.x, tid = threadIdx.x;
  const SelWindow q = sel_stage(a, w, s_id, s_mark);
  const int n_new = q.np - q.s, max_tracked = a.state.max_tracked;
  int32_t* tracked = a.state.tracked_id + (size_t)w * max_tracked;
  const int kept = sel_walk_tracked(q, tracked, a.prune_lost, s_id, s_mark, s_keep, s_tot, [&](int id, int pos) { tracked[pos] = id; });
  __syncthreads();
  int n_app = 0;  // ids appended behind the kept ones
  if (q.init) {
    // the selected ids, in selection order: marked among the new points, appended to the list (:196)
    n_app = min(max(a.out.n_selected[w], 0), a.problem.max_features);
    const int32_t* sel = a.out.selected_ids + (size_t)w * a.problem.max_features;
    for (int k = tid; k < n_app; k += TRK_NT) {
      const int id = sel[k], p = find_id(s_id + q.s, n_new, id);
      if (p >= 0) s_mark[q.s + p] = 1;
      if (kept + k < max_tracked) tracked[kept + k] = id;
    }
  } else {
    // :172-187 - the first image: the subset becomes the new points, all of them tracked from now on; too few points: every old one joins
    const int n_used = block_compact(q.s, s_tot, [&](int i) { return s_mark[i] != 0; }, [](int, int) {});
    const bool all_old = (q.first ? n_new : n_used) < a.init_thresh;
    for (int i = tid; i < q.np; i += TRK_NT) s_mark[i] = i >= q.s ? q.first : (all_old || (!q.first && s_mark[i] != 0));
    if (q.first) {
      n_app = n_new;
      for (int j = tid; j < n_new; j += TRK_NT)
        if (kept + j < max_tracked) tracked[kept + j] = s_id[q.s + j];
    }
  }
  __syncthreads();
  const avm_image_batch& O = a.image_out;
  const double* ixy = a.image.xy + (size_t)w * a.image.max_pts * 2;
  const double* itd = a.image.vel_td ? a.image.vel_td + (size_t)w * a.image.max_pts * 4 : nullptr;
  int32_t* oid = const_cast<int32_t*>(O.feature_id) + (size_t)w * O.max_pts;
  double* oxy = const_cast<double*>(O.xy) + (size_t)w * O.max_pts * 2;
  double* otd = itd ? const_cast<double*>(O.vel_td) + (size_t)w * O.max_pts * 4 : nullptr;
  const int n_out = block_compact(q.np, s_tot, [&](int i) { return s_mark[i] != 0; },
                                  [&](int i, int rank) {
                                    if (rank >= O.max_pts) return;
                                    oid[rank] = s_id[i];
                                    *reinterpret_cast<d2*>(oxy + 2 * (size_t)rank) = *reinterpret_cast<const d2*>(ixy + 2 * (size_t)i);
                                    if (otd) *reinterpret_cast<d4*>(otd + 4 * (size_t)rank) = *reinterpret_cast<const d4*>(itd + 4 * (size_t)i);
                                  });
  if (tid != 0) return;
  const_cast<int32_t*>(O.n_pts)[w] = min(n_out, O.max_pts);
  a.state.n_tracked[w] = min(kept + n_app, max_tracked);
  if (n_new > 0) a.state.last_feature_id[w] = s_id[q.np - 1];
  if (!q.init && q.first) a.state.first_image[w] = 0;
}

}  // namespace

hipError_t launch_add_image_check(const avm_window_batch& b, const int32_t* feat_id, const avm_image_batch& img, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(add_image_check_kernel, dim3(b.n_windows), dim3(TRK_NT), 0, stream, b, feat_id, img, first_bad);
  return hipGetLastError();
}

hipError_t launch_add_image(const avm_window_batch& b, int32_t* feat_id, const avm_image_batch& img, hipStream_t stream) {
  hipLaunchKernelGGL(add_image_kernel, dim3(b.n_windows), dim3(TRK_NT), 0, stream, b, feat_id, img);
  return hipGetLastError();
}

hipError_t launch_imu_push_check(const avm_window_batch& b, const int32_t* n, int max_in, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(imu_push_check_kernel, dim3((b.n_windows + 63) / 64), dim3(64), 0, stream, b, n, max_in, first_bad);
  return hipGetLastError();
}

hipError_t launch_imu_push(const avm_window_batch& b, const int32_t* n, int max_in, const double* dt, const double* acc, const double* gyr,
                           hipStream_t stream) {
  hipLaunchKernelGGL(imu_push_kernel, dim3(b.n_windows), dim3(64), 0, stream, b, n, max_in, dt, acc, gyr);
  return hipGetLastError();
}

hipError_t launch_solve_view_check(const avm_window_batch& full, const avm_window_batch& view, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(solve_view_check_kernel, dim3(full.n_windows), dim3(TRK_NT), 0, stream, full, view, first_bad);
  return hipGetLastError();
}

hipError_t launch_solve_view(const avm_window_batch& full, const avm_window_batch& view, int32_t* view_row, hipStream_t stream) {
  hipLaunchKernelGGL(solve_view_kernel, dim3(full.n_windows), dim3(TRK_NT), 0, stream, full, view, view_row);
  return hipGetLastError();
}

hipError_t launch_store_depths_check(const avm_window_batch& full, const avm_window_batch& view, const int32_t* view_row, int* first_bad,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(store_depths_check_kernel, dim3(full.n_windows), dim3(64), 0, stream, full, view, view_row, first_bad);
  return hipGetLastError();
}

hipError_t launch_store_depths(const avm_window_batch& full, const avm_window_batch& view, const int32_t* view_row, hipStream_t stream) {
  hipLaunchKernelGGL(store_depths_kernel, dim3(full.n_windows), dim3(TRK_NT), 0, stream, full, view, view_row);
  return hipGetLastError();
}

hipError_t launch_prior_keep_check(const avm_window_batch& b, const avm_prior_out& po, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(prior_keep_check_kernel, dim3((b.n_windows + 63) / 64), dim3(64), 0, stream, b, po, first_bad);
  return hipGetLastError();
}

hipError_t launch_prior_keep(const avm_window_batch& b, const avm_prior_out& po, hipStream_t stream) {
  hipLaunchKernelGGL(prior_keep_kernel, dim3(b.n_windows), dim3(TRK_NT), 0, stream, b, po);
  return hipGetLastError();
}

hipError_t launch_select_image_check(const SelectImageArgs& a, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(select_image_check_kernel, dim3(a.image.n_windows), dim3(TRK_NT), 0, stream, a, first_bad);
  return hipGetLastError();
}

hipError_t launch_select_split(const SelectImageArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(select_split_kernel, dim3(a.image.n_windows), dim3(TRK_NT), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_select_merge(const SelectImageArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(select_merge_kernel, dim3(a.image.n_windows), dim3(TRK_NT), 0, stream, a);
  return hipGetLastError();
}

}  // namespace avm
