// kernels.hpp — argument blocks shared by the host C-ABI layer (avm_api.hip) and the kernels.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/avm.h"
#include "sfm/rules.hpp"  // (with include/avm_init.h)

namespace avm {

// compile-time problem limits of the window-solve kernel (WINDOW_SIZE = 10 => 11 frames)
constexpr int NFR = AVM_NFRAMES;       // 11
// The solve kernel is compiled twice from the same source (csrc/Makefile):
//   window_solve.o    the reference's default configuration (ESTIMATE_EXTRINSIC = 0, ESTIMATE_TD = 0, no relocalization frame):
//                     f-block = pose 66 | speed-bias 99 = 165 columns
//   window_solve_x.o  (-DAVM_X) every optional member of the problem: the dense "pose-like" part grows to
//                     pose 66 | relo_Pose 6 | ex_pose 6 | td 1 = 79 columns (relo_Pose is treated as a 12th frame), then
//                     speed-bias 99 = 178 columns; members that are switched off keep a unit diagonal
#ifdef AVM_X
constexpr int NFRP = NFR + 1;          // pose-like frames of the projection factors: 11 window frames + relo_Pose
constexpr int NPOSE = NFRP * 6 + 7;    // 79 dense columns in front of the speed-biases
constexpr int XC_EX = NFRP * 6;        // 72: first ex_pose column
constexpr int XC_TD = XC_EX + 6;       // 78: the td column
#else
constexpr int NFRP = NFR;
constexpr int NPOSE = NFR * 6;         // 66 pose columns (local)
#endif
constexpr int NF = NPOSE + NFR * 9;    // 165 (178) f-block columns: poses (+ relo, ex, td) first, then speed-bias
constexpr int SB0 = NPOSE;             // column of speedbias[0]
constexpr int MAXE = 150;              // inverse depths (e-blocks)
constexpr int NCOL = NF + MAXE;        // 315 (328)
constexpr int MAXOBS = MAXE * NFR;     // 1650 observation slots
constexpr int MAXPRIOR = 96;           // prior residual dimension limit
constexpr int MAXKEEP = 76;            // rows a marginalization may keep (prior_eig.hip holds A' and V in half a CU's LDS); this problem keeps <= 75
constexpr int MAXPBLK = 16;

struct PreintArgs {
  int n_windows, max_samp;
  const int32_t* imu_n;
  const double *imu_dt, *imu_acc, *imu_gyr, *imu_lin_ba, *imu_lin_bg;
  double acc_n, gyr_n, acc_w, gyr_w;
  double *out_delta, *out_jacobian, *out_covariance, *out_sum_dt, *out_sqrt_info;
  // null: every interval.  Else the intervals launch_preint_match listed, todo[0 .. todo_count[0]) (both device memory): only they are
  // integrated and stored, the results of the others stay as they are
  const int32_t *todo = nullptr, *todo_count = nullptr;
};

// The ctx's record of what the stored pre-integrations were computed from (avm_api.hip, run_preint; preint.hip, preint_match_kernel)
constexpr long preint_key_words(int max_samp) { return 13 + 7 * (long)max_samp; }  // 64-bit words of an interval's key
struct PreintKeys {
  unsigned long long* key;     // [n_windows * 10][preint_key_words(max_samp)]
  int32_t* valid;              // [n_windows * 10] 1: the key is what the interval's stored results were computed from
  int32_t* todo;               // [n_windows * 10] out: the intervals to integrate
  int32_t *count, *count_next; // out: their number (zero on entry); zeroed for the next call
};
struct PreintRoll {
  int n_windows, key_words;
  const int32_t* flags;  // [n_windows] device, or null: every window takes `flag`
  int flag;
  unsigned long long* key;
  int32_t* valid;
  double *delta, *jac, *cov, *sqrt_info, *sum_dt;
};

// per-slot global scratch layout (doubles), one slot per resident workgroup (stays L2 resident)
// (one layout for every build of the solve kernel and the marginalization kernel: the slots are shared.  The regions and their sizes are here, because
//  the host sizes the slots from TOTAL; what lies inside each region is in solve/slot.hpp, which holds every layout against these sizes)
struct Scratch {
  static constexpr size_t PF_N = 17 * (size_t)MAXOBS;           // 17 quantities x observation slots
  static constexpr size_t PART_N = 9600;
  static constexpr size_t IJRAW_N = 4656;
  static constexpr size_t W_N = (size_t)80 * 152;               // 80 columns x 152 features
  static constexpr size_t HP_N = (size_t)MAXPRIOR * MAXPRIOR;
  static constexpr size_t PF = 0;                               // per-factor products with Je, feature-major
  static constexpr size_t PART = PF + PF_N;                     // partial blocks of the frame tasks
  static constexpr size_t IJRAW = PART + PART_N;                // IMU residual + Jacobian before sqrt_info
  static constexpr size_t W = IJRAW + IJRAW_N;                  // E^T F, feature-major
  static constexpr size_t HP = W + W_N;                         // the prior's packed J0^T J0 and its destinations; the speculation's backup
  static constexpr size_t TOTAL = HP + HP_N;
};
constexpr int ISCRATCH = MAXOBS + (NFR + 1) * MAXE;  // ints per slot: observation slot -> feature, then cov[12][150] (row 11: the relocalization frame)

constexpr int PROF_SLOTS = 64;
struct SolveArgs {
  avm_window_batch b;  // device pointers
  avm_options opt;
  const double *pre_delta, *pre_jac, *pre_sqrt, *pre_sum_dt;  // [B][10][...]
  double* scratch;                                            // [n_slots][Scratch::TOTAL]
  int32_t* iscratch;                                          // [n_slots][ISCRATCH]
  avm_solve_summary* summary;                                 // [B] or null
  int n_slots;
  long long* prof;  // optional [n_slots][PROF_SLOTS] per-phase shader-clock accumulators (debug)
  int speculate;    // 1: evaluate the Jacobian at the candidate directly while steps keep being accepted (solve/solve_kernel.hpp)
  long long time_cap_ticks;  // avm_options::max_solver_time_s in ticks of the device wall clock (wall_clock64); 0 = no cap
  const int32_t* marg_flags;  // [B] device, or null: every window takes opt.marginalization_flag (read by the -DAVM_MARG_MIXED marginalization kernels only)
};
// The argument block of the -DAVM_WIN_LIST builds of the solve kernel (window_solve_list.o, _x_list.o, _tp_list.o): SolveArgs with
// the window list appended.  (A block of its own and not three more members of SolveArgs: the kernel-argument size of every existing
// kernel is part of its code object's .note, and those code objects stay byte for byte what they were.)
struct SolveListArgs : SolveArgs {
  const int32_t* win_list;     // [n_list] device: the windows this launch solves, ascending; null: windows 0 .. n_list - 1
  int n_list;
  const int32_t* relo_active;  // [B] device, or null: a window has a relocalization frame only where this is != 0 (extended build)
};
// avm_window_solve_batch_relo's split of a batch: list[0 .. B) = the windows with relo_active == 0, list[B .. 2 B) = the others, both
// ascending; counts[0] = the number of the others (the first list holds the rest).  One workgroup; solve_split.hip
hipError_t launch_solve_partition(int n_windows, const int32_t* relo_active, int32_t* list, int* counts, hipStream_t stream);
hipError_t launch_window_solve_list(const SolveListArgs& a, hipStream_t stream);     // window_solve_list.o: the latency build over a list
hipError_t launch_window_solve_x_list(const SolveListArgs& a, hipStream_t stream);   // window_solve_x_list.o: the extended build
hipError_t launch_window_solve_tp_list(const SolveListArgs& a, hipStream_t stream);  // window_solve_tp_list.o: the throughput build
int window_solve_tp_list_occupancy();

struct EvalArgs {
  avm_window_batch b;
  avm_options opt;
  const double *pre_delta, *pre_jac, *pre_sqrt, *pre_sum_dt;
  int apply_loss;
  double *proj_r, *proj_J, *imu_r, *imu_J, *prior_res, *cost;
};

// device work buffers of the feature selector (owned by the ctx)
constexpr int FS_SYNC_INTS = 64 + 16 * 32 + 16 * 2 * 2 * 512 * 4;  // header, 16 team headers, per team (fValue, ub) x two parities x 512 16-byte records
constexpr int FS_MAX_CLOUD = 4096;  // depth-cloud points per frame the kd-tree builder has LDS for (28 bytes each; the reference's cloud is the window's <= 150 landmarks)
struct FselBuffers {
  double *C, *dpp, *consts, *delta, *delta_pk, *ddiag, *delta_u, *fval, *ub;
  double* kd;  // [P][8 + 11 max_cloud] the frames' kd-trees over their depth clouds (csrc/fsel/kdtree.hpp, fsel_kdtree_kernel)
  int32_t *valid, *valid_u, *black, *nsel, *done, *live, *pos, *nlive;
  int32_t* sync;  // [FS_SYNC_INTS] slot counter / failure flag / cycle trace / per-slot records of the single-frame kernel (csrc/fsel/frame_kernel.hpp)
};

// ---- table validation (every entry point that takes tables runs it before any kernel indexes with them) -----------
// Which groups of an avm_window_batch an entry point reads.
enum { CHK_TRACKS = 1, CHK_IMU = 2, CHK_PRIOR = 4 };
// 0 = fine; otherwise the first violated rule (messages in avm_api.hip, table_rule_text)
enum { BAD_NFEAT = 1, BAD_TRACK = 2, BAD_ORDER = 3, BAD_OBS = 4, BAD_IMU = 5, BAD_PRIOR = 6, BAD_FSEL = 7 };
constexpr int BAD_FLAG = 7;  // (windows; BAD_FSEL is the selector frames' only rule) a per-window marginalization flag outside the set the entry point takes

// The per-window marginalization flags of an entry point, checked in the same pass as the tables: `allowed` has bit f set for every
// value f the entry point takes.  flags == null: nothing to check.
struct FlagRule {
  const int32_t* flags = nullptr;
  unsigned allowed = 0;
};
__host__ __device__ inline bool flag_allowed(const FlagRule& fr, int w) {
  const int f = fr.flags[w];
  return f >= 0 && f < 32 && ((fr.allowed >> f) & 1u);
}

// The lowest-numbered violated rule of window w (0 = fine), looking at features e = first, first + stride, ... only, so
// that the host (first 0, stride 1) and a wavefront (first = lane, stride 64, then a min over the lanes) agree.
__host__ __device__ inline int check_window_tables(const avm_window_batch& B, int w, int what, int first = 0, int stride = 1) {
  int bad = 1 << 30;
  auto rule = [&](int r) { bad = r < bad ? r : bad; };
  if (what & CHK_TRACKS) {
    const int nf = B.n_feat[w];
    if (nf < 0 || nf > B.max_feat) return BAD_NFEAT;
    for (int e = first; e < nf; e += stride) {
      const size_t k = (size_t)w * B.max_feat + e;
      const int a = B.feat_start[k], no = B.feat_nobs[k], ob = B.feat_obs_begin[k];
      if (a < 0 || no < 1 || a + no > AVM_NFRAMES) rule(BAD_TRACK);
      if (e > 0 && a < B.feat_start[k - 1]) rule(BAD_ORDER);
      if (ob < 0 || ob + no > B.max_obs) rule(BAD_OBS);
    }
  }
  if (first == 0) {
    if (what & CHK_IMU)
      for (int j = 0; j < AVM_WINDOW_SIZE; j++) {
        const int n = B.imu_n[(size_t)w * AVM_WINDOW_SIZE + j];
        if (n < 0 || n > B.max_samp) rule(BAD_IMU);
      }
    if ((what & CHK_PRIOR) && B.prior_n) {
      const int pn = B.prior_n[w];
      if (pn < 0 || pn > B.max_prior) rule(BAD_PRIOR);
      else if (pn > 0) {
        const int nb = B.prior_nblk[w];
        if (nb < 1 || nb > B.max_pblk) rule(BAD_PRIOR);
        else {
          int off = 0;
          for (int k = 0; k < nb; k++) {
            const int kind = B.prior_blk_kind[(size_t)w * B.max_pblk + k], fr = B.prior_blk_frame[(size_t)w * B.max_pblk + k];
            if (kind < AVM_BLK_POSE || kind > AVM_BLK_TD || fr < 0 || fr >= AVM_NFRAMES) rule(BAD_PRIOR);
            off += kind == AVM_BLK_SPEEDBIAS ? 9 : (kind == AVM_BLK_TD ? 1 : 6);
          }
          if (off != pn) rule(BAD_PRIOR);
        }
      }
    }
  }
  return bad == (1 << 30) ? 0 : bad;
}

__host__ __device__ inline int check_fsel_tables(const avm_fsel_batch& b, int p) {
  if (b.n_cand[p] < 0 || b.n_cand[p] > b.max_cand) return BAD_FSEL;
  if (b.n_used && (b.n_used[p] < 0 || b.n_used[p] > b.max_used)) return BAD_FSEL;
  if (b.n_cloud && (b.n_cloud[p] < 0 || b.n_cloud[p] > b.max_cloud)) return BAD_FSEL;
  if (b.nr_imu[p] < 0) return BAD_FSEL;
  return 0;
}

// The throughput form of the solve (window_solve_tp.o) keeps the speed-bias rows of the system in their structural form plus ONE strip
// "the prior's speed-bias block x every pose" (solve/lds.hpp, s_off): a prior with more than one speed-bias block does not fit it.
// The reference never builds one (estimator.cpp:904-916 keeps para_SpeedBias[1] only); such a batch simply takes the other kernel.
// The throughput form of the marginalization (marginalize_tp_kernel, round 5) holds the joint system over poses | speed-biases 0, 1 |
// ex_pose | td only: a prior with a speed-bias block of a later frame does not fit it (the reference keeps frame 1's, as frame 0).
// Returns a bit mask of what window w's prior does NOT fit: bit 0 the throughput solve, bit 1 the throughput marginalization.
__host__ __device__ inline int window_prior_tp_misfit(const avm_window_batch& B, int w) {
  if (!B.prior_n || B.prior_n[w] <= 0) return 0;
  int nsb = 0, late = 0, later = 0;
  const int nb = B.prior_nblk[w];
  for (int k = 0; k < nb && k < B.max_pblk; k++)
    if (B.prior_blk_kind[(size_t)w * B.max_pblk + k] == AVM_BLK_SPEEDBIAS) {
      const int fr = B.prior_blk_frame[(size_t)w * B.max_pblk + k];
      nsb++, late |= fr > 1, later |= fr > 0;
    }
  // (the throughput solve eliminates the speed-bias blocks last frame first, so that the one block the prior couples to every pose comes
  //  last of them: solve/chol_regs_tables.hpp - a prior whose block is not frame 0's would fill the factor in)
  return (nsb > 1 || later ? 1 : 0) | (late ? 2 : 0);
}

// ---- Estimator::visualInitialAlign (visual_align.hip) -------------------------------------------------------------------------------
struct AlignArgs {
  avm_align_batch a;   // device pointers
  avm_window_batch w;  // device pointers; only read when has_windows
  int has_windows;
  double g_norm;       // G.norm()
  avm_align_out out;   // device pointers (ok, delta_bg, g_c0, x always; g_world with windows)
  double *delta, *sum_dt;  // [B][max_frames - 1][10], [B][max_frames - 1]: the repropagated pre-integrations
};
enum { BAD_ALIGN_FRAMES = 1, BAD_ALIGN_IMU = 2, BAD_ALIGN_KEYS = 3 };
// 0 = fine; otherwise the first violated rule of window b (keys: key_index is read)
__host__ __device__ inline int check_align_tables(const avm_align_batch& A, int b, bool keys) {
  const int F = A.n_frames[b];
  if (F < 2 || F > A.max_frames) return BAD_ALIGN_FRAMES;
  for (int j = 0; j < F - 1; j++) {
    const int n = A.imu_n[(size_t)b * (A.max_frames - 1) + j];
    if (n < 0 || n > A.max_samp) return BAD_ALIGN_IMU;
  }
  if (keys)
    for (int i = 0; i < AVM_NFRAMES; i++) {
      const int k = A.key_index[(size_t)b * AVM_NFRAMES + i];
      if (k < 0 || k >= F || (i > 0 && k <= A.key_index[(size_t)b * AVM_NFRAMES + i - 1])) return BAD_ALIGN_KEYS;
    }
  return 0;
}
hipError_t launch_validate_align(const avm_align_batch& a, bool keys, int* first_bad, hipStream_t stream);
hipError_t launch_align_gyro_bias(const AlignArgs& a, hipStream_t stream);
hipError_t launch_align_solve(const AlignArgs& a, hipStream_t stream);
hipError_t launch_align_prepare(const AlignArgs& a, hipStream_t stream);
hipError_t launch_align_apply(const AlignArgs& a, hipStream_t stream);

// ---- the deterministic half of Estimator::initialStructure (global_sfm.hip; the table check: sfm/rules.hpp) -----------------------------
struct SfmArgs {
  avm_sfm_batch s;       // device pointers
  avm_window_batch w;    // device pointers: the track tables and ex_pose of `full`
  const int32_t* feat_id;
  avm_sfm_out out;       // device pointers
  // stages, committed per stream by sfm_commit_kernel: st [B] 0 = the BA was accepted, else the stream's ok; fst [B][max_frames] a frame's
  // outcome (0 / 3); q [B][11][4], T [B][11][3], point [B][max_feat][3], state [B][max_feat], frame_R / frame_T as the outputs
  int32_t *st, *fst, *sstate;
  double *sq, *sT, *spoint, *sR, *sfT;
};
hipError_t launch_validate_sfm(const avm_sfm_batch& s, int* first_bad, hipStream_t stream);
hipError_t launch_sfm_chain_ba(const SfmArgs& a, hipStream_t stream);
hipError_t launch_sfm_frame_pnp(const SfmArgs& a, hipStream_t stream);
hipError_t launch_sfm_commit(const SfmArgs& a, hipStream_t stream);

// Launch of a kernel whose dynamic LDS exceeds the default limit.  hipFuncAttributeMaxDynamicSharedMemorySize is set once per process
// and kernel, by the first call: a function-local static per Kernel, initialised under the language's guard, so concurrent first calls from
// two threads are safe.  A failed hipFuncSetAttribute is remembered and returned by every later call as well; it is not tried again.
template <auto Kernel>
hipError_t lds_attr_once(int lds_bytes) {
  static const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
  return e;
}
// A kernel that is asked for another LDS size from call to call: the attribute once, to `lds_ceiling`, the largest size it can be asked
// for (set from the first call's size, a later, larger call would fail); the launch with what this call needs (more than the ceiling: the
// launch's own error).
template <auto Kernel, class... Args>
hipError_t launch_lds_below(dim3 grid, dim3 block, int lds_ceiling, int lds_bytes, hipStream_t stream, const Args&... args) {
  const hipError_t e = lds_attr_once<Kernel>(lds_ceiling);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(Kernel, grid, block, lds_bytes, stream, args...);
  return hipGetLastError();
}
template <auto Kernel, class... Args>
hipError_t launch_lds(dim3 grid, dim3 block, int lds_bytes, hipStream_t stream, const Args&... args) {
  return launch_lds_below<Kernel>(grid, block, lds_bytes, lds_bytes, stream, args...);
}

// first_bad: THREE ints.  [0]: INT_MAX when every window / problem passes, else (index * 8 + rule) of the lowest failing index;
// [1] (windows, with CHK_PRIOR): the OR of window_prior_tp_misfit() over the windows (left alone when every prior fits);
// [2] (windows, with flags): the OR of 1 << flag over the windows whose flag is allowed
hipError_t launch_validate_windows(const avm_window_batch& b, int what, int* first_bad, hipStream_t stream, const FlagRule& fr = FlagRule());
hipError_t launch_validate_fsel(const avm_fsel_batch& b, int* first_bad, hipStream_t stream);

void launch_preint(const PreintArgs& a, hipStream_t stream);
void launch_preint_match(const PreintArgs& a, const PreintKeys& k, hipStream_t stream);  // before launch_preint with a.todo = k.todo, a.todo_count = k.count
void launch_preint_roll(const PreintRoll& r, hipStream_t stream);
hipError_t launch_fsel(const avm_fsel_batch& b, const FselBuffers& w, const avm_fsel_out& out, double* omega_out, bool run_rounds,
                       int frame_mode, const int* vflag, hipStream_t stream);
bool fsel_horizon_supported(int H);
hipError_t launch_fsel_build_cloud(const avm_window_batch& b, const double* k1_pos, const double* k1_quat, int max_cloud, int32_t* n_cloud,
                                   double* cloud_xy, double* cloud_depth, hipStream_t stream);
hipError_t launch_fsel_nn_depth(const avm_fsel_batch& b, double* kd, double* depth_out, hipStream_t stream);
size_t fsel_kd_doubles(const avm_fsel_batch& b);  // doubles of FselBuffers::kd / the kd argument above for this batch
hipError_t launch_fsel_horizon_imu(const avm_fsel_horizon_in& in, double* hor_pos, double* hor_quat, hipStream_t stream);
// zero_tic: triangulate on the camera positions themselves (visualInitialAlign, estimator.cpp:383-388); only: optional [B] device mask, windows with 0 are left alone
hipError_t launch_triangulate(const avm_window_batch& b, double init_depth, hipStream_t stream, int zero_tic = 0, const int32_t* only = nullptr);
hipError_t launch_imu_propagate(const avm_window_batch& b, const double* g, hipStream_t stream);
// flags: [B] device, or null: every window takes `flag`; remove_failures: FeatureManager::removeFailures() behind the roll
// feat_id ([B][max_feat] device, nullable): compacted with the per-feature arrays; move_td: removeFront shifts b.obs_vel_td with obs_xy
hipError_t launch_slide_window(const avm_window_batch& b, const int32_t* flags, int flag, int shift_depth, double init_depth, int remove_failures,
                               int* err, hipStream_t stream, int32_t* feat_id = nullptr, int move_td = 0);

// ---- the feature manager on device-resident tables (tracks.hip) ----------------------------------------------------------------------
// The checks write first_bad like launch_validate_windows: it stays as it was while every window passes, else min over the failing
// windows of (window * 8 + rule).  They index with n_feat / the track tables, which the caller has validated (CHK_TRACKS / CHK_IMU).
enum { TRK_BAD_NPTS = 1, TRK_BAD_IDS = 2, TRK_BAD_FULL = 3, TRK_BAD_LOST = 4, TRK_BAD_DUP = 5, TRK_CAP_FEAT = 6, TRK_CAP_OBS = 7 };  // add_image
enum { PUSH_BAD_N = 1, PUSH_CAP = 2 };                                                                                                // imu_push
enum { VIEW_CAP_FEAT = 1, VIEW_CAP_OBS = 2 };                                                                                         // solve_view
enum { DEPTH_BAD_NFEAT = 1, DEPTH_BAD_ROW = 2 };                                                                                      // store_depths
hipError_t launch_add_image_check(const avm_window_batch& b, const int32_t* feat_id, const avm_image_batch& img, int* first_bad, hipStream_t stream);
hipError_t launch_add_image(const avm_window_batch& b, int32_t* feat_id, const avm_image_batch& img, hipStream_t stream);
hipError_t launch_imu_push_check(const avm_window_batch& b, const int32_t* n, int max_in, int* first_bad, hipStream_t stream);
hipError_t launch_imu_push(const avm_window_batch& b, const int32_t* n, int max_in, const double* dt, const double* acc, const double* gyr,
                           hipStream_t stream);
hipError_t launch_solve_view_check(const avm_window_batch& full, const avm_window_batch& view, int* first_bad, hipStream_t stream);
hipError_t launch_solve_view(const avm_window_batch& full, const avm_window_batch& view, int32_t* view_row, hipStream_t stream);
hipError_t launch_store_depths_check(const avm_window_batch& full, const avm_window_batch& view, const int32_t* view_row, int* first_bad,
                                     hipStream_t stream);
hipError_t launch_store_depths(const avm_window_batch& full, const avm_window_batch& view, const int32_t* view_row, hipStream_t stream);
// FeatureManager::addFeatureCheckParallax's return value per window; last_track_num / parallax ([B][2]: sum, num) may be null
hipError_t launch_keyframe_decision(const avm_window_batch& b, double min_parallax, int32_t* flags, int32_t* last_track_num, double* parallax,
                                    hipStream_t stream);
// Estimator::failureDetection per window: failed[w] = 0, or the number of the first rule that fired
hipError_t launch_failure_detection(const avm_window_batch& b, const double* last_P, int32_t* failed, hipStream_t stream);
hipError_t launch_projection_td_eval(const avm_td_factor_batch& f, double* residual, double* jac, hipStream_t stream);
hipError_t launch_window_solve(const SolveArgs& a, hipStream_t stream);
hipError_t launch_window_solve_x(const SolveArgs& a, hipStream_t stream);  // window_solve_x.o: estimate_extrinsic / estimate_td / relocalization
int window_solve_x_lds_bytes();
hipError_t launch_window_solve_tp(const SolveArgs& a, hipStream_t stream);  // window_solve_tp.o: two 256-thread workgroups per CU (large batches)
int window_solve_tp_lds_bytes();
int window_solve_tp_occupancy();
int window_solve_tp_pattern(int* out);  // the throughput factorization's tile pattern / ownership / elimination order (tests)
int window_solve_pattern(int* out);     // ... the latency build's (the same pattern from the packed triangle, same owners)
int window_solve_x_pattern(int* out);   // ... the extended build's (twelve tile columns on eight wavefronts)
hipError_t launch_eval_factors(const EvalArgs& a, hipStream_t stream);
// scale: [n_windows][po.max_prior] device array: the magnitude every diagonal entry of A' was formed at (for launch_prior_eig's noise test)
hipError_t launch_marginalize(const SolveArgs& a, const avm_prior_out& po, int* err, double* scale, hipStream_t stream);
// window_solve_tp.o: the same marginalization as two 256-thread workgroups per CU (a.n_slots = the throughput solve's 2 x CUs slots)
hipError_t launch_marginalize_tp(const SolveArgs& a, const avm_prior_out& po, int* err, double* scale, hipStream_t stream);
// window_solve_mm.o / window_solve_tp_mm.o: the same two with the flag per window, a.marg_flags[w] (solve/marg_kernel.hpp, AVM_MARG_MIXED)
hipError_t launch_marginalize_mixed(const SolveArgs& a, const avm_prior_out& po, int* err, double* scale, hipStream_t stream);
hipError_t launch_marginalize_tp_mixed(const SolveArgs& a, const avm_prior_out& po, int* err, double* scale, hipStream_t stream);
// second half of the marginalization: eigen-decomposition of A' (left in po.J / po.r by launch_marginalize) -> sqrt prior
// noise_rel: avm_options::marg_noise_rel (0 = the reference-literal clamp S > eps and nothing else)
hipError_t launch_prior_eig(const avm_prior_out& po, int n_windows, double eps, double noise_rel, const double* scale, long long* prof,
                            int* done /* [n_windows] device scratch, may be null */, hipStream_t stream);
int window_solve_lds_bytes();

// ---- relocalization and the prior hand-over in the stream loop (relo.hip; the copy-only prior kernel: tracks.hip) ----------------------
// Every struct holds device pointers.  The checks write first_bad like the feature manager's: min over the failing windows of
// (window * 8 + rule); they run on their own, before the kernel that writes.
enum { HDR_BAD_FLAG = 1 };                                                                                             // headers_step
enum { SETRELO_BAD_NMATCH = 1, SETRELO_BAD_IDS = 2 };                                                                  // set_relo_frame
enum { RESOLVE_BAD_ROW = 1, RESOLVE_BAD_FRAME = 2, RESOLVE_BAD_NMATCH = 3, RESOLVE_BAD_VIEW_IDS = 4, RESOLVE_BAD_MATCH_IDS = 5 };  // relo_resolve
enum { FINISH_BAD_FRAME = 1 };                                                                                         // relo_finish
enum { KEEP_BAD_NBLK = 1, KEEP_CAP = 2 };                                                                              // prior_keep
struct ReloResolveArgs {
  avm_window_batch view;  // n_feat, feat_start are read (validated: CHK_TRACKS)
  const int32_t *feat_id, *view_row;
  int full_max_feat;
  avm_relo_state state;
  int32_t *relo_n, *relo_frame, *relo_feat;
  double* relo_xy;
  int32_t* n_active;  // one int, zero on entry: counts the windows with relocalization_info != 0
};
hipError_t launch_headers_step_check(int n_windows, const int32_t* flags, int* first_bad, hipStream_t stream);
hipError_t launch_headers_step(int n_windows, double* stamp, const int32_t* flags, const double* new_stamp, hipStream_t stream);
hipError_t launch_set_relo_frame_check(const avm_relo_msg_batch& msg, int* first_bad, hipStream_t stream);
hipError_t launch_set_relo_frame(const avm_window_batch& b, const double* stamp, const avm_relo_msg_batch& msg, const avm_relo_state& state,
                                 hipStream_t stream);
hipError_t launch_relo_resolve_check(const ReloResolveArgs& a, int* first_bad, hipStream_t stream);
hipError_t launch_relo_resolve(const ReloResolveArgs& a, hipStream_t stream);
hipError_t launch_relo_finish_check(int n_windows, const avm_relo_state& state, int* first_bad, hipStream_t stream);
hipError_t launch_relo_finish(const avm_window_batch& b, const avm_relo_state& state, hipStream_t stream);
// b's prior tables have passed CHK_PRIOR
hipError_t launch_prior_keep_check(const avm_window_batch& b, const avm_prior_out& po, int* first_bad, hipStream_t stream);
hipError_t launch_prior_keep(const avm_window_batch& b, const avm_prior_out& po, hipStream_t stream);

}  // namespace avm
