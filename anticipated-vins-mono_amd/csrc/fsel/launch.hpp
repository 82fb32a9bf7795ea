// fsel/launch.hpp - the host side of a select: LDS sizes, the table of instantiated sizes, launch_fsel
// Part of fsel.hip, which includes it inside namespace avm, after the anonymous namespace of the kernels; no translation unit of its own.
// Every kernel with dynamic LDS goes through launch_lds / launch_lds_below (kernels.hpp): the LDS attribute once per process and kernel.

constexpr int FS_MAX_H = 13;  // the largest horizon fsel_horizon_supported (aux_kernels.hpp) accepts

constexpr size_t fsel_kdtree_lds_bytes(int max_cloud) { return (size_t)max_cloud * (2 * sizeof(double) + 3 * sizeof(int)) + KD_STACK * sizeof(KdPending) + 16; }
constexpr size_t fsel_setup_lds_bytes(int H) {
  const int N = 9 * (H + 1);
  return sizeof(double) * ((size_t)N * N + 3 * (H + 1) * 81 + (H + 1) * 30 + N + 64) + sizeof(int) * N + 16;
}
constexpr size_t fsel_setup_lds_bytes_compact(int H) {  // the candidate slices: C_h / W and the Delta tile of four wavefronts, the camera frames
  const int T = 3 * H;
  return sizeof(double) * ((size_t)(FS_NT / 64) * (FS_CPW * (6 * H + 9) + T * T) + (H + 1) * 30) + 16;
}
// These two kernels are asked for another size from call to call (max_cloud and the horizon are free per call, and the candidate slices take
// the compact carve): the attribute is set to the largest, the launch asks for what it needs - that size decides the occupancy.
constexpr int FS_KDTREE_LDS_MAX = (int)fsel_kdtree_lds_bytes(FS_MAX_CLOUD);
constexpr int FS_SETUP_LDS_MAX = (int)fsel_setup_lds_bytes(FS_MAX_H);
static_assert(FS_SETUP_LDS_MAX == 159624 && FS_SETUP_LDS_MAX <= 160 * 1024 && FS_KDTREE_LDS_MAX <= 160 * 1024, "a compute unit has 160 KB of LDS");
static_assert(fsel_setup_lds_bytes_compact(FS_MAX_H) <= FS_SETUP_LDS_MAX, "the compact carve is the smaller one");

// the kd-tree of every frame's depth cloud -> kd[P][kd_stride(max_cloud)] (what the setup kernel and fsel_nn_depth_kernel search)
static hipError_t launch_fsel_kdtree(const FselDev& d, hipStream_t stream) {
  const avm_fsel_batch& b = d.b;
  if (b.n_problems == 0 || !b.n_cloud || b.max_cloud <= 0) return hipSuccess;
  if (b.max_cloud > FS_MAX_CLOUD) return hipErrorInvalidValue;
  return launch_lds_below<fsel_kdtree_kernel>(b.n_problems, 64, FS_KDTREE_LDS_MAX, (int)fsel_kdtree_lds_bytes(b.max_cloud), stream, d);
}

// The sizes the greedy kernels are instantiated for, stated here and nowhere else: T = 3 H rows of the reduced system as NB block rows of
// BS <= 16 lanes (logdet4.hpp).  f(T, BS, NB) gets them as integral_constants, i.e. as template arguments; any other T is an error.
template <class F>
hipError_t fsel_with_size(int T, F&& f) {
  using std::integral_constant;
  switch (T) {
    case 6: return f(integral_constant<int, 6>{}, integral_constant<int, 6>{}, integral_constant<int, 1>{});
    case 9: return f(integral_constant<int, 9>{}, integral_constant<int, 9>{}, integral_constant<int, 1>{});
    case 15: return f(integral_constant<int, 15>{}, integral_constant<int, 15>{}, integral_constant<int, 1>{});
    case 30: return f(integral_constant<int, 30>{}, integral_constant<int, 15>{}, integral_constant<int, 2>{});
    case 39: return f(integral_constant<int, 39>{}, integral_constant<int, 13>{}, integral_constant<int, 3>{});
    default: return hipErrorInvalidValue;
  }
}
static_assert(3 * FS_MAX_H == 39, "the table's last row is the largest horizon");

// The switches a test or a developer sets in the environment, read on every call (tests change them between calls of one process).
// Returns AVM_FSEL_TEST_DROP: the candidate whose values never arrive in the frame kernel -> timeout -> fallback (-1: none).
static int fsel_env_switches(FselDev& d) {
  const char* nk = getenv("AVM_FSEL_NO_KEY_RULE");
  d.no_key_rule = (nk && nk[0] == '1') ? 1 : 0;
  const char* lt = getenv("AVM_FSEL_LAZY_TAU");  // (development: any value gives the same result, see fsel_solo_kernel)
  d.lazy_tau = lt ? atof(lt) : 0.95;
  const char* ls = getenv("AVM_FSEL_LAZY_STATS");
  d.lazy_stats = (ls && ls[0] == '1') ? 1 : 0;
  const char* td = getenv("AVM_FSEL_TEST_DROP");
  return td ? atoi(td) : -1;
}

static int fsel_cu_count() {  // (one device per process: include/avm.h)
  static const int ncu = [] {
    int dev = 0, v = 0;
    return (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
  }();
  return ncu;
}

// Launches setup (+ optional rounds).  All pointers in `d` are device pointers.
// frame_mode: 0 = one launch per greedy round, 1 = fsel_frame_kernel on all XCDs (a single frame), 2 = a team per XCD, 3 = fsel_solo_kernel
hipError_t launch_fsel(const avm_fsel_batch& b, const FselBuffers& w, const avm_fsel_out& out, double* omega_out, bool run_rounds,
                       int frame_mode, const int* vflag, hipStream_t stream) {
  FselDev d;
  d.b = b;
  d.vflag = vflag;
  const int test_drop = fsel_env_switches(d);
  d.delta_pk = frame_mode == 3 ? w.delta_pk : nullptr;
  d.ddiag = w.ddiag;
  d.C = w.C, d.dpp = w.dpp, d.consts = w.consts, d.delta = w.delta, d.delta_u = w.delta_u, d.valid = w.valid, d.valid_u = w.valid_u;
  d.black = w.black, d.fval = w.fval, d.ub = w.ub, d.nsel = w.nsel, d.done = w.done, d.omega_out = omega_out, d.out = out;
  d.live = w.live, d.pos = w.pos, d.nlive = w.nlive;
  d.kd = w.kd;
  hipError_t e = launch_fsel_kdtree(d, stream);  // initKDTree: the setup kernel's findNNDepth walks it
  if (e != hipSuccess) return e;
  const int P = b.n_problems, H = b.horizon, T = 3 * H;
  const int lds = (int)fsel_setup_lds_bytes(H);
  const int cand_per_wg = (FS_NT / 64) * FS_CPW;
  const int nslices = (b.max_cand + cand_per_wg - 1) / cand_per_wg;
  if (P < 16) {  // few frames: one launch, slice 0 beside the candidate slices (a single frame: 1.29 ms against 1.38 in two)
    e = launch_lds_below<fsel_setup_kernel>(dim3(P, 1 + nslices), FS_NT, FS_SETUP_LDS_MAX, lds, stream, d, 0, 0);
  } else {
    e = launch_lds_below<fsel_setup_kernel>(dim3(P, 1), FS_NT, FS_SETUP_LDS_MAX, lds, stream, d, 0, 0);
    if (e == hipSuccess && nslices > 0)
      e = launch_lds_below<fsel_setup_kernel>(dim3(P, nslices), FS_NT, FS_SETUP_LDS_MAX, (int)fsel_setup_lds_bytes_compact(H), stream, d, 1, 1);
  }
  if (e != hipSuccess || !run_rounds) return e;
  if (frame_mode == 3) {  // one workgroup per frame, lazy evaluation (fsel_solo_kernel): batches of many frames
    if (b.max_cand > FS_FRAME_MAXC || T > 39) return hipErrorInvalidValue;
    if ((e = hipMemsetAsync(w.sync, 0, sizeof(int32_t) * (FS_SYNC_HDR + 64), stream)) != hipSuccess) return e;
    const int dl = (int)((T > 30 ? sizeof(float) : sizeof(double)) * (size_t)FS_FRAME_MAXC * T);  // [T][512]
    const int gridx = std::max(1, std::min(P, fsel_cu_count()));
    return fsel_with_size(T, [&](auto t, auto bs, auto nb) { return launch_lds<fsel_solo_kernel<t, bs, nb>>(gridx, FS_SOLO_NT, dl, stream, d, w.sync); });
  }
  const int ns = (b.max_cand + FS_CPWG - 1) / FS_CPWG;  // workgroups per frame: four candidates per wavefront
  if (frame_mode != 0) {  // (every frame's rounds in one launch, see fsel_frame_kernel)
    if (b.max_cand > FS_FRAME_MAXC || b.max_features >= 4096 || (frame_mode == 1 && P != 1)) return hipErrorInvalidValue;
    // teams per XCD: 0 = one team over the whole device (a single frame), 1, or 2 when there are frames for more than eight teams
    // and two workgroups fit a compute unit's LDS (3H <= 30)
    const int tpx = frame_mode == 2 ? ((P > 8 && T <= 30) ? 2 : 1) : 0;
    if ((e = hipMemsetAsync(w.sync, 0, sizeof(int32_t) * FS_SYNC_INTS, stream)) != hipSuccess) return e;
    return fsel_with_size(T, [&](auto t, auto bs, auto nb) {
      // the Delta copies in LDS: packed lower triangles where two workgroups share a compute unit or 3H > 30, else full blocks
      const int dl = (int)sizeof(double) * FS_CPWG * ((t > 30 || tpx == 2) ? t * (t + 1) / 2 : t * t);
      const int grid = tpx ? ns * 8 * tpx : ns;
      // (fsel_frame_kernel_mf<39, 13, 3> is instantiated and never launched: tpx == 2 implies 3H <= 30)
      if (tpx == 2) return launch_lds<fsel_frame_kernel_mf<t, bs, nb>>(grid, FS_NT, dl, stream, d, w.sync, ns, test_drop);
      if (tpx == 1) return launch_lds<fsel_frame_kernel<t, bs, nb, 1>>(grid, FS_NT, dl, stream, d, w.sync, ns, test_drop);
      return launch_lds<fsel_frame_kernel<t, bs, nb, 0>>(grid, FS_NT, dl, stream, d, w.sync, ns, test_drop);
    });
  }
  hipLaunchKernelGGL(fsel_live_init_kernel, dim3(P), dim3(64), 0, stream, d);
  return fsel_with_size(T, [&](auto t, auto bs, auto nb) {
    for (int r = 0; r <= b.max_features; r++)  // launch r: the winner of round r - 1, then the values of round r
      hipLaunchKernelGGL((fsel_round_kernel<t, bs, nb>), dim3(ns, P), dim3(FS_NT), 0, stream, d, r);
    return hipGetLastError();
  });
}
