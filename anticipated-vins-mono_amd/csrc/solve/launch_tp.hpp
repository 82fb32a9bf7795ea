// solve/launch_tp.hpp - throughput build: launchers and test exports
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
int window_solve_tp_lds_bytes() { return L_END * 8; }
// the factorization's compile-time tables for the tests (tests/test_tp_pattern.py states them in numpy): out[0..120] = TPP.h, [121..241] = TPP.nz
// (both [k][i]), [242..252] = tp_owner, [253 ..] = tp_perm of the 176 positions (-1: padding)
int window_solve_tp_pattern(int* out) { return tp_pattern_export(out); }
// workgroups of the throughput kernel the runtime says a CU can hold (2 is what the kernel is built for)
int window_solve_tp_occupancy() {
  int n = 0;
  (void)lds_attr_once<window_solve_tp_kernel>(L_END * 8);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, window_solve_tp_kernel, NT, L_END * 8) != hipSuccess) return -1;
  return n;
}

// Throughput form of the solve (window_solve_tp.o): two 256-thread workgroups per CU, a.n_slots = 2 x CUs scratch slots.
// (launch_lds: the LDS attribute once per process, a failure to set it remembered - kernels.hpp)
hipError_t launch_window_solve_tp(const SolveArgs& a, hipStream_t stream) {
  return launch_lds<window_solve_tp_kernel>(a.b.n_windows < a.n_slots ? a.b.n_windows : a.n_slots, NT, L_END * 8, stream, a);
}

// Throughput form of the marginalization: two 256-thread workgroups per CU, a.n_slots = 2 x CUs scratch slots (the solve's)
hipError_t launch_marginalize_tp(const SolveArgs& a, const avm_prior_out& po, int* err, double* scale, hipStream_t stream) {
  return launch_lds<marginalize_tp_kernel>(a.b.n_windows < a.n_slots ? a.b.n_windows : a.n_slots, NT, L_END * 8, stream, a, po, err, scale);
}
