// solve/launch_x.hpp - extended build: launcher and test exports
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
int window_solve_x_lds_bytes() { return L_END * 8; }
int window_solve_x_pattern(int* out) { return tp_pattern_export(out); }

// the solve with ex_pose / td / relo_Pose as (optional) variables: 178 x 178 reduced system
// (launch_lds: the LDS attribute once per process, a failure to set it remembered - kernels.hpp)
hipError_t launch_window_solve_x(const SolveArgs& a, hipStream_t stream) {
  return launch_lds<window_solve_x_kernel>(a.b.n_windows < a.n_slots ? a.b.n_windows : a.n_slots, NT, L_END * 8, stream, a);
}
