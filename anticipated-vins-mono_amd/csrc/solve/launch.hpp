// solve/launch.hpp - latency build: launchers and test exports
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
int window_solve_lds_bytes() { return L_END * 8; }
int window_solve_pattern(int* out) { return tp_pattern_export(out); }

// one workgroup per scratch slot, at most one per window (launch_lds: the LDS attribute once per process, a failure to set it remembered - kernels.hpp)
hipError_t launch_window_solve(const SolveArgs& a, hipStream_t stream) {
  return launch_lds<window_solve_kernel>(a.b.n_windows < a.n_slots ? a.b.n_windows : a.n_slots, NT, L_END * 8, stream, a);
}

hipError_t launch_marginalize(const SolveArgs& a, const avm_prior_out& po, int* err, double* scale, hipStream_t stream) {
  return launch_lds<marginalize_kernel>(a.b.n_windows < a.n_slots ? a.b.n_windows : a.n_slots, NT, L_END * 8, stream, a, po, err, scale);
}

hipError_t launch_eval_factors(const EvalArgs& a, hipStream_t stream) {
  return launch_lds<eval_factors_kernel>(a.b.n_windows, NT, L_END * 8, stream, a);
}
