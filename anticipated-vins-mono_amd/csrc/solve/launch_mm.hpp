// solve/launch_mm.hpp - the builds with the marginalization flag per window (-DAVM_MARG_MIXED): their launcher
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// a.marg_flags: [B] device, checked by the caller; grid and slots as the marginalization of the same form with one flag (launch.hpp, launch_tp.hpp)
#ifdef AVM_TP
hipError_t launch_marginalize_tp_mixed(const SolveArgs& a, const avm_prior_out& po, int* err, double* scale, hipStream_t stream) {
  return launch_lds<marginalize_tp_mixed_kernel>(a.b.n_windows < a.n_slots ? a.b.n_windows : a.n_slots, NT, L_END * 8, stream, a, po, err, scale);
}
#else
hipError_t launch_marginalize_mixed(const SolveArgs& a, const avm_prior_out& po, int* err, double* scale, hipStream_t stream) {
  return launch_lds<marginalize_mixed_kernel>(a.b.n_windows < a.n_slots ? a.b.n_windows : a.n_slots, NT, L_END * 8, stream, a, po, err, scale);
}
#endif
