// solve/launch_list.hpp - the builds of the solve kernel over a list of windows (-DAVM_WIN_LIST): their launcher
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// a.win_list: [a.n_list] device (null: windows 0 .. n_list - 1), written by solve_partition_kernel or staged by the host; one workgroup
// per scratch slot, at most one per listed window.  LDS and slots as the same build without a list (launch.hpp, launch_x.hpp, launch_tp.hpp).
#if defined(AVM_X)
hipError_t launch_window_solve_x_list(const SolveListArgs& a, hipStream_t stream) {
  return launch_lds<window_solve_x_list_kernel>(a.n_list < a.n_slots ? a.n_list : a.n_slots, NT, L_END * 8, stream, a);
}
#elif defined(AVM_TP)
// workgroups of the kernel the runtime says a CU can hold (2, as window_solve_tp_kernel)
int window_solve_tp_list_occupancy() {
  int n = 0;
  (void)lds_attr_once<window_solve_tp_list_kernel>(L_END * 8);
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, window_solve_tp_list_kernel, NT, L_END * 8) != hipSuccess) return -1;
  return n;
}
hipError_t launch_window_solve_tp_list(const SolveListArgs& a, hipStream_t stream) {
  return launch_lds<window_solve_tp_list_kernel>(a.n_list < a.n_slots ? a.n_list : a.n_slots, NT, L_END * 8, stream, a);
}
#else
hipError_t launch_window_solve_list(const SolveListArgs& a, hipStream_t stream) {
  return launch_lds<window_solve_list_kernel>(a.n_list < a.n_slots ? a.n_list : a.n_slots, NT, L_END * 8, stream, a);
}
#endif
