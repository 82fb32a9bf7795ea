// api/debug.hpp - the avm_debug_* hooks (not in avm.h)

extern "C" {
// debug hook (not in avm.h): per-phase shader clocks of the last solve, summed over slots, [PROF_SLOTS = 64]
int avm_debug_copy_profile(avm_ctx* c, long long* host_out) {
  if (!c || !c->prof) return AVM_ERR_INVALID;
  std::vector<long long> h((size_t)PROF_SLOTS * 2 * c->n_slots);
  HIPCHK(c, hipMemcpy(h.data(), c->prof, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < PROF_SLOTS; k++) host_out[k] = 0;
  for (int s = 0; s < 2 * c->n_slots; s++)
    for (int k = 0; k < PROF_SLOTS; k++) host_out[k] += h[(size_t)s * PROF_SLOTS + k];
  return AVM_OK;
}

// test / bench hook (not in avm.h): 1 when the last avm_window_solve_batch ran the throughput form of the solve kernel
int avm_debug_last_solve_form(const avm_ctx* c) { return c ? (c->last_solve_tp ? 1 : 0) : -1; }
// ... 1 when its marginalization ran the throughput form (marginalize_tp_kernel: two 256-thread workgroups per CU)
int avm_debug_last_marg_form(const avm_ctx* c) { return c ? (c->last_marg_tp ? 1 : 0) : -1; }
// ... how it split the batch (avm_window_solve_batch_relo): out[0] = windows solved as plain ones, out[1] = windows that took the extended kernel,
// out[2] = the plain ones' form (0 latency, 1 throughput, -1 there were none), out[3] = 1 when the list builds of the kernels ran
int avm_debug_last_split(const avm_ctx* c, int64_t* out) {
  if (!c || !out) return AVM_ERR_INVALID;
  for (int k = 0; k < 4; k++) out[k] = c->last_split[k];
  return AVM_OK;
}
// ... and which form the last avm_fsel_select_batch STARTED in: 3 = one workgroup per frame with lazy evaluation (fsel_solo_kernel), 2 / 1 = the
// frame kernel's teams, 0 = one launch per greedy round
int avm_debug_last_fsel_form(const avm_ctx* c) { return c ? c->last_fsel_mode : -1; }

// test / bench hook (not in avm.h): out[0] = workgroups of the throughput kernel per CU (runtime's occupancy query), out[1] = its LDS bytes
int avm_debug_solve_tp_occupancy(int* out) {
  out[0] = window_solve_tp_occupancy(), out[1] = window_solve_tp_lds_bytes();
  return 2;
}

// ... and of its build over a window list (window_solve_tp_list_kernel): out[0] = workgroups per CU
int avm_debug_solve_tp_list_occupancy(int* out) {
  out[0] = window_solve_tp_list_occupancy();
  return 1;
}

// test hook (not in avm.h): the compile-time tables of the throughput solve's sparse factorization (solve/chol_regs_tables.hpp; exported by solve/chol_regs.hpp); out: >= 512 ints
// which = 0: throughput build, 1: latency build, 2: extended build
int avm_debug_solve_pattern(int which, int* out) {
  return which == 0 ? window_solve_tp_pattern(out) : (which == 1 ? window_solve_pattern(out) : window_solve_x_pattern(out));
}
int avm_debug_solve_tp_pattern(int* out) { return avm_debug_solve_pattern(0, out); }

// test / bench hook (not in avm.h): out[0] = device / pinned (re)allocations of this ctx so far, out[1] = windows of the last
// marginalization whose square root the one-wavefront kernel (prior_chol_kernel) finished, out[2] = windows of that marginalization
// (out[2] - out[1] went through prior_eig_kernel's pivoted path), out[3] = 1 if the last solve took the throughput form
int avm_debug_counters(avm_ctx* c, int64_t* out) {
  if (!c || !out) return AVM_ERR_INVALID;
  out[0] = c->n_allocs, out[1] = 0, out[2] = c->last_marg_windows, out[3] = c->last_solve_tp ? 1 : 0;
  auto it = c->pool.find("pe_done");
  if (c->last_marg_windows > 0 && it != c->pool.end() && it->second.first) {
    std::vector<int> h((size_t)c->last_marg_windows);
    HIPCHK(c, hipMemcpy(h.data(), it->second.first, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
    for (int v : h) out[1] += v != 0;
  }
  return AVM_OK;
}

// test / bench hook (not in avm.h): out[0] = intervals the last pre-integration examined, out[1] = intervals it integrated (all of them
// with AVM_PREINT_CACHE=0), out[2] = windows whose cached pre-integrations the last avm_slide_window* rolled (0: it left the cache alone)
int avm_debug_preint_cache(avm_ctx* c, int64_t* out) {
  if (!c || !out) return AVM_ERR_INVALID;
  out[0] = c->pk.examined, out[1] = c->pk.recomputed, out[2] = c->pk.rolled;
  if (c->pk.recomputed < 0 && c->pk.last_count) {
    int32_t n = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&n, c->pk.last_count, sizeof n, hipMemcpyDeviceToHost));
    out[1] = n;
  }
  return AVM_OK;
}

// bench hook (not in avm.h): candidate evaluations the last avm_fsel_select_batch executed on the device - counted by fsel_solo_kernel
// (the lazy form scores a fraction of the live candidates per round); -1 for the forms that score every live candidate every round
int avm_debug_fsel_evaluations(avm_ctx* c, int64_t* out) {
  if (!c || !out) return AVM_ERR_INVALID;
  *out = c->last_fsel_evals;
  return AVM_OK;
}

// test hook (not in avm.h): the table sizes of avm.h as this library was compiled with them, for the ctypes mirror check
int avm_debug_table_limits(int* out) {
  out[0] = AVM_MAX_FEAT, out[1] = AVM_MAX_OBS, out[2] = AVM_MAX_FEAT_WIDE, out[3] = AVM_MAX_OBS_WIDE;
  return 4;
}

// test hook (not in avm.h): sizeof of every ABI struct, for the ctypes mirror check
int avm_debug_struct_sizes(int* out) {
  out[0] = (int)sizeof(avm_options), out[1] = (int)sizeof(avm_window_batch), out[2] = (int)sizeof(avm_prior_out);
  out[3] = (int)sizeof(avm_solve_summary), out[4] = (int)sizeof(avm_fsel_batch), out[5] = (int)sizeof(avm_fsel_out);
  out[6] = (int)sizeof(avm_config);
  return 7;
}

// test hook (not in avm.h): sizeof and the member offsets of avm_image_batch, and AVM_MAX_IMAGE_PTS, for the ctypes mirror check; out: >= 8 ints
int avm_debug_track_struct_sizes(int* out) {
  int n = 0;
  out[n++] = (int)sizeof(avm_image_batch), out[n++] = AVM_MAX_IMAGE_PTS;
  for (size_t o : {offsetof(avm_image_batch, n_windows), offsetof(avm_image_batch, max_pts), offsetof(avm_image_batch, n_pts),
                   offsetof(avm_image_batch, feature_id), offsetof(avm_image_batch, xy), offsetof(avm_image_batch, vel_td)})
    out[n++] = (int)o;
  return n;
}

// test hook (not in avm.h): sizeof of avm_relo_msg_batch / avm_relo_state and the offsets of their first and last pointer members, for the
// ctypes mirror check; out: >= 6 ints
int avm_debug_relo_struct_sizes(int* out) {
  int n = 0;
  out[n++] = (int)sizeof(avm_relo_msg_batch), out[n++] = (int)sizeof(avm_relo_state);
  for (size_t o : {offsetof(avm_relo_msg_batch, has_msg), offsetof(avm_relo_msg_batch, prev_relo_q), offsetof(avm_relo_state, relocalization_info),
                   offsetof(avm_relo_state, relo_relative_yaw)})
    out[n++] = (int)o;
  return n;
}

// test hook (not in avm.h): sizeof and the member offsets of avm_align_batch / avm_align_out, for the ctypes mirror check; out: >= 23 ints
int avm_debug_align_layout(int* out) {
  int n = 0;
  out[n++] = (int)sizeof(avm_align_batch), out[n++] = (int)sizeof(avm_align_out), out[n++] = AVM_MAX_ALIGN_FRAMES;
  for (size_t o : {offsetof(avm_align_batch, n_windows), offsetof(avm_align_batch, max_frames), offsetof(avm_align_batch, max_samp),
                   offsetof(avm_align_batch, n_frames), offsetof(avm_align_batch, frame_R), offsetof(avm_align_batch, frame_T),
                   offsetof(avm_align_batch, tic), offsetof(avm_align_batch, imu_n), offsetof(avm_align_batch, imu_dt),
                   offsetof(avm_align_batch, imu_acc), offsetof(avm_align_batch, imu_gyr), offsetof(avm_align_batch, imu_lin_ba),
                   offsetof(avm_align_batch, imu_lin_bg), offsetof(avm_align_batch, key_index), offsetof(avm_align_out, ok),
                   offsetof(avm_align_out, delta_bg), offsetof(avm_align_out, g_c0), offsetof(avm_align_out, x),
                   offsetof(avm_align_out, g_world), offsetof(avm_align_out, deltas)})
    out[n++] = (int)o;
  return n;
}

// test hook (not in avm.h): sqrt_info of the last pre-integration, [B][10][15][15]
int avm_debug_copy_sqrt_info(avm_ctx* c, int n_windows, double* host_out) {
  if (!c || !c->pre_sqrt) return AVM_ERR_INVALID;
  HIPCHK(c, hipMemcpy(host_out, c->pre_sqrt, sizeof(double) * (size_t)n_windows * 2250, hipMemcpyDeviceToHost));
  return AVM_OK;
}
}  // extern "C"
