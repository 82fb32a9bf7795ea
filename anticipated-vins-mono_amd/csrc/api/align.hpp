// api/align.hpp - avm_visual_initial_align_batch

extern "C" {
int avm_visual_initial_align_batch(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_align_batch* al, avm_window_batch* win,
                                   avm_align_out* out) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!opt || !al || !out || al->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (al->max_frames > AVM_MAX_ALIGN_FRAMES) return fail(c, AVM_ERR_CAPACITY, "max_frames > 64 (AVM_MAX_ALIGN_FRAMES)");
  if (c->max_windows > 0 && al->n_windows > c->max_windows) return fail(c, AVM_ERR_CAPACITY, "more windows than avm_config::max_windows");
  if (al->max_frames < 2 || al->max_samp < 0) return fail(c, AVM_ERR_INVALID, "max_frames < 2 or max_samp < 0");
  for (const Field& f : ALIGN)
    if (!get_ptr(al, f) && (win || f.offset != offsetof(avm_align_batch, key_index))) return fail(c, AVM_ERR_INVALID, "a table of avm_align_batch is NULL");
  if (!out->ok || !out->delta_bg || !out->g_c0 || !out->x || (win && !out->g_world))
    return fail(c, AVM_ERR_INVALID, "avm_align_out: ok, delta_bg, g_c0, x (and g_world with windows) must be given");
  int rc;
  if (win) {
    if (win->n_windows != al->n_windows) return fail(c, AVM_ERR_INVALID, "windows->n_windows differs from align->n_windows");
    if (!win->pose || !win->speedbias || !win->ex_pose || !win->inv_depth || !win->obs_xy) return fail(c, AVM_ERR_INVALID, "null state array of the window batch");
    if ((rc = check_wide_strides(c, win)) != AVM_OK) return rc;
  }
  if (al->n_windows == 0) return AVM_OK;
  // table checks, before any kernel indexes with them
  if (mem == AVM_MEM_HOST) {
    for (int b = 0; b < al->n_windows; b++) {
      const int rule = check_align_tables(*al, b, win != nullptr);
      if (rule) return report_bad(c, b * 8 + rule, "window", ALIGN_RULES);
    }
  } else {
    FlagCheck f;
    if ((rc = flag_begin(c, 1, [&](int* flag) { return launch_validate_align(*al, win != nullptr, flag, c->stream); }, &f)) != AVM_OK) return rc;
    if ((rc = flag_end(c, f, "window", ALIGN_RULES)) != AVM_OK) return rc;
  }
  if (win && (rc = validate_windows(c, mem, win, CHK_TRACKS)) != AVM_OK) return rc;

  AlignArgs aa;
  std::memset(&aa.w, 0, sizeof aa.w);
  if ((rc = on_device(c, mem, ALIGN, U_WHOLE, al, &aa.a)) != AVM_OK) return rc;
  if (win && (rc = on_device(c, mem, WINDOWS, U_ALIGN, win, &aa.w)) != AVM_OK) return rc;
  aa.has_windows = win ? 1 : 0;
  aa.g_norm = std::sqrt(opt->g[0] * opt->g[0] + opt->g[1] * opt->g[1] + opt->g[2] * opt->g[2]);
  avm_align_out want = *out;  // what this call returns: g_world only with windows
  if (!win) want.g_world = nullptr;
  aa.out = want;
  if (mem == AVM_MEM_HOST && alloc_out(c, ALIGN_OUT, &want, &aa.out, al) != AVM_OK) return fail(c, AVM_ERR_HIP, "hipMalloc failed (align out)");
  const size_t n_iv = (size_t)al->n_windows * (al->max_frames - 1);
  aa.delta = aa.out.deltas ? aa.out.deltas : static_cast<double*>(pool_get(c, "al_delta", sizeof(double) * n_iv * 10));
  aa.sum_dt = static_cast<double*>(pool_get(c, "al_sum_dt", sizeof(double) * n_iv));
  if (!aa.delta || !aa.sum_dt) return fail(c, AVM_ERR_HIP, "hipMalloc failed (align pre-integrations)");
  // (the rows of intervals beyond n_frames - 1 are never written by the kernels: defined values for the caller)
  HIPCHK(c, hipMemsetAsync(aa.delta, 0, sizeof(double) * n_iv * 10, c->stream));

  HIPCHK(c, mark(c, M_ALIGN_GYRO_BIAS));
  HIPCHK(c, launch_align_gyro_bias(aa, c->stream));
  HIPCHK(c, mark(c, M_ALIGN_SOLVE));
  HIPCHK(c, launch_align_solve(aa, c->stream));
  HIPCHK(c, mark(c, M_ALIGN_APPLY));
  if (win) {
    HIPCHK(c, launch_align_prepare(aa, c->stream));
    HIPCHK(c, launch_triangulate(aa.w, 5.0 /* INIT_DEPTH, parameters.cpp:113 */, c->stream, 1, aa.out.ok));
    HIPCHK(c, launch_align_apply(aa, c->stream));
  }
  HIPCHK(c, mark(c, M_ALIGN_END));
  if (win && (rc = copy_back(c, mem, WINDOWS, U_ALIGN, win, &aa.w, win)) != AVM_OK) return rc;
  if ((rc = copy_back(c, mem, ALIGN_OUT, U_WHOLE, &want, &aa.out, al)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  store_elapsed(c, "align_gyro_bias", M_ALIGN_GYRO_BIAS, M_ALIGN_SOLVE);
  store_elapsed(c, "align_solve", M_ALIGN_SOLVE, M_ALIGN_APPLY);
  store_elapsed(c, "align_apply", M_ALIGN_APPLY, M_ALIGN_END);
  return AVM_OK;
}
}  // extern "C"
