// api/window_ops.hpp - the smaller window calls: triangulate, the slide family, propagate, keyframe decision, failure detection

namespace {
// the roll: flags ([B], in `mem` space) per window, or flags == null and `flag` for every window
// feat_id ([B][max_feat] in `mem` space, nullable): avm_slide_window_tracks - the ids are compacted with the rows, and the rows of
// obs_vel_td (when the batch has them) move with those of obs_xy
int slide_window(avm_ctx* c, avm_mem mem, avm_window_batch* batch, const int32_t* flags, int32_t flag, int32_t shift_depth, double init_depth,
                 int32_t remove_failures, int32_t* feat_id = nullptr) {
  c->pk.rolled = 0, c->last_ms["preint_roll"] = 0.0f;  // (a slide that returns before its roll reports none)
  if (batch->n_windows == 0) return AVM_OK;
  // (the flags are checked with the tables, before the kernel reads either)
  const FlagRule fr{flags, (1u << AVM_MARGIN_OLD) | (1u << AVM_MARGIN_SECOND_NEW)};
  int rc = validate_windows(c, mem, batch, CHK_TRACKS | CHK_IMU, nullptr, fr, ROLL_FLAG_RULES);
  if (rc != AVM_OK) return rc;
  avm_window_batch d;
  const unsigned use = U_SLIDE | (feat_id ? U_SLIDE_TD : 0u);
  if ((rc = on_device(c, mem, WINDOWS, use, batch, &d)) != AVM_OK) return rc;
  const size_t B = batch->n_windows;
  int32_t* dfid;
  const int32_t* dflags;
  if ((rc = array_inout(c, mem, "w_feat_id", feat_id, B * batch->max_feat, &dfid)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "w_roll_flags", flags, B, &dflags)) != AVM_OK) return rc;
  int* derr = static_cast<int*>(pool_get(c, "slide_err", sizeof(int)));
  if (!derr) return fail(c, AVM_ERR_HIP, "hipMalloc failed (slide flag)");
  HIPCHK(c, hipMemsetAsync(derr, 0, sizeof(int), c->stream));
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_slide_window(d, dflags, flag, shift_depth, init_depth, remove_failures, derr, c->stream, dfid, feat_id ? 1 : 0));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = roll_preint_cache(c, d, dflags, flag)) != AVM_OK) return rc;
  int herr = 0;
  HIPCHK(c, hipMemcpyAsync(&herr, derr, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if ((rc = copy_back(c, mem, WINDOWS, use, batch, &d, batch)) != AVM_OK) return rc;  // (everything the roll rewrites)
  if ((rc = array_back(c, mem, feat_id, dfid, B * batch->max_feat)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  store_elapsed(c, "slide_window", M_KERNELS, M_KERNELS_END);
  if (c->pk.rolled) store_elapsed(c, "preint_roll", M_ROLL, M_ROLL_END);
  if (herr) return fail(c, AVM_ERR_CAPACITY, "MARGIN_SECOND_NEW: interval 8 + interval 9 exceed max_samp samples");
  return AVM_OK;
}
}  // namespace

extern "C" {
int avm_triangulate_batch(avm_ctx* c, avm_mem mem, avm_window_batch* batch, double init_depth) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!batch || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  int rc = check_wide_strides(c, batch);  // (the API's table contract: the kernel runs one thread per feature, any count)
  if (rc != AVM_OK) return rc;
  if (batch->n_windows == 0) return AVM_OK;
  if ((rc = validate_windows(c, mem, batch, CHK_TRACKS)) != AVM_OK) return rc;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_TRI, batch, &d)) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_triangulate(d, init_depth, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = copy_back(c, mem, WINDOWS, U_TRI, batch, &d, batch)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  store_elapsed(c, "triangulate", M_KERNELS, M_KERNELS_END);
  return AVM_OK;
}

int avm_slide_window(avm_ctx* c, avm_mem mem, avm_window_batch* batch, int32_t flag, int32_t shift_depth, double init_depth) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!batch || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (flag != AVM_MARGIN_OLD && flag != AVM_MARGIN_SECOND_NEW) return fail(c, AVM_ERR_INVALID, "marginalization_flag must be MARGIN_OLD or MARGIN_SECOND_NEW");
  return slide_window(c, mem, batch, nullptr, flag, shift_depth, init_depth, 0);
}

int avm_slide_window_flags(avm_ctx* c, avm_mem mem, avm_window_batch* batch, const int32_t* flags, int32_t shift_depth, double init_depth,
                           int32_t remove_failures) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!batch || !flags || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  return slide_window(c, mem, batch, flags, AVM_MARGIN_OLD, shift_depth, init_depth, remove_failures);
}

int avm_slide_window_tracks(avm_ctx* c, avm_mem mem, avm_window_batch* batch, int32_t* feat_id, const int32_t* flags, int32_t shift_depth,
                            double init_depth, int32_t remove_failures) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!batch || !feat_id || !flags || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  return slide_window(c, mem, batch, flags, AVM_MARGIN_OLD, shift_depth, init_depth, remove_failures, feat_id);
}

int avm_imu_propagate_batch(avm_ctx* c, avm_mem mem, avm_window_batch* batch, const double g[3]) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!batch || !g || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (batch->n_windows == 0) return AVM_OK;
  int rc = validate_windows(c, mem, batch, CHK_IMU);
  if (rc != AVM_OK) return rc;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_PROP, batch, &d)) != AVM_OK) return rc;
  HIPCHK(c, launch_imu_propagate(d, g, c->stream));
  if ((rc = copy_back(c, mem, WINDOWS, U_PROP, batch, &d, batch)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

int avm_keyframe_decision_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* batch, double min_parallax, int32_t* flags, int32_t* last_track_num,
                                double* parallax) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!batch || !flags || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (!batch->obs_xy) return fail(c, AVM_ERR_INVALID, "null obs_xy");
  int rc = check_wide_strides(c, batch);  // (the API's table contract: the kernel walks the list in chunks, any count)
  if (rc != AVM_OK) return rc;
  if (batch->n_windows == 0) return AVM_OK;
  if ((rc = validate_windows(c, mem, batch, CHK_TRACKS)) != AVM_OK) return rc;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_KEYF, batch, &d)) != AVM_OK) return rc;
  const size_t B = batch->n_windows;
  int32_t *dflags, *dltn;
  double* dpar;
  if ((rc = array_out(c, mem, "k_flags", flags, B, &dflags, "keyframe decision out")) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "k_ltn", last_track_num, B, &dltn, "keyframe decision out")) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "k_par", parallax, B * 2, &dpar, "keyframe decision out")) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_keyframe_decision(d, min_parallax, dflags, dltn, dpar, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = array_back(c, mem, flags, dflags, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, last_track_num, dltn, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, parallax, dpar, B * 2)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  store_elapsed(c, "keyframe_decision", M_KERNELS, M_KERNELS_END);
  return AVM_OK;
}

int avm_failure_detection_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* batch, const double* last_P, int32_t* failed) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!batch || !last_P || !failed || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (!batch->pose || !batch->speedbias) return fail(c, AVM_ERR_INVALID, "null pose / speedbias");
  if (batch->n_windows == 0) return AVM_OK;
  int rc;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_FAIL, batch, &d)) != AVM_OK) return rc;
  const size_t B = batch->n_windows;
  const double* dlp;
  int32_t* dfailed;
  if ((rc = array_in(c, mem, "fd_last_P", last_P, B * 3, &dlp)) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "fd_failed", failed, B, &dfailed, "failure detection out")) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_failure_detection(d, dlp, dfailed, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = array_back(c, mem, failed, dfailed, B)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  store_elapsed(c, "failure_detection", M_KERNELS, M_KERNELS_END);
  return AVM_OK;
}
}  // extern "C"
