// api/tracks.hpp - the feature manager on device-resident tables (tracks.hip): add_image, imu_push, solve_view, store_depths

namespace {
const Rule ADD_IMAGE_RULES[8] = {
    {AVM_ERR_INVALID, "bad table"},
    {AVM_ERR_INVALID, "n_pts outside [0, max_pts]"},
    {AVM_ERR_INVALID, "the image's feature ids must be strictly ascending (std::map order)"},
    {AVM_ERR_INVALID, "a track already has an observation in frame 10 (feat_start + feat_nobs > 10)"},
    {AVM_ERR_INVALID, "an image id matches a track whose last observation is not in frame 9 (a lost id was issued again)"},
    {AVM_ERR_INVALID, "duplicate id in feat_id[0 .. n_feat)"},
    {AVM_ERR_CAPACITY, "n_feat + new tracks > max_feat"},
    {AVM_ERR_CAPACITY, "the observations do not fit max_obs"}};
const Rule IMU_PUSH_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                {AVM_ERR_INVALID, "n outside [0, max_in]"},
                                {AVM_ERR_CAPACITY, "interval 9 + the new samples exceed max_samp samples"}};
const Rule SOLVE_VIEW_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                  {AVM_ERR_CAPACITY, "more rows pass the solve's filter than view->max_feat"},
                                  {AVM_ERR_CAPACITY, "the observations of the rows that pass the solve's filter do not fit view->max_obs"}};
const Rule STORE_DEPTHS_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                    {AVM_ERR_INVALID, "n_feat outside [0, max_feat] (full or view)"},
                                    {AVM_ERR_INVALID, "view_row must be strictly increasing inside [0, full n_feat)"}};

// check + kernels of the call that just synchronized
void record_track_ms(avm_ctx* c, const char* key) { store_elapsed(c, key, M_CHECK, M_CHECK_END, M_KERNELS, M_KERNELS_END); }
}  // namespace

extern "C" {
int avm_add_image_batch(avm_ctx* c, avm_mem mem, avm_window_batch* win, int32_t* feat_id, const avm_image_batch* img, double min_parallax,
                        int32_t* flags_out, int32_t* last_track_num, double* parallax) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!win || !feat_id || !img || !flags_out || win->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (img->n_windows != win->n_windows) return fail(c, AVM_ERR_INVALID, "image->n_windows differs from windows->n_windows");
  if (img->max_pts < 0) return fail(c, AVM_ERR_INVALID, "max_pts < 0");
  if (img->max_pts > AVM_MAX_IMAGE_PTS) return fail(c, AVM_ERR_CAPACITY, "max_pts > 1024 (AVM_MAX_IMAGE_PTS)");
  if (!img->n_pts || (img->max_pts > 0 && (!img->feature_id || !img->xy))) return fail(c, AVM_ERR_INVALID, "null image table");
  if (!win->obs_xy || !win->inv_depth) return fail(c, AVM_ERR_INVALID, "null obs_xy / inv_depth");
  if ((win->obs_vel_td != nullptr) != (img->vel_td != nullptr))
    return fail(c, AVM_ERR_INVALID, "image->vel_td must be given if and only if windows->obs_vel_td is");
  int rc = check_wide_strides(c, win);
  if (rc != AVM_OK) return rc;
  if (win->n_windows == 0) return AVM_OK;
  if ((rc = validate_windows(c, mem, win, CHK_TRACKS)) != AVM_OK) return rc;
  const size_t B = win->n_windows;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_TRK, win, &d)) != AVM_OK) return rc;
  avm_image_batch di;
  if ((rc = on_device(c, mem, IMAGE, U_TRK, img, &di, nullptr, nullptr, "ai_")) != AVM_OK) return rc;
  int32_t *dfid, *dflags, *dltn;
  double* dpar;
  if ((rc = array_inout(c, mem, "w_feat_id", feat_id, B * win->max_feat, &dfid)) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "k_flags", flags_out, B, &dflags)) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "k_ltn", last_track_num, B, &dltn)) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "k_par", parallax, B * 2, &dpar)) != AVM_OK) return rc;
  if ((rc = track_check(c, [&](int* flag) { return launch_add_image_check(d, dfid, di, flag, c->stream); }, ADD_IMAGE_RULES)) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_add_image(d, dfid, di, c->stream));
  HIPCHK(c, launch_keyframe_decision(d, min_parallax, dflags, dltn, dpar, c->stream));  // (the decision of avm_keyframe_decision_batch, on the result)
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = copy_back(c, mem, WINDOWS, U_TRK, win, &d, win)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, feat_id, dfid, B * win->max_feat)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, flags_out, dflags, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, last_track_num, dltn, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, parallax, dpar, B * 2)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "add_image");
  return AVM_OK;
}

int avm_imu_push_batch(avm_ctx* c, avm_mem mem, avm_window_batch* win, const int32_t* n, int32_t max_in, const double* dt, const double* acc,
                       const double* gyr) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!win || !n || win->n_windows < 0 || max_in < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (max_in > 0 && (!dt || !acc || !gyr)) return fail(c, AVM_ERR_INVALID, "null sample array");
  if (!win->imu_dt || !win->imu_acc || !win->imu_gyr) return fail(c, AVM_ERR_INVALID, "null IMU table");
  if (win->n_windows == 0) return AVM_OK;
  int rc = validate_windows(c, mem, win, CHK_IMU);
  if (rc != AVM_OK) return rc;
  const size_t B = win->n_windows, M = (size_t)max_in;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_PUSH, win, &d)) != AVM_OK) return rc;
  const int32_t* dn;
  const double *ddt, *dacc, *dgyr;
  if ((rc = array_in(c, mem, "ip_n", n, B, &dn)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "ip_dt", dt, B * M, &ddt)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "ip_acc", acc, B * M * 3, &dacc)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "ip_gyr", gyr, B * M * 3, &dgyr)) != AVM_OK) return rc;
  if ((rc = track_check(c, [&](int* flag) { return launch_imu_push_check(d, dn, max_in, flag, c->stream); }, IMU_PUSH_RULES)) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_imu_push(d, dn, max_in, ddt, dacc, dgyr, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = copy_back(c, mem, WINDOWS, U_PUSH, win, &d, win)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "imu_push");
  return AVM_OK;
}

int avm_solve_view_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* full, avm_window_batch* view, int32_t* view_row) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!full || !view || !view_row || full->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (view->n_windows != full->n_windows) return fail(c, AVM_ERR_INVALID, "view->n_windows differs from full->n_windows");
  if (view->max_feat < 0 || view->max_obs < 0) return fail(c, AVM_ERR_INVALID, "negative view stride");
  if (view->max_feat > MAXE) return fail(c, AVM_ERR_CAPACITY, "view->max_feat > 150");
  if (view->max_obs > MAXOBS) return fail(c, AVM_ERR_CAPACITY, "view->max_obs > 1650");
  if (!full->obs_xy || !full->inv_depth) return fail(c, AVM_ERR_INVALID, "null obs_xy / inv_depth");
  if (!view->n_feat || !view->feat_start || !view->feat_nobs || !view->feat_obs_begin || !view->obs_xy || !view->inv_depth)
    return fail(c, AVM_ERR_INVALID, "null view table");
  if (view->obs_vel_td && !full->obs_vel_td) return fail(c, AVM_ERR_INVALID, "view->obs_vel_td is given but full->obs_vel_td is not");
  if (view->n_feat == full->n_feat || view->feat_start == full->feat_start || view->feat_nobs == full->feat_nobs ||
      view->feat_obs_begin == full->feat_obs_begin || view->obs_xy == full->obs_xy || view->inv_depth == full->inv_depth ||
      (view->obs_vel_td && view->obs_vel_td == full->obs_vel_td))
    return fail(c, AVM_ERR_INVALID, "the view's track tables must not be the full tables' own arrays");
  int rc = check_wide_strides(c, full);
  if (rc != AVM_OK) return rc;
  if (full->n_windows == 0) return AVM_OK;
  if ((rc = validate_windows(c, mem, full, CHK_TRACKS)) != AVM_OK) return rc;
  const size_t B = full->n_windows;
  avm_window_batch df, dv;
  if ((rc = on_device(c, mem, WINDOWS, U_TRK, full, &df)) != AVM_OK) return rc;
  // (the view's arrays travel in as well: the slots the gather does not write keep what they held)
  if ((rc = on_device(c, mem, WINDOWS, U_TRK, view, &dv, nullptr, nullptr, "v_")) != AVM_OK) return rc;
  int32_t* drow;
  if ((rc = array_out(c, mem, "v_row", view_row, B * view->max_feat, &drow)) != AVM_OK) return rc;
  if (mem == AVM_MEM_HOST && view->max_feat > 0)
    HIPCHK(c, hipMemcpyAsync(drow, view_row, sizeof(int32_t) * B * view->max_feat, hipMemcpyHostToDevice, c->stream));
  if ((rc = track_check(c, [&](int* flag) { return launch_solve_view_check(df, dv, flag, c->stream); }, SOLVE_VIEW_RULES)) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_solve_view(df, dv, drow, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = copy_back(c, mem, WINDOWS, U_TRK, view, &dv, view)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, view_row, drow, B * view->max_feat)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "solve_view");
  return AVM_OK;
}

int avm_solve_view_store_depths(avm_ctx* c, avm_mem mem, avm_window_batch* full, const avm_window_batch* view, const int32_t* view_row) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!full || !view || !view_row || full->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (view->n_windows != full->n_windows) return fail(c, AVM_ERR_INVALID, "view->n_windows differs from full->n_windows");
  if (view->max_feat < 0 || full->max_feat < 0) return fail(c, AVM_ERR_INVALID, "negative stride");
  if (!full->n_feat || !full->inv_depth || !view->n_feat || !view->inv_depth) return fail(c, AVM_ERR_INVALID, "null n_feat / inv_depth");
  if (full->n_windows == 0) return AVM_OK;
  int rc;
  const size_t B = full->n_windows;
  avm_window_batch df, dv;
  if ((rc = on_device(c, mem, WINDOWS, U_DEPTH, full, &df)) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, WINDOWS, U_DEPTH, view, &dv, nullptr, nullptr, "v_")) != AVM_OK) return rc;
  const int32_t* drow;
  if ((rc = array_in(c, mem, "v_row", view_row, B * view->max_feat, &drow)) != AVM_OK) return rc;
  if ((rc = track_check(c, [&](int* flag) { return launch_store_depths_check(df, dv, drow, flag, c->stream); }, STORE_DEPTHS_RULES)) != AVM_OK)
    return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_store_depths(df, dv, drow, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = copy_back(c, mem, WINDOWS, U_DEPTH, full, &df, full)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "store_depths");
  return AVM_OK;
}
}  // extern "C"
