// api/sfm.hpp - avm_global_sfm_batch (include/avm_init.h)
// Every buffer of a call comes from pool_get by name and size, every pointer is taken again in every call: a second call of another size
// is an ordinary event.

extern "C" {
int avm_global_sfm_batch(avm_ctx* c, avm_mem mem, const avm_sfm_batch* sfm, const avm_window_batch* full, const int32_t* feat_id,
                         avm_sfm_out* out) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!sfm || !full || !feat_id || !out || sfm->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (sfm->max_frames > AVM_MAX_ALIGN_FRAMES) return fail(c, AVM_ERR_CAPACITY, "max_frames > 64 (AVM_MAX_ALIGN_FRAMES)");
  if (sfm->max_pts > AVM_MAX_IMAGE_PTS) return fail(c, AVM_ERR_CAPACITY, "max_pts > 1024 (AVM_MAX_IMAGE_PTS)");
  if (c->max_windows > 0 && sfm->n_windows > c->max_windows) return fail(c, AVM_ERR_CAPACITY, "more streams than avm_config::max_windows");
  int rc;
  if ((rc = check_wide_strides(c, full)) != AVM_OK) return rc;
  if (sfm->max_frames < AVM_NFRAMES || sfm->max_pts < 0 || full->max_feat < 0 || full->max_obs < 0)
    return fail(c, AVM_ERR_INVALID, "max_frames < 11, or a negative stride");
  if (sfm->ba_max_num_iterations < 1) return fail(c, AVM_ERR_INVALID, "ba_max_num_iterations < 1");
  if (sfm->ba_max_solver_time_s != 0.0) return fail(c, AVM_ERR_INVALID, "ba_max_solver_time_s must be 0: this version has no wall-clock cap");
  if (full->n_windows != sfm->n_windows) return fail(c, AVM_ERR_INVALID, "full->n_windows differs from sfm->n_windows");
  for (const Field& f : SFM)
    if (!get_ptr(sfm, f)) return fail(c, AVM_ERR_INVALID, "a table of avm_sfm_batch is NULL");
  if (!full->obs_xy || !full->ex_pose) return fail(c, AVM_ERR_INVALID, "obs_xy / ex_pose of the feature list is NULL");
  if ((rc = null_window_tables(c, full, CHK_TRACKS)) != AVM_OK) return rc;
  for (const Field& f : SFM_OUT)
    if (!get_ptr(out, f) && f.offset != offsetof(avm_sfm_out, pnp_q) && f.offset != offsetof(avm_sfm_out, pnp_t))
      return fail(c, AVM_ERR_INVALID, "avm_sfm_out: every array but pnp_q / pnp_t must be given");
  if (sfm->n_windows == 0) return AVM_OK;
  // table checks, before any kernel indexes with them
  if (mem == AVM_MEM_HOST) {
    for (int b = 0; b < sfm->n_windows; b++) {
      const int rule = check_sfm_tables(*sfm, b);
      if (rule) return report_bad(c, b * 8 + rule, "stream", SFM_RULES);
    }
  } else {
    FlagCheck f;
    if ((rc = flag_begin(c, 1, [&](int* flag) { return launch_validate_sfm(*sfm, flag, c->stream); }, &f)) != AVM_OK) return rc;
    if ((rc = flag_end(c, f, "stream", SFM_RULES)) != AVM_OK) return rc;
  }
  if ((rc = validate_windows(c, mem, full, CHK_TRACKS)) != AVM_OK) return rc;

  SfmArgs a;
  const SfmDims dims = {sfm->n_windows, sfm->max_frames, full->max_feat};
  const size_t B = (size_t)sfm->n_windows, MF = (size_t)sfm->max_frames, MFE = (size_t)full->max_feat;
  if ((rc = on_device(c, mem, SFM, U_WHOLE, sfm, &a.s)) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, WINDOWS, U_SFM, full, &a.w)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "sf_feat_id", feat_id, B * MFE, &a.feat_id)) != AVM_OK) return rc;
  // the outputs travel in as well: the rows a stream does not write return as they came
  if ((rc = on_device(c, mem, SFM_OUT, U_WHOLE, out, &a.out, nullptr, nullptr, "", &dims)) != AVM_OK) return rc;
  a.st = static_cast<int32_t*>(pool_get(c, "sfm_st", sizeof(int32_t) * B));
  a.fst = static_cast<int32_t*>(pool_get(c, "sfm_fst", sizeof(int32_t) * B * MF));
  a.sstate = static_cast<int32_t*>(pool_get(c, "sfm_state", sizeof(int32_t) * B * MFE));
  a.sq = static_cast<double*>(pool_get(c, "sfm_q", sizeof(double) * B * AVM_NFRAMES * 4));
  a.sT = static_cast<double*>(pool_get(c, "sfm_T", sizeof(double) * B * AVM_NFRAMES * 3));
  a.spoint = static_cast<double*>(pool_get(c, "sfm_point", sizeof(double) * B * MFE * 3));
  a.sR = static_cast<double*>(pool_get(c, "sfm_frame_R", sizeof(double) * B * MF * 9));
  a.sfT = static_cast<double*>(pool_get(c, "sfm_frame_T", sizeof(double) * B * MF * 3));
  if (!a.st || !a.fst || !a.sstate || !a.sq || !a.sT || !a.spoint || !a.sR || !a.sfT) return fail(c, AVM_ERR_HIP, "hipMalloc failed (sfm stages)");

  HIPCHK(c, mark(c, M_SFM_CHAIN_BA));
  HIPCHK(c, launch_sfm_chain_ba(a, c->stream));
  HIPCHK(c, mark(c, M_SFM_FRAME_PNP));
  HIPCHK(c, launch_sfm_frame_pnp(a, c->stream));
  HIPCHK(c, launch_sfm_commit(a, c->stream));
  HIPCHK(c, mark(c, M_SFM_END));
  if ((rc = copy_back(c, mem, SFM_OUT, U_WHOLE, out, &a.out, &dims)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  store_elapsed(c, "sfm_chain_ba", M_SFM_CHAIN_BA, M_SFM_FRAME_PNP);
  store_elapsed(c, "sfm_frame_pnp", M_SFM_FRAME_PNP, M_SFM_END);
  return AVM_OK;
}
}  // extern "C"
