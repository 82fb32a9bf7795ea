// api/relo.hpp - relocalization and the prior hand-over in the stream loop (relo.hip; the prior's copy: tracks.hip): headers_step, set_relo_frame, relo_resolve, relo_finish, prior_keep

namespace {
const Rule HEADERS_STEP_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                    {AVM_ERR_INVALID, "marginalization flag must be AVM_MARGIN_OLD or AVM_MARGIN_SECOND_NEW"}};
const Rule SET_RELO_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                {AVM_ERR_INVALID, "n_match outside [0, max_match]"},
                                {AVM_ERR_INVALID, "the message's match ids must be strictly ascending"}};
const Rule RELO_RESOLVE_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                    {AVM_ERR_INVALID, "view_row must be strictly increasing inside [0, full_max_feat)"},
                                    {AVM_ERR_INVALID, "relo_frame outside [0, WINDOW_SIZE)"},
                                    {AVM_ERR_INVALID, "n_match outside [0, state->max_match]"},
                                    {AVM_ERR_INVALID, "the ids of the view's rows must be strictly ascending"},
                                    {AVM_ERR_INVALID, "the state's match ids must be strictly ascending"}};
const Rule RELO_FINISH_RULES[8] = {{AVM_ERR_INVALID, "bad table"}, {AVM_ERR_INVALID, "relo_frame outside [0, WINDOW_SIZE)"}};
const Rule PRIOR_KEEP_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                  {AVM_ERR_INVALID, "prior_nblk outside [0, max_pblk]"},
                                  {AVM_ERR_CAPACITY, "the prior the window was solved with does not fit prior->max_prior / max_pblk"}};
static_assert(HDR_BAD_FLAG == 1 && SETRELO_BAD_NMATCH == 1 && SETRELO_BAD_IDS == 2 && RESOLVE_BAD_ROW == 1 && RESOLVE_BAD_FRAME == 2 &&
                  RESOLVE_BAD_NMATCH == 3 && RESOLVE_BAD_VIEW_IDS == 4 && RESOLVE_BAD_MATCH_IDS == 5 && FINISH_BAD_FRAME == 1 && KEEP_BAD_NBLK == 1 &&
                  KEEP_CAP == 2,
              "the rows above stand in the order of the rule numbers");

// the members of the state a call reads or writes: all present
int check_relo_state(avm_ctx* c, const avm_relo_state* s, unsigned use) {
  if (s->max_match < 0) return fail(c, AVM_ERR_INVALID, "state->max_match < 0");
  if (s->max_match > AVM_MAX_IMAGE_PTS) return fail(c, AVM_ERR_CAPACITY, "state->max_match > 1024 (AVM_MAX_IMAGE_PTS)");
  for (const Field& f : RELO_STATE)
    if (((f.in | f.out) & use) && !get_ptr(s, f)) return fail(c, AVM_ERR_INVALID, "null member of the relocalization state");
  return AVM_OK;
}
}  // namespace

extern "C" {
int avm_headers_step_batch(avm_ctx* c, avm_mem mem, int32_t n_windows, double* stamp, const int32_t* flags, const double* new_stamp) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!stamp || n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (n_windows == 0 || (!flags && !new_stamp)) return AVM_OK;
  int rc;
  const size_t B = n_windows;
  double* dstamp;
  const int32_t* dflags;
  const double* dnew;
  if ((rc = array_inout(c, mem, "hs_stamp", stamp, B * AVM_NFRAMES, &dstamp)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "hs_flags", flags, B, &dflags)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "hs_new", new_stamp, B, &dnew)) != AVM_OK) return rc;
  if (flags && (rc = track_check(c, [&](int* flag) { return launch_headers_step_check(n_windows, dflags, flag, c->stream); }, HEADERS_STEP_RULES)) != AVM_OK)
    return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_headers_step(n_windows, dstamp, dflags, dnew, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = array_back(c, mem, stamp, dstamp, B * AVM_NFRAMES)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (flags) record_track_ms(c, "headers_step");
  else store_elapsed(c, "headers_step", M_KERNELS, M_KERNELS_END);
  return AVM_OK;
}

int avm_set_relo_frame_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* win, const double* stamp, const avm_relo_msg_batch* msg,
                             avm_relo_state* state) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!win || !stamp || !msg || !state || win->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (msg->n_windows != win->n_windows) return fail(c, AVM_ERR_INVALID, "msg->n_windows differs from windows->n_windows");
  if (msg->max_match < 0) return fail(c, AVM_ERR_INVALID, "max_match < 0");
  if (msg->max_match > AVM_MAX_IMAGE_PTS) return fail(c, AVM_ERR_CAPACITY, "max_match > 1024 (AVM_MAX_IMAGE_PTS)");
  if (state->max_match < msg->max_match) return fail(c, AVM_ERR_CAPACITY, "state->max_match < msg->max_match");
  if (!win->pose) return fail(c, AVM_ERR_INVALID, "null pose");
  if (!msg->has_msg || !msg->frame_stamp || !msg->n_match || !msg->prev_relo_t || !msg->prev_relo_q || (msg->max_match > 0 && (!msg->match_id || !msg->match_xy)))
    return fail(c, AVM_ERR_INVALID, "null message table");
  int rc = check_relo_state(c, state, U_RELO_SET);
  if (rc != AVM_OK) return rc;
  if (win->n_windows == 0) return AVM_OK;
  const size_t B = win->n_windows;
  avm_window_batch d;
  avm_relo_msg_batch dm;
  avm_relo_state ds;
  const double* dstamp;
  if ((rc = on_device(c, mem, WINDOWS, U_RELO_SET, win, &d)) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, RELO_MSG, U_RELO_SET, msg, &dm)) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, RELO_STATE, U_RELO_SET, state, &ds, nullptr, nullptr, "", win)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "hs_stamp", stamp, B * AVM_NFRAMES, &dstamp)) != AVM_OK) return rc;
  if ((rc = track_check(c, [&](int* flag) { return launch_set_relo_frame_check(dm, flag, c->stream); }, SET_RELO_RULES)) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_set_relo_frame(d, dstamp, dm, ds, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = copy_back(c, mem, RELO_STATE, U_RELO_SET, state, &ds, win)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "set_relo");
  return AVM_OK;
}

int avm_relo_resolve_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* view, const int32_t* feat_id, int32_t full_max_feat, const int32_t* view_row,
                           const avm_relo_state* state, int32_t* relo_n, int32_t* relo_frame, int32_t* relo_feat, double* relo_xy, int32_t* n_active) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!view || !feat_id || !view_row || !state || !relo_n || !relo_frame || !relo_feat || !relo_xy || view->n_windows < 0 || full_max_feat < 0)
    return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (view->max_feat < 0) return fail(c, AVM_ERR_INVALID, "negative view stride");
  if (view->max_feat > MAXE) return fail(c, AVM_ERR_CAPACITY, "view->max_feat > 150");
  int rc = check_relo_state(c, state, U_RELO_RESOLVE);
  if (rc != AVM_OK) return rc;
  if (view->n_windows == 0) {
    if (n_active) *n_active = 0;
    return AVM_OK;
  }
  if ((rc = validate_windows(c, mem, view, CHK_TRACKS)) != AVM_OK) return rc;
  const size_t B = view->n_windows, VF = (size_t)view->max_feat;
  ReloResolveArgs a;
  a.full_max_feat = full_max_feat;
  if ((rc = on_device(c, mem, WINDOWS, U_RELO_RESOLVE, view, &a.view, nullptr, nullptr, "v_")) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, RELO_STATE, U_RELO_RESOLVE, state, &a.state, nullptr, nullptr, "", view)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "w_feat_id", feat_id, B * full_max_feat, &a.feat_id)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "v_row", view_row, B * VF, &a.view_row)) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "rr_n", relo_n, B, &a.relo_n)) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "rr_frame", relo_frame, B, &a.relo_frame)) != AVM_OK) return rc;
  // (the slots at and beyond relo_n keep what they held: the two tables travel in as well)
  if ((rc = array_inout(c, mem, "rr_feat", relo_feat, B * VF, &a.relo_feat)) != AVM_OK) return rc;
  if ((rc = array_inout(c, mem, "rr_xy", relo_xy, B * VF * 2, &a.relo_xy)) != AVM_OK) return rc;
  a.n_active = static_cast<int32_t*>(pool_get(c, "rr_active", sizeof(int32_t)));
  int32_t* hactive = static_cast<int32_t*>(pool_get(c, "rr_active", sizeof(int32_t), PINNED));
  if (!a.n_active || !hactive) return fail(c, AVM_ERR_HIP, "allocation failed (active count)");
  if ((rc = track_check(c, [&](int* flag) { return launch_relo_resolve_check(a, flag, c->stream); }, RELO_RESOLVE_RULES)) != AVM_OK) return rc;
  HIPCHK(c, hipMemsetAsync(a.n_active, 0, sizeof(int32_t), c->stream));
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_relo_resolve(a, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  HIPCHK(c, hipMemcpyAsync(hactive, a.n_active, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if ((rc = array_back(c, mem, relo_n, a.relo_n, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, relo_frame, a.relo_frame, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, relo_feat, a.relo_feat, B * VF)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, relo_xy, a.relo_xy, B * VF * 2)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (n_active) *n_active = *hactive;
  record_track_ms(c, "relo_resolve");
  return AVM_OK;
}

int avm_relo_finish_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* win, avm_relo_state* state) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!win || !state || win->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (!win->pose) return fail(c, AVM_ERR_INVALID, "null pose");
  int rc = check_relo_state(c, state, U_RELO_FINISH);
  if (rc != AVM_OK) return rc;
  if (win->n_windows == 0) return AVM_OK;
  avm_window_batch d;
  avm_relo_state ds;
  if ((rc = on_device(c, mem, WINDOWS, U_RELO_FINISH, win, &d)) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, RELO_STATE, U_RELO_FINISH, state, &ds, nullptr, nullptr, "", win)) != AVM_OK) return rc;
  if ((rc = track_check(c, [&](int* flag) { return launch_relo_finish_check(d.n_windows, ds, flag, c->stream); }, RELO_FINISH_RULES)) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_relo_finish(d, ds, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = copy_back(c, mem, RELO_STATE, U_RELO_FINISH, state, &ds, win)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "relo_finish");
  return AVM_OK;
}

int avm_prior_keep_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* win, avm_prior_out* prior) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!win || !prior || win->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (prior->max_prior < 0 || prior->max_pblk < 0) return fail(c, AVM_ERR_INVALID, "negative prior stride");
  if (!win->prior_n || !win->prior_J || !win->prior_r || !win->prior_x0) return fail(c, AVM_ERR_INVALID, "null prior table");
  for (const Field& f : PRIOR_OUT)
    if (!get_ptr(prior, f)) return fail(c, AVM_ERR_INVALID, "null member of the prior slots");
  if (win->n_windows == 0) return AVM_OK;
  int rc = validate_windows(c, mem, win, CHK_PRIOR);
  if (rc != AVM_OK) return rc;
  avm_window_batch d;
  avm_prior_out dp;
  if ((rc = on_device(c, mem, WINDOWS, U_KEEP, win, &d)) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, PRIOR_OUT, U_KEEP, prior, &dp, nullptr, nullptr, "", win)) != AVM_OK) return rc;
  if ((rc = track_check(c, [&](int* flag) { return launch_prior_keep_check(d, dp, flag, c->stream); }, PRIOR_KEEP_RULES)) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_KERNELS));
  HIPCHK(c, launch_prior_keep(d, dp, c->stream));
  HIPCHK(c, mark(c, M_KERNELS_END));
  if ((rc = copy_back(c, mem, PRIOR_OUT, U_KEEP, prior, &dp, win)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "prior_keep");
  return AVM_OK;
}
}  // extern "C"
