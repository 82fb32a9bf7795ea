// api/fsel.hpp - the selector: its work buffers, the selection with its fallback state machine, the entry points

namespace {

int check_fsel(avm_ctx* c, const avm_fsel_batch* b) {
  if (!b || b->n_problems < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (!fsel_horizon_supported(b->horizon)) return fail(c, AVM_ERR_UNSUPPORTED, "horizon must be one of 2,3,5,10,13");
  if (b->max_cand <= 0 || b->max_features < 0) return fail(c, AVM_ERR_INVALID, "bad max_cand / max_features");
  if (b->n_cloud && b->max_cloud > FS_MAX_CLOUD) return fail(c, AVM_ERR_UNSUPPORTED, "max_cloud above 4096 (the kd-tree of the depth cloud is built in LDS)");
  return AVM_OK;
}

constexpr size_t AVM_FSEL_SOLO_MIN = 33;  // frames per call from which a batch takes the solo form of the selector.  A solo select takes 4.3 ms (H = 10; 7.2 ms at
                                          // H = 13) however few frames run side by side; the sixteen teams take 2.0 ms (3.7 ms) per sixteen frames: up to 32 frames
                                          // two passes of the teams are ahead, from the third pass on the solo form is (measured: profiles/r05_solo_crossover.txt)
// Does a select of this batch take the solo form (one workgroup per frame, lazy evaluation: fsel_solo_kernel)?  ONE rule for the mode
// choice in avm_fsel_select_batch and for the solo form's packed Delta copy in fsel_buffers (0.8 GB at 256 frames x 512 candidates,
// H = 13: not to be held by a ctx that never runs the form).  AVM_FSEL_SOLO=0/1 overrides the batch-size rule, AVM_FSEL_FRAME vetoes it.
bool fsel_takes_solo(const avm_fsel_batch* b) {
  const bool can = b->max_cand <= 512 && 3 * b->horizon <= 39 && b->n_problems >= 1;
  bool solo = can && (size_t)b->n_problems >= AVM_FSEL_SOLO_MIN && !getenv("AVM_FSEL_FRAME");
  if (const char* e = getenv("AVM_FSEL_SOLO")) solo = can && e[0] == '1';
  return solo;
}

int fsel_buffers(avm_ctx* c, const avm_fsel_batch* b, FselBuffers* w, bool may_solo) {
  const size_t P = b->n_problems, T = 3 * (size_t)b->horizon, mc = b->max_cand, mu = b->max_used > 0 ? b->max_used : 1;
#define GET(field, type, count)                                                             \
  w->field = static_cast<type*>(pool_get(c, "fw_" #field, sizeof(type) * (count)));          \
  if (!w->field) return fail(c, AVM_ERR_HIP, "hipMalloc failed (selector work buffer)");
  GET(C, double, 2 * P * T * T)  // (two buffers: csrc/fsel/pick.hpp, FselPar)
  GET(dpp, double, 2 * P * T)  // (two buffers: csrc/fsel/pick.hpp, FselPar)
  GET(consts, double, P * 4)
  GET(delta, double, P * mc * T * T)
  // (the solo form's packed copy - csrc/fsel/args.hpp, FselDev::delta_pk - exists whenever avm_fsel_select_batch can choose that form: the rule is there)
  GET(delta_pk, double, may_solo ? P * mc * (T * (T + 1) / 2) : 1)
  GET(ddiag, double, (may_solo && T > 30) ? P * mc * T : 1)
  GET(delta_u, double, P * mu * T * T)
  GET(fval, double, 2 * P * mc)  // (two buffers: csrc/fsel/pick.hpp, FselPar)
  GET(ub, double, 2 * P * mc)  // (two buffers: csrc/fsel/pick.hpp, FselPar)
  GET(valid, int32_t, P * mc)
  GET(valid_u, int32_t, P * mu)
  GET(black, int32_t, P * mc)
  GET(nsel, int32_t, P)
  GET(done, int32_t, P)
  GET(live, int32_t, 2 * P * mc)
  GET(pos, int32_t, 2 * P * mc)
  GET(nlive, int32_t, 2 * P)
  GET(sync, int32_t, FS_SYNC_INTS)
  GET(kd, double, fsel_kd_doubles(*b))
#undef GET
  return AVM_OK;
}

// The selection of avm_fsel_select_batch, from the choice of its mode to the re-runs and the fallback counters: what that entry point and
// avm_fsel_select_image_batch share.  d / dout: the problem and its outputs on the device; batch / out: the caller's (the outputs travel
// back to `out` in host mode); check: the table check in flight on the stream (check.dev == null: the tables were checked on the host).
int run_fsel_select(avm_ctx* c, avm_mem mem, const avm_fsel_batch* batch, const avm_fsel_batch& d, avm_fsel_out* out, const avm_fsel_out& dout,
                    const FlagCheck& check) {
  int rc;
  int* const vflag = check.dev;
  const size_t P = batch->n_problems, mf = batch->max_features;
  FselBuffers w;
  if ((rc = fsel_buffers(c, &d, &w, fsel_takes_solo(&d))) != AVM_OK) return rc;
  // Every frame's greedy rounds in ONE launch (csrc/fsel/frame_kernel.hpp, fsel_frame_kernel): 2 = a team of workgroups per XCD, the teams
  // take frames from a queue; 1 = one team over all XCDs (a single frame only); 0 = one launch per round.  A kernel that reports
  // a timed-out wait, or that did not finish every frame, is re-run one mode down, and the ctx stays there.
  // The downgrade is NOT sticky: a transient cause (an XCD busy with another ctx's solve, so that a team does not fill within
  // its 2 ms) costs this call one re-run and the next AVM_FSEL_REPROBE_CALLS calls the slower mode; then the fast mode is
  // probed again.  avm_fsel_fallback_stats() counts both.
  constexpr int AVM_FSEL_REPROBE_CALLS = 16, AVM_FSEL_REPROBE_MAX = 4096;
  c->fsel_calls++;
  const bool probing = c->fsel_cooldown > 0 && --c->fsel_cooldown == 0;  // this call tries the fast mode again
  if (probing) c->fsel_frame_mode = 2;
  bool rerun = false;
  int mode = (d.max_cand <= 512 && mf < 4096) ? c->fsel_frame_mode : 0;  // (512: FS_FRAME_MAXC)
  if (mode == 1 && P != 1) mode = 0;  // (the one-team-over-all-XCDs form takes one frame)
  if (const char* e = getenv("AVM_FSEL_FRAME"))
    if (e[0] >= '0' && e[0] <= '2') mode = std::min(mode, e[0] - '0');
  // 3 = one workgroup per frame with lazy evaluation (fsel_solo_kernel): what a batch of many frames takes - it has no waits between
  // workgroups, so it cannot time out and is never re-run.  AVM_FSEL_SOLO=0/1 overrides the batch-size rule (tests, measurements).
  if (fsel_takes_solo(&d)) mode = 3;
  c->last_fsel_mode = mode;
  int32_t* hsync = mode ? static_cast<int32_t*>(pool_get(c, "f_sync", sizeof(int32_t) * 64, PINNED)) : nullptr;
  if (mode && !hsync) mode = 0;
  for (;;) {
    HIPCHK(c, hipMemsetAsync(dout.n_selected, 0, sizeof(int32_t) * P, c->stream));
    HIPCHK(c, hipMemsetAsync(dout.selected_ids, 0xff, sizeof(int32_t) * P * mf, c->stream));
    HIPCHK(c, mark(c, M_KERNELS));
    HIPCHK(c, launch_fsel(d, w, dout, nullptr, true, mode, vflag, c->stream));
    HIPCHK(c, mark(c, M_KERNELS_END));
    if (mode) HIPCHK(c, hipMemcpyAsync(hsync, w.sync, sizeof(int32_t) * 64, hipMemcpyDeviceToHost, c->stream));
    if ((rc = copy_back(c, mem, FSEL_OUT, U_WHOLE, out, &dout, batch)) != AVM_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the one synchronization of the call)
    if (vflag && (rc = flag_end(c, check, "frame", FSEL_RULES)) != AVM_OK) return rc;  // (no kernel of the select has touched a table)
    if (!mode) break;
    if (getenv("AVM_FSEL_TRACE")) {  // (cycle counters of a -DFS_TRACE_EVAL build of fsel.hip; zeros otherwise)
      const long long* q = reinterpret_cast<const long long*>(hsync + 32);
      fprintf(stderr, "fsel frame kernel, mode %d (cycles): pick %lld update %lld eval %lld wait %lld | eval: loads %lld bound %lld elimination %lld logdet %lld | setup: before the elimination %lld, elimination %lld\n",
              mode, q[0], q[1], q[2], q[4], q[5], q[6], q[7], q[8], q[9], q[3]);
    }
    if (mode == 3 && getenv("AVM_FSEL_LAZY_STATS")) {  // (development: frame 0's workgroup of fsel_solo_kernel)
      const long long* q = reinterpret_cast<const long long*>(hsync + 32);
      fprintf(stderr, "fsel solo kernel, frame 0 (cycles): bounds %lld list %lld scores %lld pick+check %lld second-pass scores %lld fold %lld | %lld candidates scored in %lld rounds, %lld second passes; %lld passes of the pick, %lld with exact bounds for unscored candidates | pick: maxima %lld flags %lld hits %lld check %lld\n",
              q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[8], q[7], q[10], q[9], q[11], q[12], q[13], q[14]);
    }
    c->last_fsel_evals = mode == 3 ? *reinterpret_cast<const int64_t*>(hsync + 16) : -1;
    if (hsync[2] == 0 && hsync[4] == (int32_t)P) {
      // a fast-mode call that went through: the back-off starts from the beginning next time
      if (mode == 2 || (mode == c->fsel_frame_mode && !rerun)) c->fsel_backoff = AVM_FSEL_REPROBE_CALLS;
      break;
    }
    // (the outputs of the failed attempt are overwritten by the next one)
    c->fsel_failed_launches++;  // one per launch that did not finish; the call counts once, below
    rerun = true;
    mode = mode == 3 ? std::min(2, c->fsel_frame_mode) : mode - 1;  // (3 cannot fail; kept for completeness)
    c->fsel_frame_mode = std::min(c->fsel_frame_mode, std::max(mode, P != 1 ? 1 : 0));  // a failed batch leaves mode 1 to single frames
    // exponential back-off of the re-probe: a host where the fast mode can never become resident pays a failed launch (up to its
    // 20 ms spin time-out) after 16, 32, 64 ... 4096 calls instead of every 16
    c->fsel_cooldown = c->fsel_backoff;
    c->fsel_backoff = std::min(2 * c->fsel_backoff, AVM_FSEL_REPROBE_MAX);
    if (mode == 1 && P != 1) mode = 0;
  }
  if (rerun) c->fsel_reruns++;
  store_elapsed(c, "fsel_select", M_KERNELS, M_KERNELS_END);
  return AVM_OK;
}

const Rule SELECT_IMAGE_RULES[8] = {
    {AVM_ERR_INVALID, "bad table"},
    {AVM_ERR_INVALID, "n_pts outside [0, max_pts]"},
    {AVM_ERR_INVALID, "the image's feature ids must be strictly ascending (std::map order)"},
    {AVM_ERR_INVALID, "n_tracked outside [0, max_tracked]"},
    {AVM_ERR_CAPACITY, "more new points than problem->max_cand"},
    {AVM_ERR_CAPACITY, "more tracked points in the image than problem->max_used"},
    {AVM_ERR_CAPACITY, "the subset and the points the selection can add do not fit image_out->max_pts"},
    {AVM_ERR_CAPACITY, "the tracked ids kept and the ids the call can append do not fit state->max_tracked"}};

}  // namespace

extern "C" {
int avm_fsel_select_batch(avm_ctx* c, avm_mem mem, const avm_fsel_batch* batch, avm_fsel_out* out) {
  if (!enter(c)) return AVM_ERR_INVALID;
  int rc = check_fsel(c, batch);
  if (rc != AVM_OK) return rc;
  if (!out || !out->n_selected || !out->selected_ids) return fail(c, AVM_ERR_INVALID, "null output");
  if (batch->n_problems == 0) return AVM_OK;
  // Host tables are checked on the host.  Device-resident ones by a kernel that runs AHEAD of the select on the same stream:
  // every kernel of the select looks at its flag before it indexes with a table, and the host reads the verdict behind the
  // synchronization that brings the results (no extra round trip for the check).
  FlagCheck check;
  if ((rc = mem == AVM_MEM_HOST ? validate_fsel(c, mem, batch) : validate_fsel_begin(c, batch, &check)) != AVM_OK) return rc;
  avm_fsel_batch d;
  if ((rc = on_device(c, mem, FSEL, U_WHOLE, batch, &d, "f_pack")) != AVM_OK) return rc;
  avm_fsel_out dout = *out;
  if (mem == AVM_MEM_HOST && alloc_out(c, FSEL_OUT, out, &dout, batch) != AVM_OK) return fail(c, AVM_ERR_HIP, "hipMalloc failed (selector out)");
  return run_fsel_select(c, mem, batch, d, out, dout, check);
}

// FeatureSelector::select() around that selection, on device-resident images (tracks.hip: check, split, merge)
int avm_fsel_select_image_batch(avm_ctx* c, avm_mem mem, const avm_image_batch* img, const double* prob, const int32_t* initialized,
                                int32_t init_thresh, int32_t prune_lost, avm_select_state* st, avm_fsel_batch* problem, avm_fsel_out* out,
                                avm_image_batch* img_out) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!img || !st || !problem || !img_out || img->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  int rc = check_fsel(c, problem);
  if (rc != AVM_OK) return rc;
  if (!out || !out->n_selected || !out->selected_ids) return fail(c, AVM_ERR_INVALID, "null output");
  if (problem->n_problems != img->n_windows) return fail(c, AVM_ERR_INVALID, "problem->n_problems differs from image->n_windows");
  if (img_out->n_windows != img->n_windows) return fail(c, AVM_ERR_INVALID, "image_out->n_windows differs from image->n_windows");
  if (img->max_pts < 0 || img_out->max_pts < 0 || st->max_tracked < 0 || problem->max_used < 0)
    return fail(c, AVM_ERR_INVALID, "negative stride (max_pts / max_tracked / max_used)");
  if (img->max_pts > AVM_MAX_IMAGE_PTS) return fail(c, AVM_ERR_CAPACITY, "max_pts > 1024 (AVM_MAX_IMAGE_PTS)");
  if (!img->n_pts || (img->max_pts > 0 && (!img->feature_id || !img->xy || !prob))) return fail(c, AVM_ERR_INVALID, "null image table / prob");
  if (!st->last_feature_id || !st->n_tracked || !st->first_image || (st->max_tracked > 0 && !st->tracked_id))
    return fail(c, AVM_ERR_INVALID, "null member of state");
  if (!problem->n_cand || !problem->cand_id || !problem->cand_xy || !problem->cand_prob || !problem->n_used ||
      (problem->max_used > 0 && (!problem->used_id || !problem->used_xy)))
    return fail(c, AVM_ERR_INVALID, "null member of problem (n_cand, cand_*, n_used, used_* are written)");
  if (!img_out->n_pts || (img_out->max_pts > 0 && (!img_out->feature_id || !img_out->xy))) return fail(c, AVM_ERR_INVALID, "null table of image_out");
  if ((img->vel_td != nullptr) != (img_out->vel_td != nullptr))
    return fail(c, AVM_ERR_INVALID, "image_out->vel_td must be given if and only if image->vel_td is");
  if (img_out->n_pts == img->n_pts || (img_out->feature_id && img_out->feature_id == img->feature_id) || (img_out->xy && img_out->xy == img->xy) ||
      (img_out->vel_td && img_out->vel_td == img->vel_td))
    return fail(c, AVM_ERR_INVALID, "image_out's tables must not be image's own arrays");
  if (img->n_windows == 0) return AVM_OK;
  const size_t B = img->n_windows;
  SelectImageArgs a;
  a.init_thresh = init_thresh, a.prune_lost = prune_lost;
  if ((rc = on_device(c, mem, IMAGE, U_SELECT, img, &a.image, nullptr, nullptr, "si_")) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "si_prob", prob, B * (size_t)img->max_pts, &a.prob)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "si_init", initialized, B, &a.initialized)) != AVM_OK) return rc;
  // (what the call writes travels in as well: the slots it does not write keep what they held)
  if ((rc = on_device(c, mem, SELECT_STATE, U_SELECT, st, &a.state, nullptr, nullptr, "", img)) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, IMAGE, U_SELECT, img_out, &a.image_out, nullptr, nullptr, "so_")) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, FSEL, U_WHOLE, problem, &a.problem)) != AVM_OK) return rc;
  a.out = *out;
  if (mem == AVM_MEM_HOST && alloc_out(c, FSEL_OUT, out, &a.out, problem) != AVM_OK) return fail(c, AVM_ERR_HIP, "hipMalloc failed (selector out)");
  // the check on its own, its verdict on the host before the first kernel that writes; then the split, which writes `problem` only
  if ((rc = track_check(c, [&](int* flag) { return launch_select_image_check(a, flag, c->stream); }, SELECT_IMAGE_RULES)) != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_SPLIT));
  HIPCHK(c, launch_select_split(a, c->stream));
  HIPCHK(c, mark(c, M_SPLIT_END));
  // the caller's tables of the problem (n_cloud, nr_imu) with the counts the split wrote: the selection's own check, ahead of it on the stream
  FlagCheck check;
  if ((rc = validate_fsel_begin(c, &a.problem, &check)) != AVM_OK) return rc;
  if ((rc = run_fsel_select(c, mem, problem, a.problem, out, a.out, check)) != AVM_OK) return rc;
  store_elapsed(c, "select_split", M_CHECK, M_CHECK_END, M_SPLIT, M_SPLIT_END);
  // the selection has finished, its re-runs included: image_out and the state
  HIPCHK(c, mark(c, M_MERGE));
  HIPCHK(c, launch_select_merge(a, c->stream));
  HIPCHK(c, mark(c, M_MERGE_END));
  if ((rc = copy_back(c, mem, FSEL, U_SELECT_BACK, problem, &a.problem, problem)) != AVM_OK) return rc;
  if ((rc = copy_back(c, mem, SELECT_STATE, U_SELECT_BACK, st, &a.state, img)) != AVM_OK) return rc;
  if ((rc = copy_back(c, mem, IMAGE, U_SELECT_BACK, img_out, &a.image_out, img_out)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  store_elapsed(c, "select_merge", M_MERGE, M_MERGE_END);
  return AVM_OK;
}

int avm_fsel_select(avm_ctx* c, avm_mem mem, const avm_fsel_batch* frame, int32_t* selected_ids, int32_t* n_selected, double* fvalues_opt) {
  if (!c) return AVM_ERR_INVALID;
  if (!frame || frame->n_problems != 1) return fail(c, AVM_ERR_INVALID, "avm_fsel_select takes exactly one frame (n_problems == 1)");
  avm_fsel_out out{n_selected, selected_ids, fvalues_opt, nullptr};
  return avm_fsel_select_batch(c, mem, frame, &out);
}

int avm_fsel_fallback_stats(const avm_ctx* c, int64_t out[4]) {
  if (!c || !out) return AVM_ERR_INVALID;
  out[0] = c->fsel_reruns, out[1] = c->fsel_failed_launches, out[2] = c->fsel_frame_mode, out[3] = c->fsel_calls;
  return AVM_OK;
}

int avm_fsel_horizon_imu(avm_ctx* c, avm_mem mem, const avm_fsel_horizon_in* in, double* hor_pos, double* hor_quat) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!in || !hor_pos || !hor_quat || in->n_problems < 0 || in->horizon < 1) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (in->n_problems == 0) return AVM_OK;
  const size_t P = in->n_problems, H1 = (size_t)in->horizon + 1;
  avm_fsel_horizon_in d;
  int rc = on_device(c, mem, HORIZON_IN, U_WHOLE, in, &d);
  if (rc != AVM_OK) return rc;
  double *dp, *dq;
  if ((rc = array_out(c, mem, "h_pos", hor_pos, P * H1 * 3, &dp, "horizon out")) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "h_quat", hor_quat, P * H1 * 4, &dq, "horizon out")) != AVM_OK) return rc;
  HIPCHK(c, launch_fsel_horizon_imu(d, dp, dq, c->stream));
  if ((rc = array_back(c, mem, hor_pos, dp, P * H1 * 3)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, hor_quat, dq, P * H1 * 4)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

int avm_fsel_build_cloud(avm_ctx* c, avm_mem mem, const avm_window_batch* windows, const double* k1_pos, const double* k1_quat, int32_t max_cloud,
                         int32_t* n_cloud, double* cloud_xy, double* cloud_depth) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!windows || !k1_pos || !k1_quat || !n_cloud || !cloud_xy || !cloud_depth || windows->n_windows < 0 || max_cloud < 1)
    return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (windows->n_windows == 0) return AVM_OK;
  int rc = validate_windows(c, mem, windows, CHK_TRACKS);
  if (rc != AVM_OK) return rc;
  const size_t B = windows->n_windows;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_CLOUD, windows, &d)) != AVM_OK) return rc;
  const size_t C = B * (size_t)max_cloud;
  const double *dp, *dq;
  int32_t* dn;
  double *dxy, *ddep;
  if ((rc = array_in(c, mem, "c_k1p", k1_pos, B * 3, &dp)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "c_k1q", k1_quat, B * 4, &dq)) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "c_n", n_cloud, B, &dn, "cloud out")) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "c_xy", cloud_xy, C * 2, &dxy, "cloud out")) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "c_dep", cloud_depth, C, &ddep, "cloud out")) != AVM_OK) return rc;
  if (mem == AVM_MEM_HOST) {  // (the slots beyond a window's n_cloud: defined values for the caller)
    HIPCHK(c, hipMemsetAsync(dxy, 0, sizeof(double) * C * 2, c->stream));
    HIPCHK(c, hipMemsetAsync(ddep, 0, sizeof(double) * C, c->stream));
  }
  HIPCHK(c, launch_fsel_build_cloud(d, dp, dq, max_cloud, dn, dxy, ddep, c->stream));
  if ((rc = array_back(c, mem, n_cloud, dn, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, cloud_xy, dxy, C * 2)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, cloud_depth, ddep, C)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

int avm_fsel_nn_depth(avm_ctx* c, avm_mem mem, const avm_fsel_batch* batch, double* depth) {
  if (!enter(c)) return AVM_ERR_INVALID;
  int rc = check_fsel(c, batch);
  if (rc != AVM_OK) return rc;
  if (!depth) return fail(c, AVM_ERR_INVALID, "null depth");
  if (batch->n_problems == 0) return AVM_OK;
  if ((rc = validate_fsel(c, mem, batch)) != AVM_OK) return rc;
  avm_fsel_batch d;
  if ((rc = on_device(c, mem, FSEL, U_WHOLE, batch, &d, "f_pack")) != AVM_OK) return rc;
  const size_t n = (size_t)batch->n_problems * batch->max_cand;
  double* dd;
  if ((rc = array_out(c, mem, "fi_nn", depth, n, &dd, "nn depth")) != AVM_OK) return rc;
  HIPCHK(c, hipMemsetAsync(dd, 0, sizeof(double) * n, c->stream));
  double* kd = static_cast<double*>(pool_get(c, "fw_kd", sizeof(double) * fsel_kd_doubles(d)));
  if (!kd) return fail(c, AVM_ERR_HIP, "hipMalloc failed (kd-tree)");
  HIPCHK(c, launch_fsel_nn_depth(d, kd, dd, c->stream));
  if ((rc = array_back(c, mem, depth, dd, n)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

int avm_fsel_information(avm_ctx* c, avm_mem mem, const avm_fsel_batch* batch, double* omega, double* delta_cand, int32_t* cand_valid) {
  if (!enter(c)) return AVM_ERR_INVALID;
  int rc = check_fsel(c, batch);
  if (rc != AVM_OK) return rc;
  if (batch->n_problems == 0) return AVM_OK;
  if ((rc = validate_fsel(c, mem, batch)) != AVM_OK) return rc;
  avm_fsel_batch d;
  if ((rc = on_device(c, mem, FSEL, U_WHOLE, batch, &d, "f_pack")) != AVM_OK) return rc;
  FselBuffers w;
  if ((rc = fsel_buffers(c, &d, &w, false)) != AVM_OK) return rc;
  const size_t P = batch->n_problems, N = 9 * ((size_t)batch->horizon + 1), T = 3 * (size_t)batch->horizon, mc = batch->max_cand;
  double* d_om;
  if ((rc = array_out(c, mem, "fi_om", omega, P * N * N, &d_om, "omega")) != AVM_OK) return rc;
  avm_fsel_out none{nullptr, nullptr, nullptr, nullptr};
  HIPCHK(c, launch_fsel(d, w, none, d_om, false, 0, nullptr, c->stream));
  if ((rc = array_back(c, mem, omega, d_om, P * N * N)) != AVM_OK) return rc;
  if ((rc = array_from_ctx(c, mem, delta_cand, w.delta, P * mc * T * T)) != AVM_OK) return rc;
  if ((rc = array_from_ctx(c, mem, cand_valid, w.valid, P * mc)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}
}  // extern "C"
