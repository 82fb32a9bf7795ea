// api/checks.hpp - the argument and table checks: rule texts, the check in flight on the stream (FlagCheck), validate_windows* / validate_fsel*, the stride checks

namespace {
// What a verdict of a check turns into: one table of {status, text} per check, indexed by the rule number (verdict % 8) that
// check_*_tables (kernels.hpp) or a check kernel of tracks.hip reports; a slot without a text reads "bad table", AVM_ERR_INVALID.
struct Rule {
  int status;
  const char* text;
};
static_assert(BAD_NFEAT == 1 && BAD_TRACK == 2 && BAD_ORDER == 3 && BAD_OBS == 4 && BAD_IMU == 5 && BAD_PRIOR == 6 && BAD_FSEL == 7 && BAD_FLAG == 7,
              "the rows below stand in the order of the rule numbers");
#define WINDOW_RULE_ROWS                                                                                                                     \
  {AVM_ERR_INVALID, "bad table"}, {AVM_ERR_INVALID, "n_feat outside [0, max_feat]"},                                                        \
      {AVM_ERR_INVALID, "a feature track leaves the window (need start >= 0, nobs >= 1, start + nobs <= 11)"},                             \
      {AVM_ERR_INVALID, "feat_start must be non-decreasing in the feature index (std::list order)"},                                       \
      {AVM_ERR_INVALID, "feat_obs_begin + feat_nobs runs past max_obs"}, {AVM_ERR_INVALID, "imu_n outside [0, max_samp]"},                   \
      {AVM_ERR_INVALID, "prior tables inconsistent (prior_n / prior_nblk ranges, block kinds / frames, sizes must add up to prior_n)"}
const Rule WINDOW_RULES[8] = {WINDOW_RULE_ROWS};
// windows of an entry point that takes per-window marginalization flags: the solve's set of values, and the roll's
const Rule SOLVE_FLAG_RULES[8] = {WINDOW_RULE_ROWS, {AVM_ERR_INVALID, "marginalization flag must be AVM_MARGIN_OLD, AVM_MARGIN_SECOND_NEW or AVM_MARGIN_NONE"}};
const Rule ROLL_FLAG_RULES[8] = {WINDOW_RULE_ROWS, {AVM_ERR_INVALID, "marginalization flag must be AVM_MARGIN_OLD or AVM_MARGIN_SECOND_NEW"}};
#undef WINDOW_RULE_ROWS
// the selector's frames (BAD_FSEL is their only rule; it has BAD_FLAG's number: a unit has one or the other)
const Rule FSEL_RULES[8] = {{AVM_ERR_INVALID, "bad table"}, {}, {}, {}, {}, {}, {}, {AVM_ERR_INVALID, "n_cand / n_used / n_cloud outside their strides, or nr_imu < 0"}};
static_assert(BAD_ALIGN_FRAMES == 1 && BAD_ALIGN_IMU == 2 && BAD_ALIGN_KEYS == 3, "the rows below stand in the order of the rule numbers");
const Rule ALIGN_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                             {AVM_ERR_INVALID, "n_frames outside [2, max_frames]"},
                             {AVM_ERR_INVALID, "imu_n outside [0, max_samp]"},
                             {AVM_ERR_INVALID, "key_index must be strictly increasing inside [0, n_frames)"}};

static_assert(BAD_SFM_L == 1 && BAD_SFM_FRAMES == 2 && BAD_SFM_KEYS == 3 && BAD_SFM_NPTS == 4 && BAD_SFM_IDS == 5, "the rows below stand in the order of the rule numbers");
const Rule SFM_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                           {AVM_ERR_INVALID, "l outside [0, 9]"},
                           {AVM_ERR_INVALID, "n_frames outside [11, max_frames]"},
                           {AVM_ERR_INVALID, "key_index must be strictly increasing inside [0, n_frames)"},
                           {AVM_ERR_INVALID, "frame_n_pts outside [0, max_pts]"},
                           {AVM_ERR_INVALID, "frame_pt_id must be strictly increasing within a frame"}};

int report_bad(avm_ctx* c, int first_bad, const char* unit, const Rule* rules) {
  const Rule& r = rules[first_bad % 8];
  c->err = std::string(unit) + " " + std::to_string(first_bad / 8) + ": " + (r.text ? r.text : "bad table");
  return r.text ? r.status : AVM_ERR_INVALID;
}

// ---- table checks ----
// They run before any kernel indexes with the caller's tables: host tables are checked on the host, device-resident ones by a
// one-thread-per-window (or per-frame) kernel.  Its verdict is a word that stays 0x7f7f7f7f while every table passes and otherwise names
// the first window / frame that does not (8 * index + rule); the check of windows has a second word, tp_misfit, and with per-window
// marginalization flags a third: which flag values occur.
// flag_begin enqueues the check, the copy of its verdict into pinned memory and an event; flag_end waits for that event only.  What a
// caller enqueues in between (the solve: its pre-integration, which clamps the one table entry it indexes with; the selector: the whole
// select, whose kernels look at the device flag before they index with a table) runs while the host reads the verdict and prepares the next
// launches, instead of the device idling through a blocking round trip.  On a failed check flag_end drains the stream before it reports,
// so the caller's buffers are no longer being read when the error returns.
struct FlagCheck {
  int* dev = nullptr;   // non-null: a check is in flight
  int* host = nullptr;  // pinned copy of the verdict, valid after flag_end
};

template <class Launch>
int flag_begin(avm_ctx* c, int words, Launch launch, FlagCheck* f) {
  int* dev = static_cast<int*>(pool_get(c, "v_flag", 4 * sizeof(int)));
  f->host = static_cast<int*>(pool_get(c, "v_flag_h", 4 * sizeof(int), PINNED));
  if (!dev || !f->host) return fail(c, AVM_ERR_HIP, "allocation failed (validation flag)");
  HIPCHK(c, hipMemsetAsync(dev, 0x7f, sizeof(int), c->stream));
  if (words > 1) HIPCHK(c, hipMemsetAsync(dev + 1, 0, (words - 1) * sizeof(int), c->stream));
  HIPCHK(c, launch(dev));
  HIPCHK(c, hipMemcpyAsync(f->host, dev, words * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipEventRecord(c->ev_flag, c->stream));
  f->dev = dev;
  return AVM_OK;
}

int flag_end(avm_ctx* c, const FlagCheck& f, const char* unit, const Rule* rules, int* tp_misfit = nullptr) {
  HIPCHK(c, hipEventSynchronize(c->ev_flag));
  if (tp_misfit) *tp_misfit = f.host[1];
  if (f.host[0] == 0x7f7f7f7f) return AVM_OK;
  (void)hipStreamSynchronize(c->stream);
  return report_bad(c, f.host[0], unit, rules);
}

// A check kernel of tracks.hip, on its own: its verdict is on the host before the kernel that writes is launched, so a refused batch
// leaves every window as it was.  Device time between M_CHECK and M_CHECK_END.
template <class Launch>
int track_check(avm_ctx* c, Launch launch, const Rule* rules) {
  FlagCheck f;
  HIPCHK(c, mark(c, M_CHECK));
  const int rc = flag_begin(c, 1, launch, &f);
  if (rc != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_CHECK_END));
  return flag_end(c, f, "window", rules);
}

int null_window_tables(avm_ctx* c, const avm_window_batch* b, int what) {
  if ((what & CHK_TRACKS) && (!b->n_feat || !b->feat_start || !b->feat_nobs || !b->feat_obs_begin)) return fail(c, AVM_ERR_INVALID, "null feature table");
  if ((what & CHK_IMU) && !b->imu_n) return fail(c, AVM_ERR_INVALID, "null imu_n");
  if ((what & CHK_PRIOR) && b->prior_n && (!b->prior_nblk || !b->prior_blk_kind || !b->prior_blk_frame)) return fail(c, AVM_ERR_INVALID, "null prior table");
  return AVM_OK;
}

// fr: per-window marginalization flags (device memory, like the tables) checked in the same pass; flag_end then leaves the values that occur,
// as bits, in f->host[2]
int validate_windows_begin(avm_ctx* c, const avm_window_batch* b, int what, FlagCheck* f, const FlagRule& fr = FlagRule()) {
  const int rc = null_window_tables(c, b, what);
  if (rc != AVM_OK) return rc;
  return flag_begin(c, fr.flags ? 3 : 2, [&](int* flag) { return launch_validate_windows(*b, what, flag, c->stream, fr); }, f);
}

// tp_misfit (optional, with CHK_PRIOR): bit 0 set when some window's prior does not fit the throughput form of the solve, bit 1 when one
// does not fit the throughput form of the marginalization (kernels.hpp, window_prior_tp_misfit)
// fr, rules, flags_seen: per-window marginalization flags (in `mem` space) checked with the tables, the messages with the flag rule's, and
// which values occur (bit f: some window has flag f)
int validate_windows(avm_ctx* c, avm_mem mem, const avm_window_batch* b, int what, int* tp_misfit = nullptr, const FlagRule& fr = FlagRule(),
                     const Rule* rules = WINDOW_RULES, unsigned* flags_seen = nullptr) {
  if (tp_misfit) *tp_misfit = 0;
  if (flags_seen) *flags_seen = 0;
  if (mem != AVM_MEM_HOST) {
    FlagCheck f;
    int rc = validate_windows_begin(c, b, what, &f, fr);
    if (rc == AVM_OK) rc = flag_end(c, f, "window", rules, tp_misfit);
    if (rc == AVM_OK && flags_seen && fr.flags) *flags_seen = (unsigned)f.host[2];
    return rc;
  }
  const int rc = null_window_tables(c, b, what);
  if (rc != AVM_OK) return rc;
  for (int w = 0; w < b->n_windows; w++) {
    int rule = check_window_tables(*b, w, what);
    if (!rule && fr.flags && !flag_allowed(fr, w)) rule = BAD_FLAG;
    if (rule) return report_bad(c, w * 8 + rule, "window", rules);
    if (tp_misfit && (what & CHK_PRIOR)) *tp_misfit |= window_prior_tp_misfit(*b, w);
    if (flags_seen && fr.flags) *flags_seen |= 1u << fr.flags[w];
  }
  return AVM_OK;
}

int validate_fsel_begin(avm_ctx* c, const avm_fsel_batch* b, FlagCheck* f) {
  if (!b->n_cand || !b->nr_imu) return fail(c, AVM_ERR_INVALID, "null n_cand / nr_imu");
  return flag_begin(c, 1, [&](int* flag) { return launch_validate_fsel(*b, flag, c->stream); }, f);
}

int validate_fsel(avm_ctx* c, avm_mem mem, const avm_fsel_batch* b) {
  if (mem != AVM_MEM_HOST) {
    FlagCheck f;
    const int rc = validate_fsel_begin(c, b, &f);
    return rc != AVM_OK ? rc : flag_end(c, f, "frame", FSEL_RULES);
  }
  if (!b->n_cand || !b->nr_imu) return fail(c, AVM_ERR_INVALID, "null n_cand / nr_imu");
  for (int p = 0; p < b->n_problems; p++) {
    const int rule = check_fsel_tables(*b, p);
    if (rule) return report_bad(c, p * 8 + rule, "frame", FSEL_RULES);
  }
  return AVM_OK;
}

static_assert(MAXE == AVM_MAX_FEAT && MAXOBS == AVM_MAX_OBS, "avm.h states the solve kernels' limits");
static_assert(AVM_MAX_FEAT_WIDE == 384 && AVM_MAX_OBS_WIDE == 4224, "the messages below name the limits");
int check_wide_strides(avm_ctx* c, const avm_window_batch* b) {
  if (b->max_feat > AVM_MAX_FEAT_WIDE) return fail(c, AVM_ERR_CAPACITY, "max_feat > 384 (AVM_MAX_FEAT_WIDE)");
  if (b->max_obs > AVM_MAX_OBS_WIDE) return fail(c, AVM_ERR_CAPACITY, "max_obs > 4224 (AVM_MAX_OBS_WIDE)");
  return AVM_OK;
}

// wide: the pre-integration (it reads no feature table) takes the strides the API accepts for a window, AVM_MAX_FEAT_WIDE /
// AVM_MAX_OBS_WIDE - a contract of avm.h, no limit of its kernels; the solve's LDS carve - and the factor evaluation's, which
// stages the inverse depths in the same state vector - holds AVM_MAX_FEAT / AVM_MAX_OBS (avm.h)
int check_window_batch(avm_ctx* c, const avm_options* opt, const avm_window_batch* b, bool wide = false) {
  if (!opt || !b || b->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (opt->estimate_td && (!b->obs_vel_td || !b->td))
    return fail(c, AVM_ERR_INVALID, "estimate_td != 0 needs obs_vel_td (velocity, cur_td, uv.y per observation) and td");
  if (opt->estimate_td && !(opt->row > 0.0)) return fail(c, AVM_ERR_INVALID, "estimate_td != 0 needs opt->row (image height) > 0");
  if (b->relo_n && (!b->relo_feat || !b->relo_xy || !b->relo_pose))
    return fail(c, AVM_ERR_INVALID, "relo_n is set but relo_feat / relo_xy / relo_pose is NULL");
  if (b->failure_occur && !b->last_pose0) return fail(c, AVM_ERR_INVALID, "failure_occur is set but last_pose0 is NULL");
  if (wide) {
    const int rc = check_wide_strides(c, b);
    if (rc != AVM_OK) return rc;
  } else {
    if (b->max_feat > MAXE) return fail(c, AVM_ERR_CAPACITY, "max_feat > 150");
    if (b->max_obs > MAXOBS) return fail(c, AVM_ERR_CAPACITY, "max_obs > 1650");
  }
  if (b->max_prior > MAXPRIOR || b->max_pblk > MAXPBLK) return fail(c, AVM_ERR_CAPACITY, "prior larger than 96 / 16 blocks");
  if (opt->max_num_iterations > AVM_MAX_ITER_TRACE) return fail(c, AVM_ERR_CAPACITY, "max_num_iterations > 16");
  return AVM_OK;
}
}  // namespace
