// api/solve.hpp - the window solve: forms, solve, marginalization; its entry points and the factor evaluations

namespace {
// ---- the steps of avm_window_solve_batch ----
// Which forms of the kernels a batch takes.  The solve: the throughput form (two 256-thread workgroups per CU, window_solve_tp.o) for
// batches that give every CU more than one window, the latency form (one 512-thread workgroup per CU) otherwise - and always for the
// extended problem or a prior the structural form cannot hold (tp_misfit bit 0).  (Round 5: a wall-clock cap no longer forces the latency
// form - both kernels check options.max_solver_time_in_seconds against a clock that starts with the window's own solve, and a batch that
// is larger than the CU count is not a real-time call.  A window shares its CU there and runs 1.6 ms instead of 0.9: a cap between those
// two durations ends it an iteration earlier than the latency form would - wall-clock semantics.)  AVM_SOLVE_TP=0 / 1 forces the choice
// where both are possible (tests, A/B runs).
// The marginalization follows the solve: its throughput form (two 256-thread workgroups per CU on the solve's 2 x CUs slots) for the
// batches that took the throughput solve - and for a batch of the extended problem that is larger than the CU count (big_x): the
// marginalization is the same problem whatever the solve estimated -, unless a prior keeps a speed-bias block beyond frame 1 (tp_misfit
// bit 1; AVM_MARG_TP=0: never).
// The environment is read on every call: tests flip it in-process.
struct SolveForms {
  bool tp, big_x, marg_tp;
};
SolveForms choose_forms(int n_windows, int n_slots, bool extended, bool marg, int tp_misfit) {
  bool tp = n_windows > n_slots;
  if (const char* e = getenv("AVM_SOLVE_TP")) tp = e[0] == '1' ? true : (e[0] == '0' ? false : tp);
  tp = tp && !extended && (tp_misfit & 1) == 0;
  const bool big_x = extended && marg && n_windows > n_slots;
  bool marg_tp = (tp || big_x) && (tp_misfit & 2) == 0;
  if (const char* e = getenv("AVM_MARG_TP")) marg_tp = marg_tp && e[0] != '0';
  return {tp, big_x, marg_tp};
}

int check_prior_out(avm_ctx* c, const avm_prior_out* po) {
  bool all = po != nullptr;
  for (const Field& f : PRIOR_OUT) all = all && get_ptr(po, f);
  if (!all) return fail(c, AVM_ERR_INVALID, "prior_out (or one of its arrays) is NULL but marginalization_flag != AVM_MARGIN_NONE (or per-window flags are given)");
  if (po->max_prior > MAXPRIOR || po->max_prior < 1 || po->max_pblk < 1) return fail(c, AVM_ERR_CAPACITY, "prior_out dims");
  return AVM_OK;
}

SolveArgs solve_args(const avm_ctx* c, const avm_options* opt, const avm_window_batch& d, avm_solve_summary* d_sum) {
  SolveArgs sa;
  sa.b = d, sa.opt = *opt;
  sa.pre_delta = c->pre_delta, sa.pre_jac = c->pre_jac, sa.pre_sqrt = c->pre_sqrt, sa.pre_sum_dt = c->pre_sum;
  sa.scratch = c->scratch, sa.iscratch = c->iscratch, sa.summary = d_sum, sa.n_slots = c->n_slots;
  sa.prof = c->prof;
  sa.marg_flags = nullptr;  // (avm_window_solve_batch_flags sets it for the marginalization)
  // (a cap that is not finite, or beyond 1e9 s, means "no cap": the conversion to device ticks must not overflow)
  sa.time_cap_ticks = (opt->max_solver_time_s > 0.0 && opt->max_solver_time_s <= 1.0e9) ? (long long)(opt->max_solver_time_s * c->wall_clock_hz) + 1 : 0;
  const char* ns = getenv("AVM_NO_SPECULATE");
  sa.speculate = (ns && ns[0] == '1') ? 0 : 1;
  return sa;
}

// the solve kernel in the chosen form; leaves sa.n_slots as the marginalization takes it (two workgroups per CU in its throughput form, else one)
int run_solve(avm_ctx* c, SolveArgs& sa, bool extended, const SolveForms& forms) {
  if (c->prof) HIPCHK(c, hipMemsetAsync(c->prof, 0, sizeof(long long) * PROF_SLOTS * 2 * c->n_slots, c->stream));
  if (forms.tp) {
    sa.n_slots = 2 * c->n_slots;
    if (const char* e = getenv("AVM_TP_GRID")) sa.n_slots = std::max(1, std::min(atoi(e), 2 * c->n_slots));  // (experiments: fewer resident workgroups)
    HIPCHK(c, launch_window_solve_tp(sa, c->stream));
  } else {
    // (ex_pose / td as variables, relocalization factors: the build of the solve kernel with the wider dense block)
    HIPCHK(c, extended ? launch_window_solve_x(sa, c->stream) : launch_window_solve(sa, c->stream));
  }
  sa.n_slots = forms.marg_tp ? 2 * c->n_slots : c->n_slots;
  c->last_solve_tp = forms.tp;
  c->last_marg_tp = false;
  return AVM_OK;
}

// avm_window_solve_batch_relo's solve when a batch has windows of both kinds: the plain list in its form (forms.tp), then the extended
// list, one after the other on the ctx stream - they share the scratch slots.  lists: [2 B] device, the plain windows from 0 and the
// extended ones from B (solve_partition_kernel's layout); n_ext of them extended.  lists == null: every window through the extended list
// build in batch order (estimate_extrinsic / estimate_td: relo_active then only decides which windows have a relocalization frame).
int run_solve_split(avm_ctx* c, SolveArgs& sa, const SolveForms& forms, const int32_t* lists, int n_ext, const int32_t* relo_active) {
  if (c->prof) HIPCHK(c, hipMemsetAsync(c->prof, 0, sizeof(long long) * PROF_SLOTS * 2 * c->n_slots, c->stream));
  const int B = sa.b.n_windows;
  SolveListArgs la;
  static_cast<SolveArgs&>(la) = sa;
  la.relo_active = relo_active;
  if (lists) {
    la.win_list = lists, la.n_list = B - n_ext;
    la.n_slots = forms.tp ? 2 * c->n_slots : c->n_slots;
    HIPCHK(c, forms.tp ? launch_window_solve_tp_list(la, c->stream) : launch_window_solve_list(la, c->stream));
  }
  la.win_list = lists ? lists + B : nullptr, la.n_list = lists ? n_ext : B;
  la.n_slots = c->n_slots;
  HIPCHK(c, launch_window_solve_x_list(la, c->stream));
  sa.n_slots = forms.marg_tp ? 2 * c->n_slots : c->n_slots;
  c->last_solve_tp = lists && forms.tp;
  c->last_marg_tp = false;
  return AVM_OK;
}

// Marginalization and the square root of the new prior, into prior_out (host mode: into the ctx's block, and the copy back enqueued).
// *marg_err: the device flag the kernel raises when a window's kept set does not fit (prior_out->max_prior / max_pblk, or the 76 rows /
// 16 blocks the eigen-solver holds): the call then fails with AVM_ERR_CAPACITY instead of returning a truncated prior.
int run_marginalize(avm_ctx* c, const avm_options* opt, avm_mem mem, const SolveArgs& sa, bool marg_tp, avm_prior_out* prior_out, int** marg_err,
                    PackedBack* back) {
  const avm_window_batch* dims = &sa.b;
  const size_t B = sa.b.n_windows;
  avm_prior_out dpo = *prior_out;
  size_t po_bytes = 0;
  if (mem == AVM_MEM_HOST) {
    if (alloc_out(c, PRIOR_OUT, prior_out, &dpo, dims, "po_pack", &po_bytes) != AVM_OK) return fail(c, AVM_ERR_HIP, "hipMalloc failed (prior out)");
    HIPCHK(c, hipMemsetAsync(dpo.n, 0, po_bytes, c->stream));  // (n is the head of the block)
  }
  *marg_err = static_cast<int*>(pool_get(c, "marg_err", sizeof(int)));
  if (!*marg_err) return fail(c, AVM_ERR_HIP, "hipMalloc failed (marginalization flag)");
  HIPCHK(c, hipMemsetAsync(*marg_err, 0x7f, sizeof(int), c->stream));
  // the magnitude every diagonal entry of A' was formed at (marginalize_kernel -> the eigenvalue clamp's noise test): the ctx's own array
  double* marg_scale = static_cast<double*>(pool_get(c, "marg_scale", sizeof(double) * B * prior_out->max_prior));
  if (!marg_scale) return fail(c, AVM_ERR_HIP, "hipMalloc failed (marginalization scales)");
  HIPCHK(c, mark(c, M_MARGINALIZE));
  if (sa.marg_flags)  // (the flag per window: the kernels of window_solve_mm.o / window_solve_tp_mm.o)
    HIPCHK(c, marg_tp ? launch_marginalize_tp_mixed(sa, dpo, *marg_err, marg_scale, c->stream) : launch_marginalize_mixed(sa, dpo, *marg_err, marg_scale, c->stream));
  else
    HIPCHK(c, marg_tp ? launch_marginalize_tp(sa, dpo, *marg_err, marg_scale, c->stream) : launch_marginalize(sa, dpo, *marg_err, marg_scale, c->stream));
  c->last_marg_tp = marg_tp;
  HIPCHK(c, mark(c, M_PRIOR_ROOT));
  int* pe_done = static_cast<int*>(pool_get(c, "pe_done", sizeof(int) * B));
  if (!pe_done) return fail(c, AVM_ERR_HIP, "hipMalloc failed (prior flags)");
  const double noise_rel = (opt->marg_noise_rel > 0.0 && opt->marg_noise_rel < 1.0) ? opt->marg_noise_rel : 0.0;
  HIPCHK(c, launch_prior_eig(dpo, B, opt->marg_eps, noise_rel, marg_scale, c->prof, pe_done, c->stream));
  c->last_marg_windows = (int)B;
  HIPCHK(c, mark(c, M_PRIOR_ROOT_END));
  return copy_back(c, mem, PRIOR_OUT, U_WHOLE, prior_out, &dpo, dims, po_bytes <= PACK_LIMIT ? (int)PRIOR_OUT.n : 0, "po_pack", back);
}

void record_solve_timings(avm_ctx* c, bool marg) {
  store_elapsed(c, "preint", M_PREINT, M_SOLVE);
  store_elapsed(c, "window_solve", M_SOLVE, M_SOLVE_END);
  c->last_ms["marginalize"] = 0.f, c->last_ms["prior_eig"] = 0.f;
  if (marg) store_elapsed(c, "marginalize", M_MARGINALIZE, M_PRIOR_ROOT);
  if (marg) store_elapsed(c, "prior_eig", M_PRIOR_ROOT, M_PRIOR_ROOT_END);
}
}  // namespace

extern "C" {
int avm_window_solve_batch(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* batch, avm_prior_out* prior_out,
                           avm_solve_summary* summary) {
  return avm_window_solve_batch_flags(c, opt, mem, batch, nullptr, prior_out, summary);
}

int avm_window_solve_batch_flags(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* batch, const int32_t* flags,
                                 avm_prior_out* prior_out, avm_solve_summary* summary) {
  return avm_window_solve_batch_relo(c, opt, mem, batch, flags, nullptr, prior_out, summary);
}

// relo_active == null: the call avm_window_solve_batch_flags always was.  With it, the batch is split (include/avm.h has the contract):
// the windows without a pending relocalization take the kernel form the batch would get without the relocalization arrays, the others
// the extended kernel, both through the list builds of the kernels; the marginalization runs once on the whole batch.
int avm_window_solve_batch_relo(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* batch, const int32_t* flags,
                                const int32_t* relo_active, avm_prior_out* prior_out, avm_solve_summary* summary) {
  if (!enter(c)) return AVM_ERR_INVALID;
  int rc = check_window_batch(c, opt, batch);
  if (rc != AVM_OK) return rc;
  if (relo_active && (!batch->relo_n || !batch->relo_frame))
    return fail(c, AVM_ERR_INVALID, "relo_active is given but relo_n / relo_frame / relo_feat / relo_xy / relo_pose of the batch is NULL");
  // (with per-window flags the forms and the buffers are chosen as for a marginalizing batch: which values occur is known after the check)
  bool marg = flags || opt->marginalization_flag != AVM_MARGIN_NONE;
  if (marg && (rc = check_prior_out(c, prior_out)) != AVM_OK) return rc;
  if (batch->n_windows == 0) return AVM_OK;
  // table check: host tables on the host, now; device-resident ones by a kernel whose verdict is read while the pre-integration runs.
  // On the early error paths below a check in flight is drained before the caller may free its tables.  The per-window flags are checked
  // in the same pass: no kernel reads a flag before the verdict is in.
  int tp_misfit = 0;
  unsigned flags_seen = 0;
  FlagCheck check;
  const FlagRule fr{flags, (1u << AVM_MARGIN_OLD) | (1u << AVM_MARGIN_SECOND_NEW) | (1u << AVM_MARGIN_NONE)};
  // relo_active: the two lists of windows.  Host memory: built here and staged; device memory: by a kernel that runs in the table check's
  // pass, the number of extended windows travels back as the verdict's fourth word (no wait of its own).  With estimate_extrinsic /
  // estimate_td every window is an extended one: no lists, relo_active goes to the kernel as it is.
  const bool est_x = opt->estimate_extrinsic != 0 || opt->estimate_td != 0;
  const bool split = relo_active != nullptr && !est_x;
  const int B = batch->n_windows;
  const int32_t *d_lists = nullptr, *d_active = relo_active;
  int n_ext = 0;
  std::vector<int32_t> h_lists;  // (alive until the call's synchronize)
  if (mem == AVM_MEM_HOST) {
    rc = validate_windows(c, mem, batch, CHK_TRACKS | CHK_IMU | CHK_PRIOR, &tp_misfit, fr, SOLVE_FLAG_RULES, &flags_seen);
    if (rc == AVM_OK && split) {
      h_lists.resize(2 * (size_t)B);
      int n_plain = 0;
      for (int w = 0; w < B; w++) {
        if (relo_active[w]) h_lists[(size_t)B + n_ext++] = w;
        else h_lists[n_plain++] = w;
      }
      const void* dl;
      if ((rc = stage_array(c, "w_lists", h_lists.data(), sizeof(int32_t) * h_lists.size(), &dl)) == AVM_OK) d_lists = static_cast<const int32_t*>(dl);
    }
    if (rc == AVM_OK && relo_active) {
      const void* da;
      if ((rc = stage_array(c, "w_relo_active", relo_active, sizeof(int32_t) * B, &da)) == AVM_OK) d_active = static_cast<const int32_t*>(da);
    }
  } else if (split) {
    int32_t* lists = static_cast<int32_t*>(pool_get(c, "w_lists", sizeof(int32_t) * 2 * (size_t)B));
    if (!lists) return fail(c, AVM_ERR_HIP, "hipMalloc failed (window lists)");
    d_lists = lists;
    if ((rc = null_window_tables(c, batch, CHK_TRACKS | CHK_IMU | CHK_PRIOR)) != AVM_OK) return rc;
    rc = flag_begin(
        c, 4,
        [&](int* flag) {
          const hipError_t e = launch_validate_windows(*batch, CHK_TRACKS | CHK_IMU | CHK_PRIOR, flag, c->stream, fr);
          return e != hipSuccess ? e : launch_solve_partition(B, relo_active, lists, flag + 3, c->stream);
        },
        &check);
  } else {
    rc = validate_windows_begin(c, batch, CHK_TRACKS | CHK_IMU | CHK_PRIOR, &check, fr);
  }
  if (rc != AVM_OK) return rc;

  // choose forms (the slots for the throughput forms are sized before the priors' verdict is in: a batch that then takes the latency forms uses half of them)
  // (split: the plain windows' forms from the WHOLE batch as if it had no relocalization arrays; the marginalization takes the throughput form
  //  when either view of the batch gives it)
  const bool extended = est_x || batch->relo_n != nullptr;
  auto forms_of = [&](int misfit) {
    SolveForms f = choose_forms(B, c->n_slots, extended && !split, marg, misfit);
    if (split) {
      const SolveForms fx = choose_forms(B, c->n_slots, true, marg, misfit);
      f.big_x = fx.big_x, f.marg_tp = f.marg_tp || fx.marg_tp;
    }
    return f;
  };
  SolveForms forms = forms_of(0);
  if ((rc = ensure_window_buffers(c, batch->n_windows, batch->max_samp, forms.tp || forms.big_x)) != AVM_OK) {
    if (check.dev) (void)hipStreamSynchronize(c->stream);
    return rc;
  }

  // stage
  avm_window_batch d;
  bool packed;
  if ((rc = windows_on_device(c, mem, batch, &d, &packed)) != AVM_OK) return rc;
  avm_solve_summary* d_sum = summary;
  if (mem == AVM_MEM_HOST && summary) {
    d_sum = static_cast<avm_solve_summary*>(pool_get(c, "w_summary", sizeof(avm_solve_summary) * batch->n_windows));
    if (!d_sum) return fail(c, AVM_ERR_HIP, "hipMalloc failed (summary)");
  }

  // pre-integrate, and the verdict of the table check
  HIPCHK(c, mark(c, M_PREINT));
  if ((rc = run_preint(c, opt, &d)) != AVM_OK) {
    if (check.dev) (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  HIPCHK(c, mark(c, M_SOLVE));
  if (check.dev && (rc = flag_end(c, check, "window", SOLVE_FLAG_RULES, &tp_misfit)) != AVM_OK) return rc;
  if (check.dev && flags) flags_seen = (unsigned)check.host[2];
  if (check.dev && split) n_ext = check.host[3];
  forms = forms_of(tp_misfit);
  if (split && n_ext == B) forms.tp = false;  // (no plain window: the extended kernel has the latency form only)

  // solve (a split batch whose windows are all of one kind: the launches without a list)
  SolveArgs sa = solve_args(c, opt, d, d_sum);
  const bool lists_run = relo_active && (est_x || (n_ext > 0 && n_ext < B));
  if (lists_run)
    rc = run_solve_split(c, sa, forms, est_x ? nullptr : d_lists, n_ext, d_active);
  else
    rc = run_solve(c, sa, split ? n_ext == B : extended, forms);
  if (rc != AVM_OK) return rc;
  HIPCHK(c, mark(c, M_SOLVE_END));
  {
    const int64_t nx = relo_active ? (est_x ? B : n_ext) : (extended ? B : 0);
    c->last_split[0] = B - nx, c->last_split[1] = nx, c->last_split[2] = nx == B ? -1 : (forms.tp ? 1 : 0), c->last_split[3] = lists_run ? 1 : 0;
  }

  // marginalize and take the square root.  Per-window flags that are all AVM_MARGIN_NONE: no launch, every window reports n = -1
  int* marg_err = nullptr;
  PackedBack prior_back;
  if (flags && flags_seen == 1u << AVM_MARGIN_NONE) {
    marg = false;
    const size_t nb = sizeof(int32_t) * batch->n_windows;
    if (mem == AVM_MEM_HOST) {
      std::memset(prior_out->n, 0xff, nb), std::memset(prior_out->nblk, 0, nb);
    } else {
      HIPCHK(c, hipMemsetAsync(prior_out->n, 0xff, nb, c->stream));
      HIPCHK(c, hipMemsetAsync(prior_out->nblk, 0, nb, c->stream));
    }
  }
  if (marg && flags) {
    const void* dflags = flags;
    if (mem == AVM_MEM_HOST && (rc = stage_array(c, "w_marg_flags", flags, sizeof(int32_t) * batch->n_windows, &dflags)) != AVM_OK) return rc;
    sa.marg_flags = static_cast<const int32_t*>(dflags);
  }
  if (marg && (rc = run_marginalize(c, opt, mem, sa, forms.marg_tp, prior_out, &marg_err, &prior_back)) != AVM_OK) return rc;

  // return outputs: the states (a packed batch: its four head blocks as one copy), para_Td / relo_Pose, the summaries - one synchronize
  PackedBack states_back;
  if ((rc = copy_back(c, mem, WINDOWS, U_WHOLE, batch, &d, batch, packed ? N_STATES : 0, "w_states", &states_back)) != AVM_OK) return rc;
  if (mem == AVM_MEM_HOST && summary)
    HIPCHK(c, hipMemcpyAsync(summary, d_sum, sizeof(avm_solve_summary) * batch->n_windows, hipMemcpyDeviceToHost, c->stream));
  int marg_err_host = 0x7f7f7f7f;
  if (marg_err) HIPCHK(c, hipMemcpyAsync(&marg_err_host, marg_err, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  scatter(WINDOWS, U_WHOLE, batch, batch, states_back);  // (also before a capacity error: the states WERE solved)
  if (marg_err_host != 0x7f7f7f7f) {
    c->err = "window " + std::to_string(marg_err_host) +
             ": the new prior does not fit (prior_out->max_prior / max_pblk too small, or more than 76 rows / 16 blocks to keep); "
             "the states were solved, prior_out is not valid";
    return AVM_ERR_CAPACITY;
  }
  if (marg) scatter(PRIOR_OUT, U_WHOLE, prior_out, batch, prior_back);

  record_solve_timings(c, marg);
  return AVM_OK;
}

int avm_window_solve(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* window, avm_prior_out* prior_out,
                     avm_solve_summary* summary) {
  if (!c) return AVM_ERR_INVALID;
  if (!window || window->n_windows != 1) return fail(c, AVM_ERR_INVALID, "avm_window_solve takes exactly one window (n_windows == 1)");
  return avm_window_solve_batch(c, opt, mem, window, prior_out, summary);
}

int avm_window_eval_factors(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* batch, int apply_loss,
                            double* proj_r, double* proj_J, double* imu_r, double* imu_J, double* prior_res, double* cost) {
  if (!enter(c)) return AVM_ERR_INVALID;
  int rc = check_window_batch(c, opt, batch);
  if (rc != AVM_OK) return rc;
  if (batch->n_windows == 0) return AVM_OK;
  if ((rc = validate_windows(c, mem, batch, CHK_TRACKS | CHK_IMU | CHK_PRIOR)) != AVM_OK) return rc;
  if ((rc = ensure_window_buffers(c, batch->n_windows, batch->max_samp)) != AVM_OK) return rc;
  avm_window_batch d;
  if ((rc = windows_on_device(c, mem, batch, &d)) != AVM_OK) return rc;
  const size_t B = batch->n_windows;
  EvalArgs ea;
  struct Out {
    double** dst;
    double* host;
    size_t n;
    const char* name;
  };
  Out outs[6] = {{&ea.proj_r, proj_r, B * batch->max_obs * 2, "e_pr"},   {&ea.proj_J, proj_J, B * batch->max_obs * 26, "e_pJ"},
                 {&ea.imu_r, imu_r, B * 150, "e_ir"},                      {&ea.imu_J, imu_J, B * 4500, "e_iJ"},
                 {&ea.prior_res, prior_res, B * batch->max_prior, "e_pres"}, {&ea.cost, cost, B, "e_cost"}};
  for (auto& o : outs) {
    if ((rc = array_out(c, mem, o.name, o.host, o.n, o.dst, "eval out")) != AVM_OK) return rc;
    if (mem == AVM_MEM_HOST && o.host) HIPCHK(c, hipMemsetAsync(*o.dst, 0, o.n * sizeof(double), c->stream));
  }
  if ((rc = run_preint(c, opt, &d)) != AVM_OK) return rc;
  ea.b = d, ea.opt = *opt, ea.apply_loss = apply_loss;
  ea.pre_delta = c->pre_delta, ea.pre_jac = c->pre_jac, ea.pre_sqrt = c->pre_sqrt, ea.pre_sum_dt = c->pre_sum;
  HIPCHK(c, launch_eval_factors(ea, c->stream));
  for (auto& o : outs)
    if ((rc = array_back(c, mem, o.host, *o.dst, o.n)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

int avm_projection_td_eval(avm_ctx* c, avm_mem mem, const avm_td_factor_batch* f, double* residual, double* jac) {
  if (!enter(c)) return AVM_ERR_INVALID;
  if (!f || !residual || f->n < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (f->n == 0) return AVM_OK;
  const size_t n = f->n;
  avm_td_factor_batch d;
  int rc = on_device(c, mem, TD_FACTORS, U_WHOLE, f, &d);
  if (rc != AVM_OK) return rc;
  double *dr, *dj;
  if ((rc = array_out(c, mem, "td_res", residual, n * 2, &dr, "td factor out")) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "td_jac", jac, n * 40, &dj, "td factor out")) != AVM_OK) return rc;
  HIPCHK(c, launch_projection_td_eval(d, dr, dj, c->stream));
  if ((rc = array_back(c, mem, residual, dr, n * 2)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, jac, dj, n * 40)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}
}  // extern "C"
