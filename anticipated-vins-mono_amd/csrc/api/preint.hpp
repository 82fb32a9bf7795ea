// api/preint.hpp - the ctx's window buffers, the pre-integration with its content-checked cache, avm_imu_preintegrate_batch

namespace {
// AVM_PREINT_CACHE=0: run_preint integrates every interval on every call and keeps no keys (read on every call: tests, A/B runs)
bool preint_cache_enabled() {
  const char* e = getenv("AVM_PREINT_CACHE");
  return !(e && e[0] == '0');
}

int ensure_window_buffers(avm_ctx* c, int n_windows, int max_samp, bool tp = false) {
  // (the throughput form of the solve runs two workgroups per CU: twice the slots; allocated when a batch first takes it)
  const int want = tp ? 2 * c->n_slots : c->n_slots;
  // the keys of the pre-integration cache: sized by the samples per interval as well, so they grow on their own when only max_samp does
  const size_t key_want = preint_cache_enabled() && max_samp >= 0 ? (size_t)n_windows * 10 * (size_t)preint_key_words(max_samp) : 0;
  if (!c->scratch || c->scratch_slots < want || (size_t)n_windows > c->pre_cap || key_want > c->pk.key_cap) c->n_allocs++;
  if (!c->scratch || c->scratch_slots < want) {
    if (c->scratch) (void)hipFree(c->scratch), c->scratch = nullptr;
    if (c->iscratch) (void)hipFree(c->iscratch), c->iscratch = nullptr;
    c->scratch_slots = 0;
    HIPCHK(c, hipMalloc(&c->scratch, sizeof(double) * Scratch::TOTAL * want));
    HIPCHK(c, hipMalloc(&c->iscratch, sizeof(int32_t) * ISCRATCH * want));
    HIPCHK(c, hipMemsetAsync(c->scratch, 0, sizeof(double) * Scratch::TOTAL * want, c->stream));
    HIPCHK(c, hipMemsetAsync(c->iscratch, 0, sizeof(int32_t) * ISCRATCH * want, c->stream));
    c->scratch_slots = want;
  }
  if ((size_t)n_windows > c->pre_cap) {
    c->pre_cap = 0;  // a failed hipMalloc below must not leave the old capacity next to freed / partial buffers
    for (double** p : {&c->pre_delta, &c->pre_jac, &c->pre_cov, &c->pre_sqrt, &c->pre_sum})
      if (*p) (void)hipFree(*p), *p = nullptr;
    for (int32_t** p : {&c->pk.valid, &c->pk.todo, &c->pk.count})
      if (*p) (void)hipFree(*p), *p = nullptr;
    c->pk.all_void = true;  // the results the keys stood for are gone
    const size_t iv = (size_t)n_windows * 10;
    HIPCHK(c, hipMalloc(&c->pre_delta, sizeof(double) * iv * 10));
    HIPCHK(c, hipMalloc(&c->pre_jac, sizeof(double) * iv * 225));
    HIPCHK(c, hipMalloc(&c->pre_cov, sizeof(double) * iv * 225));
    HIPCHK(c, hipMalloc(&c->pre_sqrt, sizeof(double) * iv * 225));
    HIPCHK(c, hipMalloc(&c->pre_sum, sizeof(double) * iv));
    HIPCHK(c, hipMalloc(&c->pk.valid, sizeof(int32_t) * iv));
    HIPCHK(c, hipMalloc(&c->pk.todo, sizeof(int32_t) * iv));
    HIPCHK(c, hipMalloc(&c->pk.count, sizeof(int32_t) * 2));
    HIPCHK(c, hipMemsetAsync(c->pk.count, 0, sizeof(int32_t) * 2, c->stream));
    c->pk.turn = 0, c->pk.last_count = nullptr, c->pk.recomputed = 0;
    c->pre_cap = n_windows;
  }
  if (key_want > c->pk.key_cap) {
    c->pk.key_cap = 0, c->pk.all_void = true;
    if (c->pk.key) (void)hipFree(c->pk.key), c->pk.key = nullptr;
    HIPCHK(c, hipMalloc(&c->pk.key, sizeof(unsigned long long) * key_want));
    c->pk.key_cap = key_want;
  }
  return AVM_OK;
}

int run_preint(avm_ctx* c, const avm_options* opt, const avm_window_batch* d) {
  PreintArgs pa;
  pa.n_windows = d->n_windows, pa.max_samp = d->max_samp;
  pa.imu_n = d->imu_n, pa.imu_dt = d->imu_dt, pa.imu_acc = d->imu_acc, pa.imu_gyr = d->imu_gyr;
  pa.imu_lin_ba = d->imu_lin_ba, pa.imu_lin_bg = d->imu_lin_bg;
  pa.acc_n = opt->acc_n, pa.gyr_n = opt->gyr_n, pa.acc_w = opt->acc_w, pa.gyr_w = opt->gyr_w;
  pa.out_delta = c->pre_delta, pa.out_jacobian = c->pre_jac, pa.out_covariance = c->pre_cov, pa.out_sum_dt = c->pre_sum,
  pa.out_sqrt_info = c->pre_sqrt;
  // The stored results depend on the IMU tables and the four noise densities only, and in a stream one image changes one interval of ten:
  // preint_match_kernel compares every interval's inputs with the copy its stored results were computed from and lists the ones that
  // differ; the two kernels then work from that list (no host read of its length: their grid is sized for every interval).  The host
  // only knows what makes every key void: another batch shape, other noise densities, reallocated buffers, a call that went without.
  avm_ctx::PreintCache& k = c->pk;
  const int64_t n_iv = (int64_t)d->n_windows * 10;
  k.examined = n_iv;
  const bool cached = preint_cache_enabled() && d->max_samp >= 0 && k.key && k.valid &&
                      (size_t)n_iv * (size_t)preint_key_words(d->max_samp) <= k.key_cap && (size_t)d->n_windows <= c->pre_cap;
  if (!cached) {
    k.all_void = true, k.recomputed = n_iv;
    launch_preint(pa, c->stream);
    HIPCHK(c, hipGetLastError());
    return AVM_OK;
  }
  const double noise[4] = {opt->acc_n, opt->gyr_n, opt->acc_w, opt->gyr_w};
  if (k.all_void || k.n_windows != d->n_windows || k.max_samp != d->max_samp || std::memcmp(k.noise, noise, sizeof noise) != 0) {
    HIPCHK(c, hipMemsetAsync(k.valid, 0, sizeof(int32_t) * (size_t)n_iv, c->stream));
    k.all_void = false, k.n_windows = d->n_windows, k.max_samp = d->max_samp;
    std::memcpy(k.noise, noise, sizeof noise);
  }
  PreintKeys pk;
  pk.key = k.key, pk.valid = k.valid, pk.todo = k.todo;
  pk.count = k.count + k.turn, pk.count_next = k.count + (1 - k.turn);
  launch_preint_match(pa, pk, c->stream);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    k.all_void = true;
    c->err = std::string("launch_preint_match: ") + hipGetErrorString(e);
    return AVM_ERR_HIP;
  }
  k.turn = 1 - k.turn, k.last_count = pk.count, k.recomputed = -1;
  pa.todo = k.todo, pa.todo_count = pk.count;
  launch_preint(pa, c->stream);
  if (const hipError_t e = hipGetLastError(); e != hipSuccess) {
    k.all_void = true;  // the comparison has stored keys for results that were never computed
    c->err = std::string("launch_preint: ") + hipGetErrorString(e);
    return AVM_ERR_HIP;
  }
  return AVM_OK;
}

// The cache follows a roll of the windows (avm_slide_window*), when its keys belong to a batch of this shape: otherwise - and whenever the
// caller slid other windows than it last pre-integrated - the next comparison simply finds more intervals changed.
int roll_preint_cache(avm_ctx* c, const avm_window_batch& d, const int32_t* dflags, int flag) {
  avm_ctx::PreintCache& k = c->pk;
  k.rolled = 0;
  c->last_ms["preint_roll"] = 0.0f;
  if (!preint_cache_enabled() || k.all_void || !k.key || k.n_windows != d.n_windows || k.max_samp != d.max_samp) return AVM_OK;
  PreintRoll r;
  r.n_windows = d.n_windows, r.key_words = (int)preint_key_words(d.max_samp), r.flags = dflags, r.flag = flag;
  r.key = k.key, r.valid = k.valid;
  r.delta = c->pre_delta, r.jac = c->pre_jac, r.cov = c->pre_cov, r.sqrt_info = c->pre_sqrt, r.sum_dt = c->pre_sum;
  HIPCHK(c, mark(c, M_ROLL));
  launch_preint_roll(r, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, mark(c, M_ROLL_END));
  k.rolled = d.n_windows;
  return AVM_OK;
}
}  // namespace

extern "C" {
int avm_imu_preintegrate_batch(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* batch, double* out_delta,
                               double* out_jacobian, double* out_covariance, double* out_sum_dt) {
  if (!enter(c)) return AVM_ERR_INVALID;
  int rc = check_window_batch(c, opt, batch, true);
  if (rc != AVM_OK) return rc;
  if (batch->n_windows == 0) return AVM_OK;
  if ((rc = validate_windows(c, mem, batch, CHK_IMU)) != AVM_OK) return rc;
  if ((rc = ensure_window_buffers(c, batch->n_windows, batch->max_samp)) != AVM_OK) return rc;
  avm_window_batch d;
  if ((rc = windows_on_device(c, mem, batch, &d)) != AVM_OK) return rc;
  if ((rc = run_preint(c, opt, &d)) != AVM_OK) return rc;
  const size_t iv = (size_t)batch->n_windows * 10;
  if ((rc = array_from_ctx(c, mem, out_delta, c->pre_delta, iv * 10)) != AVM_OK) return rc;
  if ((rc = array_from_ctx(c, mem, out_jacobian, c->pre_jac, iv * 225)) != AVM_OK) return rc;
  if ((rc = array_from_ctx(c, mem, out_covariance, c->pre_cov, iv * 225)) != AVM_OK) return rc;
  if ((rc = array_from_ctx(c, mem, out_sum_dt, c->pre_sum, iv)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}
}  // extern "C"
