// api/ctx.hpp - the ctx and what every entry point starts from: avm_ctx, HIPCHK, enter, fail, the pool, the timing marks; create / destroy / last_error / stream / last_kernel_ms, the default options

// The timing marks of the entry points: one event per name, each named for the span it opens (X_END closes the last span of its
// group), so no two meanings share an event and any two helpers may be composed in one call.  mark() records one on the ctx's stream;
// store_elapsed() puts the time between two - of a call that has synchronized - under a key of avm_last_kernel_ms.
enum Mark {
  M_CHECK, M_CHECK_END,                                                                  // a check kernel that runs on its own (track_check)
  M_KERNELS, M_KERNELS_END,                                                              // the kernels of an entry point that has one span
  M_PREINT, M_SOLVE, M_SOLVE_END,                                                        // avm_window_solve_batch: pre-integration | solve
  M_MARGINALIZE, M_PRIOR_ROOT, M_PRIOR_ROOT_END,                                         // ... marginalization | square root of the prior
  M_ROLL, M_ROLL_END,                                                                    // the pre-integration cache's roll behind a slide
  M_ALIGN_GYRO_BIAS, M_ALIGN_SOLVE, M_ALIGN_APPLY, M_ALIGN_END,                          // avm_visual_initial_align_batch
  M_SPLIT, M_SPLIT_END, M_MERGE, M_MERGE_END,                                            // avm_fsel_select_image_batch around the selection
  M_GATHER, M_GATHER_END,                                                                // avm_gather_states
  M_SFM_CHAIN_BA, M_SFM_FRAME_PNP, M_SFM_END,                                            // avm_global_sfm_batch
  N_MARKS
};

struct avm_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
  int n_slots = 0;
  int max_windows = 0;  // avm_config::max_windows (0: no limit stated); avm_visual_initial_align_batch refuses larger batches
  // device buffers owned by the ctx
  double* scratch = nullptr;
  int32_t* iscratch = nullptr;
  int64_t n_allocs = 0;       // device / pinned (re)allocations since avm_create (avm_debug_counters: a timed region should see none)
  int last_marg_windows = 0;  // batch size of the last marginalization (its per-window "the one-wavefront kernel finished it" flags: pool "pe_done")
  bool last_solve_tp = false;  // which form of the solve kernel the last avm_window_solve_batch took (avm_debug_last_solve_form)
  bool last_marg_tp = false;   // ... and which form of the marginalization kernel (avm_debug_last_marg_form)
  // avm_debug_last_split: windows the last solve took as plain / as extended, the plain ones' form (0 latency, 1 throughput, -1 none), 1: the list builds ran
  int64_t last_split[4] = {0, 0, -1, 0};
  int scratch_slots = 0;  // slots allocated (n_slots, or 2 n_slots once a batch has taken the throughput form of the solve)
  double *pre_delta = nullptr, *pre_jac = nullptr, *pre_cov = nullptr, *pre_sqrt = nullptr, *pre_sum = nullptr;
  size_t pre_cap = 0;  // windows
  // What pre_* were computed from (run_preint): per interval a copy of the inputs preint_kernel read (its key) and whether that copy is
  // valid, the list of intervals the last comparison found changed, and two counters that take turns.  The device-side comparison is
  // the only thing that declares an interval unchanged; the host only remembers what makes EVERY key void.
  struct PreintCache {
    unsigned long long* key = nullptr;  // [pre_cap * 10][preint_key_words(max_samp)], key_cap words
    size_t key_cap = 0;
    int32_t *valid = nullptr, *todo = nullptr, *count = nullptr;  // [pre_cap * 10], [pre_cap * 10], [2]
    bool all_void = true;                                         // buffers (re)allocated, or pre_* written without the comparison
    int n_windows = -1, max_samp = -1;                            // of the call the keys belong to
    double noise[4] = {0, 0, 0, 0};                               // acc_n, gyr_n, acc_w, gyr_w of that call
    int turn = 0;                                                 // which counter the next comparison counts in
    // avm_debug_preint_cache: the last run_preint and the last slide
    int64_t examined = 0, recomputed = 0;  // recomputed < 0: on the device, in *last_count
    const int32_t* last_count = nullptr;
    int64_t rolled = 0;
  } pk;
  long long* prof = nullptr;  // [n_slots][32], enabled by AVM_PROFILE=1
  // staging pool for AVM_MEM_HOST calls (pool_get): name -> (ptr, bytes), device memory ...
  std::map<std::string, std::pair<void*, size_t>> pool;
  // ... and pinned host memory (small AVM_MEM_HOST batches travel as one packed copy each way)
  std::map<std::string, std::pair<void*, size_t>> pinned;
  hipEvent_t marks[N_MARKS];  // created by avm_create
  hipEvent_t ev_flag = nullptr;  // recorded behind the copy of a table check's verdict (flag_begin)
  std::map<std::string, float> last_ms;
  int last_fsel_mode = -1;  // the form the last avm_fsel_select_batch took (3: fsel_solo_kernel)
  int64_t last_fsel_evals = -1;  // candidate evaluations the last select executed on the device (solo form: counted by the kernel; else -1)
  int fsel_frame_mode = 2;  // how a single-frame select runs (avm_fsel_select_batch); AVM_FSEL_FRAME=0/1/2 caps it
  ncclComm_t comm = nullptr;  // avm_comm_init
  int comm_ranks = 0;
  double wall_clock_hz = 1.0e8;  // rate of wall_clock64() (hipDeviceAttributeWallClockRate; 100 MHz on gfx950)
  // fallbacks of the selector's all-rounds-in-one-launch kernel (avm_fsel_fallback_stats)
  int64_t fsel_calls = 0, fsel_reruns = 0, fsel_failed_launches = 0;
  int fsel_cooldown = 0;  // calls left before a degraded ctx probes the fast mode again
  int fsel_backoff = 16;  // the next cool-down (doubles with every failed probe up to 4096 calls, back to 16 after a fast-mode call that went through)
};

namespace {
#define HIPCHK(ctx, call)                                                                  \
  do {                                                                                     \
    hipError_t e__ = (call);                                                               \
    if (e__ != hipSuccess) {                                                               \
      (ctx)->err = std::string(#call) + ": " + hipGetErrorString(e__);                     \
      return AVM_ERR_HIP;                                                                  \
    }                                                                                      \
  } while (0)

// what an entry point that touches the device begins with: false for a null ctx, else the ctx's device made current
bool enter(avm_ctx* c) { return c && ((void)hipSetDevice(c->device), true); }

int fail(avm_ctx* c, int code, const char* msg) {
  c->err = msg;
  return code;
}

// A buffer the ctx keeps under `name` and hands to every later call that asks for it by that name: device memory, or (PINNED) page-locked
// host memory - the two kinds have name spaces of their own.  It grows, never shrinks; avm_debug_counters reports the (re)allocations.
constexpr bool PINNED = true;
void* pool_get(avm_ctx* c, const std::string& name, size_t bytes, bool pinned = false) {
  auto& e = (pinned ? c->pinned : c->pool)[name];
  if (e.second < bytes || e.first == nullptr) {
    c->n_allocs++;
    if (e.first) (void)(pinned ? hipHostFree(e.first) : hipFree(e.first));
    e.first = nullptr;
    const size_t n = bytes ? bytes : 8;
    if ((pinned ? hipHostMalloc(&e.first, n, hipHostMallocDefault) : hipMalloc(&e.first, n)) != hipSuccess) return nullptr;
    e.second = bytes;
  }
  return e.first;
}

hipError_t mark(avm_ctx* c, Mark m) { return hipEventRecord(c->marks[m], c->stream); }
// key = (a1 - a0) + (b1 - b0), the second span optional; a span whose marks were never recorded leaves the key as it was
void store_elapsed(avm_ctx* c, const char* key, Mark a0, Mark a1, Mark b0 = N_MARKS, Mark b1 = N_MARKS) {
  float a = 0, b = 0;
  if (hipEventElapsedTime(&a, c->marks[a0], c->marks[a1]) != hipSuccess) return;
  if (b0 != N_MARKS && hipEventElapsedTime(&b, c->marks[b0], c->marks[b1]) != hipSuccess) return;
  c->last_ms[key] = a + b;
}
}  // namespace

extern "C" {
const char* avm_version(void) { return "avm-mi355x 0.1 (gfx950, fp64)"; }
int avm_abi_version(void) { return AVM_ABI_VERSION; }

int avm_default_options(avm_options* o) {
  if (!o) return AVM_ERR_INVALID;
  std::memset(o, 0, sizeof *o);
  o->max_num_iterations = 8;  // config/euroc/euroc_config.yaml:55
  o->estimate_extrinsic = 0;
  o->estimate_td = 0;
  o->marginalization_flag = AVM_MARGIN_OLD;
  o->focal_length = 460.0;  // parameters.h:13
  o->g[0] = 0, o->g[1] = 0, o->g[2] = 9.81007;
  o->acc_n = 0.08, o->gyr_n = 0.004, o->acc_w = 0.00004, o->gyr_w = 2.0e-6;
  o->cauchy_a = 1.0;
  o->max_sum_dt = 10.0;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
  o->marg_eps = 1e-8;
  o->tr = 0.0, o->row = 480.0;  // global shutter (config/euroc/euroc_config.yaml:66), image_height
  o->max_solver_time_s = 0.0;   // no wall-clock cap (the host sets SOLVER_TIME, estimator.cpp:803-806; avm_host.hpp does)
  o->marg_noise_rel = 1e-18;    // the eigenvalue clamp also tests against the rounding noise of the eigenvector's variables (0: literal).  Round 5: 1e-18
                                // (was 1e-16, which dropped GENUINE weak directions on 11 of 160 stream frames: profiles/r05_noise_rel.md)
  return AVM_OK;
}

int avm_create(const avm_config* cfg, avm_ctx** out) {
  if (!out) return AVM_ERR_INVALID;
  *out = nullptr;
  if (cfg && cfg->abi_version != AVM_ABI_VERSION) return AVM_ERR_INVALID;  // a caller compiled against another avm.h: before anything reads its structs
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return AVM_ERR_NO_DEVICE;
  const int dev = cfg ? cfg->device : 0;
  if (dev < 0 || dev >= ndev) return AVM_ERR_INVALID;
  if (hipSetDevice(dev) != hipSuccess) return AVM_ERR_HIP;
  avm_ctx* c = new avm_ctx();
  c->device = dev;
  c->max_windows = cfg ? cfg->max_windows : 0;
  // A BLOCKING stream (not hipStreamNonBlocking): device-resident buffers are usually produced on the legacy default
  // stream (PyTorch's current stream, plain hipMemcpy), and a blocking stream is ordered after that work and before
  // whatever the default stream does next - AVM_MEM_DEVICE calls need no extra synchronization from such callers.
  // Producers on other streams order themselves against avm_ctx_stream() (see avm.h).
  if (hipStreamCreateWithFlags(&c->stream, hipStreamDefault) != hipSuccess) {
    delete c;
    return AVM_ERR_HIP;
  }
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
    delete c;
    return AVM_ERR_HIP;
  }
  // one resident 512-thread workgroup per CU (the solve kernel takes ~158 KiB of the 160 KiB LDS)
  c->n_slots = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
  {
    int khz = 0;
    if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, dev) == hipSuccess && khz > 0) c->wall_clock_hz = 1.0e3 * khz;
  }
  for (auto& e : c->marks) (void)hipEventCreate(&e);
  (void)hipEventCreateWithFlags(&c->ev_flag, hipEventDisableTiming);
  if (const char* pe = getenv("AVM_PROFILE"))
    if (pe[0] == '1') (void)hipMalloc(&c->prof, sizeof(long long) * PROF_SLOTS * 2 * c->n_slots);  // (two workgroups per CU in the throughput form)
  *out = c;
  return AVM_OK;
}

void avm_destroy(avm_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  (void)avm_comm_destroy(c);
  for (auto& kv : c->pool)
    if (kv.second.first) (void)hipFree(kv.second.first);
  for (auto& kv : c->pinned)
    if (kv.second.first) (void)hipHostFree(kv.second.first);
  for (void* p : {(void*)c->scratch, (void*)c->iscratch, (void*)c->pre_delta, (void*)c->pre_jac, (void*)c->pre_cov, (void*)c->pre_sqrt,
                  (void*)c->pre_sum, (void*)c->pk.key, (void*)c->pk.valid, (void*)c->pk.todo, (void*)c->pk.count})
    if (p) (void)hipFree(p);
  for (auto& e : c->marks) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* avm_last_error(const avm_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

int avm_ctx_stream(const avm_ctx* c, void** stream) {
  if (!c || !stream) return AVM_ERR_INVALID;
  *stream = reinterpret_cast<void*>(c->stream);
  return AVM_OK;
}

int avm_last_kernel_ms(const avm_ctx* c, const char* which, float* ms) {
  if (!c || !which || !ms) return AVM_ERR_INVALID;
  auto it = c->last_ms.find(which);
  if (it == c->last_ms.end()) return AVM_ERR_INVALID;
  *ms = it->second;
  return AVM_OK;
}
}  // extern "C"
