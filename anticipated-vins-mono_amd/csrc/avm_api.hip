// avm_api.hip — the C ABI of include/avm.h on top of the gfx950 kernels.
// Host language is C++ (the reference's host code is C++: vins_estimator/src/estimator.cpp,
// feature_selector.cpp).  No torch types, no exceptions across the boundary.  There is no CPU
// fallback: without a HIP device avm_create() fails with AVM_ERR_NO_DEVICE.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <type_traits>
#include <vector>

#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: the library is dlopen'ed (avm_comm_*), a single-GPU host never needs it

#include "kernels.hpp"
#include "select_image.hpp"

using namespace avm;

namespace {
// raw rccl.h entry points, resolved on first use
struct Rccl {
  void* lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*AllGather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  const char* (*GetErrorString)(ncclResult_t) = nullptr;
  bool ok = false;  // every symbol resolved; decided once for the process
  std::once_flag once;
  bool load() {
    std::call_once(once, [this] {
      for (const char* name : {"librccl.so.1", "librccl.so"}) {
        lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);  // (a process that already maps an RCCL under this soname, e.g. PyTorch's, gets that one)
        if (lib) break;
      }
      if (!lib) return;
      GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
      CommInitRank = reinterpret_cast<decltype(CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
      AllGather = reinterpret_cast<decltype(AllGather)>(dlsym(lib, "ncclAllGather"));
      CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
      GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
      ok = GetUniqueId && CommInitRank && AllGather && CommDestroy && GetErrorString;
      if (!ok) {  // a library without the five entry points is no RCCL for us: never call through a null pointer later
        dlclose(lib);
        lib = nullptr;
      }
    });
    return ok;
  }
};
Rccl& rccl() {
  static Rccl r;
  return r;
}
}  // namespace

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
  avm_solve_summary* d_summary = nullptr;
  long long* prof = nullptr;  // [n_slots][32], enabled by AVM_PROFILE=1
  size_t summary_cap = 0;
  // staging pool for AVM_MEM_HOST calls (pool_get): name -> (ptr, bytes), device memory ...
  std::map<std::string, std::pair<void*, size_t>> pool;
  // ... and pinned host memory (small AVM_MEM_HOST batches travel as one packed copy each way)
  std::map<std::string, std::pair<void*, size_t>> pinned;
  hipEvent_t ev[8];
  hipEvent_t ev_flag = nullptr;  // recorded behind the copy of a table check's verdict (flag_begin)
  std::map<std::string, float> last_ms;
  int last_fsel_mode = -1;  // the form the last avm_fsel_select_batch took (3: fsel_solo_kernel)
  int64_t last_fsel_evals = -1;  // candidate evaluations the last select executed on the device (solo form: counted by the kernel; else -1)
  int fsel_frame_mode = 2;  // how a single-frame select runs (avm_fsel_select_batch); AVM_FSEL_FRAME=0/1/2 caps it
  ncclComm_t comm = nullptr;  // avm_comm_init
  int comm_ranks = 0, comm_rank = 0;
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

const char* table_rule_text(int rule) {
  switch (rule) {
    case BAD_NFEAT: return "n_feat outside [0, max_feat]";
    case BAD_TRACK: return "a feature track leaves the window (need start >= 0, nobs >= 1, start + nobs <= 11)";
    case BAD_ORDER: return "feat_start must be non-decreasing in the feature index (std::list order)";
    case BAD_OBS: return "feat_obs_begin + feat_nobs runs past max_obs";
    case BAD_IMU: return "imu_n outside [0, max_samp]";
    case BAD_PRIOR: return "prior tables inconsistent (prior_n / prior_nblk ranges, block kinds / frames, sizes must add up to prior_n)";
    case BAD_FSEL: return "n_cand / n_used / n_cloud outside their strides, or nr_imu < 0";
  }
  return "bad table";
}

// windows of an entry point that takes per-window marginalization flags (BAD_FLAG is the selector's BAD_FSEL number: a unit has one or the other)
const char* solve_flag_rule_text(int rule) {
  return rule == BAD_FLAG ? "marginalization flag must be AVM_MARGIN_OLD, AVM_MARGIN_SECOND_NEW or AVM_MARGIN_NONE" : table_rule_text(rule);
}
const char* roll_flag_rule_text(int rule) {
  return rule == BAD_FLAG ? "marginalization flag must be AVM_MARGIN_OLD or AVM_MARGIN_SECOND_NEW" : table_rule_text(rule);
}

const char* align_rule_text(int rule) {
  switch (rule) {
    case BAD_ALIGN_FRAMES: return "n_frames outside [2, max_frames]";
    case BAD_ALIGN_IMU: return "imu_n outside [0, max_samp]";
    case BAD_ALIGN_KEYS: return "key_index must be strictly increasing inside [0, n_frames)";
  }
  return "bad table";
}

int report_bad(avm_ctx* c, int first_bad, const char* unit, const char* (*text)(int) = table_rule_text) {
  c->err = std::string(unit) + " " + std::to_string(first_bad / 8) + ": " + text(first_bad % 8);
  return AVM_ERR_INVALID;
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

int flag_end(avm_ctx* c, const FlagCheck& f, const char* unit, int* tp_misfit = nullptr, const char* (*text)(int) = table_rule_text) {
  HIPCHK(c, hipEventSynchronize(c->ev_flag));
  if (tp_misfit) *tp_misfit = f.host[1];
  if (f.host[0] == 0x7f7f7f7f) return AVM_OK;
  (void)hipStreamSynchronize(c->stream);
  return report_bad(c, f.host[0], unit, text);
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
// fr, text, flags_seen: per-window marginalization flags (in `mem` space) checked with the tables, the messages with the flag rule's, and
// which values occur (bit f: some window has flag f)
int validate_windows(avm_ctx* c, avm_mem mem, const avm_window_batch* b, int what, int* tp_misfit = nullptr, const FlagRule& fr = FlagRule(),
                     const char* (*text)(int) = table_rule_text, unsigned* flags_seen = nullptr) {
  if (tp_misfit) *tp_misfit = 0;
  if (flags_seen) *flags_seen = 0;
  if (mem != AVM_MEM_HOST) {
    FlagCheck f;
    int rc = validate_windows_begin(c, b, what, &f, fr);
    if (rc == AVM_OK) rc = flag_end(c, f, "window", tp_misfit, text);
    if (rc == AVM_OK && flags_seen && fr.flags) *flags_seen = (unsigned)f.host[2];
    return rc;
  }
  const int rc = null_window_tables(c, b, what);
  if (rc != AVM_OK) return rc;
  for (int w = 0; w < b->n_windows; w++) {
    int rule = check_window_tables(*b, w, what);
    if (!rule && fr.flags && !flag_allowed(fr, w)) rule = BAD_FLAG;
    if (rule) return report_bad(c, w * 8 + rule, "window", text);
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
    return rc != AVM_OK ? rc : flag_end(c, f, "frame");
  }
  if (!b->n_cand || !b->nr_imu) return fail(c, AVM_ERR_INVALID, "null n_cand / nr_imu");
  for (int p = 0; p < b->n_problems; p++) {
    const int rule = check_fsel_tables(*b, p);
    if (rule) return report_bad(c, p * 8 + rule, "frame");
  }
  return AVM_OK;
}

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

// ---- the arrays of the ABI structs, and how they travel ----
// One descriptor per array: where its pointer sits in the struct, how many elements it has for the struct's dims, and which entry points
// read it (in) and return it to the caller (out).  Every size is written here once; staging, packing and the copies back walk the tables.
struct Field {
  const char* pool;                                  // its staging buffer in the ctx's pool
  size_t offset, elem;                               // the pointer member in the struct; bytes per element
  size_t (*count)(const void* s, const void* dims);  // elements; dims: the batch struct the sizes of an output struct come from (else s itself)
  unsigned in, out;                                  // masks of U_*
  size_t bytes(const void* s, const void* dims) const { return elem * count(s, dims); }
};
struct Table {
  const Field* first;
  size_t n;
  const Field* begin() const { return first; }
  const Field* end() const { return first + n; }
};
template <size_t N>
constexpr Table table_of(const Field (&f)[N]) {
  return {f, N};
}
inline void* get_ptr(const void* s, const Field& f) {
  void* p;
  std::memcpy(&p, static_cast<const char*>(s) + f.offset, sizeof p);
  return p;
}
inline void set_ptr(void* s, const Field& f, const void* p) { std::memcpy(static_cast<char*>(s) + f.offset, &p, sizeof p); }

// who uses an array: the calls that take the whole batch (solve, pre-integration, factor evaluation; struct-valued outputs), and the ones
// that take a subset of the window tables (U_KEYF: the keyframe decision, U_FAIL: the failure detection; the feature manager's calls -
// U_TRK: the track tables of a window with its depths and td rows, U_DEPTH: setDepth, U_PUSH: the raw IMU samples, U_SLIDE_TD: the td rows
// beside U_SLIDE in avm_slide_window_tracks)
enum : unsigned { U_WHOLE = 1, U_TRI = 2, U_SLIDE = 4, U_PROP = 8, U_CLOUD = 16, U_ALIGN = 32, U_KEYF = 64, U_FAIL = 128,
                  U_TRK = 256, U_DEPTH = 512, U_PUSH = 1024, U_SLIDE_TD = 2048 };
constexpr unsigned U_GEOM = U_WHOLE | U_TRI | U_SLIDE | U_CLOUD, U_IMU = U_WHOLE | U_SLIDE | U_PROP;

// S: the struct of the member; D, nmember: the struct the dims come from (`d` in `count`) and its batch size (`N` in `count`)
#define FIELD(S, D, nmember, pool, member, type, count, in, out)                                                              \
  {pool, offsetof(S, member), sizeof(type),                                                                                   \
   [](const void* sp, const void* dp) -> size_t {                                                                             \
     static_assert(std::is_same<std::remove_cv_t<std::remove_pointer_t<decltype(S::member)>>, type>::value, #member);         \
     const S& s = *static_cast<const S*>(sp);                                                                                 \
     const D& d = *static_cast<const D*>(dp);                                                                                 \
     const size_t N = d.nmember;                                                                                              \
     return count;                                                                                                            \
   },                                                                                                                         \
   in, out},

// avm_window_batch.  The four state arrays come first so that the packed path can bring them back with one copy (N_STATES).
#define WIN(member, type, count, in, out) FIELD(avm_window_batch, avm_window_batch, n_windows, "w_" #member, member, type, count, in, out)
const Field WINDOW_FIELDS[] = {
    WIN(pose, double, N * 77, U_GEOM | U_PROP | U_ALIGN | U_FAIL, U_WHOLE | U_SLIDE | U_PROP | U_ALIGN)
    WIN(speedbias, double, N * 99, U_IMU | U_ALIGN | U_FAIL, U_WHOLE | U_SLIDE | U_PROP | U_ALIGN)
    WIN(ex_pose, double, N * 7, U_GEOM | U_ALIGN, U_WHOLE | U_SLIDE)
    WIN(inv_depth, double, N * d.max_feat, U_GEOM | U_ALIGN | U_TRK | U_DEPTH, U_WHOLE | U_TRI | U_SLIDE | U_ALIGN | U_TRK | U_DEPTH)
    WIN(n_feat, int32_t, N, U_GEOM | U_ALIGN | U_KEYF | U_TRK | U_DEPTH, U_SLIDE | U_TRK)
    WIN(feat_start, int32_t, N * d.max_feat, U_GEOM | U_ALIGN | U_KEYF | U_TRK, U_SLIDE | U_TRK)
    WIN(feat_nobs, int32_t, N * d.max_feat, U_WHOLE | U_TRI | U_SLIDE | U_ALIGN | U_KEYF | U_TRK, U_SLIDE | U_TRK)
    WIN(feat_obs_begin, int32_t, N * d.max_feat, U_GEOM | U_ALIGN | U_KEYF | U_TRK, U_SLIDE | U_TRK)
    WIN(obs_xy, double, N * d.max_obs * 2, U_GEOM | U_ALIGN | U_KEYF | U_TRK, U_SLIDE | U_TRK)
    WIN(imu_n, int32_t, N * 10, U_IMU | U_PUSH, U_SLIDE | U_PUSH)
    WIN(imu_dt, double, N * 10 * d.max_samp, U_IMU | U_PUSH, U_SLIDE | U_PUSH)
    WIN(imu_acc, double, N * 10 * (d.max_samp + 1) * 3, U_IMU | U_PUSH, U_SLIDE | U_PUSH)
    WIN(imu_gyr, double, N * 10 * (d.max_samp + 1) * 3, U_IMU | U_PUSH, U_SLIDE | U_PUSH)
    WIN(imu_lin_ba, double, N * 30, U_WHOLE | U_SLIDE, U_SLIDE)
    WIN(imu_lin_bg, double, N * 30, U_WHOLE | U_SLIDE, U_SLIDE)
    WIN(prior_n, int32_t, N, U_WHOLE, 0)
    WIN(prior_nblk, int32_t, N, U_WHOLE, 0)
    WIN(prior_blk_kind, int32_t, N * d.max_pblk, U_WHOLE, 0)
    WIN(prior_blk_frame, int32_t, N * d.max_pblk, U_WHOLE, 0)
    WIN(prior_J, double, N * d.max_prior * d.max_prior, U_WHOLE, 0)
    WIN(prior_r, double, N * d.max_prior, U_WHOLE, 0)
    WIN(prior_x0, double, N * d.max_pblk * 9, U_WHOLE, 0)
    WIN(obs_vel_td, double, N * d.max_obs * 4, U_WHOLE | U_TRK | U_SLIDE_TD, U_TRK | U_SLIDE_TD)
    WIN(td, double, N, U_WHOLE, U_WHOLE)  // para_Td: in/out
    WIN(relo_n, int32_t, N, U_WHOLE, 0)
    WIN(relo_frame, int32_t, N, U_WHOLE, 0)
    WIN(relo_feat, int32_t, N * d.max_feat, U_WHOLE, 0)
    WIN(relo_xy, double, N * d.max_feat * 2, U_WHOLE, 0)
    WIN(relo_pose, double, N * 7, U_WHOLE, U_WHOLE)  // relo_Pose: in/out
    WIN(failure_occur, int32_t, N, U_WHOLE, 0)
    WIN(last_pose0, double, N * 7, U_WHOLE, 0)};
#undef WIN
constexpr Table WINDOWS = table_of(WINDOW_FIELDS);
constexpr int N_STATES = 4;  // pose | speedbias | ex_pose | inv_depth

// avm_prior_out of a batch (one device block "po_pack" in host mode: one memset, and for small batches one copy back)
#define PO(member, type, count) FIELD(avm_prior_out, avm_window_batch, n_windows, "po_" #member, member, type, count, 0, U_WHOLE)
const Field PRIOR_OUT_FIELDS[] = {
    PO(n, int32_t, N) PO(nblk, int32_t, N) PO(blk_kind, int32_t, N * s.max_pblk) PO(blk_frame, int32_t, N * s.max_pblk)
    PO(J, double, N * s.max_prior * s.max_prior) PO(r, double, N * s.max_prior) PO(x0, double, N * s.max_pblk * 9)};
#undef PO
constexpr Table PRIOR_OUT = table_of(PRIOR_OUT_FIELDS);

#define FS(member, type, count) FIELD(avm_fsel_batch, avm_fsel_batch, n_problems, "f_" #member, member, type, count, U_WHOLE, 0)
const Field FSEL_FIELDS[] = {
    FS(hor_pos, double, N * (d.horizon + 1) * 3) FS(hor_quat, double, N * (d.horizon + 1) * 4) FS(nr_imu, int32_t, N) FS(delta_imu, double, N)
    FS(n_cand, int32_t, N) FS(cand_id, int32_t, N * d.max_cand) FS(cand_xy, double, N * d.max_cand * 2) FS(cand_prob, double, N * d.max_cand)
    FS(n_used, int32_t, N) FS(used_id, int32_t, N * d.max_used) FS(used_xy, double, N * d.max_used * 2)
    FS(n_cloud, int32_t, N) FS(cloud_xy, double, N * d.max_cloud * 2) FS(cloud_depth, double, N * d.max_cloud)};
#undef FS
constexpr Table FSEL = table_of(FSEL_FIELDS);

#define FO(pool, member, type) FIELD(avm_fsel_out, avm_fsel_batch, n_problems, pool, member, type, N * d.max_features, 0, U_WHOLE)
const Field FSEL_OUT_FIELDS[] = {FIELD(avm_fsel_out, avm_fsel_batch, n_problems, "fo_n", n_selected, int32_t, N, 0, U_WHOLE)
                                 FO("fo_ids", selected_ids, int32_t) FO("fo_fv", fvalues, double) FO("fo_gap", min_gap, double)};
#undef FO
constexpr Table FSEL_OUT = table_of(FSEL_OUT_FIELDS);

#define TD(member, per) FIELD(avm_td_factor_batch, avm_td_factor_batch, n, "td_" #member, member, double, N * per, U_WHOLE, 0)
const Field TD_FIELDS[] = {TD(pose_i, 7) TD(pose_j, 7) TD(ex_pose, 7) TD(inv_depth, 1) TD(td, 1) TD(pts_i, 2) TD(pts_j, 2)
                           TD(vel_i, 2) TD(vel_j, 2) TD(td_i, 1) TD(td_j, 1) TD(row_i, 1) TD(row_j, 1)};
#undef TD
constexpr Table TD_FACTORS = table_of(TD_FIELDS);

#define HZ(member, type, per) FIELD(avm_fsel_horizon_in, avm_fsel_horizon_in, n_problems, "h_" #member, member, type, N * per, U_WHOLE, 0)
const Field HORIZON_FIELDS[] = {HZ(k_pos, double, 3) HZ(k_quat, double, 4) HZ(k_ba, double, 3) HZ(k1_pos, double, 3) HZ(k1_vel, double, 3)
                                HZ(k1_quat, double, 4) HZ(acc, double, 3) HZ(gyr, double, 3) HZ(nr_imu, int32_t, 1) HZ(delta_imu, double, 1)};
#undef HZ
constexpr Table HORIZON_IN = table_of(HORIZON_FIELDS);

// avm_align_batch / avm_align_out (avm_visual_initial_align_batch)
#define AL(member, type, count) FIELD(avm_align_batch, avm_align_batch, n_windows, "al_" #member, member, type, count, U_WHOLE, 0)
const Field ALIGN_FIELDS[] = {
    AL(n_frames, int32_t, N) AL(frame_R, double, N * d.max_frames * 9) AL(frame_T, double, N * d.max_frames * 3) AL(tic, double, N * 3)
    AL(imu_n, int32_t, N * (d.max_frames - 1)) AL(imu_dt, double, N * (d.max_frames - 1) * d.max_samp)
    AL(imu_acc, double, N * (d.max_frames - 1) * (d.max_samp + 1) * 3) AL(imu_gyr, double, N * (d.max_frames - 1) * (d.max_samp + 1) * 3)
    AL(imu_lin_ba, double, N * (d.max_frames - 1) * 3) AL(imu_lin_bg, double, N * (d.max_frames - 1) * 3) AL(key_index, int32_t, N * AVM_NFRAMES)};
#undef AL
constexpr Table ALIGN = table_of(ALIGN_FIELDS);
#define AO(member, type, count) FIELD(avm_align_out, avm_align_batch, n_windows, "ao_" #member, member, type, count, 0, U_WHOLE)
const Field ALIGN_OUT_FIELDS[] = {AO(ok, int32_t, N) AO(delta_bg, double, N * 3) AO(g_c0, double, N * 3) AO(x, double, N * (3 * d.max_frames + 1))
                                  AO(g_world, double, N * 3) AO(deltas, double, N * (d.max_frames - 1) * 10)};
#undef AO
constexpr Table ALIGN_OUT = table_of(ALIGN_OUT_FIELDS);

constexpr size_t PACK_LIMIT = 4u << 20;  // batches up to 4 MiB (a few windows: the real-time use) travel packed
inline size_t pack_up(size_t n) { return (n + 63) & ~size_t(63); }

// one host array into the pool buffer `name`; a null or empty array gives a null device pointer
int stage_array(avm_ctx* c, const char* name, const void* host, size_t bytes, const void** dev) {
  *dev = nullptr;
  if (!host || bytes == 0) return AVM_OK;
  void* d = pool_get(c, name, bytes);
  if (!d) return fail(c, AVM_ERR_HIP, "hipMalloc failed (staging)");
  HIPCHK(c, hipMemcpyAsync(d, host, bytes, hipMemcpyHostToDevice, c->stream));
  *dev = d;
  return AVM_OK;
}

// Copies the tables of the host struct *h that entry point `use` reads to the device and points *d (a copy of *h) at them.  pack: the pool
// name of the one block - 64-byte aligned parts, in table order, absent tables left out - that the batch travels in when all of it fits
// PACK_LIMIT: one pinned buffer and one copy (22 pageable copies of a few hundred bytes each cost more than the solve's pre-integration
// kernel); nullptr: table by table, each into the pool buffer of its name (behind `prefix`: a call that stages two structs of one kind).
int stage(avm_ctx* c, Table t, unsigned use, const void* h, void* d, const char* pack, bool* packed, const char* prefix = "") {
  size_t total = 0;
  for (const Field& f : t)
    if ((f.in & use) && get_ptr(h, f)) total += pack_up(f.bytes(h, h));
  const bool pk = pack && total <= PACK_LIMIT;
  if (packed) *packed = pk;
  if (!pk) {
    for (const Field& f : t) {
      if (!(f.in & use)) continue;
      const void* dev;
      const int rc = stage_array(c, (std::string(prefix) + f.pool).c_str(), get_ptr(h, f), f.bytes(h, h), &dev);
      if (rc != AVM_OK) return rc;
      set_ptr(d, f, dev);
    }
    return AVM_OK;
  }
  char* hp = static_cast<char*>(pool_get(c, pack, total, PINNED));
  char* dp = static_cast<char*>(pool_get(c, pack, total));
  if (!hp || !dp) return fail(c, AVM_ERR_HIP, "allocation failed (packed staging)");
  size_t off = 0;
  for (const Field& f : t) {
    const void* host = get_ptr(h, f);
    if (!(f.in & use) || !host) continue;
    std::memcpy(hp + off, host, f.bytes(h, h));
    set_ptr(d, f, dp + off);
    off += pack_up(f.bytes(h, h));
  }
  HIPCHK(c, hipMemcpyAsync(dp, hp, total, hipMemcpyHostToDevice, c->stream));
  return AVM_OK;
}

// The caller's struct as the kernels take it: the struct itself (AVM_MEM_DEVICE), or staged (AVM_MEM_HOST).  The entry points that take
// a subset of the window tables never pack.
template <class S>
int on_device(avm_ctx* c, avm_mem mem, Table t, unsigned use, const S* h, S* d, const char* pack = nullptr, bool* packed = nullptr,
              const char* prefix = "") {
  *d = *h;
  if (packed) *packed = false;
  return mem == AVM_MEM_HOST ? stage(c, t, use, h, d, pack, packed, prefix) : AVM_OK;
}

// the whole window batch: packed when it is small and has its four state arrays, the head of the block
int windows_on_device(avm_ctx* c, avm_mem mem, const avm_window_batch* h, avm_window_batch* d, bool* packed = nullptr) {
  const bool states = h->pose && h->speedbias && h->ex_pose && h->inv_depth;
  return on_device(c, mem, WINDOWS, U_WHOLE, h, d, states ? "w_pack" : nullptr, packed);
}

// AVM_MEM_HOST: device arrays for the outputs the caller asked for (the non-null members of *h) in *d, a copy of *h - as parts of one
// block `pack` (its size to *pack_bytes), or each under its own pool name
int alloc_out(avm_ctx* c, Table t, const void* h, void* d, const void* dims, const char* pack = nullptr, size_t* pack_bytes = nullptr) {
  size_t total = 0;
  for (const Field& f : t)
    if (get_ptr(h, f)) total += pack_up(f.bytes(h, dims));
  char* block = pack ? static_cast<char*>(pool_get(c, pack, total)) : nullptr;
  if (pack && !block) return AVM_ERR_HIP;
  if (pack) *pack_bytes = total;
  size_t off = 0;
  for (const Field& f : t) {
    void* dev = nullptr;
    if (get_ptr(h, f)) {
      dev = pack ? block + off : pool_get(c, f.pool, f.bytes(h, dims));
      if (!dev) return AVM_ERR_HIP;
      off += pack_up(f.bytes(h, dims));
    }
    set_ptr(d, f, dev);
  }
  return AVM_OK;
}

// what copy_back left in pinned memory for scatter
struct PackedBack {
  const char* pinned = nullptr;
  int n = 0;
};

// AVM_MEM_HOST: the arrays entry point `use` returns, device -> host, enqueued behind the kernels.  The first n_packed of them are the
// head of one packed block on the device: one copy takes them to the pinned buffer `pin`, and scatter() hands them out after the
// synchronize.  The others go straight into the caller's arrays.
int copy_back(avm_ctx* c, avm_mem mem, Table t, unsigned use, const void* h, const void* d, const void* dims, int n_packed = 0,
              const char* pin = nullptr, PackedBack* back = nullptr) {
  if (mem != AVM_MEM_HOST) return AVM_OK;
  int k = 0;
  size_t bytes = 0;
  const void* head = nullptr;
  for (const Field& f : t) {
    void* host = get_ptr(h, f);
    if (!(f.out & use) || !host) continue;
    const void* dev = get_ptr(d, f);
    if (k++ < n_packed) {
      if (!head) head = dev;
      bytes += pack_up(f.bytes(h, dims));
      if (k < n_packed) continue;
      char* hp = static_cast<char*>(pool_get(c, pin, bytes, PINNED));
      if (!hp) return fail(c, AVM_ERR_HIP, "allocation failed (packed copy back)");
      HIPCHK(c, hipMemcpyAsync(hp, head, bytes, hipMemcpyDeviceToHost, c->stream));
      back->pinned = hp, back->n = n_packed;
    } else if (dev) {
      HIPCHK(c, hipMemcpyAsync(host, dev, f.bytes(h, dims), hipMemcpyDeviceToHost, c->stream));
    }
  }
  return AVM_OK;
}

// after the synchronize: the packed arrays into the caller's own
void scatter(Table t, unsigned use, const void* h, const void* dims, const PackedBack& back) {
  int k = 0;
  size_t off = 0;
  for (const Field& f : t) {
    void* host = get_ptr(h, f);
    if (!(f.out & use) || !host) continue;
    if (k++ == back.n) break;
    std::memcpy(host, back.pinned + off, f.bytes(h, dims));
    off += pack_up(f.bytes(h, dims));
  }
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
  HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
  launch_preint_roll(r, c->stream);
  HIPCHK(c, hipGetLastError());
  HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
  k.rolled = d.n_windows;
  return AVM_OK;
}


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
  HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
  if (sa.marg_flags)  // (the flag per window: the kernels of window_solve_mm.o / window_solve_tp_mm.o)
    HIPCHK(c, marg_tp ? launch_marginalize_tp_mixed(sa, dpo, *marg_err, marg_scale, c->stream) : launch_marginalize_mixed(sa, dpo, *marg_err, marg_scale, c->stream));
  else
    HIPCHK(c, marg_tp ? launch_marginalize_tp(sa, dpo, *marg_err, marg_scale, c->stream) : launch_marginalize(sa, dpo, *marg_err, marg_scale, c->stream));
  c->last_marg_tp = marg_tp;
  HIPCHK(c, hipEventRecord(c->ev[7], c->stream));
  int* pe_done = static_cast<int*>(pool_get(c, "pe_done", sizeof(int) * B));
  if (!pe_done) return fail(c, AVM_ERR_HIP, "hipMalloc failed (prior flags)");
  const double noise_rel = (opt->marg_noise_rel > 0.0 && opt->marg_noise_rel < 1.0) ? opt->marg_noise_rel : 0.0;
  HIPCHK(c, launch_prior_eig(dpo, B, opt->marg_eps, noise_rel, marg_scale, c->prof, pe_done, c->stream));
  c->last_marg_windows = (int)B;
  HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
  return copy_back(c, mem, PRIOR_OUT, U_WHOLE, prior_out, &dpo, dims, po_bytes <= PACK_LIMIT ? (int)PRIOR_OUT.n : 0, "po_pack", back);
}

void record_solve_timings(avm_ctx* c, bool marg) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->last_ms["preint"] = ms;
  if (hipEventElapsedTime(&ms, c->ev[1], c->ev[2]) == hipSuccess) c->last_ms["window_solve"] = ms;
  c->last_ms["marginalize"] = 0.f, c->last_ms["prior_eig"] = 0.f;
  if (marg && hipEventElapsedTime(&ms, c->ev[6], c->ev[7]) == hipSuccess) c->last_ms["marginalize"] = ms;
  if (marg && hipEventElapsedTime(&ms, c->ev[7], c->ev[5]) == hipSuccess) c->last_ms["prior_eig"] = ms;
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
  for (auto& e : c->ev) (void)hipEventCreate(&e);
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
                  (void*)c->pre_sum, (void*)c->d_summary, (void*)c->pk.key, (void*)c->pk.valid, (void*)c->pk.todo, (void*)c->pk.count})
    if (p) (void)hipFree(p);
  for (auto& e : c->ev) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

const char* avm_last_error(const avm_ctx* c) { return c ? c->err.c_str() : "null ctx"; }

// ---- multi-GPU: raw RCCL (rccl.h) all-gather of the final states, one communicator per ctx ---------------------------------
#define RCCLCHK(ctx, call)                                                                                  \
  do {                                                                                                      \
    ncclResult_t r__ = (call);                                                                              \
    if (r__ != ncclSuccess) {                                                                               \
      (ctx)->err = std::string(#call) + ": " + (rccl().GetErrorString ? rccl().GetErrorString(r__) : "rccl error");  \
      return AVM_ERR_HIP;                                                                                   \
    }                                                                                                       \
  } while (0)

int avm_comm_unique_id(avm_ctx* c, void* id) {
  if (!c || !id) return AVM_ERR_INVALID;
  if (!rccl().load()) return fail(c, AVM_ERR_UNSUPPORTED, "librccl.so.1 could not be loaded (dlopen)");
  static_assert(sizeof(ncclUniqueId) == AVM_COMM_ID_BYTES, "ncclUniqueId is 128 bytes");
  ncclUniqueId u;
  RCCLCHK(c, rccl().GetUniqueId(&u));
  std::memcpy(id, &u, sizeof u);
  return AVM_OK;
}

int avm_comm_init(avm_ctx* c, int32_t n_ranks, int32_t rank, const void* id) {
  if (!c || !id || n_ranks < 1 || rank < 0 || rank >= n_ranks) return c ? fail(c, AVM_ERR_INVALID, "bad rank / n_ranks / id") : AVM_ERR_INVALID;
  if (c->comm) return fail(c, AVM_ERR_INVALID, "this ctx already has a communicator (avm_comm_destroy first)");
  if (!rccl().load()) return fail(c, AVM_ERR_UNSUPPORTED, "librccl.so.1 could not be loaded (dlopen)");
  (void)hipSetDevice(c->device);
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  RCCLCHK(c, rccl().CommInitRank(&c->comm, n_ranks, u, rank));
  c->comm_ranks = n_ranks, c->comm_rank = rank;
  return AVM_OK;
}

int avm_gather_states(avm_ctx* c, const double* send, double* recv, size_t count) {
  if (!c || !send || !recv) return c ? fail(c, AVM_ERR_INVALID, "null buffer") : AVM_ERR_INVALID;
  if (!c->comm) return fail(c, AVM_ERR_INVALID, "avm_comm_init has not been called on this ctx");
  (void)hipSetDevice(c->device);
  if (count == 0) return AVM_OK;
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  RCCLCHK(c, rccl().AllGather(send, recv, count, ncclDouble, c->comm, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[3], c->ev[4]) == hipSuccess) c->last_ms["gather_states"] = ms;
  return AVM_OK;
}

int avm_comm_destroy(avm_ctx* c) {
  if (!c) return AVM_ERR_INVALID;
  if (c->comm) {
    (void)hipSetDevice(c->device);
    (void)rccl().CommDestroy(c->comm);
    c->comm = nullptr, c->comm_ranks = 0;
  }
  return AVM_OK;
}

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

int avm_window_solve_batch(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* batch, avm_prior_out* prior_out,
                           avm_solve_summary* summary) {
  return avm_window_solve_batch_flags(c, opt, mem, batch, nullptr, prior_out, summary);
}

int avm_window_solve_batch_flags(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* batch, const int32_t* flags,
                                 avm_prior_out* prior_out, avm_solve_summary* summary) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  int rc = check_window_batch(c, opt, batch);
  if (rc != AVM_OK) return rc;
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
  rc = mem == AVM_MEM_HOST ? validate_windows(c, mem, batch, CHK_TRACKS | CHK_IMU | CHK_PRIOR, &tp_misfit, fr, solve_flag_rule_text, &flags_seen)
                           : validate_windows_begin(c, batch, CHK_TRACKS | CHK_IMU | CHK_PRIOR, &check, fr);
  if (rc != AVM_OK) return rc;

  // choose forms (the slots for the throughput forms are sized before the priors' verdict is in: a batch that then takes the latency forms uses half of them)
  const bool extended = opt->estimate_extrinsic != 0 || opt->estimate_td != 0 || batch->relo_n != nullptr;
  SolveForms forms = choose_forms(batch->n_windows, c->n_slots, extended, marg, 0);
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
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  if ((rc = run_preint(c, opt, &d)) != AVM_OK) {
    if (check.dev) (void)hipStreamSynchronize(c->stream);
    return rc;
  }
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  if (check.dev && (rc = flag_end(c, check, "window", &tp_misfit, solve_flag_rule_text)) != AVM_OK) return rc;
  if (check.dev && flags) flags_seen = (unsigned)check.host[2];
  forms = choose_forms(batch->n_windows, c->n_slots, extended, marg, tp_misfit);

  // solve
  SolveArgs sa = solve_args(c, opt, d, d_sum);
  if ((rc = run_solve(c, sa, extended, forms)) != AVM_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));

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

int avm_imu_preintegrate_batch(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* batch, double* out_delta,
                               double* out_jacobian, double* out_covariance, double* out_sum_dt) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  int rc = check_window_batch(c, opt, batch, true);
  if (rc != AVM_OK) return rc;
  if (batch->n_windows == 0) return AVM_OK;
  if ((rc = validate_windows(c, mem, batch, CHK_IMU)) != AVM_OK) return rc;
  if ((rc = ensure_window_buffers(c, batch->n_windows, batch->max_samp)) != AVM_OK) return rc;
  avm_window_batch d;
  if ((rc = windows_on_device(c, mem, batch, &d)) != AVM_OK) return rc;
  if ((rc = run_preint(c, opt, &d)) != AVM_OK) return rc;
  const size_t iv = (size_t)batch->n_windows * 10;
  const hipMemcpyKind kind = mem == AVM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (out_delta) HIPCHK(c, hipMemcpyAsync(out_delta, c->pre_delta, sizeof(double) * iv * 10, kind, c->stream));
  if (out_jacobian) HIPCHK(c, hipMemcpyAsync(out_jacobian, c->pre_jac, sizeof(double) * iv * 225, kind, c->stream));
  if (out_covariance) HIPCHK(c, hipMemcpyAsync(out_covariance, c->pre_cov, sizeof(double) * iv * 225, kind, c->stream));
  if (out_sum_dt) HIPCHK(c, hipMemcpyAsync(out_sum_dt, c->pre_sum, sizeof(double) * iv, kind, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

// debug hook (not in avm.h): per-phase shader clocks of the last solve, summed over slots, [PROF_SLOTS = 64]
int avm_debug_copy_profile(avm_ctx* c, long long* host_out) {
  if (!c || !c->prof) return AVM_ERR_INVALID;
  std::vector<long long> h((size_t)PROF_SLOTS * 2 * c->n_slots);
  HIPCHK(c, hipMemcpy(h.data(), c->prof, sizeof(long long) * h.size(), hipMemcpyDeviceToHost));
  for (int k = 0; k < PROF_SLOTS; k++) host_out[k] = 0;
  for (int s = 0; s < 2 * c->n_slots; s++)
    for (int k = 0; k < PROF_SLOTS; k++) host_out[k] += h[(size_t)s * PROF_SLOTS + k];
  return AVM_OK;
}

// test / bench hook (not in avm.h): 1 when the last avm_window_solve_batch ran the throughput form of the solve kernel
int avm_debug_last_solve_form(const avm_ctx* c) { return c ? (c->last_solve_tp ? 1 : 0) : -1; }
// ... 1 when its marginalization ran the throughput form (marginalize_tp_kernel: two 256-thread workgroups per CU)
int avm_debug_last_marg_form(const avm_ctx* c) { return c ? (c->last_marg_tp ? 1 : 0) : -1; }
// ... and which form the last avm_fsel_select_batch STARTED in: 3 = one workgroup per frame with lazy evaluation (fsel_solo_kernel), 2 / 1 = the
// frame kernel's teams, 0 = one launch per greedy round
int avm_debug_last_fsel_form(const avm_ctx* c) { return c ? c->last_fsel_mode : -1; }

// test / bench hook (not in avm.h): out[0] = workgroups of the throughput kernel per CU (runtime's occupancy query), out[1] = its LDS bytes
int avm_debug_solve_tp_occupancy(int* out) {
  out[0] = window_solve_tp_occupancy(), out[1] = window_solve_tp_lds_bytes();
  return 2;
}

// test hook (not in avm.h): the compile-time tables of the throughput solve's sparse factorization (solve/chol_regs_tables.hpp; exported by solve/chol_regs.hpp); out: >= 512 ints
// which = 0: throughput build, 1: latency build, 2: extended build
int avm_debug_solve_pattern(int which, int* out) {
  return which == 0 ? window_solve_tp_pattern(out) : (which == 1 ? window_solve_pattern(out) : window_solve_x_pattern(out));
}
int avm_debug_solve_tp_pattern(int* out) { return avm_debug_solve_pattern(0, out); }

// test / bench hook (not in avm.h): out[0] = device / pinned (re)allocations of this ctx so far, out[1] = windows of the last
// marginalization whose square root the one-wavefront kernel (prior_chol_kernel) finished, out[2] = windows of that marginalization
// (out[2] - out[1] went through prior_eig_kernel's pivoted path), out[3] = 1 if the last solve took the throughput form
int avm_debug_counters(avm_ctx* c, int64_t* out) {
  if (!c || !out) return AVM_ERR_INVALID;
  out[0] = c->n_allocs, out[1] = 0, out[2] = c->last_marg_windows, out[3] = c->last_solve_tp ? 1 : 0;
  auto it = c->pool.find("pe_done");
  if (c->last_marg_windows > 0 && it != c->pool.end() && it->second.first) {
    std::vector<int> h((size_t)c->last_marg_windows);
    HIPCHK(c, hipMemcpy(h.data(), it->second.first, sizeof(int) * h.size(), hipMemcpyDeviceToHost));
    for (int v : h) out[1] += v != 0;
  }
  return AVM_OK;
}

// test / bench hook (not in avm.h): out[0] = intervals the last pre-integration examined, out[1] = intervals it integrated (all of them
// with AVM_PREINT_CACHE=0), out[2] = windows whose cached pre-integrations the last avm_slide_window* rolled (0: it left the cache alone)
int avm_debug_preint_cache(avm_ctx* c, int64_t* out) {
  if (!c || !out) return AVM_ERR_INVALID;
  out[0] = c->pk.examined, out[1] = c->pk.recomputed, out[2] = c->pk.rolled;
  if (c->pk.recomputed < 0 && c->pk.last_count) {
    int32_t n = 0;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(&n, c->pk.last_count, sizeof n, hipMemcpyDeviceToHost));
    out[1] = n;
  }
  return AVM_OK;
}

// bench hook (not in avm.h): candidate evaluations the last avm_fsel_select_batch executed on the device - counted by fsel_solo_kernel
// (the lazy form scores a fraction of the live candidates per round); -1 for the forms that score every live candidate every round
int avm_debug_fsel_evaluations(avm_ctx* c, int64_t* out) {
  if (!c || !out) return AVM_ERR_INVALID;
  *out = c->last_fsel_evals;
  return AVM_OK;
}

// test hook (not in avm.h): the table sizes of avm.h as this library was compiled with them, for the ctypes mirror check
int avm_debug_table_limits(int* out) {
  out[0] = AVM_MAX_FEAT, out[1] = AVM_MAX_OBS, out[2] = AVM_MAX_FEAT_WIDE, out[3] = AVM_MAX_OBS_WIDE;
  return 4;
}

// test hook (not in avm.h): sizeof of every ABI struct, for the ctypes mirror check
int avm_debug_struct_sizes(int* out) {
  out[0] = (int)sizeof(avm_options), out[1] = (int)sizeof(avm_window_batch), out[2] = (int)sizeof(avm_prior_out);
  out[3] = (int)sizeof(avm_solve_summary), out[4] = (int)sizeof(avm_fsel_batch), out[5] = (int)sizeof(avm_fsel_out);
  out[6] = (int)sizeof(avm_config);
  return 7;
}

// test hook (not in avm.h): sizeof and the member offsets of avm_image_batch, and AVM_MAX_IMAGE_PTS, for the ctypes mirror check; out: >= 8 ints
int avm_debug_track_struct_sizes(int* out) {
  int n = 0;
  out[n++] = (int)sizeof(avm_image_batch), out[n++] = AVM_MAX_IMAGE_PTS;
  for (size_t o : {offsetof(avm_image_batch, n_windows), offsetof(avm_image_batch, max_pts), offsetof(avm_image_batch, n_pts),
                   offsetof(avm_image_batch, feature_id), offsetof(avm_image_batch, xy), offsetof(avm_image_batch, vel_td)})
    out[n++] = (int)o;
  return n;
}

// test hook (not in avm.h): sizeof and the member offsets of avm_align_batch / avm_align_out, for the ctypes mirror check; out: >= 23 ints
int avm_debug_align_layout(int* out) {
  int n = 0;
  out[n++] = (int)sizeof(avm_align_batch), out[n++] = (int)sizeof(avm_align_out), out[n++] = AVM_MAX_ALIGN_FRAMES;
  for (size_t o : {offsetof(avm_align_batch, n_windows), offsetof(avm_align_batch, max_frames), offsetof(avm_align_batch, max_samp),
                   offsetof(avm_align_batch, n_frames), offsetof(avm_align_batch, frame_R), offsetof(avm_align_batch, frame_T),
                   offsetof(avm_align_batch, tic), offsetof(avm_align_batch, imu_n), offsetof(avm_align_batch, imu_dt),
                   offsetof(avm_align_batch, imu_acc), offsetof(avm_align_batch, imu_gyr), offsetof(avm_align_batch, imu_lin_ba),
                   offsetof(avm_align_batch, imu_lin_bg), offsetof(avm_align_batch, key_index), offsetof(avm_align_out, ok),
                   offsetof(avm_align_out, delta_bg), offsetof(avm_align_out, g_c0), offsetof(avm_align_out, x),
                   offsetof(avm_align_out, g_world), offsetof(avm_align_out, deltas)})
    out[n++] = (int)o;
  return n;
}

// test hook (not in avm.h): sqrt_info of the last pre-integration, [B][10][15][15]
int avm_debug_copy_sqrt_info(avm_ctx* c, int n_windows, double* host_out) {
  if (!c || !c->pre_sqrt) return AVM_ERR_INVALID;
  HIPCHK(c, hipMemcpy(host_out, c->pre_sqrt, sizeof(double) * (size_t)n_windows * 2250, hipMemcpyDeviceToHost));
  return AVM_OK;
}

int avm_triangulate_batch(avm_ctx* c, avm_mem mem, avm_window_batch* batch, double init_depth) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!batch || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  int rc = check_wide_strides(c, batch);  // (the API's table contract: the kernel runs one thread per feature, any count)
  if (rc != AVM_OK) return rc;
  if (batch->n_windows == 0) return AVM_OK;
  if ((rc = validate_windows(c, mem, batch, CHK_TRACKS)) != AVM_OK) return rc;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_TRI, batch, &d)) != AVM_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, launch_triangulate(d, init_depth, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  if ((rc = copy_back(c, mem, WINDOWS, U_TRI, batch, &d, batch)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[3], c->ev[4]) == hipSuccess) c->last_ms["triangulate"] = ms;
  return AVM_OK;
}

int avm_visual_initial_align_batch(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_align_batch* al, avm_window_batch* win,
                                   avm_align_out* out) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
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
      if (rule) return report_bad(c, b * 8 + rule, "window", align_rule_text);
    }
  } else {
    FlagCheck f;
    if ((rc = flag_begin(c, 1, [&](int* flag) { return launch_validate_align(*al, win != nullptr, flag, c->stream); }, &f)) != AVM_OK) return rc;
    if ((rc = flag_end(c, f, "window", nullptr, align_rule_text)) != AVM_OK) return rc;
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

  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  HIPCHK(c, launch_align_gyro_bias(aa, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, launch_align_solve(aa, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[2], c->stream));
  if (win) {
    HIPCHK(c, launch_align_prepare(aa, c->stream));
    HIPCHK(c, launch_triangulate(aa.w, 5.0 /* INIT_DEPTH, parameters.cpp:113 */, c->stream, 1, aa.out.ok));
    HIPCHK(c, launch_align_apply(aa, c->stream));
  }
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  if (win && (rc = copy_back(c, mem, WINDOWS, U_ALIGN, win, &aa.w, win)) != AVM_OK) return rc;
  if ((rc = copy_back(c, mem, ALIGN_OUT, U_WHOLE, &want, &aa.out, al)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->last_ms["align_gyro_bias"] = ms;
  if (hipEventElapsedTime(&ms, c->ev[1], c->ev[2]) == hipSuccess) c->last_ms["align_solve"] = ms;
  if (hipEventElapsedTime(&ms, c->ev[2], c->ev[3]) == hipSuccess) c->last_ms["align_apply"] = ms;
  return AVM_OK;
}

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
  int rc = validate_windows(c, mem, batch, CHK_TRACKS | CHK_IMU, nullptr, fr, roll_flag_rule_text);
  if (rc != AVM_OK) return rc;
  avm_window_batch d;
  const unsigned use = U_SLIDE | (feat_id ? U_SLIDE_TD : 0u);
  if ((rc = on_device(c, mem, WINDOWS, use, batch, &d)) != AVM_OK) return rc;
  const void* dfid = feat_id;
  const size_t fid_bytes = sizeof(int32_t) * (size_t)batch->n_windows * batch->max_feat;
  if (feat_id && mem == AVM_MEM_HOST && (rc = stage_array(c, "w_feat_id", feat_id, fid_bytes, &dfid)) != AVM_OK) return rc;
  const void* dflags = flags;
  if (flags && mem == AVM_MEM_HOST && (rc = stage_array(c, "w_roll_flags", flags, sizeof(int32_t) * batch->n_windows, &dflags)) != AVM_OK) return rc;
  int* derr = static_cast<int*>(pool_get(c, "slide_err", sizeof(int)));
  if (!derr) return fail(c, AVM_ERR_HIP, "hipMalloc failed (slide flag)");
  HIPCHK(c, hipMemsetAsync(derr, 0, sizeof(int), c->stream));
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, launch_slide_window(d, static_cast<const int32_t*>(dflags), flag, shift_depth, init_depth, remove_failures, derr, c->stream,
                                static_cast<int32_t*>(const_cast<void*>(dfid)), feat_id ? 1 : 0));
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  if ((rc = roll_preint_cache(c, d, static_cast<const int32_t*>(dflags), flag)) != AVM_OK) return rc;
  int herr = 0;
  HIPCHK(c, hipMemcpyAsync(&herr, derr, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if ((rc = copy_back(c, mem, WINDOWS, use, batch, &d, batch)) != AVM_OK) return rc;  // (everything the roll rewrites)
  if (feat_id && mem == AVM_MEM_HOST && dfid) HIPCHK(c, hipMemcpyAsync(feat_id, dfid, fid_bytes, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[3], c->ev[4]) == hipSuccess) c->last_ms["slide_window"] = ms;
  if (c->pk.rolled && hipEventElapsedTime(&ms, c->ev[5], c->ev[6]) == hipSuccess) c->last_ms["preint_roll"] = ms;
  if (herr) return fail(c, AVM_ERR_CAPACITY, "MARGIN_SECOND_NEW: interval 8 + interval 9 exceed max_samp samples");
  return AVM_OK;
}
}  // namespace

int avm_slide_window(avm_ctx* c, avm_mem mem, avm_window_batch* batch, int32_t flag, int32_t shift_depth, double init_depth) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!batch || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (flag != AVM_MARGIN_OLD && flag != AVM_MARGIN_SECOND_NEW) return fail(c, AVM_ERR_INVALID, "marginalization_flag must be MARGIN_OLD or MARGIN_SECOND_NEW");
  return slide_window(c, mem, batch, nullptr, flag, shift_depth, init_depth, 0);
}

int avm_slide_window_flags(avm_ctx* c, avm_mem mem, avm_window_batch* batch, const int32_t* flags, int32_t shift_depth, double init_depth,
                           int32_t remove_failures) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!batch || !flags || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  return slide_window(c, mem, batch, flags, AVM_MARGIN_OLD, shift_depth, init_depth, remove_failures);
}

int avm_slide_window_tracks(avm_ctx* c, avm_mem mem, avm_window_batch* batch, int32_t* feat_id, const int32_t* flags, int32_t shift_depth,
                            double init_depth, int32_t remove_failures) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!batch || !feat_id || !flags || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  return slide_window(c, mem, batch, flags, AVM_MARGIN_OLD, shift_depth, init_depth, remove_failures, feat_id);
}

}  // extern "C"

// ---- the feature manager on device-resident tables (tracks.hip) ----
namespace {
struct TrackRule {
  int status;
  const char* text;
};
const TrackRule ADD_IMAGE_RULES[8] = {
    {AVM_ERR_INVALID, "bad table"},
    {AVM_ERR_INVALID, "n_pts outside [0, max_pts]"},
    {AVM_ERR_INVALID, "the image's feature ids must be strictly ascending (std::map order)"},
    {AVM_ERR_INVALID, "a track already has an observation in frame 10 (feat_start + feat_nobs > 10)"},
    {AVM_ERR_INVALID, "an image id matches a track whose last observation is not in frame 9 (a lost id was issued again)"},
    {AVM_ERR_INVALID, "duplicate id in feat_id[0 .. n_feat)"},
    {AVM_ERR_CAPACITY, "n_feat + new tracks > max_feat"},
    {AVM_ERR_CAPACITY, "the observations do not fit max_obs"}};
const TrackRule IMU_PUSH_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                     {AVM_ERR_INVALID, "n outside [0, max_in]"},
                                     {AVM_ERR_CAPACITY, "interval 9 + the new samples exceed max_samp samples"}};
const TrackRule SOLVE_VIEW_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                       {AVM_ERR_CAPACITY, "more rows pass the solve's filter than view->max_feat"},
                                       {AVM_ERR_CAPACITY, "the observations of the rows that pass the solve's filter do not fit view->max_obs"}};
const TrackRule STORE_DEPTHS_RULES[8] = {{AVM_ERR_INVALID, "bad table"},
                                         {AVM_ERR_INVALID, "n_feat outside [0, max_feat] (full or view)"},
                                         {AVM_ERR_INVALID, "view_row must be strictly increasing inside [0, full n_feat)"}};

// A check kernel of tracks.hip, on its own: its verdict is on the host before the kernel that writes is launched, so a refused batch
// leaves every window as it was.  Device time between ev[0] and ev[1].
template <class Launch>
int track_check(avm_ctx* c, Launch launch, const TrackRule* rules) {
  FlagCheck f;
  HIPCHK(c, hipEventRecord(c->ev[0], c->stream));
  const int rc = flag_begin(c, 1, launch, &f);
  if (rc != AVM_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev[1], c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int v = f.host[0];
  if (v == 0x7f7f7f7f) return AVM_OK;
  const TrackRule& r = rules[v % 8];
  c->err = "window " + std::to_string(v / 8) + ": " + (r.text ? r.text : "bad table");
  return r.text ? r.status : AVM_ERR_INVALID;
}

// check (ev[0] .. ev[1]) + kernels (ev[3] .. ev[4]) of the call that just synchronized
void record_track_ms(avm_ctx* c, const char* key) {
  float a = 0, b = 0;
  if (hipEventElapsedTime(&a, c->ev[0], c->ev[1]) == hipSuccess && hipEventElapsedTime(&b, c->ev[3], c->ev[4]) == hipSuccess) c->last_ms[key] = a + b;
}

// an array beside the structs, in `mem` space: the caller's pointer, or (AVM_MEM_HOST) a staged copy / a device buffer to copy back from
template <class T>
int array_in(avm_ctx* c, avm_mem mem, const char* pool, const T* p, size_t n, const T** d) {
  *d = p;
  if (mem != AVM_MEM_HOST) return AVM_OK;
  const void* dev = nullptr;
  const int rc = stage_array(c, pool, p, sizeof(T) * n, &dev);
  *d = static_cast<const T*>(dev);
  return rc;
}
template <class T>
int array_out(avm_ctx* c, avm_mem mem, const char* pool, T* p, size_t n, T** d) {
  *d = p;
  if (mem != AVM_MEM_HOST || !p) return AVM_OK;
  *d = static_cast<T*>(pool_get(c, pool, sizeof(T) * n));
  return *d ? AVM_OK : fail(c, AVM_ERR_HIP, "hipMalloc failed (output array)");
}
template <class T>
int array_back(avm_ctx* c, avm_mem mem, T* p, const T* d, size_t n) {
  if (mem == AVM_MEM_HOST && p && d && n) HIPCHK(c, hipMemcpyAsync(p, d, sizeof(T) * n, hipMemcpyDeviceToHost, c->stream));
  return AVM_OK;
}
}  // namespace

extern "C" {

int avm_add_image_batch(avm_ctx* c, avm_mem mem, avm_window_batch* win, int32_t* feat_id, const avm_image_batch* img, double min_parallax,
                        int32_t* flags_out, int32_t* last_track_num, double* parallax) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
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
  const size_t B = win->n_windows, P = (size_t)img->max_pts;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_TRK, win, &d)) != AVM_OK) return rc;
  avm_image_batch di = *img;
  const int32_t* dfid_in;
  if ((rc = array_in(c, mem, "ai_n_pts", img->n_pts, B, &di.n_pts)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "ai_ids", img->feature_id, B * P, &di.feature_id)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "ai_xy", img->xy, B * P * 2, &di.xy)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "ai_vel_td", img->vel_td, B * P * 4, &di.vel_td)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "w_feat_id", static_cast<const int32_t*>(feat_id), B * win->max_feat, &dfid_in)) != AVM_OK) return rc;
  int32_t* dfid = const_cast<int32_t*>(dfid_in);
  int32_t *dflags, *dltn;
  double* dpar;
  if ((rc = array_out(c, mem, "k_flags", flags_out, B, &dflags)) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "k_ltn", last_track_num, B, &dltn)) != AVM_OK) return rc;
  if ((rc = array_out(c, mem, "k_par", parallax, B * 2, &dpar)) != AVM_OK) return rc;
  if ((rc = track_check(c, [&](int* flag) { return launch_add_image_check(d, dfid, di, flag, c->stream); }, ADD_IMAGE_RULES)) != AVM_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, launch_add_image(d, dfid, di, c->stream));
  HIPCHK(c, launch_keyframe_decision(d, min_parallax, dflags, dltn, dpar, c->stream));  // (the decision of avm_keyframe_decision_batch, on the result)
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
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
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
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
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, launch_imu_push(d, dn, max_in, ddt, dacc, dgyr, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  if ((rc = copy_back(c, mem, WINDOWS, U_PUSH, win, &d, win)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "imu_push");
  return AVM_OK;
}

int avm_solve_view_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* full, avm_window_batch* view, int32_t* view_row) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
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
  if ((rc = on_device(c, mem, WINDOWS, U_TRK, static_cast<const avm_window_batch*>(view), &dv, nullptr, nullptr, "v_")) != AVM_OK) return rc;
  int32_t* drow;
  if ((rc = array_out(c, mem, "v_row", view_row, B * view->max_feat, &drow)) != AVM_OK) return rc;
  if (mem == AVM_MEM_HOST && view->max_feat > 0)
    HIPCHK(c, hipMemcpyAsync(drow, view_row, sizeof(int32_t) * B * view->max_feat, hipMemcpyHostToDevice, c->stream));
  if ((rc = track_check(c, [&](int* flag) { return launch_solve_view_check(df, dv, flag, c->stream); }, SOLVE_VIEW_RULES)) != AVM_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, launch_solve_view(df, dv, drow, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  if ((rc = copy_back(c, mem, WINDOWS, U_TRK, view, &dv, view)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, view_row, drow, B * view->max_feat)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "solve_view");
  return AVM_OK;
}

int avm_solve_view_store_depths(avm_ctx* c, avm_mem mem, avm_window_batch* full, const avm_window_batch* view, const int32_t* view_row) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!full || !view || !view_row || full->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (view->n_windows != full->n_windows) return fail(c, AVM_ERR_INVALID, "view->n_windows differs from full->n_windows");
  if (view->max_feat < 0 || full->max_feat < 0) return fail(c, AVM_ERR_INVALID, "negative stride");
  if (!full->n_feat || !full->inv_depth || !view->n_feat || !view->inv_depth) return fail(c, AVM_ERR_INVALID, "null n_feat / inv_depth");
  if (full->n_windows == 0) return AVM_OK;
  int rc;
  const size_t B = full->n_windows;
  avm_window_batch df, dv;
  if ((rc = on_device(c, mem, WINDOWS, U_DEPTH, static_cast<const avm_window_batch*>(full), &df)) != AVM_OK) return rc;
  if ((rc = on_device(c, mem, WINDOWS, U_DEPTH, view, &dv, nullptr, nullptr, "v_")) != AVM_OK) return rc;
  const int32_t* drow;
  if ((rc = array_in(c, mem, "v_row", view_row, B * view->max_feat, &drow)) != AVM_OK) return rc;
  if ((rc = track_check(c, [&](int* flag) { return launch_store_depths_check(df, dv, drow, flag, c->stream); }, STORE_DEPTHS_RULES)) != AVM_OK)
    return rc;
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, launch_store_depths(df, dv, drow, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  if ((rc = copy_back(c, mem, WINDOWS, U_DEPTH, full, &df, full)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  record_track_ms(c, "store_depths");
  return AVM_OK;
}

int avm_keyframe_decision_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* batch, double min_parallax, int32_t* flags, int32_t* last_track_num,
                                double* parallax) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!batch || !flags || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (!batch->obs_xy) return fail(c, AVM_ERR_INVALID, "null obs_xy");
  int rc = check_wide_strides(c, batch);  // (the API's table contract: the kernel walks the list in chunks, any count)
  if (rc != AVM_OK) return rc;
  if (batch->n_windows == 0) return AVM_OK;
  if ((rc = validate_windows(c, mem, batch, CHK_TRACKS)) != AVM_OK) return rc;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_KEYF, batch, &d)) != AVM_OK) return rc;
  const size_t B = batch->n_windows;
  int32_t *dflags = flags, *dltn = last_track_num;
  double* dpar = parallax;
  if (mem == AVM_MEM_HOST) {
    dflags = static_cast<int32_t*>(pool_get(c, "k_flags", sizeof(int32_t) * B));
    dltn = last_track_num ? static_cast<int32_t*>(pool_get(c, "k_ltn", sizeof(int32_t) * B)) : nullptr;
    dpar = parallax ? static_cast<double*>(pool_get(c, "k_par", sizeof(double) * B * 2)) : nullptr;
    if (!dflags || (last_track_num && !dltn) || (parallax && !dpar)) return fail(c, AVM_ERR_HIP, "hipMalloc failed (keyframe decision out)");
  }
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, launch_keyframe_decision(d, min_parallax, dflags, dltn, dpar, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  if (mem == AVM_MEM_HOST) {
    HIPCHK(c, hipMemcpyAsync(flags, dflags, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
    if (last_track_num) HIPCHK(c, hipMemcpyAsync(last_track_num, dltn, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
    if (parallax) HIPCHK(c, hipMemcpyAsync(parallax, dpar, sizeof(double) * B * 2, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[3], c->ev[4]) == hipSuccess) c->last_ms["keyframe_decision"] = ms;
  return AVM_OK;
}

int avm_failure_detection_batch(avm_ctx* c, avm_mem mem, const avm_window_batch* batch, const double* last_P, int32_t* failed) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!batch || !last_P || !failed || batch->n_windows < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (!batch->pose || !batch->speedbias) return fail(c, AVM_ERR_INVALID, "null pose / speedbias");
  if (batch->n_windows == 0) return AVM_OK;
  int rc;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_FAIL, batch, &d)) != AVM_OK) return rc;
  const size_t B = batch->n_windows;
  const void* dlp = last_P;
  int32_t* dfailed = failed;
  if (mem == AVM_MEM_HOST) {
    if ((rc = stage_array(c, "fd_last_P", last_P, sizeof(double) * B * 3, &dlp)) != AVM_OK) return rc;
    dfailed = static_cast<int32_t*>(pool_get(c, "fd_failed", sizeof(int32_t) * B));
    if (!dfailed) return fail(c, AVM_ERR_HIP, "hipMalloc failed (failure detection out)");
  }
  HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
  HIPCHK(c, launch_failure_detection(d, static_cast<const double*>(dlp), dfailed, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
  if (mem == AVM_MEM_HOST) HIPCHK(c, hipMemcpyAsync(failed, dfailed, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[3], c->ev[4]) == hipSuccess) c->last_ms["failure_detection"] = ms;
  return AVM_OK;
}

int avm_imu_propagate_batch(avm_ctx* c, avm_mem mem, avm_window_batch* batch, const double g[3]) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
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

int avm_projection_td_eval(avm_ctx* c, avm_mem mem, const avm_td_factor_batch* f, double* residual, double* jac) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!f || !residual || f->n < 0) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (f->n == 0) return AVM_OK;
  const size_t n = f->n;
  avm_td_factor_batch d;
  const int rc = on_device(c, mem, TD_FACTORS, U_WHOLE, f, &d);
  if (rc != AVM_OK) return rc;
  double *dr = residual, *dj = jac;
  if (mem == AVM_MEM_HOST) {
    dr = static_cast<double*>(pool_get(c, "td_res", sizeof(double) * n * 2));
    dj = jac ? static_cast<double*>(pool_get(c, "td_jac", sizeof(double) * n * 40)) : nullptr;
    if (!dr || (jac && !dj)) return fail(c, AVM_ERR_HIP, "hipMalloc failed (td factor out)");
  }
  HIPCHK(c, launch_projection_td_eval(d, dr, dj, c->stream));
  if (mem == AVM_MEM_HOST) {
    HIPCHK(c, hipMemcpyAsync(residual, dr, sizeof(double) * n * 2, hipMemcpyDeviceToHost, c->stream));
    if (jac) HIPCHK(c, hipMemcpyAsync(jac, dj, sizeof(double) * n * 40, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

int avm_window_eval_factors(avm_ctx* c, const avm_options* opt, avm_mem mem, const avm_window_batch* batch, int apply_loss,
                            double* proj_r, double* proj_J, double* imu_r, double* imu_J, double* prior_res, double* cost) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
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
    *o.dst = o.host;
    if (mem == AVM_MEM_HOST && o.host) {
      *o.dst = static_cast<double*>(pool_get(c, o.name, o.n * sizeof(double)));
      if (!*o.dst) return fail(c, AVM_ERR_HIP, "hipMalloc failed (eval out)");
      HIPCHK(c, hipMemsetAsync(*o.dst, 0, o.n * sizeof(double), c->stream));
    }
  }
  if ((rc = run_preint(c, opt, &d)) != AVM_OK) return rc;
  ea.b = d, ea.opt = *opt, ea.apply_loss = apply_loss;
  ea.pre_delta = c->pre_delta, ea.pre_jac = c->pre_jac, ea.pre_sqrt = c->pre_sqrt, ea.pre_sum_dt = c->pre_sum;
  HIPCHK(c, launch_eval_factors(ea, c->stream));
  if (mem == AVM_MEM_HOST)
    for (auto& o : outs)
      if (o.host) HIPCHK(c, hipMemcpyAsync(o.host, *o.dst, o.n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

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
    HIPCHK(c, hipEventRecord(c->ev[3], c->stream));
    HIPCHK(c, launch_fsel(d, w, dout, nullptr, true, mode, vflag, c->stream));
    HIPCHK(c, hipEventRecord(c->ev[4], c->stream));
    if (mode) HIPCHK(c, hipMemcpyAsync(hsync, w.sync, sizeof(int32_t) * 64, hipMemcpyDeviceToHost, c->stream));
    if ((rc = copy_back(c, mem, FSEL_OUT, U_WHOLE, out, &dout, batch)) != AVM_OK) return rc;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // (the one synchronization of the call)
    if (vflag && (rc = flag_end(c, check, "frame")) != AVM_OK) return rc;  // (no kernel of the select has touched a table)
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
  float ms = 0;
  if (hipEventElapsedTime(&ms, c->ev[3], c->ev[4]) == hipSuccess) c->last_ms["fsel_select"] = ms;
  return AVM_OK;
}

const TrackRule SELECT_IMAGE_RULES[8] = {
    {AVM_ERR_INVALID, "bad table"},
    {AVM_ERR_INVALID, "n_pts outside [0, max_pts]"},
    {AVM_ERR_INVALID, "the image's feature ids must be strictly ascending (std::map order)"},
    {AVM_ERR_INVALID, "n_tracked outside [0, max_tracked]"},
    {AVM_ERR_CAPACITY, "more new points than problem->max_cand"},
    {AVM_ERR_CAPACITY, "more tracked points in the image than problem->max_used"},
    {AVM_ERR_CAPACITY, "the subset and the points the selection can add do not fit image_out->max_pts"},
    {AVM_ERR_CAPACITY, "the tracked ids kept and the ids the call can append do not fit state->max_tracked"}};

}  // namespace

int avm_fsel_select_batch(avm_ctx* c, avm_mem mem, const avm_fsel_batch* batch, avm_fsel_out* out) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
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
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
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
  const size_t B = img->n_windows, P = (size_t)img->max_pts, PO = (size_t)img_out->max_pts, T = (size_t)st->max_tracked;
  SelectImageArgs a;
  a.image = *img, a.init_thresh = init_thresh, a.prune_lost = prune_lost, a.state = *st, a.image_out = *img_out;
  if ((rc = array_in(c, mem, "si_n_pts", img->n_pts, B, &a.image.n_pts)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "si_ids", img->feature_id, B * P, &a.image.feature_id)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "si_xy", img->xy, B * P * 2, &a.image.xy)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "si_vel_td", img->vel_td, B * P * 4, &a.image.vel_td)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "si_prob", prob, B * P, &a.prob)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "si_init", initialized, B, &a.initialized)) != AVM_OK) return rc;
  // (what the call writes travels in as well: the slots it does not write keep what they held)
  const int32_t *s_last, *s_nt, *s_ids, *s_first, *o_n, *o_ids;
  const double *o_xy, *o_td;
  if ((rc = array_in(c, mem, "ss_last", static_cast<const int32_t*>(st->last_feature_id), B, &s_last)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "ss_n", static_cast<const int32_t*>(st->n_tracked), B, &s_nt)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "ss_ids", static_cast<const int32_t*>(st->tracked_id), B * T, &s_ids)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "ss_first", static_cast<const int32_t*>(st->first_image), B, &s_first)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "so_n_pts", img_out->n_pts, B, &o_n)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "so_ids", img_out->feature_id, B * PO, &o_ids)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "so_xy", img_out->xy, B * PO * 2, &o_xy)) != AVM_OK) return rc;
  if ((rc = array_in(c, mem, "so_vel_td", img_out->vel_td, B * PO * 4, &o_td)) != AVM_OK) return rc;
  a.state.last_feature_id = const_cast<int32_t*>(s_last), a.state.n_tracked = const_cast<int32_t*>(s_nt);
  a.state.tracked_id = const_cast<int32_t*>(s_ids), a.state.first_image = const_cast<int32_t*>(s_first);
  a.image_out.n_pts = o_n, a.image_out.feature_id = o_ids, a.image_out.xy = o_xy, a.image_out.vel_td = o_td;
  if ((rc = on_device(c, mem, FSEL, U_WHOLE, static_cast<const avm_fsel_batch*>(problem), &a.problem)) != AVM_OK) return rc;
  a.out = *out;
  if (mem == AVM_MEM_HOST && alloc_out(c, FSEL_OUT, out, &a.out, problem) != AVM_OK) return fail(c, AVM_ERR_HIP, "hipMalloc failed (selector out)");
  // the check on its own, its verdict on the host before the first kernel that writes; then the split, which writes `problem` only
  if ((rc = track_check(c, [&](int* flag) { return launch_select_image_check(a, flag, c->stream); }, SELECT_IMAGE_RULES)) != AVM_OK) return rc;
  HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
  HIPCHK(c, launch_select_split(a, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
  // the caller's tables of the problem (n_cloud, nr_imu) with the counts the split wrote: the selection's own check, ahead of it on the stream
  FlagCheck check;
  if ((rc = validate_fsel_begin(c, &a.problem, &check)) != AVM_OK) return rc;
  if ((rc = run_fsel_select(c, mem, problem, a.problem, out, a.out, check)) != AVM_OK) return rc;
  float t_check = 0, t_split = 0, t_merge = 0;
  if (hipEventElapsedTime(&t_check, c->ev[0], c->ev[1]) == hipSuccess && hipEventElapsedTime(&t_split, c->ev[5], c->ev[6]) == hipSuccess)
    c->last_ms["select_split"] = t_check + t_split;
  // the selection has finished, its re-runs included: image_out and the state
  HIPCHK(c, hipEventRecord(c->ev[5], c->stream));
  HIPCHK(c, launch_select_merge(a, c->stream));
  HIPCHK(c, hipEventRecord(c->ev[6], c->stream));
  const avm_fsel_batch& dp = a.problem;
  const size_t mc = (size_t)problem->max_cand, mu = (size_t)problem->max_used;
  if ((rc = array_back(c, mem, const_cast<int32_t*>(problem->n_cand), dp.n_cand, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<int32_t*>(problem->cand_id), dp.cand_id, B * mc)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<double*>(problem->cand_xy), dp.cand_xy, B * mc * 2)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<double*>(problem->cand_prob), dp.cand_prob, B * mc)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<int32_t*>(problem->n_used), dp.n_used, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<int32_t*>(problem->used_id), dp.used_id, B * mu)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<double*>(problem->used_xy), dp.used_xy, B * mu * 2)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, st->last_feature_id, s_last, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, st->n_tracked, s_nt, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, st->tracked_id, s_ids, B * T)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, st->first_image, s_first, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<int32_t*>(img_out->n_pts), o_n, B)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<int32_t*>(img_out->feature_id), o_ids, B * PO)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<double*>(img_out->xy), o_xy, B * PO * 2)) != AVM_OK) return rc;
  if ((rc = array_back(c, mem, const_cast<double*>(img_out->vel_td), o_td, B * PO * 4)) != AVM_OK) return rc;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  if (hipEventElapsedTime(&t_merge, c->ev[5], c->ev[6]) == hipSuccess) c->last_ms["select_merge"] = t_merge;
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
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!in || !hor_pos || !hor_quat || in->n_problems < 0 || in->horizon < 1) return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (in->n_problems == 0) return AVM_OK;
  const size_t P = in->n_problems, H1 = (size_t)in->horizon + 1;
  avm_fsel_horizon_in d;
  const int rc = on_device(c, mem, HORIZON_IN, U_WHOLE, in, &d);
  if (rc != AVM_OK) return rc;
  double *dp = hor_pos, *dq = hor_quat;
  if (mem == AVM_MEM_HOST) {
    dp = static_cast<double*>(pool_get(c, "h_pos", sizeof(double) * P * H1 * 3));
    dq = static_cast<double*>(pool_get(c, "h_quat", sizeof(double) * P * H1 * 4));
    if (!dp || !dq) return fail(c, AVM_ERR_HIP, "hipMalloc failed (horizon out)");
  }
  HIPCHK(c, launch_fsel_horizon_imu(d, dp, dq, c->stream));
  if (mem == AVM_MEM_HOST) {
    HIPCHK(c, hipMemcpyAsync(hor_pos, dp, sizeof(double) * P * H1 * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(hor_quat, dq, sizeof(double) * P * H1 * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

int avm_fsel_build_cloud(avm_ctx* c, avm_mem mem, const avm_window_batch* windows, const double* k1_pos, const double* k1_quat, int32_t max_cloud,
                         int32_t* n_cloud, double* cloud_xy, double* cloud_depth) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  if (!windows || !k1_pos || !k1_quat || !n_cloud || !cloud_xy || !cloud_depth || windows->n_windows < 0 || max_cloud < 1)
    return fail(c, AVM_ERR_INVALID, "null/negative argument");
  if (windows->n_windows == 0) return AVM_OK;
  int rc = validate_windows(c, mem, windows, CHK_TRACKS);
  if (rc != AVM_OK) return rc;
  const size_t B = windows->n_windows;
  avm_window_batch d;
  if ((rc = on_device(c, mem, WINDOWS, U_CLOUD, windows, &d)) != AVM_OK) return rc;
  const void *dp = k1_pos, *dq = k1_quat;
  int32_t* dn = n_cloud;
  double *dxy = cloud_xy, *ddep = cloud_depth;
  if (mem == AVM_MEM_HOST) {
    if ((rc = stage_array(c, "c_k1p", k1_pos, sizeof(double) * B * 3, &dp)) != AVM_OK) return rc;
    if ((rc = stage_array(c, "c_k1q", k1_quat, sizeof(double) * B * 4, &dq)) != AVM_OK) return rc;
    dn = static_cast<int32_t*>(pool_get(c, "c_n", sizeof(int32_t) * B));
    dxy = static_cast<double*>(pool_get(c, "c_xy", sizeof(double) * B * max_cloud * 2));
    ddep = static_cast<double*>(pool_get(c, "c_dep", sizeof(double) * B * max_cloud));
    if (!dn || !dxy || !ddep) return fail(c, AVM_ERR_HIP, "hipMalloc failed (cloud out)");
    HIPCHK(c, hipMemsetAsync(dxy, 0, sizeof(double) * B * max_cloud * 2, c->stream));
    HIPCHK(c, hipMemsetAsync(ddep, 0, sizeof(double) * B * max_cloud, c->stream));
  }
  HIPCHK(c, launch_fsel_build_cloud(d, static_cast<const double*>(dp), static_cast<const double*>(dq), max_cloud, dn, dxy, ddep, c->stream));
  if (mem == AVM_MEM_HOST) {
    HIPCHK(c, hipMemcpyAsync(n_cloud, dn, sizeof(int32_t) * B, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cloud_xy, dxy, sizeof(double) * B * max_cloud * 2, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(cloud_depth, ddep, sizeof(double) * B * max_cloud, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

int avm_fsel_nn_depth(avm_ctx* c, avm_mem mem, const avm_fsel_batch* batch, double* depth) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  int rc = check_fsel(c, batch);
  if (rc != AVM_OK) return rc;
  if (!depth) return fail(c, AVM_ERR_INVALID, "null depth");
  if (batch->n_problems == 0) return AVM_OK;
  if ((rc = validate_fsel(c, mem, batch)) != AVM_OK) return rc;
  avm_fsel_batch d;
  if ((rc = on_device(c, mem, FSEL, U_WHOLE, batch, &d, "f_pack")) != AVM_OK) return rc;
  const size_t n = (size_t)batch->n_problems * batch->max_cand;
  double* dd = mem == AVM_MEM_HOST ? static_cast<double*>(pool_get(c, "fi_nn", sizeof(double) * n)) : depth;
  if (!dd) return fail(c, AVM_ERR_HIP, "hipMalloc failed (nn depth)");
  HIPCHK(c, hipMemsetAsync(dd, 0, sizeof(double) * n, c->stream));
  double* kd = static_cast<double*>(pool_get(c, "fw_kd", sizeof(double) * fsel_kd_doubles(d)));
  if (!kd) return fail(c, AVM_ERR_HIP, "hipMalloc failed (kd-tree)");
  HIPCHK(c, launch_fsel_nn_depth(d, kd, dd, c->stream));
  if (mem == AVM_MEM_HOST) HIPCHK(c, hipMemcpyAsync(depth, dd, sizeof(double) * n, hipMemcpyDeviceToHost, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

int avm_fsel_information(avm_ctx* c, avm_mem mem, const avm_fsel_batch* batch, double* omega, double* delta_cand, int32_t* cand_valid) {
  if (!c) return AVM_ERR_INVALID;
  (void)hipSetDevice(c->device);
  int rc = check_fsel(c, batch);
  if (rc != AVM_OK) return rc;
  if (batch->n_problems == 0) return AVM_OK;
  if ((rc = validate_fsel(c, mem, batch)) != AVM_OK) return rc;
  avm_fsel_batch d;
  if ((rc = on_device(c, mem, FSEL, U_WHOLE, batch, &d, "f_pack")) != AVM_OK) return rc;
  FselBuffers w;
  if ((rc = fsel_buffers(c, &d, &w, false)) != AVM_OK) return rc;
  const size_t P = batch->n_problems, N = 9 * ((size_t)batch->horizon + 1), T = 3 * (size_t)batch->horizon, mc = batch->max_cand;
  double* d_om = nullptr;
  if (omega) {
    d_om = mem == AVM_MEM_HOST ? static_cast<double*>(pool_get(c, "fi_om", sizeof(double) * P * N * N)) : omega;
    if (!d_om) return fail(c, AVM_ERR_HIP, "hipMalloc failed (omega)");
  }
  avm_fsel_out none{nullptr, nullptr, nullptr, nullptr};
  HIPCHK(c, launch_fsel(d, w, none, d_om, false, 0, nullptr, c->stream));
  const hipMemcpyKind kind = mem == AVM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
  if (omega && mem == AVM_MEM_HOST) HIPCHK(c, hipMemcpyAsync(omega, d_om, sizeof(double) * P * N * N, kind, c->stream));
  if (delta_cand) HIPCHK(c, hipMemcpyAsync(delta_cand, w.delta, sizeof(double) * P * mc * T * T, kind, c->stream));
  if (cand_valid) HIPCHK(c, hipMemcpyAsync(cand_valid, w.valid, sizeof(int32_t) * P * mc, kind, c->stream));
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return AVM_OK;
}

}  // extern "C"
