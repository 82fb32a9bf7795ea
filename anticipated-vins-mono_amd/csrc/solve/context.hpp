// solve/context.hpp - global pointers typed by address space, WinCtx and the options in LDS, build_frames, ric_of, td_shift
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// Global-memory pointers carried into the outlined phases are typed with their address space: behind a struct
// reference the compiler cannot prove it and would fall back to flat_load/flat_store, which count against the LDS
// counter too (every LDS wait then also waits for HBM).
typedef double dv2 __attribute__((ext_vector_type(2)));
#if defined(__HIP_DEVICE_COMPILE__)
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) const double gcdouble;
typedef __attribute__((address_space(1))) int32_t gint;
typedef __attribute__((address_space(1))) long long glong;
typedef __attribute__((address_space(1))) const dv2 gcdv2;
template <class T> AVM_DEV __attribute__((address_space(1))) T* as_global(T* p) { return (__attribute__((address_space(1))) T*)p; }
#else  // host pass of the same translation unit: plain pointers
typedef double gdouble;
typedef const double gcdouble;
typedef int32_t gint;
typedef long long glong;
typedef const dv2 gcdv2;
template <class T> AVM_DEV T* as_global(T* p) { return p; }
#endif

struct WinCtx {
  glong* prof;
  gdouble* sc;   // global scratch slot
  gint* osf;     // observation slot -> feature
  gint* cov;     // [11][150] features observed in frame b, in feature order
  int w, nf, nobs_tot, pn, pnblk;
  gcdouble* obs;   // [max_obs][2]
  gcdouble *pdelta, *pjac, *psqrt, *psum;  // this window's 10 intervals
  gcdouble *lba, *lbg;
  gcdouble *pJ, *pr, *px0;  // prior
  int ldp;
  // optional members of the problem (the solve reads them in the AVM_X build only, the marginalization in both)
  gcdouble* aux;      // [max_obs][4] velocity.x, velocity.y, cur_td, uv.y per observation slot (null unless estimate_td)
  gcdouble* relo_xy;  // [relo_n][2] match points
  int relo_n;         // > 0: the relocalization frame takes part (frame 11)
  int has_relo;       // relocalization_info: relo_Pose is frame 11 of the state and goes through the gauge fix, even with no match (relo_n == 0)
  int est_ex, est_td;
};

static_assert(sizeof(WinCtx) <= 32 * 8, "WinCtx outgrew its LDS slot");
// The per-window context and the options live in LDS: handed to the outlined phases by reference they would sit in
// the caller's private (scratch) memory and every field access would be a flat load from it.
AVM_DEV const WinCtx& lds_ctx() { return *reinterpret_cast<const WinCtx*>(LDS() + L_CTX); }
AVM_DEV const avm_options& lds_opt() { return *reinterpret_cast<const avm_options*>(LDS() + L_OPT); }
AVM_DEV void lds_store_ctx(const WinCtx& cl, const avm_options& ol) {  // call by all threads, then barrier
  if (threadIdx.x == 0) *reinterpret_cast<WinCtx*>(LDS() + L_CTX) = cl;
  const int nw = (int)(sizeof(avm_options) / 4);
  const int* src = reinterpret_cast<const int*>(&ol);
  int* dst = reinterpret_cast<int*>(LDS() + L_OPT);
  for (int i = threadIdx.x; i < nw; i += NT) dst[i] = src[i];
}

// frames: R_f and A_f = ric^T R_f^T for state vector xs into frame slot `which`
AVM_DEV void build_frames(int xs_off, int which) {
  double* lds = LDS();
  const double* xs = lds + xs_off;
  const int t = threadIdx.x;
  double* R = lds + L_FR + which * FRS;
  double* A = R + 9 * NFRP;
#ifdef AVM_X
  // ex_pose is part of the state here: every thread that needs ric recomputes it (thread NFRP publishes it for the factors)
  double ricv[9];
  q2R(quat{xs[XEX + 6], xs[XEX + 3], xs[XEX + 4], xs[XEX + 5]}, ricv);
  const double* ric = ricv;
  if (t == NFRP) {
    double* dst = lds + L_RIC + which * 12;
    for (int k = 0; k < 9; k++) dst[k] = ricv[k];
    for (int k = 0; k < 3; k++) dst[9 + k] = xs[XEX + k];
  }
#else
  const double* ric = lds + L_RIC;
#endif
  if (t < NFRP) {
    quat q{xs[t * 7 + 6], xs[t * 7 + 3], xs[t * 7 + 4], xs[t * 7 + 5]};
    double Rm[9];
    q2R(q, Rm);
    for (int k = 0; k < 9; k++) R[t * 9 + k] = Rm[k];
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) A[t * 9 + a * 3 + b] = ric[0 * 3 + a] * Rm[b * 3 + 0] + ric[1 * 3 + a] * Rm[b * 3 + 1] + ric[2 * 3 + a] * Rm[b * 3 + 2];
  }
}

// ric / tic the factors of frames slot `which` are evaluated with
AVM_DEV const double* ric_of(int which) {
#ifdef AVM_X
  return LDS() + L_RIC + which * 12;
#else
  (void)which;
  return LDS() + L_RIC;
#endif
}

// the td-shifted pair of observations of one ProjectionTdFactor (projection_td_factor.cpp:50-52) and the two velocities:
// ob = {pts_i.x, pts_i.y, pts_j.x, pts_j.y}, ai / aj = {velocity.x, velocity.y, cur_td, uv.y} of the two observations
AVM_DEV void td_shift(double* ob, const double* ai, const double* aj, double td, double tr, double row) {
  const double si = td - ai[2] + tr / row * (ai[3] - row / 2), sj = td - aj[2] + tr / row * (aj[3] - row / 2);
  ob[0] -= si * ai[0], ob[1] -= si * ai[1], ob[2] -= sj * aj[0], ob[3] -= sj * aj[1];
}
