// solve/pinv16.hpp - the 16 x 16 pseudo-inverse's Cholesky fast path (pinv16_cholesky)
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// Fast path of the 16 x 16 pseudo-inverse of the marginalization (Amm^+ = V diag(lambda > eps ? 1 / lambda : 0) V^T,
// marginalization_factor.cpp:283-286) for the usual case that NO eigenvalue is clamped: then Amm^+ is the plain inverse,
// which one wavefront gets from the same register-resident square-root-free Cholesky as the solve's diagonal blocks
// (lanes 0..15 = rows, lanes 16..31 = rows of the identity -> L^-T), ~3K cycles instead of ~135K for the Jacobi sweeps.
// The condition is checked rigorously: lambda_min >= 1 / trace(Amm^-1), so "trace(Amm^-1) < 1 / eps" (and positive
// pivots) proves that every eigenvalue is above eps; otherwise the caller falls back to the eigen-decomposition.
// On success the result is handed over in the eigen-solver's output format: EV[i][c] = (L D^1/2)^-T rows, diag(EA) = the
// pivots d_c, so that EV diag(1 / d) EV^T = Amm^-1.  EA is left untouched on failure.  Call with one full wavefront.
AVM_NOINL bool pinv16_cholesky(double* EA, double* EV, int m, double eps) {  // (outlined: its sixteen-register row was spilled inside the kernel body)
  constexpr int NB = 16;
  const int r = threadIdx.x & 63;
  const bool idl = (r & 48) == 16;
  double a[NB];
  {
    const int rc = r & 15;
#pragma unroll
    for (int k = 0; k < NB; k++) a[k] = idl ? (rc == k ? 1.0 : 0.0) : EA[rc * NB + min(k, rc)];
  }
  double uprev = 0.0, dvec = 1.0;
#pragma unroll
  for (int j = 0; j < NB; j++) {
    if (j > 0) a[j] = fma(-uprev, readlane_d(a[j - 1], j), a[j]);
    const double djj = readlane_d(a[j], j);
    dvec = (r & 15) == j ? djj : dvec;
    double y = __builtin_amdgcn_rcp(djj), e = 0;
    AVM_PIVOT_TAIL(0, false)
    e = fma(-djj, y, 1.0);
    AVM_PIVOT_TAIL(1, false)
    y = fma(y, e, y);
    AVM_PIVOT_TAIL(2, false)
    e = fma(-djj, y, 1.0);
    AVM_PIVOT_TAIL(3, false)
    y = fma(y, e, y);
    AVM_PIVOT_TAIL(4, false)
    uprev = a[j] * y;
  }
  // trace(Amm^-1) = sum_i sum_c x_i[c]^2 / d_c over the real indices; pivots must be positive
  double tr = 0.0;
  bool bad = false;
#pragma unroll
  for (int c = 0; c < NB; c++) {
    const double dc = readlane_d(dvec, c);
    if (c < m) {
      bad |= !(dc > 0.0);
      tr = fma(a[c] * a[c], 1.0 / dc, tr);
    }
  }
  tr = (idl && (r & 15) < m) ? tr : 0.0;
  tr = wave_sum(tr);
  const bool fast = !bad && tr * eps < 1.0;  // (NaN compares false)
  if (fast) {
    if (idl) {
#pragma unroll
      for (int c = 0; c < NB; c++) EV[(r & 15) * NB + c] = a[c];
    }
    wave_lds_sync();
    if (r < NB) EA[r * NB + r] = dvec;  // pad indices (>= m) carry pivot 1 and are masked by the consumer
  }
  return fast;
}
