// solve/prior_jtj.hpp - the prior's J0^T J0 on the matrix cores (prior_jtj_add_lds, prior_jtj_packed)
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// Prior J0^T J0 on the matrix cores (16x16 tiles, K = prior rows), marginalization-kernel variant: the tiles are
// added straight into the packed system in LDS at the
// columns pidx[] maps the prior's columns to (every lower entry is produced exactly once, so the wavefronts never
// touch the same element).  All operand loads of a tile are issued before the MFMA chain.
AVM_NOINL void prior_jtj_add_lds(gcdouble* pJ, int ldp, int pn, int s_off) {
  double* lds = LDS();
  const int* pidx = reinterpret_cast<const int*>(lds + L_INT) + I_PIDX;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int ntl = (pn + 15) >> 4;
  for (int tile = wv; tile < ntl * (ntl + 1) / 2; tile += NT / 64) {
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= tile) ti++;
    const int tj = tile - ti * (ti + 1) / 2;
    const int ca = min(16 * ti + (lane & 15), pn - 1), cb = min(16 * tj + (lane & 15), pn - 1);
    const bool va = 16 * ti + (lane & 15) < pn, vb = 16 * tj + (lane & 15) < pn;
    double av[MAXPRIOR / 4], bv[MAXPRIOR / 4];
#pragma unroll
    for (int m = 0; m < MAXPRIOR / 4; m++) {
      const int r = 4 * m + (lane >> 4), rc = min(r, pn - 1);
      const double a = pJ[(size_t)rc * ldp + ca], b = pJ[(size_t)rc * ldp + cb];
      av[m] = (r < pn && va) ? a : 0.0;
      bv[m] = (r < pn && vb) ? b : 0.0;
    }
    d4 D = {0, 0, 0, 0};
#pragma unroll
    for (int m = 0; m < MAXPRIOR / 4; m++) D = __builtin_amdgcn_mfma_f64_16x16x4f64(av[m], bv[m], D, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int gi = 16 * ti + (lane >> 4) + 4 * r, gj = 16 * tj + (lane & 15);
      if (gi < pn && gj <= gi) {
        const int ip = pidx[gi], iq = pidx[gj];
        if (ip >= 0 && iq >= 0) lds[s_off + roff(max(ip, iq)) + min(ip, iq)] += D[r];
      }
    }
  }
}

// Solve-kernel variant: lower triangle packed by idx = p (p + 1) / 2 + q into HPk, plus the destination of every
// entry inside the packed S (or -1 if the prior column is not a state of the solve) - the per-iteration add is then
// a flat gather (solve/slot.hpp: the HP region).  All operand loads of a tile are issued before the MFMA chain.
AVM_NOINL void prior_jtj_packed(gcdouble* pJ, int ldp, int pn, gdouble* HPk, gint* dst) {
  const int* pidx = reinterpret_cast<const int*>(LDS() + L_INT) + I_PIDX;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int ntl = (pn + 15) >> 4;
  for (int tile = wv; tile < ntl * (ntl + 1) / 2; tile += NT / 64) {
    int ti = 0;
    while ((ti + 1) * (ti + 2) / 2 <= tile) ti++;
    const int tj = tile - ti * (ti + 1) / 2;
    const int ca = 16 * ti + (lane & 15), cb = 16 * tj + (lane & 15);
    // all 48 loads in flight (clamped to a valid element, masked afterwards: a predicated load is a branch with its own
    // s_waitcnt), four independent MFMA chains
    double av[MAXPRIOR / 4], bv[MAXPRIOR / 4];
    const int cac = min(ca, pn - 1), cbc = min(cb, pn - 1);
#pragma unroll
    for (int m = 0; m < MAXPRIOR / 4; m++) {
      const int r = min(4 * m + (lane >> 4), pn - 1);
      av[m] = pJ[(size_t)r * ldp + cac];
      bv[m] = pJ[(size_t)r * ldp + cbc];
    }
    d4 Dq[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
#pragma unroll
    for (int m = 0; m < MAXPRIOR / 4; m++) {
      const bool rv = 4 * m + (lane >> 4) < pn;
      const double a = (rv && ca < pn) ? av[m] : 0.0, b = (rv && cb < pn) ? bv[m] : 0.0;
      Dq[m & 3] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, Dq[m & 3], 0, 0, 0);
    }
    const d4 D = (Dq[0] + Dq[1]) + (Dq[2] + Dq[3]);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int gi = 16 * ti + (lane >> 4) + 4 * r, gj = 16 * tj + (lane & 15);
      if (gi < pn && gj <= gi) {
        const int idx = gi * (gi + 1) / 2 + gj;
        const int ip = pidx[gi], iq = pidx[gj];
        HPk[idx] = D[r];
#ifdef AVM_TP
        dst[idx] = (ip < 0 || iq < 0) ? -1 : s_off(max(ip, iq), min(ip, iq)) - L_S;  // (-1 also where the structural form has no slot: see tp_prior_ok)
#else
        dst[idx] = (ip < 0 || iq < 0) ? -1 : roff(max(ip, iq)) + min(ip, iq);
#endif
      }
    }
  }
}
