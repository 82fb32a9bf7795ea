// solve/jacobi_eig_lds.hpp - cyclic Jacobi eigen-decomposition of a symmetric matrix in LDS (jacobi_eig_lds)
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// Cyclic Jacobi eigen-decomposition of the symmetric n x n matrix A (row-major, leading dimension ld) in LDS.
// Only the LOWER triangle of A is read and written.  On return the diagonal of A holds the eigenvalues and
// the columns of V the eigenvectors (A0 = V diag V^T).
// Round-robin pairing: n/2 disjoint rotations per step.  A <- J^T A J is applied as independent 2x2 blocks
// (rows of pair k1, columns of pair k2, k1 >= k2); V <- V J with threads grouped by pair so the rotation is
// loaded once for several rows.  The step is LDS-instruction bound, so every access is kept to the minimum:
// rotation table read as double2 / int2, no mirrored writes.  Two barriers per step.
template <int NTH>
AVM_NOINL int jacobi_eig_lds(int A_off, int V_off, int n, int ld, int rot_off) {
  double* A = LDS() + A_off;
  double* V = LDS() + V_off;
  double2* rcs = reinterpret_cast<double2*>(LDS() + rot_off);        // [np] (c, s)
  int2* rpq = reinterpret_cast<int2*>(LDS() + rot_off + 2 * 64);     // [np] (p, q), p < q
  double* red = LDS() + L_RED;
  constexpr bool WAVE = NTH == 64;  // a single wavefront: wave-level ordering of its LDS traffic is enough
  auto sync = [&]() {
    if (WAVE)
      wave_lds_sync();
    else
      __syncthreads();
  };
  const int t = WAVE ? (threadIdx.x & 63) : threadIdx.x;
  const int ne = (n + 1) & ~1, np = ne >> 1;
  for (int i = t; i < n * n; i += NTH) V[(i / n) * ld + i % n] = (i / n == i % n) ? 1.0 : 0.0;
  // static work assignment
  //  - blocks (k1 >= k2): up to MAXB per thread
  //  - V: thread -> pair kv = t / tpp, rows (t % tpp) + tpp * m
  constexpr int MAXB = 3, MAXR = 8;
  const int nblk = np * (np + 1) / 2;
  short bk1[MAXB], bk2[MAXB];
#pragma unroll
  for (int u = 0; u < MAXB; u++) {
    const int idx = t + u * NTH;
    bk1[u] = -1, bk2[u] = 0;
    if (idx < nblk) {
      int k1 = (int)((sqrt(8.0 * idx + 1.0) - 1.0) * 0.5);
      while ((k1 + 1) * (k1 + 2) / 2 <= idx) k1++;
      while (k1 * (k1 + 1) / 2 > idx) k1--;
      bk1[u] = (short)k1, bk2[u] = (short)(idx - k1 * (k1 + 1) / 2);
    }
  }
  const int tpp = max(1, NTH / np);          // threads per pair for the V update
  const int kv = t / tpp, rv0 = t % tpp;     // pair and first row of this thread (kv >= np: idle)
  sync();
  auto Lw = [&](int i, int j) -> double& { return A[max(i, j) * ld + min(i, j)]; };
  int sweeps = 0;
  for (int sweep = 0; sweep < 20; sweep++) {
    // converged when every |a_pq| <= tol sqrt(a_pp a_qq) (relative criterion: keeps the small eigenvalues
    // accurate, which matters for the 1e-8 clamp next to eigenvalues of 1e12)
    double off = 0;
    for (int i = t; i < n * n; i += NTH) {
      const int r = i / n, q = i % n;
      if (r <= q) continue;
      const double v = fabs(A[r * ld + q]);
      const double sc = sqrt(fabs(A[r * ld + r]) * fabs(A[q * ld + q]));
      off = fmax(off, sc > 0.0 ? v / sc : (v > 0.0 ? 1.0 : 0.0));
    }
    if (WAVE) {
      off = wave_max(off);
    } else {
      off = block_max<NTH>(off, red);
    }
    if (off <= 1e-15) break;
    sweeps++;
    for (int step = 0; step < ne - 1; step++) {
      if (t < np) {
        const int a = t == 0 ? ne - 1 : (step + t) % (ne - 1);
        const int b = t == 0 ? step : (step - t + (ne - 1)) % (ne - 1);
        const int pI = min(a, b), qI = max(a, b);
        double cs = 1.0, sn = 0.0;
        if (qI < n) {
          const double apq = A[qI * ld + pI];
          if (fabs(apq) > 1e-300) {
            const double tau = (A[qI * ld + qI] - A[pI * ld + pI]) / (2.0 * apq);
            const double tt = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            cs = fast_rsqrt(1.0 + tt * tt);
            sn = tt * cs;
          }
        }
        rcs[t] = double2{cs, sn};
        rpq[t] = int2{pI, qI};
      }
      sync();
#pragma unroll
      for (int u = 0; u < MAXB; u++) {
        if (bk1[u] < 0) continue;
        const int k1 = bk1[u], k2 = bk2[u];
        const int2 pq1 = rpq[k1], pq2 = rpq[k2];
        const double2 r1v = rcs[k1], r2v = rcs[k2];
        const int p1 = pq1.x, q1 = pq1.y, p2 = pq2.x, q2 = pq2.y;
        const double c1 = r1v.x, s1 = r1v.y, c2 = r2v.x, s2 = r2v.y;
        const bool r1 = q1 < n, r2 = q2 < n;  // a dummy partner (odd n) leaves its line untouched (c = 1, s = 0)
        if (k1 != k2) {
          double& e00 = Lw(p1, p2);
          const double a00 = e00, a01 = r2 ? Lw(p1, q2) : 0.0, a10 = r1 ? Lw(q1, p2) : 0.0, a11 = (r1 && r2) ? Lw(q1, q2) : 0.0;
          const double b00 = c1 * a00 - s1 * a10, b01 = c1 * a01 - s1 * a11;
          const double b10 = s1 * a00 + c1 * a10, b11 = s1 * a01 + c1 * a11;
          e00 = c2 * b00 - s2 * b01;
          if (r2) Lw(p1, q2) = s2 * b00 + c2 * b01;
          if (r1) Lw(q1, p2) = c2 * b10 - s2 * b11;
          if (r1 && r2) Lw(q1, q2) = s2 * b10 + c2 * b11;
        } else {
          // diagonal block of the pair itself: [app apq; apq aqq] -> diag(app - t apq, aqq + t apq)
          const double app = A[p1 * ld + p1];
          if (r1) {
            const double aqq = A[q1 * ld + q1], apq = A[q1 * ld + p1];
            A[p1 * ld + p1] = c1 * c1 * app - 2.0 * c1 * s1 * apq + s1 * s1 * aqq;
            A[q1 * ld + q1] = s1 * s1 * app + 2.0 * c1 * s1 * apq + c1 * c1 * aqq;
            A[q1 * ld + p1] = (c1 * c1 - s1 * s1) * apq + c1 * s1 * (app - aqq);
          }
        }
      }
      if (kv < np) {
        const int2 pq = rpq[kv];
        if (pq.y < n) {
          const double2 cs2 = rcs[kv];
#pragma unroll
          for (int m = 0; m < MAXR; m++) {
            const int i = rv0 + tpp * m;
            if (i < n) {
              const double x = V[i * ld + pq.x], y = V[i * ld + pq.y];
              V[i * ld + pq.x] = cs2.x * x - cs2.y * y;
              V[i * ld + pq.y] = cs2.y * x + cs2.x * y;
            }
          }
        }
      }
      sync();
    }
  }
  return sweeps;
}
