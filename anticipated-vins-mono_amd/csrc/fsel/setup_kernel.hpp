// fsel/setup_kernel.hpp - fsel_setup_kernel: Omega, the partial Cholesky of its non-position rows, Delta of every feature
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

// Eigen's Quaternion::slerp, which createLinearImuMatrices interpolates a pair's rotations with
AVM_DEV quat slerp_eigen(quat a, double t, quat b) {
  const double one = 1.0 - DBL_EPSILON;
  const double d = a.w * b.w + a.x * b.x + a.y * b.y + a.z * b.z;
  const double ad = fabs(d);
  double s0, s1;
  if (ad >= one) {
    s0 = 1.0 - t;
    s1 = t;
  } else {
    const double th = acos(ad), st = sin(th);
    s0 = sin((1.0 - t) * th) / st;
    s1 = sin(t * th) / st;
  }
  if (d < 0) s1 = -s1;
  return quat{s0 * a.w + s1 * b.w, s0 * a.x + s1 * b.x, s0 * a.y + s1 * b.y, s0 * a.z + s1 * b.z};
}

// ---- setup: Omega, partial Cholesky of the non-position rows, Delta of every feature ------
// (round 4) Two launches: slice 0 of every frame with the whole carve (N x N doubles of Omega: 104 KB at H = 10, one workgroup per CU), and
// the candidate slices (slice_base = 1, compact) with only what they touch - the camera frames, four wavefronts' C_h / W and Delta tiles,
// 35 KB: four workgroups per CU.  In one launch the candidate slices of a 256-frame batch (8192 workgroups) went through the CUs one at a
// time: 3.2 ms of its 10.4 (profiles/r04c_fsel.md).
__global__ __launch_bounds__(FS_NT) void fsel_setup_kernel(FselDev A, int slice_base, int compact) {
  FS_TABLES_GUARD(A);
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  double* lds = reinterpret_cast<double*>(smem_raw);
  const avm_fsel_batch& b = A.b;
  const int p = blockIdx.x, t = threadIdx.x;
  const int slice = blockIdx.y + slice_base;  // 0: Omega, its partial factorization, the used features; >= 1: candidates [16 (slice-1), 16 slice)
#ifdef FS_TRACE_EVAL
  const long long ts0 = clock64();
#endif
  const int H = b.horizon, N = 9 * (H + 1), T = 3 * H;
  double* Om = lds;                 // N*N (compact: the candidate slices' share of it, see fsel_setup_lds_bytes)
  double* Wh = Om + (compact ? (FS_NT / 64) * (FS_CPW * (6 * H + 9) + T * T) : N * N);  // [H+1][81] Omega_h (h>=1)
  double* Ah = Wh + (H + 1) * 81;   // [H+1][81] Ablk_h
  double* Th = Ah + (H + 1) * 81;   // [H+1][81] At*Omega
  double* cam = compact ? Wh : Th + (H + 1) * 81;  // [H+1][30]
  double* col = cam + (H + 1) * 30; // N
  double* red = col + N;            // 64
  int* isp = reinterpret_cast<int*>(red + 64);  // N: position-row flag
  const double* hp = b.hor_pos + (size_t)p * (H + 1) * 3;
  const double* hq = b.hor_quat + (size_t)p * (H + 1) * 4;
  const quat qic{b.q_ic[3], b.q_ic[0], b.q_ic[1], b.q_ic[2]};
  if (!compact) {
    for (int i = t; i < N * N; i += FS_NT) Om[i] = 0.0;
    for (int i = t; i < N; i += FS_NT) isp[i] = (i >= 9 && (i % 9) < 3) ? 1 : 0;
  }
  // per consecutive pair: createLinearImuMatrices (only slice 0 needs them).  The nr interpolated rotations of a pair are
  // independent: one thread each first (parked in Omega's storage, re-zeroed below), then thread h sums them in the
  // reference's order.  More rotations than fit there: thread h computes them in its loop as before.
  const int nri = b.nr_imu[p];
  const bool rpar = slice == 0 && nri > 0 && (long long)H * nri * 9 <= (long long)N * N;
  if (rpar) {
    __syncthreads();
    for (int idx = t; idx < H * nri; idx += FS_NT) {
      const int h = 1 + idx / nri, i = idx % nri;
      const quat Qi{hq[(h - 1) * 4 + 3], hq[(h - 1) * 4], hq[(h - 1) * 4 + 1], hq[(h - 1) * 4 + 2]};
      const quat Qj{hq[h * 4 + 3], hq[h * 4], hq[h * 4 + 1], hq[h * 4 + 2]};
      q2R(slerp_eigen(Qi, i / (double)nri, Qj), Om + (size_t)idx * 9);
    }
    __syncthreads();
  }
  if (slice == 0 && t >= 1 && t <= H) {
    const int h = t;
    const quat Qi{hq[(h - 1) * 4 + 3], hq[(h - 1) * 4], hq[(h - 1) * 4 + 1], hq[(h - 1) * 4 + 2]};
    const quat Qj{hq[h * 4 + 3], hq[h * 4], hq[h * 4 + 1], hq[h * 4 + 2]};
    const double nr = (double)b.nr_imu[p], dI = b.delta_imu[p];
    double Nij[9], Mij[9];
    for (int k = 0; k < 9; k++) Nij[k] = 0, Mij[k] = 0;
    double c11 = 0, c12 = 0;
    for (int i = 0; i < nr; ++i) {
      double R[9];
      if (rpar) {
        for (int k = 0; k < 9; k++) R[k] = Om[((size_t)(h - 1) * nri + i) * 9 + k];
      } else {
        q2R(slerp_eigen(Qi, i / nr, Qj), R);
      }
      const double jkh = (nr - i - 0.5);
      for (int k = 0; k < 9; k++) Nij[k] += jkh * R[k], Mij[k] += R[k];
      c11 += jkh * jkh;
      c12 += jkh;
    }
    const double d2 = dI * dI, d3 = d2 * dI, d4 = d3 * dI;
    const double ca = 1.0 * nr * c11 * d4 * b.acc_var, cb = 1.0 * c12 * d3 * b.acc_var, cd = 1.0 * nr * d2 * b.acc_var,
                 cc = 1.0 * nr * b.acc_bias_var;
    // inverse of [[ca I, cb I, 0],[cb I, cd I, 0],[0,0,cc I]]
    const double det = ca * cd - cb * cb;
    double* W = Wh + h * 81;
    double* Am = Ah + h * 81;
    for (int k = 0; k < 81; k++) W[k] = 0, Am[k] = 0;
    for (int i = 0; i < 3; i++) {
      W[i * 9 + i] = cd / det, W[i * 9 + 3 + i] = -cb / det, W[(3 + i) * 9 + i] = -cb / det, W[(3 + i) * 9 + 3 + i] = ca / det;
      W[(6 + i) * 9 + 6 + i] = 1.0 / cc;
    }
    for (int i = 0; i < 9; i++) Am[i * 9 + i] = -1.0;
    for (int i = 0; i < 3; i++) Am[i * 9 + 3 + i] = -1.0 * nr * dI;
    for (int a = 0; a < 3; a++)
      for (int c = 0; c < 3; c++) Am[a * 9 + 6 + c] = Nij[a * 3 + c] * d2, Am[(3 + a) * 9 + 6 + c] = Mij[a * 3 + c] * dI;
  }
  // camera frames for calcInfoFromFeatures
  if (t >= 64 && t <= 64 + H) {
    const int h = t - 64;
    const quat q{hq[h * 4 + 3], hq[h * 4], hq[h * 4 + 1], hq[h * 4 + 2]};
    const v3 tw = mk3(hp[h * 3], hp[h * 3 + 1], hp[h * 3 + 2]) + qrot(q, mk3(b.t_ic[0], b.t_ic[1], b.t_ic[2]));
    const quat qwc = qmul(q, qic);
    double* c = cam + h * 30;
    c[0] = tw.x, c[1] = tw.y, c[2] = tw.z;
    q2R(qinv(qwc), c + 3);                 // q_WC^-1
    q2R(qinv(qmul(qwc, qic)), c + 12);     // (q_WC * q_IC)^-1 : q_IC twice, bug-compatible (:304,:321)
    q2R(qwc, c + 21);                      // q_WC (frame k+1 back-projection)
  }
  __syncthreads();
  if (slice > 0) {
    // Delta of this slice's candidates (the camera frames above are all they need), FS_CPW candidates per wavefront: every
    // lane runs the short front part (uniform), lane 0 parks C_h and W in LDS, then the H (H + 1) / 2 block pairs go one
    // per lane - the T x T block is written by 64 lanes at once instead of 900 scattered stores from one thread.
    const int lane = t & 63, wv = t >> 6;
    // (round 4: the four candidates' front parts run side by side, a frame per lane - feature_front4; then the block pairs and the
    //  stores candidate by candidate through the wavefront's one tile)
    const int WS = 6 * H + 9;                                   // a candidate's record: C_h (6 H) | W (9)
    double* wl0 = Om + (wv * FS_CPW) * WS;                      // (Omega's storage is unused in these slices)
    double* tile = Om + (FS_NT / 64) * FS_CPW * WS + wv * T * T;  // (16 (6 H + 9) + 36 H^2 <= 81 (H + 1)^2 doubles of Omega's storage)
    const int npair = H * (H + 1) / 2;
    const int k0 = ((slice - 1) * (FS_NT / 64) + wv) * FS_CPW;
    if (k0 >= b.n_cand[p]) return;  // (wave-uniform)
    const int ku = k0 + (lane >> 4);
    const bool oku = feature_front4(b, A.kd, p, cam, ku, ku < b.n_cand[p], H, wl0 + (lane >> 4) * WS);
    wave_lds_sync();
    for (int u = 0; u < FS_CPW; u++) {
      const int k = k0 + u;
      if (k >= b.n_cand[p]) break;  // (wave-uniform)
      const bool ok = __shfl(oku ? 1 : 0, 16 * u, 64) != 0;
      if (ok) {
        const double* wl = wl0 + u * WS;
        double* out = A.delta + ((size_t)p * b.max_cand + k) * T * T;
        // the block pairs are put together in this wavefront's LDS tile and go out as whole rows (written pair by pair - 24-byte
        // pieces, ten to a row, from different lanes at different times - a batch's Deltas cost 6.8 x their size in write traffic)
        for (int q = lane; q < npair; q += 64) {
          int j = 1, rem = q;  // pairs in the order j = 1..H, i = j..H
          while (rem >= H - j + 1) rem -= H - j + 1, j++;
          feature_pair(wl, wl + 6 * H, j + rem, j, T, tile);
        }
        wave_lds_sync();
        for (int idx = lane; idx < T * T; idx += 64) out[idx] = tile[idx];
        if (A.delta_pk) {  // ... and the lower triangle by columns, for the solo form
          double* opk = A.delta_pk + ((size_t)p * b.max_cand + k) * (T * (T + 1) / 2);
          for (int cc = 0; cc < T; cc++)
            if (cc + lane < T) opk[cc * T - cc * (cc - 1) / 2 + lane] = tile[cc * T + cc + lane];  // (row cc of the symmetric tile = column cc)
        }
        __builtin_amdgcn_wave_barrier();
      }
      if (lane == 0) A.valid[(size_t)p * b.max_cand + k] = ok, A.black[(size_t)p * b.max_cand + k] = 0;
    }
    return;
  }
  if (rpar)
    for (int idx = t; idx < H * nri * 9; idx += FS_NT) Om[idx] = 0.0;  // (the parked rotations)
  for (int idx = t; idx < H * 81; idx += FS_NT) {  // Th = A^T W
    const int h = 1 + idx / 81, i = (idx % 81) / 9, j = idx % 9;
    double s = 0;
    for (int k = 0; k < 9; k++) s += Ah[h * 81 + k * 9 + i] * Wh[h * 81 + k * 9 + j];
    Th[h * 81 + i * 9 + j] = s;
  }
  __syncthreads();
  // assemble Omega: diagonal block d = Omega_d (pair d) + At*Omega*A (pair d+1) [+ I for d == 0]
  for (int idx = t; idx < (H + 1) * 81; idx += FS_NT) {
    const int d = idx / 81, i = (idx % 81) / 9, j = idx % 9;
    double s = 0;
    if (d >= 1) s += Wh[d * 81 + i * 9 + j];
    if (d < H) {  // At*Omega*A of pair d+1
      double s1 = 0;
      for (int k = 0; k < 9; k++) s1 += Th[(d + 1) * 81 + i * 9 + k] * Ah[(d + 1) * 81 + k * 9 + j];
      s += s1;
    }
    if (d == 0 && i == j) s += 1.0;
    Om[(d * 9 + i) * N + d * 9 + j] = s;
  }
  for (int idx = t; idx < H * 81; idx += FS_NT) {
    const int h = 1 + idx / 81, i = (idx % 81) / 9, j = idx % 9;
    const double v = Th[h * 81 + i * 9 + j];
    Om[((h - 1) * 9 + i) * N + h * 9 + j] = v;  // At*Omega
    Om[(h * 9 + j) * N + (h - 1) * 9 + i] = v;  // its transpose
  }
  __syncthreads();
  if (A.omega_out)
    for (int i = t; i < N * N; i += FS_NT) A.omega_out[(size_t)p * N * N + i] = Om[i];
  // constants of the Hadamard bound + original position diagonal
  double kn = 0;
  for (int i = t; i < N; i += FS_NT)
    if (!isp[i]) kn += log(Om[i * N + i]);
  kn = block_sum<FS_NT>(kn, red);
  if (t < T) A.dpp[(size_t)p * T + t] = Om[(9 * (1 + t / 3) + t % 3) * (N + 1)];
  __syncthreads();
  // Partial right-looking elimination of the non-position rows (ascending order), square-root free: row i loses
  // (A_ik / d_k) A_kj.  Omega is block tridiagonal, so a pivot of state s only reaches the rows of states s and s + 1 and -
  // through fill - the position rows of the states before s: at most 3 (s - 1) + 18 <= 54 rows, listed once per state.  Four
  // threads per listed row, every fourth listed column each (<= 14): all loads of a pivot are in flight at once, one trip
  // through LDS and ONE workgroup barrier per pivot - nobody writes row k while it is being read, and the multiplier is the
  // row's own column-k entry.  Column k is zeroed as it is consumed, so eliminated columns need no mask later; the pivots
  // are parked for the logarithms.  (The previous form - two threads per row over all columns, a column buffer and two
  // barriers per pivot - took 150 us of a single frame's select.)
  double* piv = col;  // (col[] has no other use any more)
#ifdef FS_TRACE_EVAL
  const long long ts1 = clock64();
#endif
  for (int st = 0; st <= H; st++) {
    const int npre = st >= 1 ? 3 * (st - 1) : 0;
    const int na = npre + 9 + (st < H ? 9 : 0);
    auto rowof = [&](int a) { return a < npre ? 9 * (1 + a / 3) + a % 3 : 9 * st + (a - npre); };
    const int a = t >> 2, q = t & 3;
    const int i = rowof(min(a, na - 1));
    const bool ipos = i >= 9 && (i % 9) < 3;
    constexpr int MC = 14;  // ceil(54 / 4)
    int cj[MC];
#pragma unroll
    for (int m = 0; m < MC; m++) cj[m] = q + 4 * m < na ? rowof(q + 4 * m) : -1;
    double* row = Om + i * N;
    for (int kk = st == 0 ? 0 : 3; kk < 9; kk++) {
      const int k = 9 * st + kk;
      const double dkk = Om[k * N + k];
      double inv = __builtin_amdgcn_rcp(dkk), e = fma(-dkk, inv, 1.0);
      inv = fma(inv, e, inv);
      e = fma(-dkk, inv, 1.0);
      inv = fma(inv, e, inv);
      const bool act = a < na && i != k && (i > k || ipos);
      // (every load of the pivot is requested before the first use: one trip through LDS)
      const double* rk = Om + k * N;
      const double xik = row[k];
      double rv[MC], xk[MC];
#pragma unroll
      for (int m = 0; m < MC; m++) rv[m] = row[max(cj[m], 0)], xk[m] = rk[max(cj[m], 0)];
      const double li = act ? xik * inv : 0.0;
      if (li != 0.0) {
#pragma unroll
        for (int m = 0; m < MC; m++)  // (an unlisted slot goes to a dump slot: no predicated LDS store)
          *(cj[m] >= 0 ? row + cj[m] : red + (t & 63)) = cj[m] == k ? 0.0 : rv[m] - li * xk[m];
      }
      __syncthreads();
      if (t == 0) piv[k] = dkk;
    }
  }
  __syncthreads();
  double ld = 0;
  for (int i = t; i < N; i += FS_NT)
    if (!isp[i]) ld += log(piv[i]);
  ld = 0.5 * block_sum<FS_NT>(ld, red);
#ifdef FS_TRACE_EVAL
  if (t == 0) A.consts[(size_t)p * 4 + 2] = (double)(clock64() - ts1), A.consts[(size_t)p * 4 + 3] = (double)(ts1 - ts0);
#endif
  double* C = A.C + (size_t)p * T * T;
  for (int idx = t; idx < T * T; idx += FS_NT) {
    const int i = idx / T, j = idx % T;
    C[idx] = Om[(9 * (1 + i / 3) + i % 3) * N + 9 * (1 + j / 3) + j % 3];
  }
  if (t == 0) {
    A.consts[(size_t)p * 4] = 2.0 * ld;
    A.consts[(size_t)p * 4 + 1] = kn;
    A.nsel[p] = 0;
    A.done[p] = 0;
  }
  // Delta of the already-used subset (the candidates are done by the other slices of the grid).  feature_delta writes
  // every entry of the T x T block unless it returns false, and an invalid feature's block is never read.
  const int nu = b.n_used ? b.n_used[p] : 0;
  for (int k = t; k < nu; k += FS_NT) {
    const double* xy = b.used_xy + ((size_t)p * b.max_used + k) * 2;
    A.valid_u[(size_t)p * b.max_used + k] = feature_delta(b, A.kd, p, cam, xy[0], xy[1], H, A.delta_u + ((size_t)p * b.max_used + k) * T * T);
  }
  __syncthreads();
  // Omega += sum of Delta_used (ascending id order = input order)
  for (int idx = t; idx < T * T; idx += FS_NT) {
    double s = C[idx], dd = 0;
    for (int u = 0; u < nu; u++)
      if (A.valid_u[(size_t)p * b.max_used + u]) {
        const double v = A.delta_u[((size_t)p * b.max_used + u) * T * T + idx];
        s += v;
        dd += v;
      }
    C[idx] = s;
    if (idx / T == idx % T) A.dpp[(size_t)p * T + idx / T] += dd;
  }
}
