// solve/imu_mfma.hpp - one IMU factor on the matrix cores: ImuOperands, imu_factor_load, imu_factor_mfma
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// One wavefront, one IMU factor i: J = sqrt_info * [r | J_raw] (15 x 31) and its Gram matrix on v_mfma_f64_16x16x4,
// then S += J^T J (lower), g += J^T r; returns 0.5 r^T r on lane 0 (0 elsewhere).
// The two 16-column accumulator tiles of J are, register for register, both the A operand (J^T) and the B operand
// (J) of the Gram products, so nothing moves between the two steps.  Factors sharing a frame must not run
// concurrently (the caller alternates even / odd factors).
struct ImuOperands {
  double ua[4], b0[4], b1[4];
};
// operands of factor i: clamped unconditional loads (issued for both factors of a wavefront before the first is used)
AVM_DEV void imu_factor_load(int i, ImuOperands& o) {
  const WinCtx& c = lds_ctx();
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  gcdouble* U = c.psqrt + i * 225;                 // upper triangular, zeros stored below the diagonal
  gcdouble* raw = c.sc + Scratch::IJRAW + i * IJBLK; // [15][31]: column 0 = residual, 1..30 = Jacobian
  const int lic = min(li, 14);
  // The combined columns are taken in the order residual | pose i | pose i + 1 | speed-bias i | speed-bias i + 1, the
  // order of the state columns themselves (12 consecutive pose columns, 18 consecutive speed-bias entries), so that the scatter of
  // imu_factor_mfma needs no ordering of (row, column) and its offsets are linear in i.  raw's own order is pose i | sb i | pose i + 1 | sb i + 1.
  auto rawcol = [](int cc) { return cc <= 6 ? cc : (cc <= 12 ? cc + 9 : (cc <= 21 ? cc - 6 : cc)); };
  const int c0 = rawcol(li), c1 = rawcol(16 + lic);
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const int k = min(lk + 4 * m, 14);
    o.ua[m] = U[lic * 15 + k], o.b0[m] = raw[k * 31 + c0], o.b1[m] = raw[k * 31 + c1];
  }
#pragma unroll
  for (int m = 0; m < 4; m++) {
    const bool kv = lk + 4 * m < 15;
    o.ua[m] = (li < 15 && kv) ? o.ua[m] : 0.0;
    o.b0[m] = kv ? o.b0[m] : 0.0;
    o.b1[m] = (kv && li < 15) ? o.b1[m] : 0.0;
  }
}

AVM_DEV double imu_factor_mfma(const WinCtx&, int i, const ImuOperands& ops) {
  double* lds = LDS();
  const int lane = threadIdx.x & 63, li = lane & 15, lk = lane >> 4;
  double ua[4], b0[4], b1[4];
#pragma unroll
  for (int m = 0; m < 4; m++) ua[m] = ops.ua[m], b0[m] = ops.b0[m], b1[m] = ops.b1[m];
  d4 D0 = {0, 0, 0, 0}, D1 = {0, 0, 0, 0};
#pragma unroll
  for (int m = 0; m < 4; m++) {
    D0 = __builtin_amdgcn_mfma_f64_16x16x4f64(ua[m], b0[m], D0, 0, 0, 0);
    D1 = __builtin_amdgcn_mfma_f64_16x16x4f64(ua[m], b1[m], D1, 0, 0, 0);
  }
  d4 G00 = {0, 0, 0, 0}, G10 = {0, 0, 0, 0}, G11 = {0, 0, 0, 0};
#pragma unroll
  for (int m = 0; m < 4; m++) {
    G00 = __builtin_amdgcn_mfma_f64_16x16x4f64(D0[m], D0[m], G00, 0, 0, 0);
    G10 = __builtin_amdgcn_mfma_f64_16x16x4f64(D1[m], D0[m], G10, 0, 0, 0);
    G11 = __builtin_amdgcn_mfma_f64_16x16x4f64(D1[m], D1[m], G11, 0, 0, 0);
  }
  // scatter: combined index 0 = residual, p + 1 = local column p.  Branch-free: every lane computes the destination of
  // its (up to) 12 entries - or its private dump slot in the scratch tile - then all reads, all adds, all writes
  // (a predicated LDS read-modify-write is a branch with its own s_waitcnt; 16 of them in a row cost ~2K cycles).
  double half_rr = 0;
  // (round 5) combined index cc: 0 = residual, 1..12 = pose column 6 i + cc - 1, 13..30 = speed-bias entry 9 i + cc - 13 (rows of the compact
  // speed-bias storage, s_off): rows and columns ascend together, and everything but the row term is a constant of the lane
  {
    auto gcol = [&](int cc) { return cc <= 12 ? 6 * i + cc - 1 : SB0 + 9 * i + cc - 13; };  // state column of combined column cc >= 1
#ifdef AVM_TP
    const int psb = reinterpret_cast<const int*>(lds + L_INT)[I_PSB];
    auto dest = [&](int R, int C) {  // R >= C >= 1
      if (R <= 12) return L_S + roff(6 * i + R - 1) + 6 * i + C - 1;
      const int qq = R - 13, second = qq >= 9 ? 1 : 0;
      const int row = L_SBC + (9 * i + qq) * SBW;
      if (C > 12) return row + 18 + (C - 13) + 9 - 9 * second;
      return (i + second == psb) ? L_STRIP + (qq - 9 * second) * NPOSE + 6 * i + C - 1 : row + (C - 1) + 6 - 6 * second;
    };
#else
    auto dest = [&](int R, int C) { return L_S + roff(gcol(R)) + gcol(C); };  // R >= C >= 1: the packed triangle
#endif
    // entries of S are written Jacobi-scaled (see frame_task); the gradient is scaled afterwards, as a vector
    auto scl = [&](int g) { return lds[L_SC + g]; };
    const int dump = L_DUMP + lane;
    const double sc0 = li > 0 ? scl(gcol(li)) : 1.0, sc1 = li < 15 ? scl(gcol(16 + li)) : 1.0;
    int off[12];
    double val[12];
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int R0 = lk + 4 * r, R1 = 16 + R0;  // combined rows in tile 0 / tile 1 (31 = padding)
      const double sr0 = scl(gcol(max(R0, 1))), sr1 = scl(gcol(min(R1, 30)));
      if (R0 == 0 && li == 0) half_rr = 0.5 * G00[r];
      const bool v00 = R0 > 0 && li <= R0, v10 = R1 < 31, v11 = R1 < 31 && li < 15 && 16 + li <= R1;
      off[3 * r] = !v00 ? dump : (li == 0 ? L_G + gcol(max(R0, 1)) : dest(max(R0, 1), max(li, 1)));
      val[3 * r] = G00[r] * (li == 0 ? 1.0 : sr0 * sc0);
      off[3 * r + 1] = !v10 ? dump : (li == 0 ? L_G + gcol(min(R1, 30)) : dest(min(R1, 30), max(li, 1)));
      val[3 * r + 1] = G10[r] * (li == 0 ? 1.0 : sr1 * sc0);
      off[3 * r + 2] = !v11 ? dump : dest(min(R1, 30), min(16 + li, min(R1, 30)));
      val[3 * r + 2] = G11[r] * (sr1 * sc1);
    }
    double cur[12];
#pragma unroll
    for (int q = 0; q < 12; q++) cur[q] = lds[off[q]];
#pragma unroll
    for (int q = 0; q < 12; q++) lds[off[q]] = cur[q] + val[q];
    return half_rr;
  }
}
