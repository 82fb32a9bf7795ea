// visual_align.hip — Estimator::visualInitialAlign on gfx950 (vins_estimator/src/estimator.cpp:355-431) with
// VisualIMUAlignment (vins_estimator/src/initial/initial_aligment.cpp:199-207): the step that starts a stream.  Restated literally,
// quirks included: every formula carries its file:line.
// Mapping: one 64-lane wavefront per window in every kernel, lane = interval of all_image_frame (AVM_MAX_ALIGN_FRAMES = 64 frames give
// 63 intervals).
//  align_gyro_bias_kernel  midpoint pre-integration of the lane's interval (delta p, q, v, sum_dt and the d theta / d bg block, whose
//                          recursion J <- (I - [w]x dt) J - I dt does not involve the rest of the 15 x 15 jacobian), the 3 x 3 system of
//                          solveGyroscopeBias through the butterfly wave_sum, Bgs += delta_bg, and the repropagation with (0, Bgs[0]).
//  align_solve_kernel      LinearAlignment + RefineGravity.  The lane forms the Gram matrix of its 6 x 10 (6 x 9) block; the system
//                          lives in LDS in its structural form - the band of the block-tridiagonal velocity part (3F rows x 6), the
//                          border rows (g | s, or w1 w2 | s) and the right-hand side as one more border row, the corner -, never dense.
//                          Two rows of frames share a diagonal block: the lanes add their halves in two phases, no atomics.  Factorization:
//                          right-looking Cholesky of the arrow matrix, a serial chain over the 3F columns; the <= 55 entries a column
//                          updates (band 15, border x band 25, corner 15) are one lane each.  The right-hand side rides along as a border
//                          row, so the forward substitution is part of the factorization.
//  align_prepare_kernel /  the change of state (estimator.cpp:367-426) around triangulate_kernel (zero tic): key-frame poses in, depths
//  align_apply_kernel      to -1, then scale, velocities, gravity alignment.
// Deviation (stated in avm.h): a non-positive or non-finite pivot ends the window with ok = 0, where Eigen's pivoted LDLT returns some
// vector the reference gives no meaning to; fewer than 4 frames (6 (F - 1) < 3 F + 4 equations) are refused the same way.
#include "devmath.hpp"
#include "kernels.hpp"

namespace avm {

namespace {
constexpr int AMF = AVM_MAX_ALIGN_FRAMES;  // 64
constexpr int ANV = 3 * AMF;               // 192 velocity unknowns
constexpr int ABR = 5;                     // border rows held: g (3) | s | right-hand side

struct AlignSys {
  double band[ANV][6];   // band[r][d] = A(r, r - d): the lower band of the velocity part
  double bord[ABR][ANV]; // bord[c][r] = A(3F + c, r); row nb: the right-hand side
  double corner[ABR][ABR];
};
struct AlignLds {
  AlignSys acc;  // the accumulated system (RefineGravity keeps adding to it, initial_aligment.cpp:63-66)
  AlignSys wrk;  // the copy that is factorized
  double x[ANV + 4];
  int flag;
};

AVM_DEV bool finite3(v3 a) { return isfinite(a.x) && isfinite(a.y) && isfinite(a.z); }
AVM_DEV v3 ld3(const double* p) { return mk3(p[0], p[1], p[2]); }
AVM_DEV v3 normalized3(v3 a) { return (1.0 / sqrt(dot(a, a))) * a; }  // (Eigen: v / norm)

struct AlignPre {
  v3 dp, dv;
  quat dq;
  double sum_dt;
  double J[9];  // jacobian.block<3, 3>(O_R, O_BG)
};

// IntegrationBase::midPointIntegration / propagate (integration_base.h:54-158) for one interval, serial over its samples
AVM_DEV AlignPre align_preintegrate(const avm_align_batch& a, long iv, int ns, v3 lba, v3 lbg) {
  const double* acc = a.imu_acc + iv * (a.max_samp + 1) * 3;
  const double* gyr = a.imu_gyr + iv * (a.max_samp + 1) * 3;
  const double* dts = a.imu_dt + iv * a.max_samp;
  AlignPre o;
  o.dp = mk3(0, 0, 0), o.dv = mk3(0, 0, 0), o.dq = quat{1, 0, 0, 0}, o.sum_dt = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) o.J[k] = 0;
  v3 acc0 = ld3(acc), gyr0 = ld3(gyr);
  for (int s = 0; s < ns; s++) {
    const double dt = dts[s];
    const v3 acc1 = ld3(acc + 3 * (s + 1)), gyr1 = ld3(gyr + 3 * (s + 1));
    // integration_base.h:63-69
    const v3 un_acc_0 = qrot(o.dq, acc0 - lba);
    const v3 un_gyr = 0.5 * (gyr0 + gyr1) - lbg;
    const quat rq = qmul(o.dq, quat{1, un_gyr.x * dt / 2, un_gyr.y * dt / 2, un_gyr.z * dt / 2});
    const v3 un_acc_1 = qrot(rq, acc1 - lba);
    const v3 un_acc = 0.5 * (un_acc_0 + un_acc_1);
    o.dp = o.dp + dt * o.dv + (0.5 * dt * dt) * un_acc;
    o.dv = o.dv + dt * un_acc;
    // rows theta of F (integration_base.h:96,98): F(theta, theta) = I - R_w_x dt, F(theta, bg) = -I dt; row bg of the jacobian stays I
    double Fw[9], Jn[9];
    skew9(un_gyr, Fw);
#pragma unroll
    for (int k = 0; k < 9; k++) Fw[k] = ((k % 4 == 0) ? 1.0 : 0.0) - Fw[k] * dt;
    mat3mul(Fw, o.J, Jn);
#pragma unroll
    for (int k = 0; k < 9; k++) o.J[k] = Jn[k] - ((k % 4 == 0) ? dt : 0.0);
    o.dq = qnormalized(rq);  // integration_base.h:153
    o.sum_dt += dt;
    acc0 = acc1, gyr0 = gyr1;
  }
  return o;
}

AVM_DEV int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }
}  // namespace

// ---- table validation, one thread per window (kernels.hpp: check_align_tables) ----------------------------------------------------
__global__ __launch_bounds__(64) void validate_align_kernel(avm_align_batch a, int keys, int* first_bad) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= a.n_windows) return;
  const int rule = check_align_tables(a, b, keys != 0);
  if (rule) atomicMin(first_bad, b * 8 + rule);
}

hipError_t launch_validate_align(const avm_align_batch& a, bool keys, int* first_bad, hipStream_t stream) {
  hipLaunchKernelGGL(validate_align_kernel, dim3((a.n_windows + 63) / 64), dim3(64), 0, stream, a, keys ? 1 : 0, first_bad);
  return hipGetLastError();
}

// ---- solveGyroscopeBias (initial_aligment.cpp:3-37) ----------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void align_gyro_bias_kernel(AlignArgs A) {
  const avm_align_batch& a = A.a;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int MF = a.max_frames, F = clampi(a.n_frames[b], 2, MF);
  const bool on = lane < F - 1;
  const int j = on ? lane : 0;
  const long iv = (long)b * (MF - 1) + j;
  const int ns = on ? clampi(a.imu_n[iv], 0, a.max_samp) : 0;
  AlignPre p = align_preintegrate(a, iv, ns, ld3(a.imu_lin_ba + iv * 3), ld3(a.imu_lin_bg + iv * 3));
  double S[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // A00 A10 A11 A20 A21 A22 | b0 b1 b2
  if (on) {
    const double* Ri = a.frame_R + ((size_t)b * MF + j) * 9;
    const double* Rj = Ri + 9;
    double M[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) M[r * 3 + c] = Ri[r] * Rj[c] + Ri[3 + r] * Rj[3 + c] + Ri[6 + r] * Rj[6 + c];  // R_i^T R_j
    const quat q_ij = R2q(M);                    // Eigen::Quaterniond(Matrix3d), branches kept (:19)
    const quat d = qmul(qinv(p.dq), q_ij);       // delta_q.inverse() = conj / |q|^2 (:21)
    const double tb[3] = {2 * d.x, 2 * d.y, 2 * d.z};
    int k = 0;
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c <= r; c++) S[k++] = p.J[r] * p.J[c] + p.J[3 + r] * p.J[3 + c] + p.J[6 + r] * p.J[6 + c];  // J^T J (:22)
#pragma unroll
    for (int r = 0; r < 3; r++) S[6 + r] = p.J[r] * tb[0] + p.J[3 + r] * tb[1] + p.J[6 + r] * tb[2];  // J^T tmp_b (:23)
  }
#pragma unroll
  for (int k = 0; k < 9; k++) S[k] = wave_sum(S[k]);
  // A.ldlt().solve(b) (:26) as an unpivoted 3 x 3 Cholesky
  bool ok = true;
  v3 dbg = mk3(0, 0, 0);
  {
    const double l00 = sqrt(S[0]);
    ok = ok && S[0] > 0 && isfinite(S[0]);
    const double l10 = S[1] / l00, l20 = S[3] / l00;
    const double d1 = S[2] - l10 * l10;
    ok = ok && d1 > 0 && isfinite(d1);
    const double l11 = sqrt(d1), l21 = (S[4] - l20 * l10) / l11;
    const double d2 = S[5] - l20 * l20 - l21 * l21;
    ok = ok && d2 > 0 && isfinite(d2);
    const double l22 = sqrt(d2);
    const double y0 = S[6] / l00, y1 = (S[7] - l10 * y0) / l11, y2 = (S[8] - l20 * y0 - l21 * y1) / l22;
    const double x2 = y2 / l22, x1 = (y1 - l21 * x2) / l11, x0 = (y0 - l10 * x1 - l20 * x2) / l00;
    dbg = mk3(x0, x1, x2);
    ok = ok && finite3(dbg);
    if (!ok) dbg = mk3(0, 0, 0);  // a window that fails here keeps its biases
  }
  // Bgs[i] += delta_bg (:29-30), then repropagate(0, Bgs[0]) for every interval (:32-36).  Without a window batch Bgs[0] is the
  // linearization bias of interval 0 (avm.h)
  double* sb = A.has_windows ? A.w.speedbias + (size_t)b * NFR * 9 : nullptr;
  const v3 bg0 = sb ? ld3(sb + 6) : ld3(a.imu_lin_bg + (size_t)b * (MF - 1) * 3);
  const v3 bgn = bg0 + dbg;
  p = align_preintegrate(a, iv, ns, mk3(0, 0, 0), bgn);
  if (on) {
    double* od = A.delta + iv * 10;
    od[0] = p.dp.x, od[1] = p.dp.y, od[2] = p.dp.z;
    od[3] = p.dq.x, od[4] = p.dq.y, od[5] = p.dq.z, od[6] = p.dq.w;
    od[7] = p.dv.x, od[8] = p.dv.y, od[9] = p.dv.z;
    A.sum_dt[iv] = p.sum_dt;
  }
  __syncthreads();  // (every lane has read Bgs[0])
  if (sb && lane < NFR) {
    sb[lane * 9 + 6] += dbg.x, sb[lane * 9 + 7] += dbg.y, sb[lane * 9 + 8] += dbg.z;
  }
  if (lane == 0) {
    A.out.delta_bg[b * 3] = dbg.x, A.out.delta_bg[b * 3 + 1] = dbg.y, A.out.delta_bg[b * 3 + 2] = dbg.z;
    A.out.ok[b] = ok ? 1 : 0;
  }
}

namespace {

AVM_DEV void sys_zero(AlignSys& s, int lane) {
  for (int i = lane; i < ANV * 6; i += 64) (&s.band[0][0])[i] = 0.0;
  for (int i = lane; i < ABR * ANV; i += 64) (&s.bord[0][0])[i] = 0.0;
  if (lane < ABR * ABR) (&s.corner[0][0])[lane] = 0.0;
}
AVM_DEV void sys_scale_copy(AlignSys& s, AlignSys& w, double f, int lane) {  // A = A * 1000, b = b * 1000 (:115-116, :177-178)
  for (int i = lane; i < ANV * 6; i += 64) (&w.band[0][0])[i] = (&s.band[0][0])[i] = (&s.band[0][0])[i] * f;
  for (int i = lane; i < ABR * ANV; i += 64) (&w.bord[0][0])[i] = (&s.bord[0][0])[i] = (&s.bord[0][0])[i] * f;
  if (lane < ABR * ABR) (&w.corner[0][0])[lane] = (&s.corner[0][0])[lane] = (&s.corner[0][0])[lane] * f;
}

// The lane's 6 x (6 + NB) block T and right-hand side tb into the accumulated system: r_A = T^T T, r_b = T^T tb (:103-113, :165-175).
// Rows 3i+3..3i+5 in the first phase, rows 3i..3i+2 - which lane i - 1 has just written - in the second.
template <int NB>
AVM_DEV void sys_add(AlignSys& s, const double (&T)[6][6 + NB], const double (&tb)[6], bool on, int i, int lane) {
  constexpr int NC = 6 + NB;
  double G[NC][NC], rb[NC];
#pragma unroll
  for (int p = 0; p < NC; p++) {
#pragma unroll
    for (int q = 0; q <= p; q++) {
      double v = 0;
#pragma unroll
      for (int r = 0; r < 6; r++) v += T[r][p] * T[r][q];
      G[p][q] = on ? v : 0.0;
    }
    double v = 0;
#pragma unroll
    for (int r = 0; r < 6; r++) v += T[r][p] * tb[r];
    rb[p] = on ? v : 0.0;
  }
#pragma unroll
  for (int ph = 1; ph >= 0; ph--) {
    if (on) {
#pragma unroll
      for (int pp = 0; pp < 3; pp++) {
        const int p = 3 * ph + pp, row = 3 * i + p;
#pragma unroll
        for (int q = 0; q <= p; q++) s.band[row][p - q] += G[p][q];
#pragma unroll
        for (int c = 0; c < NB; c++) s.bord[c][row] += G[6 + c][p];
        s.bord[NB][row] += rb[p];
      }
    }
    wave_lds_sync();
  }
  // the corner and the tail of b: every interval adds to them (:109-110, :171-172) - fixed-order butterfly
#pragma unroll
  for (int c = 0; c < NB; c++) {
#pragma unroll
    for (int d = 0; d <= c; d++) {
      const double v = wave_sum(G[6 + c][6 + d]);
      if (lane == 0) s.corner[c][d] += v;
    }
    const double v = wave_sum(rb[6 + c]);
    if (lane == 0) s.corner[NB][c] += v;
  }
  wave_lds_sync();
}

// Cholesky of the arrow system in w (nv band rows, nb border rows, the right-hand side as border row nb) and the solve; the solution
// in x[0 .. nv + nb).  false: a pivot that is not a positive finite number.
AVM_DEV bool sys_solve(AlignLds& L, int nv, int nb, int lane) {
  AlignSys& w = L.wrk;
  const int nb1 = nb + 1;
  // what this lane updates in a step: 0 band (row k + p, column k + q), 1 border c x band column k + p, 2 corner (p, q)
  int role = -1, p = 0, q = 0;
  if (lane < 15) {
    role = 0;
    int t = lane;
    p = 1;
    while (t >= p) t -= p, p++;
    q = t + 1;  // 1 <= q <= p <= 5
  } else if (lane < 15 + 5 * nb1) {
    role = 1, p = (lane - 15) / 5, q = (lane - 15) % 5 + 1;  // border row p, band offset q
  } else if (lane >= 40 && lane < 55) {
    int t = lane - 40;
    p = 0;
    while (t > p) t -= p + 1, p++;
    q = t;  // 0 <= q <= p <= 4
    role = p < nb1 ? 2 : -1;
  }
  bool ok = true;
  for (int k = 0; k < nv; k++) {
    const double piv = w.band[k][0];
    if (!(piv > 0.0) || !isfinite(piv)) {
      ok = false;
      break;  // (uniform)
    }
    const double l = sqrt(piv);
    if (lane < 5) {
      if (k + lane + 1 < nv) w.band[k + lane + 1][lane + 1] /= l;
    } else if (lane < 5 + nb1) {
      w.bord[lane - 5][k] /= l;
    } else if (lane == 63) {
      w.band[k][0] = l;
    }
    wave_lds_sync();
    if (role == 0) {
      if (k + p < nv) w.band[k + p][p - q] -= w.band[k + p][p] * w.band[k + q][q];
    } else if (role == 1) {
      if (k + q < nv) w.bord[p][k + q] -= w.bord[p][k] * w.band[k + q][q];
    } else if (role == 2) {
      w.corner[p][q] -= w.bord[p][k] * w.bord[q][k];
    }
    wave_lds_sync();
  }
  // the corner: dense Cholesky of nb x nb with the right-hand side row, then its back substitution
  if (lane == 0) {
    bool cok = ok;
    for (int jj = 0; jj < nb && cok; jj++) {
      double d = w.corner[jj][jj];
      for (int t = 0; t < jj; t++) d -= w.corner[jj][t] * w.corner[jj][t];
      if (!(d > 0.0) || !isfinite(d)) {
        cok = false;
        break;
      }
      d = sqrt(d);
      w.corner[jj][jj] = d;
      for (int ii = jj + 1; ii <= nb; ii++) {
        double v = w.corner[ii][jj];
        for (int t = 0; t < jj; t++) v -= w.corner[ii][t] * w.corner[jj][t];
        w.corner[ii][jj] = v / d;
      }
    }
    if (cok)
      for (int c = nb - 1; c >= 0; c--) {
        double v = w.corner[nb][c];
        for (int ii = c + 1; ii < nb; ii++) v -= w.corner[ii][c] * L.x[nv + ii];
        L.x[nv + c] = v / w.corner[c][c];
      }
    L.flag = cok ? 1 : 0;
  }
  wave_lds_sync();
  if (L.flag == 0) return false;
  // z = y - (border)^T x_t for every row, then the serial chain of the band
  for (int r = lane; r < nv; r += 64) {
    double v = w.bord[nb][r];
    for (int c = 0; c < nb; c++) v -= w.bord[c][r] * L.x[nv + c];
    L.x[r] = v;
  }
  wave_lds_sync();
  if (lane == 0) {
    for (int r = nv - 1; r >= 0; r--) {
      double v = L.x[r];
      for (int m = 1; m <= 5 && r + m < nv; m++) v -= w.band[r + m][m] * L.x[r + m];
      L.x[r] = v / w.band[r][0];
    }
  }
  wave_lds_sync();
  return true;
}
}  // namespace

// ---- LinearAlignment (initial_aligment.cpp:125-197) with RefineGravity (:55-123) and TangentBasis (:40-53) ---------------------------
__global__ __launch_bounds__(64) void align_solve_kernel(AlignArgs A) {
  __shared__ AlignLds L;
  const avm_align_batch& a = A.a;
  const int b = blockIdx.x, lane = threadIdx.x;
  const int MF = a.max_frames, F = clampi(a.n_frames[b], 2, MF);
  const bool on = lane < F - 1;
  const int i = on ? lane : 0;
  const long iv = (long)b * (MF - 1) + i;
  const int nv = 3 * F;
  const double Gn = A.g_norm;
  // the lane's interval
  const double* Ri = a.frame_R + ((size_t)b * MF + i) * 9;
  const double* Rj = Ri + 9;
  const v3 Ti = ld3(a.frame_T + ((size_t)b * MF + i) * 3), Tj = ld3(a.frame_T + ((size_t)b * MF + i) * 3 + 3);
  const v3 tic = ld3(a.tic + (size_t)b * 3);
  const double* dl = A.delta + iv * 10;
  const v3 dp = ld3(dl), dv = ld3(dl + 7);
  const double dt = A.sum_dt[iv];
  double RiTRj[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) RiTRj[r * 3 + c] = Ri[r] * Rj[c] + Ri[3 + r] * Rj[3 + c] + Ri[6 + r] * Rj[6 + c];
  const v3 dT = (1.0 / 100.0) * RTmul(Ri, Tj - Ti);               // R_i^T (T_j - T_i) / 100 (:151)
  const v3 bp = dp + Rmul(RiTRj, tic) - tic;                      // delta_p + R_i^T R_j TIC - TIC (:152)
  bool ok = A.out.ok[b] != 0 && F >= 4;  // 6 (F - 1) equations for 3 F + 4 unknowns

  sys_zero(L.acc, lane);
  wave_lds_sync();
  {
    double T[6][10], tb[6];
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double I = r == c ? 1.0 : 0.0;
        T[r][c] = -dt * I, T[r][3 + c] = 0.0, T[r][6 + c] = Ri[c * 3 + r] * dt * dt / 2;  // (:149-150)
        T[3 + r][c] = -I, T[3 + r][3 + c] = RiTRj[r * 3 + c], T[3 + r][6 + c] = Ri[c * 3 + r] * dt;  // (:154-156)
      }
      T[r][9] = get(dT, r), T[3 + r][9] = 0.0;
      tb[r] = get(bp, r), tb[3 + r] = get(dv, r);  // (:152, :157)
    }
    sys_add<4>(L.acc, T, tb, on, i, lane);
  }
  sys_scale_copy(L.acc, L.wrk, 1000.0, lane);
  wave_lds_sync();
  ok = sys_solve(L, nv, 4, lane) && ok;
  v3 g = mk3(0, 0, 0);
  double s = 0;
  if (ok) {
    g = mk3(L.x[nv], L.x[nv + 1], L.x[nv + 2]);  // (:182)
    s = L.x[nv + 3] / 100.0;                     // (:180)
    const double gn = sqrt(dot(g, g));
    ok = finite3(g) && isfinite(s) && !(fabs(gn - Gn) > 1.0 || s < 0);  // (:184)
  }
  double* xo = A.out.x + (size_t)b * (3 * MF + 1);
  for (int r = lane; r < 3 * MF + 1; r += 64) xo[r] = (ok && r < nv) ? L.x[r] : 0.0;
  wave_lds_sync();
  if (ok) {
    // RefineGravity: A and b live outside the k loop and are neither cleared nor un-scaled between the passes (:63-66, :115-116)
    v3 g0 = Gn * normalized3(g);  // (:57)
    sys_zero(L.acc, lane);
    wave_lds_sync();
    for (int k = 0; k < 4 && ok; k++) {
      // TangentBasis (:40-53)
      const v3 an = normalized3(g0);
      v3 tmp = mk3(0, 0, 1);
      if (an.x == 0.0 && an.y == 0.0 && an.z == 1.0) tmp = mk3(1, 0, 0);
      const v3 lx = normalized3(tmp - dot(an, tmp) * an);
      const v3 ly = cross(an, lx);
      double T[6][9], tb[6];
      const v3 Rg = RTmul(Ri, g0);
#pragma unroll
      for (int r = 0; r < 3; r++) {
        const v3 RiTr = mk3(Ri[r], Ri[3 + r], Ri[6 + r]);  // row r of R_i^T
#pragma unroll
        for (int c = 0; c < 3; c++) {
          const double I = r == c ? 1.0 : 0.0;
          T[r][c] = -dt * I, T[r][3 + c] = 0.0;
          T[3 + r][c] = -I, T[3 + r][3 + c] = RiTRj[r * 3 + c];
        }
        const double wx = dot(RiTr, lx), wy = dot(RiTr, ly);
        T[r][6] = dt * dt / 2 * wx, T[r][7] = dt * dt / 2 * wy, T[r][8] = get(dT, r);  // (:88-89)
        T[3 + r][6] = dt * wx, T[3 + r][7] = dt * wy, T[3 + r][8] = 0.0;               // (:94)
        tb[r] = get(bp, r) - dt * dt / 2 * get(Rg, r);                                 // (:90)
        tb[3 + r] = get(dv, r) - dt * get(Rg, r);                                      // (:95)
      }
      sys_add<3>(L.acc, T, tb, on, i, lane);
      sys_scale_copy(L.acc, L.wrk, 1000.0, lane);
      wave_lds_sync();
      ok = sys_solve(L, nv, 3, lane);
      if (!ok) break;
      const double d0 = L.x[nv], d1 = L.x[nv + 1];
      g0 = Gn * normalized3(g0 + d0 * lx + d1 * ly);  // (:118-119)
      ok = finite3(g0);
    }
    if (ok) {
      s = L.x[nv + 2] / 100.0;  // (:190-191)
      ok = isfinite(s) && !(s < 0.0);
      g = g0;
    }
    // (a window that fails in here returns no x: the linear solve's velocities above are taken back)
    for (int r = lane; r < nv; r += 64) xo[r] = ok ? L.x[r] : 0.0;
  }
  if (lane == 0) {
    xo[3 * MF] = ok ? s : 0.0;
    A.out.g_c0[b * 3] = ok ? g.x : 0.0, A.out.g_c0[b * 3 + 1] = ok ? g.y : 0.0, A.out.g_c0[b * 3 + 2] = ok ? g.z : 0.0;
    A.out.ok[b] = ok ? 1 : 0;
    if (A.has_windows) A.out.g_world[b * 3] = 0.0, A.out.g_world[b * 3 + 1] = 0.0, A.out.g_world[b * 3 + 2] = 0.0;  // (align_apply_kernel writes it for ok windows)
  }
}

// ---- the change of state (estimator.cpp:367-426) ---------------------------------------------------------------------------------
// first half: Ps / Rs from the key frames (:368-375), every depth to -1 (:377-380); triangulate_kernel follows with a zero tic (:383-388)
__global__ __launch_bounds__(64) void align_prepare_kernel(AlignArgs A) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (!A.out.ok[b]) return;
  const int MF = A.a.max_frames;
  if (lane < NFR) {
    const int k = A.a.key_index[(size_t)b * NFR + lane];
    const double* R = A.a.frame_R + ((size_t)b * MF + k) * 9;
    const double* T = A.a.frame_T + ((size_t)b * MF + k) * 3;
    double* pose = A.w.pose + ((size_t)b * NFR + lane) * 7;
    const quat q = R2q(R);
    pose[0] = T[0], pose[1] = T[1], pose[2] = T[2], pose[3] = q.x, pose[4] = q.y, pose[5] = q.z, pose[6] = q.w;
  }
  const int nf = clampi(A.w.n_feat[b], 0, A.w.max_feat);
  for (int e = lane; e < nf; e += 64) A.w.inv_depth[(size_t)b * A.w.max_feat + e] = -1.0;
}

// second half (:390-426)
__global__ __launch_bounds__(64) void align_apply_kernel(AlignArgs A) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (!A.out.ok[b]) return;
  const int MF = A.a.max_frames;
  const int* key = A.a.key_index + (size_t)b * NFR;
  const double* xo = A.out.x + (size_t)b * (3 * MF + 1);
  const double s = xo[3 * MF];  // (:390)
  const v3 g = ld3(A.out.g_c0 + b * 3);
  const v3 tic = ld3(A.w.ex_pose + (size_t)b * 7);
  const double* R0k = A.a.frame_R + ((size_t)b * MF + key[0]) * 9;
  const v3 P0k = ld3(A.a.frame_T + ((size_t)b * MF + key[0]) * 3);
  // R0 = g2R(g) (utility.cpp:3-13): FromTwoVectors(g / |g|, e_z), then the yaw of R0 removed
  double R0[9];
  {
    const v3 v0 = normalized3(g);
    const double c = v0.z;  // v1 . v0, v1 = (0, 0, 1)
    quat q;
    if (c < -1.0 + 1e-12) {
      // antipodal (Eigen takes an SVD there): any unit axis perpendicular to g will do - avm.h
      const v3 ax = fabs(v0.x) < 0.9 ? normalized3(cross(v0, mk3(1, 0, 0))) : normalized3(cross(v0, mk3(0, 1, 0)));
      const double w2 = (1.0 + c) * 0.5;
      const double sv = sqrt(1.0 - w2);
      q = quat{sqrt(w2), sv * ax.x, sv * ax.y, sv * ax.z};
    } else {
      const v3 ax = cross(v0, mk3(0, 0, 1));
      const double sq = sqrt((1.0 + c) * 2.0), inv = 1.0 / sq;
      q = quat{sq * 0.5, ax.x * inv, ax.y * inv, ax.z * inv};
    }
    double Rq[9], Rz[9];
    q2R(q, Rq);
    // R2ypr(R).x() in degrees and ypr2R{-yaw, 0, 0} (utility.h:66-108)
    const double yaw = atan2(Rq[3], Rq[0]) / M_PI * 180.0;
    const double y = -yaw / 180.0 * M_PI;
    Rz[0] = cos(y), Rz[1] = -sin(y), Rz[2] = 0, Rz[3] = sin(y), Rz[4] = cos(y), Rz[5] = 0, Rz[6] = 0, Rz[7] = 0, Rz[8] = 1;
    double Ra[9], Rb[9];
    mat3mul(Rz, Rq, Ra);
    // yaw of R0 * Rs[0] removed (:416-417)
    mat3mul(Ra, R0k, Rb);
    const double yaw2 = atan2(Rb[3], Rb[0]) / M_PI * 180.0;
    const double y2 = -yaw2 / 180.0 * M_PI;
    Rz[0] = cos(y2), Rz[1] = -sin(y2), Rz[3] = sin(y2), Rz[4] = cos(y2);
    mat3mul(Rz, Ra, R0);
  }
  if (lane < NFR) {
    const int k = key[lane];
    const double* Rk = A.a.frame_R + ((size_t)b * MF + k) * 9;
    const v3 Pk = ld3(A.a.frame_T + ((size_t)b * MF + k) * 3);
    // Ps[i] = s Ps[i] - Rs[i] TIC - (s Ps[0] - Rs[0] TIC), every frame against the ORIGINAL Ps[0] (:395-396)
    const v3 P = (s * Pk - Rmul(Rk, tic)) - (s * P0k - Rmul(R0k, tic));
    // Vs[kv] = R_key(kv) x.segment<3>(kv * 3): x is indexed by the key-frame COUNTER, not by the frame's position (:397-406)
    const v3 V = Rmul(Rk, ld3(xo + 3 * lane));
    const v3 Pw = Rmul(R0, P), Vw = Rmul(R0, V);  // (:421-426)
    double Rw[9];
    mat3mul(R0, Rk, Rw);
    const quat q = R2q(Rw);
    double* pose = A.w.pose + ((size_t)b * NFR + lane) * 7;
    double* sb = A.w.speedbias + ((size_t)b * NFR + lane) * 9;
    pose[0] = Pw.x, pose[1] = Pw.y, pose[2] = Pw.z, pose[3] = q.x, pose[4] = q.y, pose[5] = q.z, pose[6] = q.w;
    sb[0] = Vw.x, sb[1] = Vw.y, sb[2] = Vw.z;
  }
  if (lane == 0) {
    const v3 gw = Rmul(R0, g);  // (:418)
    A.out.g_world[b * 3] = gw.x, A.out.g_world[b * 3 + 1] = gw.y, A.out.g_world[b * 3 + 2] = gw.z;
  }
  // estimated_depth *= s (:407-413)
  const int nf = clampi(A.w.n_feat[b], 0, A.w.max_feat);
  for (int e = lane; e < nf; e += 64) {
    double* lam = A.w.inv_depth + (size_t)b * A.w.max_feat + e;
    *lam = 1.0 / ((1.0 / *lam) * s);
  }
}

hipError_t launch_align_gyro_bias(const AlignArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(align_gyro_bias_kernel, dim3(a.a.n_windows), dim3(64), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_align_solve(const AlignArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(align_solve_kernel, dim3(a.a.n_windows), dim3(64), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_align_prepare(const AlignArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(align_prepare_kernel, dim3(a.a.n_windows), dim3(64), 0, stream, a);
  return hipGetLastError();
}
hipError_t launch_align_apply(const AlignArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(align_apply_kernel, dim3(a.a.n_windows), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace avm
