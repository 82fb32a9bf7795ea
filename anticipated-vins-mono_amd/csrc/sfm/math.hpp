// sfm/math.hpp - the scalar pieces of the global SfM: quaternions and 3 x 3 blocks as plain arrays, Rodrigues both ways, the 4 x 4
// triangulation, the small Cholesky.  Everything here is __host__ __device__ and uses no wave primitive, so that the same text also
// compiles for the host (tests/host_cpp_init: one "thread" per stream).  Formulas follow the statement tests/golden/gen_global_sfm.py.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>

#ifndef SFM_HD
#define SFM_HD __host__ __device__ inline
#endif

namespace avm {
namespace sfm {

constexpr int NK = 11;       // key frames of the window
constexpr int NCAM = 57;     // camera unknowns of the BA: 11 x 6 less rotation l, translations l and 10
constexpr int LDS_S = 65;    // row stride of the 64 x 64 reduced camera system (row 57: the right-hand side rides along)

SFM_HD bool fin(double v) { return v - v == 0.0; }
SFM_HD double f32r(double v) { return (double)(float)v; }

// ---- quaternions (w x y z) and rotations (row-major 9) ----
SFM_HD void qmul4(const double* a, const double* b, double* o) {
  const double w = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], x = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  const double y = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], z = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
  o[0] = w, o[1] = x, o[2] = y, o[3] = z;
}
SFM_HD void qinv4(const double* q, double* o) {  // Eigen inverse(): conjugate / squaredNorm
  const double n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  o[0] = q[0] / n2, o[1] = -q[1] / n2, o[2] = -q[2] / n2, o[3] = -q[3] / n2;
}
SFM_HD void q2R9(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * (y * y + z * z), R[1] = 2 * (x * y - z * w), R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w), R[4] = 1 - 2 * (x * x + z * z), R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w), R[7] = 2 * (y * z + x * w), R[8] = 1 - 2 * (x * x + y * y);
}
SFM_HD void R2q4(const double* R, double* q) {  // Eigen::Quaterniond(Matrix3d)
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = sqrt(t + 1);
    q[0] = t / 2;
    t = 1 / (2 * t);
    q[1] = (R[7] - R[5]) * t, q[2] = (R[2] - R[6]) * t, q[3] = (R[3] - R[1]) * t;
    return;
  }
  int i = 0;
  if (R[4] > R[0]) i = 1;
  if (R[8] > R[i * 4]) i = 2;
  const int j = (i + 1) % 3, k = (i + 2) % 3;
  t = sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1);
  q[1 + i] = t / 2;
  t = 1 / (2 * t);
  q[0] = (R[k * 3 + j] - R[j * 3 + k]) * t;
  q[1 + j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
  q[1 + k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
}
SFM_HD void mul33(const double* A, const double* B, double* C) {
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
SFM_HD void mulv(const double* R, const double* v, double* o) {
  const double a = R[0] * v[0] + R[1] * v[1] + R[2] * v[2], b = R[3] * v[0] + R[4] * v[1] + R[5] * v[2], c = R[6] * v[0] + R[7] * v[1] + R[8] * v[2];
  o[0] = a, o[1] = b, o[2] = c;
}
SFM_HD void cross3(const double* a, const double* b, double* o) {
  const double x = a[1] * b[2] - a[2] * b[1], y = a[2] * b[0] - a[0] * b[2], z = a[0] * b[1] - a[1] * b[0];
  o[0] = x, o[1] = y, o[2] = z;
}
SFM_HD void qrot3(const double* q, const double* v, double* o) {  // Eigen q * v
  double uv[3], w[3];
  cross3(q + 1, v, uv);
  for (int i = 0; i < 3; i++) uv[i] = 2 * uv[i];
  cross3(q + 1, uv, w);
  for (int i = 0; i < 3; i++) o[i] = v[i] + q[0] * uv[i] + w[i];
}
SFM_HD void skew33(const double* v, double* S) {
  S[0] = 0, S[1] = -v[2], S[2] = v[1], S[3] = v[2], S[4] = 0, S[5] = -v[0], S[6] = -v[1], S[7] = v[0], S[8] = 0;
}
// QuaternionParameterization::Plus: [cos|d|, sin|d| / |d| d] * q
SFM_HD void quat_plus(const double* q, const double* d, double* o) {
  const double n = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
  if (n > 0) {
    const double s = sin(n) / n;
    const double e[4] = {cos(n), s * d[0], s * d[1], s * d[2]};
    qmul4(e, q, o);
  } else {
    for (int i = 0; i < 4; i++) o[i] = q[i];
  }
}

// ---- cvRodrigues2, matrix -> vector, without its SVD: false at theta = pi (the call then fails) ----
SFM_HD bool rodrigues_vec(const double* R, double* r) {
  const double rx = R[7] - R[5], ry = R[2] - R[6], rz = R[3] - R[1];
  const double s = sqrt((rx * rx + ry * ry + rz * rz) / 4);
  double c = (R[0] + R[4] + R[8] - 1) / 2;
  c = c > 1 ? 1 : c < -1 ? -1 : c;
  if (!(s > 1e-5)) {
    r[0] = r[1] = r[2] = 0;
    return c > 0;
  }
  const double vth = 1 / (2 * s) * acos(c);
  r[0] = rx * vth, r[1] = ry * vth, r[2] = rz * vth;
  return true;
}
// R(r) and, with dR, d R / d r_i = (r_i [r]x + [r x (I - R) e_i]x) / theta^2 R  (dR: 3 matrices of 9)
SFM_HD void rodrigues_mat(const double* r, double* R, double* dR) {
  const double th2 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2], th = sqrt(th2);
  if (th < DBL_EPSILON) {
    for (int i = 0; i < 9; i++) R[i] = (i % 4 == 0) ? 1.0 : 0.0;
    if (dR)
      for (int i = 0; i < 3; i++) {
        const double e[3] = {i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0};
        skew33(e, dR + 9 * i);
      }
    return;
  }
  const double c = cos(th), s = sin(th);
  const double k[3] = {r[0] / th, r[1] / th, r[2] / th};
  double K[9];
  skew33(k, K);
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) R[i * 3 + j] = (i == j ? c : 0.0) + k[i] * k[j] * (1 - c) + K[i * 3 + j] * s;
  if (!dR) return;
  double rx[9];
  skew33(r, rx);
  for (int i = 0; i < 3; i++) {
    const double col[3] = {(i == 0 ? 1.0 : 0.0) - R[i], (i == 1 ? 1.0 : 0.0) - R[3 + i], (i == 2 ? 1.0 : 0.0) - R[6 + i]};
    double v[3], V[9], M[9];
    cross3(r, col, v);
    skew33(v, V);
    for (int e = 0; e < 9; e++) M[e] = (rx[e] * r[i] + V[e]) / th2;
    mul33(M, R, dR + 9 * i);
  }
}

// ---- GlobalSFM::triangulatePoint: the last right singular vector of the 4 x 4 design matrix by the one-sided Jacobi of
// triangulate.hip; P0, P1: 3 x 4 row-major poses [R | t] ----
SFM_HD void triangulate_point(const double* P0, const double* P1, double u0, double v0, double u1, double v1, double* X) {
  double A[4][4];  // A[column][row]
  for (int b = 0; b < 4; b++) {
    A[b][0] = u0 * P0[8 + b] - P0[b], A[b][1] = v0 * P0[8 + b] - P0[4 + b];
    A[b][2] = u1 * P1[8 + b] - P1[b], A[b][3] = v1 * P1[8 + b] - P1[4 + b];
  }
  double V[4][4] = {{1, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 0, 0, 1}};
  for (int sweep = 0; sweep < 60; sweep++) {
    bool rotated = false;
    for (int p = 0; p < 3; p++)
      for (int q = p + 1; q < 4; q++) {
        double app = 0, aqq = 0, apq = 0;
        for (int i = 0; i < 4; i++) app += A[p][i] * A[p][i], aqq += A[q][i] * A[q][i], apq += A[p][i] * A[q][i];
        if (!(fabs(apq) > 1e-300) || fabs(apq) <= 2.3e-16 * sqrt(app * aqq)) continue;  // (a NaN product ends the sweeps)
        rotated = true;
        const double tau = (aqq - app) / (2.0 * apq);
        const double tn = (tau >= 0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
        const double c = 1.0 / sqrt(1.0 + tn * tn), s = tn * c;
        for (int i = 0; i < 4; i++) {
          const double x = A[p][i], y = A[q][i];
          A[p][i] = c * x - s * y, A[q][i] = s * x + c * y;
        }
        for (int i = 0; i < 4; i++) {
          const double x = V[i][p], y = V[i][q];
          V[i][p] = c * x - s * y, V[i][q] = s * x + c * y;
        }
      }
    if (!rotated) break;
  }
  int best = 0;
  double bn = 0;
  for (int j = 0; j < 4; j++) {
    double s = 0;
    for (int i = 0; i < 4; i++) s += A[j][i] * A[j][i];
    if (j == 0 || s < bn) bn = s, best = j;
  }
  for (int i = 0; i < 3; i++) X[i] = V[i][best] / V[3][best];
}

// A x = b, A symmetric positive definite N x N (row-major, lower triangle read), by Cholesky; false if a pivot is not positive
template <int N>
SFM_HD bool cholesky_solve(const double* A, const double* b, double* x) {
  double L[N * N], y[N];
  for (int j = 0; j < N; j++) {
    double d = A[j * N + j];
    for (int k = 0; k < j; k++) d -= L[j * N + k] * L[j * N + k];
    if (!(d > 0)) return false;
    L[j * N + j] = sqrt(d);
    for (int i = j + 1; i < N; i++) {
      double s = A[i * N + j];
      for (int k = 0; k < j; k++) s -= L[i * N + k] * L[j * N + k];
      L[i * N + j] = s / L[j * N + j];
    }
  }
  for (int i = 0; i < N; i++) {
    double s = b[i];
    for (int k = 0; k < i; k++) s -= L[i * N + k] * y[k];
    y[i] = s / L[i * N + i];
  }
  for (int i = N - 1; i >= 0; i--) {
    double s = y[i];
    for (int k = i + 1; k < N; k++) s -= L[k * N + i] * x[k];
    x[i] = s / L[i * N + i];
  }
  return true;
}

// inverse of a symmetric 3 x 3 by cofactors; M, Vi: 00 01 02 11 12 22
SFM_HD void inv3sym(const double* M, double* Vi) {
  const double a = M[0], b = M[1], c = M[2], d = M[3], e = M[4], f = M[5];
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = a * c00 + b * c01 + c * c02;
  const double c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
  Vi[0] = c00 / det, Vi[1] = c01 / det, Vi[2] = c02 / det, Vi[3] = c11 / det, Vi[4] = c12 / det, Vi[5] = c22 / det;
}
SFM_HD void sym3mulv(const double* S, const double* v, double* o) {
  const double a = S[0] * v[0] + S[1] * v[1] + S[2] * v[2], b = S[1] * v[0] + S[3] * v[1] + S[4] * v[2], c = S[2] * v[0] + S[4] * v[1] + S[5] * v[2];
  o[0] = a, o[1] = b, o[2] = c;
}

}  // namespace sfm
}  // namespace avm
