// devmath.hpp — device-side FP64 helpers for the gfx950 kernels (wave = 64 lanes): quaternions and 3 x 3 blocks, then the wave
// primitives every kernel shares, one definition each - lane exchange (dpp_mov, dpp_d, dpp_keep_d, readlane_d, lane_xor, lane_swap), the
// wave / block reductions, and wave_lds_sync, sfor, d4, fast_rcp / fast_rsqrt.
// Quaternion/rotation conventions follow vins_estimator/src/utility/utility.h:12-64 and the
// Eigen behaviours listed in SURVEY.md Appendix B (storage order in parameter blocks: x,y,z,w).
#pragma once
#include <hip/hip_runtime.h>
#include <utility>

#define AVM_DEV __device__ __forceinline__

namespace avm {

struct v3 {
  double x, y, z;
};
AVM_DEV v3 mk3(double x, double y, double z) { return v3{x, y, z}; }
AVM_DEV v3 operator+(v3 a, v3 b) { return v3{a.x + b.x, a.y + b.y, a.z + b.z}; }
AVM_DEV v3 operator-(v3 a, v3 b) { return v3{a.x - b.x, a.y - b.y, a.z - b.z}; }
AVM_DEV v3 operator-(v3 a) { return v3{-a.x, -a.y, -a.z}; }
AVM_DEV v3 operator*(double s, v3 a) { return v3{s * a.x, s * a.y, s * a.z}; }
AVM_DEV double dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
AVM_DEV v3 cross(v3 a, v3 b) { return v3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
AVM_DEV double get(v3 a, int i) { return i == 0 ? a.x : (i == 1 ? a.y : a.z); }

struct quat {  // w,x,y,z
  double w, x, y, z;
};
AVM_DEV quat qmul(quat a, quat b) {
  return quat{a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z, a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y,
              a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z, a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x};
}
AVM_DEV quat qinv(quat q) {  // Eigen inverse(): conjugate / squaredNorm
  double n2 = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
  return quat{q.w / n2, -q.x / n2, -q.y / n2, -q.z / n2};
}
AVM_DEV quat qnormalized(quat q) {
  double n = sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  return quat{q.w / n, q.x / n, q.y / n, q.z / n};
}
AVM_DEV quat deltaQ(v3 th) { return quat{1.0, th.x / 2.0, th.y / 2.0, th.z / 2.0}; }  // utility.h:12-24
AVM_DEV v3 qrot(quat q, v3 v) {  // Eigen q*v
  v3 qv = mk3(q.x, q.y, q.z);
  v3 uv = cross(qv, v);
  uv = uv + uv;
  return v + q.w * uv + cross(qv, uv);
}
// Eigen toRotationMatrix (no normalization); R row-major 9
AVM_DEV void q2R(quat q, double* R) {
  const double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z;
  const double twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
  const double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x;
  const double tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
  R[0] = 1 - (tyy + tzz), R[1] = txy - twz, R[2] = txz + twy;
  R[3] = txy + twz, R[4] = 1 - (txx + tzz), R[5] = tyz - twx;
  R[6] = txz - twy, R[7] = tyz + twx, R[8] = 1 - (txx + tyy);
}
// Eigen Quaterniond(Matrix3d)
AVM_DEV quat R2q(const double* R) {
  quat q;
  double t = R[0] + R[4] + R[8];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q.w = 0.5 * t;
    t = 0.5 / t;
    q.x = (R[7] - R[5]) * t;
    q.y = (R[2] - R[6]) * t;
    q.z = (R[3] - R[1]) * t;
  } else {
    int i = 0;
    if (R[4] > R[0]) i = 1;
    if (R[8] > R[i * 4]) i = 2;
    int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(R[i * 4] - R[j * 4] - R[k * 4] + 1.0);
    double v[3];
    v[i] = 0.5 * t;
    t = 0.5 / t;
    q.w = (R[k * 3 + j] - R[j * 3 + k]) * t;
    v[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    v[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    q.x = v[0], q.y = v[1], q.z = v[2];
  }
  return q;
}
AVM_DEV v3 Rmul(const double* R, v3 v) {
  return v3{R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z, R[6] * v.x + R[7] * v.y + R[8] * v.z};
}
AVM_DEV v3 RTmul(const double* R, v3 v) {
  return v3{R[0] * v.x + R[3] * v.y + R[6] * v.z, R[1] * v.x + R[4] * v.y + R[7] * v.z, R[2] * v.x + R[5] * v.y + R[8] * v.z};
}
AVM_DEV void skew9(v3 q, double* S) {
  S[0] = 0, S[1] = -q.z, S[2] = q.y;
  S[3] = q.z, S[4] = 0, S[5] = -q.x;
  S[6] = -q.y, S[7] = q.x, S[8] = 0;
}
AVM_DEV void mat3mul(const double* A, const double* B, double* C) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
}
// bottom-right 3x3 of Qleft(q) (utility.h:46-54): w*I + skew(v)
AVM_DEV void qleft_br(quat q, double* M) {
  M[0] = q.w, M[1] = -q.z, M[2] = q.y;
  M[3] = q.z, M[4] = q.w, M[5] = -q.x;
  M[6] = -q.y, M[7] = q.x, M[8] = q.w;
}
// bottom-right 3x3 of Qleft(a)*Qright(b): rows 1..3 of Qleft(a) times cols 1..3 of Qright(b)
AVM_DEV void qleft_qright_br(quat a, quat b, double* M) {
  // Qleft(a) rows 1..3 = [a.v | a.w I + skew(a.v)] ; Qright(b) cols 1..3 = [-b.v^T ; b.w I - skew(b.v)]
  double La[9], Rb[9];
  qleft_br(a, La);
  Rb[0] = b.w, Rb[1] = b.z, Rb[2] = -b.y;
  Rb[3] = -b.z, Rb[4] = b.w, Rb[5] = b.x;
  Rb[6] = b.y, Rb[7] = -b.x, Rb[8] = b.w;
  double av[3] = {a.x, a.y, a.z}, bv[3] = {b.x, b.y, b.z};
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      M[i * 3 + j] = av[i] * (-bv[j]) + La[i * 3] * Rb[j] + La[i * 3 + 1] * Rb[3 + j] + La[i * 3 + 2] * Rb[6 + j];
}

// ---- lane exchange with the pattern as an immediate --------------------------------------------------------------------------------
// __shfl_xor is a ds_bpermute_b32 per 32 bits with the partner's byte address in a VGPR: the compiler keeps the six address registers
// of a ladder live across the whole kernel, and in the solve kernels it spills them - every step of a reduction then began with a trip
// to scratch memory.  The forms below carry the pattern in the instruction (DPP controls, the gfx950 row / half swaps): no address
// register, no LDS pipe.  All of them are compiler builtins, so the hazard recognizer places the DPP wait states.
template <int CTRL, int ROW_MASK = 0xf>
AVM_DEV int dpp_mov(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, ROW_MASK, 0xf, true); }
// A double through one DPP control (two 32-bit moves), bound_ctrl and the full bank mask: a lane without a source, or in a row that
// ROW_MASK leaves out, gets 0 - what a sum wants, and no "old value" register has to be set up in front of every move.
template <int CTRL, int ROW_MASK = 0xf>
AVM_DEV double dpp_d(double v) {
  return __hiloint2double(dpp_mov<CTRL, ROW_MASK>(__double2hiint(v)), dpp_mov<CTRL, ROW_MASK>(__double2loint(v)));
}
// ... the keep-old-value form: such a lane keeps its own v (what a maximum wants: fmax(v, v) = v)
template <int CTRL, int ROW_MASK = 0xf>
AVM_DEV double dpp_keep_d(double v) {
  const int hi = __double2hiint(v), lo = __double2loint(v);
  return __hiloint2double(__builtin_amdgcn_update_dpp(hi, hi, CTRL, ROW_MASK, 0xf, false), __builtin_amdgcn_update_dpp(lo, lo, CTRL, ROW_MASK, 0xf, false));
}
// one lane's double to the whole wavefront through SGPRs (two v_readlane_b32)
AVM_DEV double readlane_d(double v, int srclane) {  // srclane must be wave-uniform
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_readlane(lo, srclane);
  hi = __builtin_amdgcn_readlane(hi, srclane);
  return __hiloint2double(hi, lo);
}
// the value of lane (lane ^ O), O = 1, 2, 4, 8 (inside the 16-lane rows); every lane of the wavefront active
template <int O>
AVM_DEV int lane_xor(int v) {
  static_assert(O == 1 || O == 2 || O == 4 || O == 8, "inside a DPP row");
  if constexpr (O == 1) return dpp_mov<0xB1>(v);   // quad_perm [1,0,3,2]
  if constexpr (O == 2) return dpp_mov<0x4E>(v);   // quad_perm [2,3,0,1]
  if constexpr (O == 4) return dpp_mov<0x1B>(dpp_mov<0x141>(v));  // row_half_mirror (lane ^ 7), then quad_perm [3,2,1,0] (lane ^ 3)
  return dpp_mov<0x128>(v);                        // row_ror:8
}
template <int O>
AVM_DEV double lane_xor(double v) {
  return __hiloint2double(lane_xor<O>(__double2hiint(v)), lane_xor<O>(__double2loint(v)));
}
// Steps 32 and 16 of a butterfly whose operation commutes: v_permlane32_swap / v_permlane16_swap of v with itself leave v's lower
// (even-row) copy in one register and its upper (odd-row) copy in the other, in both halves (rows of the pair) - op(a, b) is then
// op(v[lane], v[lane ^ O]) in the lower lanes and op(v[lane ^ O], v[lane]) in the upper ones: the same value for + and fmax.
struct dpair {
  double a, b;
};
template <int O>
AVM_DEV dpair lane_swap(double v) {
  static_assert(O == 16 || O == 32, "row or half swap");
  const unsigned lo = __double2loint(v), hi = __double2hiint(v);
  if constexpr (O == 32) {
    const auto l = __builtin_amdgcn_permlane32_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return dpair{__hiloint2double(h[0], l[0]), __hiloint2double(h[1], l[1])};
  } else {
    const auto l = __builtin_amdgcn_permlane16_swap(lo, lo, false, false), h = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return dpair{__hiloint2double(h[0], l[0]), __hiloint2double(h[1], l[1])};
  }
}

// ---- wave / block reductions (fixed order => deterministic) ---------------------------
// Two ladders, two summation orders: which one a kernel uses is part of its bit-exact result.
// The butterfly of a __shfl_xor ladder: partner lane ^ o, o = 32, 16, 8, 4, 2, 1 in that order; the result in every lane.
AVM_DEV double wave_sum(double v) {
  dpair p = lane_swap<32>(v);
  v = p.a + p.b;
  p = lane_swap<16>(v);
  v = p.a + p.b;
  v += lane_xor<8>(v);
  v += lane_xor<4>(v);
  v += lane_xor<2>(v);
  v += lane_xor<1>(v);
  return v;
}
AVM_DEV double wave_max(double v) {  // the same butterfly; the result in every lane
  dpair p = lane_swap<32>(v);
  v = fmax(p.a, p.b);
  p = lane_swap<16>(v);
  v = fmax(p.a, p.b);
  v = fmax(v, lane_xor<8>(v));
  v = fmax(v, lane_xor<4>(v));
  v = fmax(v, lane_xor<2>(v));
  v = fmax(v, lane_xor<1>(v));
  return v;
}
// The shift ladder (prior_eig.hip): lane i takes lane i - 1, - 2, - 4, - 8 of its 16-lane row in that order (lane 15 then holds its row:
// ((15 + 14) + (13 + 12)) + ... ), then row 0 goes to row 1 and row 2 to row 3, then row 1 to rows 2 and 3; lane 63 holds the wavefront
// and is read through SGPRs: the result is uniform.  No LDS.
AVM_DEV double wave_sum_shr(double v) {
  v += dpp_d<0x111>(v);       // row_shr:1
  v += dpp_d<0x112>(v);       // row_shr:2
  v += dpp_d<0x114>(v);       // row_shr:4
  v += dpp_d<0x118>(v);       // row_shr:8   -> lane 15 of every row holds the row sum
  v += dpp_d<0x142, 0xa>(v);  // row_bcast:15 -> rows 1 and 3
  v += dpp_d<0x143, 0xc>(v);  // row_bcast:31 -> rows 2 and 3: lane 63 holds the sum
  return readlane_d(v, 63);
}
AVM_DEV double wave_max_shr(double v) {  // the same ladder (any pairing will do for a maximum); the result uniform
  v = fmax(v, dpp_keep_d<0x111>(v));
  v = fmax(v, dpp_keep_d<0x112>(v));
  v = fmax(v, dpp_keep_d<0x114>(v));
  v = fmax(v, dpp_keep_d<0x118>(v));
  v = fmax(v, dpp_keep_d<0x142, 0xa>(v));
  v = fmax(v, dpp_keep_d<0x143, 0xc>(v));
  return readlane_d(v, 63);
}
// all threads get the result; red must hold >= 32 doubles; contains 2 __syncthreads
template <int NT>
AVM_DEV double block_sum(double v, double* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double s = 0;
#pragma unroll
  for (int i = 0; i < NT / 64; i++) s += red[i];
  return s;
}
template <int NT>
AVM_DEV double block_max(double v, double* red) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  v = wave_max(v);
  __syncthreads();
  if (lane == 0) red[wv] = v;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < NT / 64; i++) s = fmax(s, red[i]);
  return s;
}

// ---- what else every kernel shares: the wave-level LDS fence, the compile-time loop, d4, rcp / rsqrt ----------------------------------
// a wavefront's own LDS traffic put in order (its stores before the barrier visible to its loads after it); no other wavefront is waited for
AVM_DEV void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// compile-time loop, f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>): a register tile's index and the lane index of a
// DPP operand have to be constants (the one is part of the instruction, the other keeps the tile array out of scratch memory)
template <class F, int... Is>
AVM_DEV void sfor_impl(F&& f, std::integer_sequence<int, Is...>) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
AVM_DEV void sfor(F&& f) {
  sfor_impl(f, std::make_integer_sequence<int, N>{});
}

typedef double d4 __attribute__((ext_vector_type(4)));  // the accumulator of v_mfma_f64_16x16x4

// reciprocal / reciprocal square root from the hardware estimate + two Newton steps (about one ulp; the library forms spend
// two to three times as long on range handling that the operands here - depths, squared norms >= 1 - never need)
AVM_DEV double fast_rcp(double x) {
  double y = __builtin_amdgcn_rcp(x), e = fma(-x, y, 1.0);
  y = fma(y, e, y);
  e = fma(-x, y, 1.0);
  return fma(y, e, y);
}
// raw v_rsq_f64 + two Newton steps (the library rsqrt spends ~3x as long in range handling we do not need:
// pivots of an SPD matrix are normal positive numbers)
AVM_DEV double fast_rsqrt(double x) {
  double y = __builtin_amdgcn_rsq(x);
  y = y * (1.5 - (0.5 * x) * y * y);
  y = y * (1.5 - (0.5 * x) * y * y);
  return y;
}

}  // namespace avm
