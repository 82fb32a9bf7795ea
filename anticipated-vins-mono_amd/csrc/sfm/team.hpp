// sfm/team.hpp - the two teams of the global SfM on the device: a 256-thread workgroup (the chain and the BA) and one wavefront (a
// non-key frame's PnP).  Reductions are the butterfly wave_sum / wave_max of devmath.hpp, then the four wavefronts' values in index order:
// fixed orders, the result in every thread.
#pragma once
#include "../devmath.hpp"
#include "chain.hpp"

namespace avm {
namespace sfm {

struct Block256 {
  static constexpr int NT = 256;
  double* red;  // LDS, 4 * 28 doubles
  d4 acc[4];    // row tile (wavefront) x 4 column tiles of the 64 x 64 product of the chunks
  __device__ int tid() const { return threadIdx.x; }
  __device__ void sync() { __syncthreads(); }
  template <int N>
  __device__ void sum(double* v) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = wave_sum(v[i]);
    __syncthreads();
    if (lane == 0)
#pragma unroll
      for (int i = 0; i < N; i++) red[wv * N + i] = v[i];
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = ((red[i] + red[N + i]) + red[2 * N + i]) + red[3 * N + i];
  }
  __device__ double max1(double v) { return block_max<NT>(v, red); }
  __device__ void schur_zero() {
#pragma unroll
    for (int t = 0; t < 4; t++) acc[t] = d4{0, 0, 0, 0};
  }
  // acc += Y W^T over the chunk's 48 columns: v_mfma_f64_16x16x4, A[i][k] = Y[16 wv + i][k], B[k][j] = W[16 t + j][k]
  __device__ void schur_chunk(const double* Y, const double* W) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int k0 = 0; k0 < 3 * CHUNK; k0 += 4) {
      const double a = Y[(16 * wv + li) * LDW + k0 + lk];
#pragma unroll
      for (int t = 0; t < 4; t++) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, W[(16 * t + li) * LDW + k0 + lk], acc[t], 0, 0, 0);
    }
  }
  // S -= acc; the accumulator's (lane, register r) is row (lane >> 4) + 4 r, column lane & 15 of its tile
  __device__ void schur_store(double* S) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int t = 0; t < 4; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) S[(16 * wv + lk + 4 * r) * LDS_S + 16 * t + li] -= acc[t][r];
  }
};

struct Wave64 {
  static constexpr int NT = 64;
  __device__ int tid() const { return threadIdx.x; }
  __device__ void sync() { wave_lds_sync(); }
  template <int N>
  __device__ void sum(double* v) {
#pragma unroll
    for (int i = 0; i < N; i++) v[i] = wave_sum(v[i]);
  }
  __device__ double max1(double v) { return wave_max(v); }
};

}  // namespace sfm
}  // namespace avm
