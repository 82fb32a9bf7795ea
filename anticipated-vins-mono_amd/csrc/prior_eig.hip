// prior_eig.hip — second half of the marginalization (MarginalizationInfo::marginalize(),
// vins_estimator/src/factor/marginalization_factor.cpp:283-301): the symmetric eigen-decomposition of the
// reduced information matrix A' = Arr - Arm Amm^+ Amr and the "square-root" prior
//     linearized_jacobians = diag(sqrt(S))   V^T ,   linearized_residuals = diag(1/sqrt(S)) V^T b' ,
// with S the eigenvalues clamped to 0 below eps (marginalization_factor.cpp:292-299).
//
// marginalize_kernel (solve/marg_kernel.hpp) leaves A' (lower triangle is read) in PO.J[w] and b' in PO.r[w]; this
// kernel overwrites both in place.  One 256-thread workgroup per window, 48 KB of LDS: three workgroups share a CU.
//
// Method (Veselic-Hari / Drmac): A' = G G^T by a diagonally pivoted Cholesky factorization, then ONE-SIDED Jacobi on
// the columns of G.  Right rotations leave G G^T alone; once the columns g_i are orthogonal,
//     A' = sum_i g_i g_i^T  =>  S_i = |g_i|^2 ,  v_i = g_i / |g_i| ,
// so the rows of the prior Jacobian are the columns themselves, sqrt(S_i) v_i^T = g_i^T, and the residual entry is
// g_i^T b' / S_i: no eigenvector matrix is accumulated, nothing is normalised.  The implicit matrix G^T G (= L^T L, one
// LR step ahead of A' = L L^T) is much closer to diagonal than A', so the sweeps are fewer than for two-sided Jacobi
// on A' (6-7 instead of 10-11), and a rotation touches two columns instead of two rows + two columns + two columns of V.
//
//  * Cholesky: in LDS on the full symmetric [76][76] array, no physical swaps - step j picks the largest remaining
//    diagonal p_j, its scaled column overwrites the (dead) row p_j, eliminated indices are masked.  The factorization
//    stops when the largest remaining pivot is below n eps_machine max diag (rank-revealing: A' is only semi-definite
//    when the window has no gauge-fixing prior yet); the remaining columns are zero.  Which column sits where does not
//    matter to the Jacobi phase, so "column q" is simply row q of the array.
//  * Jacobi: odd-even (Brent-Luk) ordering in POSITION space.  Lane k of every wavefront holds the columns on
//    positions 2k (X) and 2k+1 (Y), wavefront w their rows 19 w .. 19 w + 18, all in registers.  An even step rotates
//    the pairs (2k, 2k+1) lane-locally and swaps their positions; for an odd step the Y columns move one lane up with
//    DPP wave shifts so that the pairs (2k-1, 2k) are lane-local too, and move back afterwards.  Per step each
//    wavefront contributes the partial dot product of its rows to a double-buffered LDS table (ONE barrier per step),
//    every wavefront sums the four partials in the same order and computes the same rotation - no rotation tables, no
//    convergence flags to exchange.  Squared norms ride along with the columns and are refreshed every sweep.
//  * The rotation angle only steers convergence, so it uses the hardware rcp / sqrt approximations; (c, s) themselves
//    are normalised to full precision.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include "devmath.hpp"
#include "kernels.hpp"

namespace avm {
namespace pe {

constexpr int NT = 256;
constexpr int NW = NT / 64;
constexpr int NMAX = MAXKEEP;         // 76: padded (even) dimension limit; kept sets of this problem have n <= 75
constexpr int NPMAX = NMAX / 2;       // 38 column pairs
constexpr int LD = NMAX;
constexpr int RW = NMAX / NW;         // 19 rows of every column per wavefront
static_assert(RW * NW == NMAX, "rows split evenly over the wavefronts");

// LDS carve (doubles)
constexpr int P_A = 0;                        // A' -> rows = columns of G
constexpr int PL = 40;                        // lanes that hold columns (np <= 38, + the boundary lane of the odd steps)
constexpr int P_PART = P_A + NMAX * LD;       // [2 buffers][2 values][NW][PL] partial dot products
constexpr int P_B = P_PART + 2 * 2 * NW * PL;
constexpr int P_DG = P_B + NMAX;              // running diagonal of the Cholesky factorization
constexpr int P_PIV = P_DG + NMAX;            // pivot sequence of the Cholesky factorization (ints), then 4 doubles of verdicts
constexpr int P_D0 = P_PIV + NMAX / 2 + 4;     // the diagonal of A' as it came in (the scale of each variable, for the clamp's noise test)
constexpr int P_END = P_D0 + NMAX;
static_assert(3 * P_END * 8 <= 163840, "three workgroups per CU");

// Wavefront shifts with bound_ctrl: a lane without a source gets 0 - exactly what the column exchange wants (the lanes
// beyond the last pair hold zero columns), and no "old value" register has to be set up in front of every DPP move.
AVM_DEV double shl_d(double v) { return dpp_d<0x130>(v); }  // wave_shl:1, lane i <- lane i+1 (the last lane gets 0)
AVM_DEV double shr_d(double v) { return dpp_d<0x138>(v); }  // wave_shr:1, lane i <- lane i-1 (lane 0 gets 0)
// (the reductions of both kernels are devmath.hpp's shift ladder, wave_sum_shr / wave_max_shr: result uniform, no LDS)

// ---- the well-conditioned case on ONE wavefront (round 3) ------------------------------------------------------------------------
// Most windows of a run - every window whose prior already pins all its directions - leave an A' that is positive definite with
// lambda_min ~ 1e2: no eigenvalue anywhere near the clamp, and ANY square root J^T J = A' with r0 = J^-T b' is the prior
// (marginalization_factor.cpp:283-301 only ever hands J and r0 to consumers that see J^T J, J^T r0 and |r0|^2, see below).  For those
// windows prior_eig_kernel's four cooperating wavefronts, two barriers per pivot and rank-revealing pivot search are the wrong tool:
// it is latency bound at ~4 K cycles per pivot (0.88 ms per 4096 windows).  Here one wavefront takes one window, the matrix lives in
// its registers as 16 x 16 tiles in the accumulator layout of v_mfma_f64_16x16x4 and never goes back to memory:
//   * A' is held as its UPPER tiles U[k][i] (k <= i): register r of lane (lk = lane / 16, lr = lane % 16) is entry (lk + 4 r, lr) of
//     the tile.  With the k index of a product running as lk + 4 r, a tile in this layout IS a B operand and, read as an A operand, its
//     transpose - so (like the selector's evaluation on the 4 x 4 x 4 form) nothing is transposed or moved between lanes:
//   * block column k:  L_kk from the diagonal tile (through a 2 KB LDS patch into lane = row form: a 16-pivot chain of v_readlane
//     broadcasts, with the rows of the identity riding along in lanes 16..31 and ending as L_kk^-T, the scheme of chol_diag_block in
//     solve/cholesky_lds.hpp);  W_i = L_kk^-1 U[k][i] (A operand = L_kk^-1 from LDS, B = the tile);  U[j][i] -= W_j^T W_i (both operands
//     straight from registers).  W_i = L_ik^T is block (k, i) of J = L^T: the factor is the output.
//   * r0 = L^-1 b' by blocks (tile^T x vector products reduced over the four row groups, the diagonal solves through L_kk^-1).
//   * certification with the EXPLICIT inverse (120 more MFMAs, column block by column block, only its norms are kept):
//     lambda_min(A') >= 1 / |L^-1|_F^2 for the eps clamp (factor 1000 to spare) and lambda_min of the row-scaled form >= 1 / |L^-1 diag(s)^1/2|_F^2
//     for the noise test of the eigen path (see the clamp below) - sqrt(n) pessimistic at worst, where the comparison-matrix bound of
//     the pivoted path is 40 - 3400 x.
//   * EXACT ZEROS of A' (ragged tracks: two thirds of the windows have two to four directions nothing constrains).  In natural order
//     such a direction shows up as ONE pivot that is zero up to the noise it was formed with, |p_j| <= pc_zero(s_j, s_j) (s_j: the
//     magnitude the diagonal entry was formed at, from marginalize_kernel).  The pivot is DELETED: column j of L is set to
//     zero (row j of J, entry j of r0 - exactly what the eigen path and the pivoted path do with a direction under the clamp), the
//     factorization continues, the inverse norms above are those of the kept part (row / column j of every L_kk^-1 are zero).  What
//     that drops is checked afterwards, row by row: |A'[j][c] - (J^T J)[j][c]| <= pc_zero(s_j, s_c) for every c - the deleted row
//     of the remainder is formation noise, not a small genuine direction (whose column would not be small: |a_jc| <= sqrt(p_j a_cc)
//     only).  A pivot between noise and genuine stays, makes |L^-1| huge and fails the certification.
// A window that fails any of it - a negative or non-finite pivot, more than PC_MAXDEL deleted pivots (no prior yet), a deleted row
// that is not noise, a bound that does not clear the thresholds - is left untouched (done[w] = 0) and taken by prior_eig_kernel.
constexpr int PC_T = 5;                                 // tiles per dimension: n <= 80
constexpr int PC_NT = PC_T * (PC_T + 1) / 2;            // 15 upper tiles
constexpr int PC_S = 17, PC_B = 16 * PC_S;                // row stride / size of a 16 x 16 block in LDS (round 6: at stride 16 the lane = row accesses put sixteen lanes on two banks -
                                                          // SQ_LDS_BANK_CONFLICT was 11 cycles per LDS instruction of this kernel)
constexpr int PC_LDS = PC_B + PC_T * PC_B + 6 * 80 + PC_B; // doubles: the diagonal patch | L_kk^-1 of every block | b', y, s, a 16-vector, a column of J, the pivots' thresholds | a 16 x 16 identity
constexpr int PC_MAXDEL = 8;                            // deleted pivots per window
__device__ __forceinline__ constexpr int pc_ti(int k, int i) { return k * PC_T - k * (k - 1) / 2 + (i - k); }
// what counts as zero for entry (i, j) of A' given the magnitudes s_i, s_j its two diagonal entries were formed at: 4000 unit roundoffs of
// sqrt(s_i s_j) - plain formation noise - or, for the small magnitudes, 1e-7 (s_i s_j)^1/4: the level the eigen path's own noise test
// works at (it drops S when S^2 <= 1e-16 g^T diag(s) g, i.e. S <= 1e-8 sqrt(s) for a coordinate direction; a factor 10 on top because
// the noise of a pivot that follows a small genuine pivot is amplified by their ratio - measured: 5e-6 at s = 3e4 behind a pivot of 0.05)
// (noise_rel = avm_options::marg_noise_rel: the constants were measured at 1e-16 and scale with its square root - a tenth of them at the
//  default of round 5, 1e-18; 0 switches the test off)
// The level the two Cholesky forms of the square root (prior_chol_kernel, the rank-r form of prior_eig_kernel) certify the noise test at.  The
// eigen form tests S^2 > noise_rel v^T diag(s) v with the caller's constant (default 1e-18 since round 5: never drop a genuine direction).  A
// direction between that and the level rounding noise was MEASURED at (1e-16: the constants of pc_zero) may be formation noise that happens to
// pass; kept, it puts v (v^T b') into J^T r0 with a v that is itself noise, and two forms that see different roundings of the same zeros would hand
// out priors with different gradients (g_scaled 5e-3 between the forms on windows without a prior).  So a Cholesky form is only handed
// out when every kept direction clears the MEASURED noise level; a window with a direction in the band between the two goes to the eigen form, which
// alone decides about it - which form finishes a window no longer changes the prior beyond rounding.
__device__ __forceinline__ double pc_cert_noise(double noise_rel) { return noise_rel > 0.0 ? fmax(noise_rel, 1e-16) : 0.0; }
__device__ __forceinline__ double pc_zero(double si, double sj, double noise_rel) {
  const double g = sqrt(si * sj), f = sqrt(noise_rel * 1e16);
  return f * fmax(1e-12 * g, 1e-7 * sqrt(g));
}
#ifndef AVM_PC_WAVES
#define AVM_PC_WAVES 2
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(AVM_PC_WAVES, AVM_PC_WAVES))) void prior_chol_kernel(avm_prior_out PO, int n_windows, double eps, double noise_rel, const double* scale, int* done) {
  __shared__ double pc_lds[PC_LDS];
  const int w = blockIdx.x, lane = threadIdx.x, lk = lane >> 4, lr = lane & 15;
  if (w >= n_windows) return;
  if (lane == 0) done[w] = 0;
  const int n = PO.n[w];
  if (n < 3 || n > 16 * PC_T) return;
  double* gJ = PO.J + (size_t)w * PO.max_prior * PO.max_prior;
  double* gr = PO.r + (size_t)w * PO.max_prior;
  const int ldj = PO.max_prior;
  double* blk = pc_lds;                 // [16][16]
  double* Linv = pc_lds + PC_B;         // [PC_T][16][PC_S]: L_kk^-1, row-major
  double* vb = Linv + PC_T * PC_B;      // b' (80)
  double* vy = vb + 80;                 // y = L^-1 b' (80)
  double* vs = vy + 80;                 // s: the magnitude every diagonal entry was formed at (marginalize_kernel), 0 on the pad
  double* vt = vs + 80;                 // a 16-vector in transit
  double* vc = vt + 80;                 // column j of J (the check of a deleted pivot)
  double* vthr = vc + 80;               // pc_zero(s_j, s_j): what counts as a zero pivot (three square roots each: once per window, not once per block)
  double* ident = vthr + 80;            // [16][16] identity: the rows the lanes 16..31 of the pivot chain start from
  // ---- load: upper tiles (A' is symmetric and stored as its lower triangle), identity on the pad
  d4 U[PC_NT];
  {
    // (entry (row, col) of an upper tile lies at [col][row] of the stored lower triangle; off the diagonal tiles row < col also after
    //  the clamp to n - 1, so one product per tile column and one add per entry address it: written with max / min of the two clamped
    //  indices the 60 loads cost 800 instructions)
    size_t cb[PC_T];
    bool cin[PC_T];
#pragma unroll
    for (int i = 0; i < PC_T; i++) cb[i] = (size_t)min(16 * i + lr, n - 1) * ldj, cin[i] = 16 * i + lr < n;
#pragma unroll
    for (int k = 0; k < PC_T; k++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int rc = min(16 * k + lk + 4 * r, n - 1);
#pragma unroll
        for (int i = k; i < PC_T; i++) {
          if (i == k) {
            const int cc = min(16 * i + lr, n - 1);
            U[pc_ti(k, i)][r] = gJ[(size_t)max(rc, cc) * ldj + min(rc, cc)];
          } else {
            U[pc_ti(k, i)][r] = gJ[cb[i] + rc];
          }
        }
      }
    // all sixty loads are out before the first is looked at.  (Left as `in ? load : pad` the selects became branches around the loads -
    // CodeGenPrepare sinks a load that only a select uses -, each with its own wait: sixty trips to memory one after the other.)
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < PC_T; k++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = 16 * k + lk + 4 * r;
        const bool rin = row < n;
#pragma unroll
        for (int i = k; i < PC_T; i++) {
          double v = U[pc_ti(k, i)][r];
          asm volatile("" : "+v"(v));
          U[pc_ti(k, i)][r] = (rin && cin[i]) ? v : (row == 16 * i + lr ? 1.0 : 0.0);
        }
      }
  }
  {
    // (b' and s: loads first, selects afterwards, as above)
    const int c0 = lane, c1 = lane + 64;
    double b0 = gr[min(c0, n - 1)], s0 = scale[(size_t)w * ldj + min(c0, n - 1)];
    double b1 = gr[min(c1, n - 1)], s1 = scale[(size_t)w * ldj + min(c1, n - 1)];
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" : "+v"(b0), "+v"(s0), "+v"(b1), "+v"(s1));
    s0 = c0 < n ? s0 : 0.0, s1 = c1 < n ? s1 : 0.0;
    vb[c0] = c0 < n ? b0 : 0.0, vs[c0] = s0, vthr[c0] = pc_zero(s0, s0, noise_rel);
    if (c1 < 80) vb[c1] = c1 < n ? b1 : 0.0, vs[c1] = s1, vthr[c1] = pc_zero(s1, s1, noise_rel);
#pragma unroll
    for (int q = 0; q < 4; q++) ident[((lane + 64 * q) >> 4) * PC_S + ((lane + 64 * q) & 15)] = ((lane + 64 * q) >> 4) == ((lane + 64 * q) & 15) ? 1.0 : 0.0;
  }
  wave_lds_sync();
  bool bad = false;
  unsigned long long dm0 = 0, dm1 = 0;  // the deleted pivots, a bit each (wave-uniform; no branch inside the pivot chain)
  // ---- factorization
#pragma unroll
  for (int k = 0; k < PC_T; k++) {
#pragma unroll
    for (int r = 0; r < 4; r++) blk[(lk + 4 * r) * PC_S + lr] = U[pc_ti(k, k)][r];
    wave_lds_sync();
    {
      // lane = row (lanes 0..15), lanes 16..31: the rows of the identity (they end as the rows of L_kk^-T); the others carry junk
      // (lanes 32..63 repeat lanes 0..31 - same loads, same arithmetic, same stores -, so that no store below is conditional)
      double a[16];
      const bool idl = (lane & 16) != 0;
      const double* src = idl ? ident + lr * PC_S : blk + lr * PC_S;  // (the diagonal tile is symmetric: its row lr)
#pragma unroll
      for (int c = 0; c < 16; c++) a[c] = src[c];
      const double thr_l = vthr[16 * k + lr];  // (off the pivot chain: lane j holds pivot j's threshold)
#pragma unroll
      for (int j = 0; j < 16; j++) {
        const double pj = readlane_d(a[j], j);
        const double thr = readlane_d(thr_l, j);
        const bool del = fabs(pj) <= thr;  // zero up to formation noise: the direction is dropped (pads: s = 0, pivot 1)
        a[j] *= del ? 0.0 : fast_rsqrt(pj);
#pragma unroll
        for (int c = j + 1; c < 16; c++) a[c] = fma(-a[j], readlane_d(a[j], c), a[c]);
      }
      wave_lds_sync();  // (every lane has read its row of the patch)
      // Row lr of L_kk goes back into the patch as COLUMN lr (the patch then holds L_kk^T = J_kk), row i of L_kk^-T (lane 16 + i) as column
      // i of L_kk^-1: both with stride 16, sixteen unconditional stores at constant offsets.  The entries c > lr of a matrix lane are
      // leftovers of the elimination, masked where the patch is read; those c < i of an identity lane are exact zeros already.
      double* dst = idl ? Linv + k * PC_B + lr : blk + lr;
#pragma unroll
      for (int c = 0; c < 16; c++) dst[c * PC_S] = a[c];
    }
    wave_lds_sync();
    {
      // What became of the sixteen pivots, read off L_kk's diagonal (in the chain this bookkeeping was twelve scalar instructions per pivot
      // on values the compiler then kept in spilled SGPRs: 2 K of the kernel's 12.8 K instructions): a deleted pivot left an exact zero
      // (a[j] *= 0), a negative or non-finite one a NaN (rsqrt), one beyond 1e300 a diagonal beyond 1e150
      const double dj = blk[lr * (PC_S + 1)];  // L_kk[lr][lr]
      bad |= !(dj == 0.0 || (dj > 0.0 && dj < 1e150));
      const unsigned long long delm = __ballot(dj == 0.0) & 0xffffull;
      if (k < 4) dm0 |= delm << (16 * k);
      else dm1 |= delm;
    }
    // J_kk = L_kk^T in the tile layout: entry (row, col) = L[col][row], zero below the diagonal
#pragma unroll
    for (int r = 0; r < 4; r++) U[pc_ti(k, k)][r] = lk + 4 * r <= lr ? blk[(lk + 4 * r) * PC_S + lr] : 0.0;
    if (k + 1 < PC_T) {
      double ao[4];  // A operand L_kk^-1[i' = lr][k' = lk + 4 r]
#pragma unroll
      for (int r = 0; r < 4; r++) ao[r] = Linv[k * PC_B + lr * PC_S + lk + 4 * r];
#pragma unroll
      for (int i = k + 1; i < PC_T; i++) {
        d4 W = {0, 0, 0, 0};
#pragma unroll
        for (int r = 0; r < 4; r++) W = __builtin_amdgcn_mfma_f64_16x16x4f64(ao[r], U[pc_ti(k, i)][r], W, 0, 0, 0);
        U[pc_ti(k, i)] = W;  // = L_ik^T = block (k, i) of J
      }
#pragma unroll
      for (int j = k + 1; j < PC_T; j++)
#pragma unroll
        for (int i = j; i < PC_T; i++)
#pragma unroll
          for (int r = 0; r < 4; r++)
            U[pc_ti(j, i)] = __builtin_amdgcn_mfma_f64_16x16x4f64(-U[pc_ti(k, j)][r], U[pc_ti(k, i)][r], U[pc_ti(j, i)], 0, 0, 0);
    }
    wave_lds_sync();  // (the patch is rewritten by the next block column)
  }
  // ---- y = L^-1 b' by blocks: v_k = b_k - sum_{i < k} L_ki y_i with L_ki = (J block (i, k))^T, then y_k = L_kk^-1 v_k
#pragma unroll
  for (int k = 0; k < PC_T; k++) {
    double p = 0.0;
#pragma unroll
    for (int i = 0; i < k; i++)
#pragma unroll
      for (int r = 0; r < 4; r++) p = fma(U[pc_ti(i, k)][r], vy[16 * i + lk + 4 * r], p);
    p += __shfl_xor(p, 16, 64);
    p += __shfl_xor(p, 32, 64);
    if (lk == 0) vt[lr] = vb[16 * k + lr] - p;
    wave_lds_sync();
    double acc = 0.0;
#pragma unroll
    for (int q = 0; q < 16; q++) acc = fma(Linv[k * PC_B + lr * PC_S + q], vt[q], acc);
    if (lk == 0) vy[16 * k + lr] = acc;
    wave_lds_sync();
  }
  // ---- |L^-1|_F^2 and |L^-1 diag(s)^1/2|_F^2 from the explicit inverse, one column block at a time
  double f2 = 0.0, fs2 = 0.0;
#pragma unroll
  for (int kk = 0; kk < PC_T; kk++) {
    d4 X[PC_T];  // X[i] = (L^-1) block (i, kk), i >= kk
    const double sc = vs[16 * kk + lr];
    const bool cin = 16 * kk + lr < n;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      X[kk][r] = Linv[kk * PC_B + (lk + 4 * r) * PC_S + lr];
      const double e2 = (cin && 16 * kk + lk + 4 * r < n) ? X[kk][r] * X[kk][r] : 0.0;
      f2 += e2, fs2 = fma(e2, sc, fs2);
    }
#pragma unroll
    for (int i = kk + 1; i < PC_T; i++) {
      d4 Sacc = {0, 0, 0, 0};
#pragma unroll
      for (int j = kk; j < i; j++)
#pragma unroll
        for (int r = 0; r < 4; r++) Sacc = __builtin_amdgcn_mfma_f64_16x16x4f64(U[pc_ti(j, i)][r], X[j][r], Sacc, 0, 0, 0);  // L_ij X_j
      d4 Xi = {0, 0, 0, 0};
#pragma unroll
      for (int r = 0; r < 4; r++) Xi = __builtin_amdgcn_mfma_f64_16x16x4f64(-Linv[i * PC_B + lr * PC_S + lk + 4 * r], Sacc[r], Xi, 0, 0, 0);
      X[i] = Xi;
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const double e2 = (cin && 16 * i + lk + 4 * r < n) ? Xi[r] * Xi[r] : 0.0;
        f2 += e2, fs2 = fma(e2, sc, fs2);
      }
    }
  }
  f2 = wave_sum_shr(f2), fs2 = wave_sum_shr(fs2);
  const int ndel = __popcll(dm0) + __popcll(dm1);
  // (the noise test is certified at PC_CERT_NOISE, not at noise_rel: see pc_cert_noise)
  bool ok = !__any(bad) && ndel <= PC_MAXDEL && f2 * (1000.0 * eps) < 1.0 && fs2 * (4.0 * pc_cert_noise(noise_rel)) < 1.0;  // (NaN compares false)
  if (!ok) return;
  // ---- the deleted pivots: row d of A' - J^T J has to be formation noise
  for (int q = 0; q < ndel; q++) {
    int d;
    if (dm0) d = __builtin_ctzll(dm0), dm0 &= dm0 - 1;
    else d = 64 + __builtin_ctzll(dm1), dm1 &= dm1 - 1;
    d = __builtin_amdgcn_readfirstlane(d);
    const int kd = d >> 4, cd = d & 15;
    // column d of J into LDS: J[row][d], rows < d (row d itself is zero, the rows below are below the diagonal)
    for (int c = lane; c < 80; c += 64) vc[c] = 0.0;
    wave_lds_sync();
#pragma unroll
    for (int k = 0; k < PC_T; k++)
      if (k <= kd && lr == cd) {
#pragma unroll
        for (int i = k; i < PC_T; i++)
          if (i == kd) {
#pragma unroll
            for (int r = 0; r < 4; r++) vc[16 * k + lk + 4 * r] = U[pc_ti(k, i)][r];
          }
      }
    wave_lds_sync();
    const double sd = vs[d];
    bool viol = false;
#pragma unroll
    for (int i = 0; i < PC_T; i++) {
      double pacc = 0.0;
#pragma unroll
      for (int k = 0; k <= i; k++)
#pragma unroll
        for (int r = 0; r < 4; r++) pacc = fma(U[pc_ti(k, i)][r], vc[16 * k + lk + 4 * r], pacc);
      pacc += __shfl_xor(pacc, 16, 64);
      pacc += __shfl_xor(pacc, 32, 64);
      const int c = 16 * i + lr;
      if (c < n) {
        const double orig = gJ[(size_t)max(d, c) * ldj + min(d, c)];
        viol |= !(fabs(orig - pacc) <= pc_zero(sd, vs[c], noise_rel));
      }
    }
    ok = ok && !__any(viol);
    wave_lds_sync();
  }
  if (!ok) return;
  // ---- the prior: linearized_jacobians = J = L^T (upper triangular), linearized_residuals = y
  // (one row base per register row; the tiles a window of n >= 64 variables covers entirely - sixteen of the twenty-five - are stored without
  //  a bounds test: a predicated store is a branch of its own)
  {
    const bool full4 = n >= 64;  // (uniform)
#pragma unroll
    for (int k = 0; k < PC_T; k++)
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int row = 16 * k + lk + 4 * r;
        double* rb = gJ + (size_t)min(row, n - 1) * ldj + lr;
        const bool rin = row < n;
#pragma unroll
        for (int i = 0; i < PC_T; i++) {
          const double v = i >= k ? U[pc_ti(min(k, i), max(k, i))][r] : 0.0;
          if (k < 4 && i < 4 && full4) rb[16 * i] = v;
          else if (rin && 16 * i + lr < n) rb[16 * i] = v;
        }
      }
  }
  for (int c = lane; c < n; c += 64) gr[c] = vy[c];
  if (lane == 0) done[w] = 1;
}

// `literal` != 0 forces the eigen-decomposition even where the Cholesky factor would do (AVM_PRIOR_LITERAL=1 / AVM_PRIOR_FORCE_EIG=1)
__global__ __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(3, 3))) void prior_eig_kernel(avm_prior_out PO, int n_windows, double eps, double noise_rel, const double* scale, long long* prof, int literal, const int* done) {
  extern __shared__ char pe_smem[];
  double* lds = reinterpret_cast<double*>(pe_smem);
  double* A = lds + P_A;
  const int t = threadIdx.x, wv = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;  // wv: provably uniform
  const int w = blockIdx.x;
  if (w >= n_windows) return;
  if (done && done[w]) return;     // prior_chol_kernel has written this window's prior (a well-conditioned A')
  const int n = PO.n[w];
  if (n <= 0 || n > NMAX) return;  // n == -1: MARGIN_SECOND_NEW had nothing to drop (the caller keeps the old prior)
  const long long t_start = prof ? (long long)__builtin_readcyclecounter() : 0;
  const int ne = (n + 1) & ~1, np = ne >> 1;
  double* gJ = PO.J + (size_t)w * PO.max_prior * PO.max_prior;
  double* gr = PO.r + (size_t)w * PO.max_prior;
  const int ldj = PO.max_prior;

  // ---- load: A' into REGISTERS (thread = columns lane, lane + 64; rows wv, wv + 4, ...), its diagonal and b' into LDS,
  // the array that will hold G zeroed (the columns of indices that are never eliminated stay zero)
  const int col0 = lane, col1 = lane + 64;  // col1 only exists on lanes < NMAX - 64
  double R0[RW], R1[RW];
#pragma unroll
  for (int q = 0; q < RW; q++) {
    const int i = wv + NW * q, ic = min(i, n - 1), c0c = min(col0, n - 1), c1c = min(col1, n - 1);
    R0[q] = gJ[(size_t)max(ic, c0c) * ldj + min(ic, c0c)];
    R1[q] = gJ[(size_t)max(ic, c1c) * ldj + min(ic, c1c)];
  }
  double* dgl = lds + P_DG;
  for (int e = t; e < NMAX * NMAX; e += NT) A[e] = 0.0;
  if (t < NMAX) lds[P_B + t] = t < n ? gr[t] : 0.0;
  double dmine = t < n ? gJ[(size_t)t * ldj + t] : 0.0;  // threads 0..75 carry the running diagonal
  // (the scale every diagonal entry was formed at: marginalize_kernel leaves it in the ctx's scale array)
  if (t < NMAX) dgl[t] = dmine, lds[P_D0 + t] = t < n ? scale[(size_t)w * ldj + t] : 0.0;
#pragma unroll
  for (int q = 0; q < RW; q++) {
    const int i = wv + NW * q;
    R0[q] = (i < n && col0 < n) ? R0[q] : 0.0;
    R1[q] = (i < n && col1 < n) ? R1[q] : 0.0;
  }
  __syncthreads();

  // ---- diagonally pivoted Cholesky.  A' stays in registers; per step only the scaled pivot row (= column of G, stored as
  // row p of the LDS array) and the running diagonal go through LDS.  The set of eliminated indices is a uniform bit mask
  // that every thread tracks (pad indices start eliminated).
  unsigned long long done_lo = n >= 64 ? 0ull : ~0ull << n, done_hi = n >= 64 ? ~0ull << (n - 64) : ~0ull;
  double dmax0 = 0.0;
  int* piv = reinterpret_cast<int*>(lds + P_PIV);
  int rank = 0;
  for (int j = 0; j < n; j++) {
    // every wavefront finds the same pivot: largest remaining diagonal (lowest index among those equal in all but the
    // last 7 mantissa bits, which carry the index through the reduction)
    double key = 0.0;
    {
      const double v0 = dgl[col0], v1 = dgl[min(col1, NMAX - 1)];
      if (!((done_lo >> lane) & 1ull) && v0 > 0.0)
        key = __longlong_as_double((__double_as_longlong(v0) & ~0x7fll) | (long long)(127 - col0));
      if (col1 < NMAX && !((done_hi >> lane) & 1ull) && v1 > 0.0)
        key = fmax(key, __longlong_as_double((__double_as_longlong(v1) & ~0x7fll) | (long long)(127 - col1)));
    }
    key = wave_max_shr(key);
    if (!(key > 0.0)) break;
    const int p = 127 - (int)(__double_as_longlong(key) & 0x7fll);
    const double bv = dgl[p];
    if (j == 0) dmax0 = bv;
    if (!(bv > (double)NMAX * 2.3e-16 * dmax0)) break;  // rank reached (uniform: every lane has the same pivot)
    const double isq = fast_rsqrt(bv);
    double* g = A + p * LD;
    if (wv == (p & (NW - 1))) {  // the wavefront that owns row p publishes g = row p / sqrt(pivot), 0 on eliminated columns
      const int qp = p >> 2;
      double r0 = 0, r1 = 0;
#pragma unroll
      for (int q = 0; q < RW; q++)
        if (q == qp) r0 = R0[q], r1 = R1[q];  // (uniform)
      g[col0] = col0 == p ? bv * isq : (((done_lo >> lane) & 1ull) ? 0.0 : r0 * isq);
      if (col1 < NMAX) g[col1] = col1 == p ? bv * isq : (((done_hi >> lane) & 1ull) ? 0.0 : r1 * isq);
    }
    if (p < 64) done_lo |= 1ull << p; else done_hi |= 1ull << (p - 64);
    if (t == 0) piv[j] = p;
    rank = j + 1;
    __syncthreads();
    // A <- A - g g^T.  Eliminated rows / columns have g = 0; row and column p are left alone (g_p is zeroed for the update)
    {
      const double g0 = col0 == p ? 0.0 : g[col0], g1 = (col1 < NMAX && col1 != p) ? g[col1] : 0.0;
      double gi[RW];
#pragma unroll
      for (int q = 0; q < RW; q++) gi[q] = g[wv + NW * q];
      if (t < NMAX) {
        const double gt = g[t];
        dmine = fma(-gt, gt, dmine);
        dgl[t] = dmine;
      }
#pragma unroll
      for (int q = 0; q < RW; q++) {
        const double gq = (wv + NW * q == p) ? 0.0 : gi[q];
        R0[q] = fma(-gq, g0, R0[q]);
        R1[q] = fma(-gq, g1, R1[q]);
      }
    }
    __syncthreads();
  }
  __syncthreads();

  // ---- The prior is a SQUARE ROOT of A' (marginalization_factor.cpp:283-301): linearized_jacobians = diag(sqrt S) V^T,
  // linearized_residuals = diag(1 / sqrt S) V^T b'.  Every consumer - MarginalizationFactor::Evaluate in the next solve and in
  // the next marginalization - sees it only as a residual block r0 + J dx without a loss function, i.e. through J^T J = A',
  // J^T r0 = b' and |r0|^2 = b'^T A'^-1 b'; any J' = Q J, r0' = Q r0 with Q orthogonal is the same prior.  When NO eigenvalue
  // is clamped (lambda_min(A') > eps), the transposed Cholesky factor is such a pair: J = G^T (rows = the columns g_p in pivot
  // order), r0 = G^-1 b' - and it is already here.  The eigen-decomposition (7-8 Jacobi sweeps, ~10x the cost of everything
  // above) is only needed when an eigenvalue may fall under the clamp.  That is decided rigorously and with a wide margin:
  //   full rank reached, and  lambda_min(A') = 1 / |G^-1|_2^2 >= 1 / (|G^-1|_1 |G^-1|_inf) > 1000 eps,
  // the two norms bounded from above by one triangular solve each with the comparison matrix M(G) (|diagonal|, -|off-diagonal|):
  // |G^-1| e <= M(G)^-1 e elementwise (Higham, Accuracy and Stability of Numerical Algorithms, section 8.2).  Typical windows with a
  // prior have lambda_min ~ 1e2 against the 1e-5 asked for.  Wavefront 0 solves for r0, wavefronts 1 and 2 for the two bounds.
  //
  // RANK-DEFICIENT A' (round 3).  When the factorization stopped at rank r < n - the window has directions nothing constrains
  // (exact zeros of A': with ragged tracks two thirds of the windows have two or four of them, tests/test_prior_truth.py) - the
  // same holds for the n x r factor G_r = [L11; L21] (pivot rows first): A' = G_r G_r^T up to the dropped remainder, which
  // the eigen path drops as well (its input IS this factor), J = G_r^T with n - r zero rows is a square root of the clamped
  // matrix, r0 = L11^-1 b'_pivots the matching residual, and no eigenvalue of the kept part is near the clamp when
  //   lambda_min+(G_r G_r^T) = sigma_min(G_r)^2 >= sigma_min(L11)^2 = 1 / |L11^-1|_2^2 > threshold,
  // bounded through the comparison matrix of L11 as before.  The threshold covers the eps clamp and the noise test of the
  // eigen path (below): max(1000 eps, 1e-16 max_i s_i).
  double* verdict = lds + P_PIV + NMAX / 2;
  // (with the reference-literal clamp, marg_noise_rel = 0, only the FULL-rank factor is the same prior: the rank-r form drops the
  //  remainder, which the literal eigen form keeps wherever FP64 leaves it above eps)
  if (!literal && rank >= 1 && (rank == n || noise_rel > 0.0)) {
    const int nr = rank;
    // entries of G in pivot order: G[p_j][i] = g_{p_i}[p_j] = A[p_i * LD + p_j], zero for i > j (p_j was eliminated before p_i)
    {
      const int i0 = lane, i1 = lane + 64;  // this lane's share of the dot products: pivots i0 and i1
      const int pi0 = piv[min(i0, nr - 1)], pi1 = piv[min(i1, nr - 1)];
      double y0 = 0.0, y1 = 0.0;  // solution entries of pivots i0, i1 (kept by their lanes)
      if (wv != 2) {
        // forward: y_j = (rhs_j -+ sum_{i < j} G[p_j][i] y_i) / G[p_j][j]
        //   wave 0: real entries, rhs = b'                               -> r0
        //   wave 1: comparison matrix, rhs = 1                           -> |L11^-1|_inf
        //   wave 3: comparison matrix of the ROW-SCALED factor diag(s)^-1/2 L11, i.e. rhs = sqrt(s_pj) -> |(diag(s)^-1/2 L11)^-1|_inf
        for (int j = 0; j < nr; j++) {
          const int pj = piv[j];
          const double a0 = i0 < j ? A[pi0 * LD + pj] : 0.0, a1 = i1 < j ? A[pi1 * LD + pj] : 0.0;
          const double sacc = wv == 0 ? wave_sum_shr(a0 * y0 + a1 * y1) : wave_sum_shr(fabs(a0) * y0 + fabs(a1) * y1);
          const double d = A[pj * LD + pj];
          const double rhs = wv == 1 ? 1.0 : sqrt(lds[P_D0 + pj]);
          const double yj = wv == 0 ? (lds[P_B + pj] - sacc) / d : (rhs + sacc) / fabs(d);
          y0 = i0 == j ? yj : y0, y1 = i1 == j ? yj : y1;
        }
        if (wv == 0) {
          if (i0 < n) gr[i0] = y0;  // (zero beyond the rank: the rows of J there are zero)
          if (i1 < n) gr[i1] = y1;
        } else {
          const double m = wave_max_shr(fmax(i0 < nr ? y0 : 0.0, i1 < nr ? y1 : 0.0));
          if (lane == 0) verdict[wv == 1 ? 0 : 2] = m;
        }
      } else {
        // backward with the transposed comparison matrix: w_j = (1 + sum_{i > j} |G[p_i][j]| w_i) / |G[p_j][j]|, G[p_i][j] = A[p_j * LD + p_i]
        for (int j = nr - 1; j >= 0; j--) {
          const int pj = piv[j];
          const double a0 = (i0 > j && i0 < nr) ? fabs(A[pj * LD + pi0]) : 0.0, a1 = (i1 > j && i1 < nr) ? fabs(A[pj * LD + pi1]) : 0.0;
          const double sacc = wave_sum_shr(a0 * y0 + a1 * y1);
          const double yj = (1.0 + sacc) / fabs(A[pj * LD + pj]);
          y0 = i0 == j ? yj : y0, y1 = i1 == j ? yj : y1;
        }
        const double m = wave_max_shr(fmax(i0 < nr ? y0 : 0.0, i1 < nr ? y1 : 0.0));  // >= |L11^-T|_inf = |L11^-1|_1
        // (the transposed solve of the row-scaled factor is this one with its solution weighted by sqrt(s_p))
        const double ms = wave_max_shr(fmax(i0 < nr ? y0 * sqrt(lds[P_D0 + pi0]) : 0.0, i1 < nr ? y1 * sqrt(lds[P_D0 + pi1]) : 0.0));
        if (lane == 0) verdict[1] = m, verdict[3] = ms;
      }
    }
    __syncthreads();
    // 1 / (v0 v1) <= lambda_min+(A'): the eps clamp does not act on the kept part (factor 1000 to spare).
    // 1 / (v2 v3) <= lambda_min of B = diag(s)^-1/2 L11 L11^T diag(s)^-1/2, and every eigenpair (S, v) of the kept part has
    // S / v^T diag(s) v >= lambda_min(B): the noise test of the eigen path (S > 1e-16 v^T diag(s) v) passes for all of them.  The
    // comparison-matrix bound is rigorous but 40 - 3400 x pessimistic, and the variables formed by cancellation (gyroscope bias:
    // 1e2 left of 5e14) put lambda_min(B) at 1e-13 .. 1e-10, so this test gets a factor 4, not 1000.
    if (verdict[0] * verdict[1] * (1000.0 * eps) < 1.0 && verdict[2] * verdict[3] * (4.0 * pc_cert_noise(noise_rel)) < 1.0) {  // (NaN compares false; pc_cert_noise: below)
      // linearized_jacobians: row j = g_{p_j}^T, zero rows beyond the rank
      for (int e = t; e < n * n; e += NT) {
        const int j = e / n, c = e - j * n;
        gJ[(size_t)j * ldj + c] = j < nr ? A[piv[min(j, nr - 1)] * LD + c] : 0.0;
      }
      if (prof && t == 0) atomicAdd(reinterpret_cast<unsigned long long*>(prof + 25), (unsigned long long)((long long)__builtin_readcyclecounter() - t_start));
      return;
    }
    __syncthreads();  // (wave 0 has overwritten b'-independent outputs only: gr is rewritten below, lds[P_B] is intact)
  }

  // ---- one-sided Jacobi on the columns of G.  Lane k: X = column on position 2k, Y = column on position 2k+1.
  double X[RW], Y[RW];
  const int r0 = wv * RW;
  {
    const int k = min(lane, NPMAX - 1);
#pragma unroll
    for (int r = 0; r < RW; r++) {
      const double x = A[(2 * k) * LD + r0 + r], y = A[(2 * k + 1) * LD + r0 + r];
      X[r] = lane < np ? x : 0.0, Y[r] = lane < np ? y : 0.0;
    }
  }
  double* part = lds + P_PART;
  int buf = 0;
  double nX = 0, nY = 0;
  // sum over the wavefronts of (v0, v1), the same order everywhere
  auto reduce2 = [&](double& v0, double& v1) {
    double* pb = part + buf * (2 * NW * PL);
    const int ll = min(lane, PL - 1);
    if (lane < PL) pb[wv * PL + lane] = v0, pb[(NW + wv) * PL + lane] = v1;
    __syncthreads();
    double s0 = 0, s1 = 0;
#pragma unroll
    for (int q = 0; q < NW; q++) s0 += pb[q * PL + ll], s1 += pb[(NW + q) * PL + ll];
    v0 = s0, v1 = s1;
    buf ^= 1;
  };
  auto reduce1 = [&](double v) {
    double* pb = part + buf * (2 * NW * PL);
    if (lane < PL) pb[wv * PL + lane] = v;
    __syncthreads();
    double s = 0;
#pragma unroll
    for (int q = 0; q < NW; q++) s += pb[q * PL + min(lane, PL - 1)];
    buf ^= 1;
    return s;
  };
  // one rotation step on the lane-local pair (L = column on the lower position, H = on the higher one); the two
  // columns swap positions afterwards.  sit_out: this lane's pair is a boundary position with a dummy partner.
  bool rotated = false, big = false;
  auto step = [&](double (&L)[RW], double (&H)[RW], double& nL, double& nH, bool sit_out) {
    double g0 = 0, g1 = 0;
#pragma unroll
    for (int r = 0; r < RW; r++) {
      if (r & 1) g1 = fma(L[r], H[r], g1); else g0 = fma(L[r], H[r], g0);
    }
    const double g = reduce1(g0 + g1);
    double cs = 1.0, sn = 0.0, nl = nH, nh = nL;  // no rotation: plain swap
    if (g * g > 1e-30 * (nL * nH) && fabs(g) > 1e-290) {
      const double d = nH - nL;
      const double h = __builtin_amdgcn_sqrt(d * d + 4.0 * g * g);
      const double tt = (d >= 0 ? 2.0 : -2.0) * g * __builtin_amdgcn_rcp(fabs(d) + h);  // tan of the rotation angle
      cs = fast_rsqrt(1.0 + tt * tt);
      sn = tt * cs;
      nl = nH + tt * g, nh = nL - tt * g;
      rotated = true;
      big |= g * g > 1e-16 * (nL * nH);
    }
    if (sit_out) cs = 0.0, sn = 1.0, nl = nL, nh = nH;  // L stays, H changes sign: no swap
#pragma unroll
    for (int r = 0; r < RW; r++) {
      const double l = L[r], hh = H[r];
      L[r] = sn * l + cs * hh;
      H[r] = cs * l - sn * hh;
    }
    nL = nl, nH = nh;
  };

  int sweeps = 0;
  for (int sweep = 0; sweep < 30; sweep++) {
    {
      double a0 = 0, a1 = 0;
#pragma unroll
      for (int r = 0; r < RW; r++) a0 = fma(X[r], X[r], a0), a1 = fma(Y[r], Y[r], a1);
      reduce2(a0, a1);
      nX = a0, nY = a1;
    }
    rotated = false, big = false;
    for (int s2 = 0; s2 < ne; s2 += 2) {
      // even step: positions (2k, 2k+1)
      step(X, Y, nX, nY, false);
      // odd step: positions (2k-1, 2k) = (Y of lane k-1, X of lane k); positions 0 and ne-1 sit out
#pragma unroll
      for (int r = 0; r < RW; r++) Y[r] = shr_d(Y[r]);
      nY = shr_d(nY);
      step(Y, X, nY, nX, lane == 0 || lane == np);
#pragma unroll
      for (int r = 0; r < RW; r++) Y[r] = shl_d(Y[r]);
      nY = shl_d(nY);
    }
    sweeps++;
    // Every wavefront computed the same rotations: a uniform decision without communication.  A sweep whose largest
    // rotation was below 1e-8 (relative) leaves off-diagonal cosines of 1e-16 behind (quadratic convergence): it was the last.
    if (!__any(big)) break;
  }

  // ---- eigenvalues S = |g|^2 (fresh), g^T b', output
  double lX, lY, vX, vY, wX, wY;  // w = g^T diag(A') g = S v^T diag(A') v: the scale of the variables this eigenvector lives on
  {
    double a0 = 0, a1 = 0, b0 = 0, b1 = 0, d0 = 0, d1 = 0;
#pragma unroll
    for (int r = 0; r < RW; r++) {
      const double bb = lds[P_B + r0 + r], dd = lds[P_D0 + r0 + r];
      a0 = fma(X[r], X[r], a0), a1 = fma(Y[r], Y[r], a1);
      b0 = fma(X[r], bb, b0), b1 = fma(Y[r], bb, b1);
      d0 = fma(X[r] * X[r], dd, d0), d1 = fma(Y[r] * Y[r], dd, d1);
    }
    reduce2(a0, a1);
    reduce2(b0, b1);
    reduce2(d0, d1);
    lX = a0, lY = a1, vX = b0, vY = b1, wX = d0, wY = d1;
  }
  // An odd n carries one pad index; its column is exactly zero and only ever got swapped around.  Any exactly-zero
  // column is as good as the pad (its output row would be zero anyway): the first one is skipped.
  int padpos = ne;
  if (ne != n) {
    const unsigned long long zx = __ballot(lane < np && lX == 0.0), zy = __ballot(lane < np && lY == 0.0);
    const int px = zx ? 2 * (int)__builtin_ctzll(zx) : ne, py = zy ? 2 * (int)__builtin_ctzll(zy) + 1 : ne;
    padpos = min(px, py);
  }
  if (lane < np) {
    const int qx = 2 * lane, qy = 2 * lane + 1;
    const int ox = qx < padpos ? qx : qx - 1, oy = qy < padpos ? qy : qy - 1;
    // The clamp of marginalization_factor.cpp:284-285 (S > eps), applied as EXACT arithmetic would apply it: an eigenvalue
    // that FP64 cannot tell from zero is zero.  A'_ij reaches this kernel with an error of about 20 u sqrt(s_i s_j), s_i the
    // magnitude its diagonal entry was formed at (a difference of information matrices: up to 2.5e12 on the gyroscope-bias rows),
    // so an eigenvalue S with unit eigenvector v is uncertain by up to 20 n u v^T diag(s) v.  A window without a gauge-fixing
    // prior has 16 .. 30 EXACT zeros in A' (gauge, unconstrained biases / extrinsic); in FP64 they come out as +-1e-10 .. 1e-2,
    // above eps at random, and one that survives puts (v^T b')^2 / S into |r0|^2 (measured against the binary128 statement of
    // the reference's algorithm, tests/test_prior_truth.py: the prior's cost came out 3x too large in 1 of 6 such windows).
    // The threshold errs on the side of KEEPING: clamping a genuine eigenvalue removes the only constraint a weakly observed
    // direction has (measured: a threshold of 1e-13 v^T diag(s) v took eigenvalues of 0.02 .. 0.5 on the bias rows of a
    // prior-less first window with it, and the stream that followed ended 0.09 away from the exact one), while a kept noise
    // eigenvalue is what the reference's own FP64 computation leaves behind as well.  Measured on two 10-frame streams against
    // the stream with exact (binary128) priors: 1e-15 v^T diag(s) v reproduces the exact clamp set in 12 of 12 prior-less
    // windows but costs the streams a factor 10 - 20 (9e-6 / 2e-4 worst state distance); 1e-16 v^T diag(s) v (= u) misses one
    // or two of the 16 .. 30 zeros in half of those windows and leaves the streams at 3.9e-7 / 1.1e-4, the values they have
    // without any noise test.  1e-16: 2.5e-4 for a pure gyroscope-bias direction (information worth sigma = 60 rad/s), 6e-7 for
    // an accelerometer-bias direction, 1e-9 for directions in the poses.
    // Round 5, eight 20-frame streams (tests/test_prior_truth.py, profiles/r05_noise_rel.md): at 1e-16 the prior drops MORE directions than the
    // exact one on 11 of 160 frames - genuine weak ones - and the states are within 1e-6 of the exact-prior stream on 54 frames; at
    // 1e-18 on 3 frames (as with no noise test at all) and 120.  Keeping a noise direction costs the states nothing, dropping a genuine
    // one does: the default is 1e-18.
    // (avm_options::marg_noise_rel, default 1e-18; 0 - also under AVM_PRIOR_LITERAL=1 - leaves the reference's S > eps alone)
    const bool kx = lX > eps && lX * lX > noise_rel * wX, ky = lY > eps && lY * lY > noise_rel * wY;
#pragma unroll
    for (int r = 0; r < RW; r++) {
      if (r0 + r < n) {
        if (qx != padpos) gJ[(size_t)ox * ldj + r0 + r] = kx ? X[r] : 0.0;
        if (qy != padpos) gJ[(size_t)oy * ldj + r0 + r] = ky ? Y[r] : 0.0;
      }
    }
    if (wv == 0) {
      if (qx != padpos) gr[ox] = kx ? vX / lX : 0.0;
      if (qy != padpos) gr[oy] = ky ? vY / lY : 0.0;
    }
  }
  if (prof && t == 0) {
    atomicAdd(reinterpret_cast<unsigned long long*>(prof + 25), (unsigned long long)((long long)__builtin_readcyclecounter() - t_start));
    atomicAdd(reinterpret_cast<unsigned long long*>(prof + 29), (unsigned long long)sweeps);
  }
}

static bool print_occupancy() {
  int nb = -1;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, reinterpret_cast<const void*>(prior_eig_kernel), NT, P_END * 8);
  fprintf(stderr, "[avm] prior_eig_kernel: %d workgroups / CU (LDS %d B)\n", nb, P_END * 8);
  return true;
}

}  // namespace pe

hipError_t launch_prior_eig(const avm_prior_out& po, int n_windows, double eps, double noise_rel, const double* scale, long long* prof, int* done,
                            hipStream_t stream) {
  // AVM_PRIOR_LITERAL=1: the reference's square root, literally - the eigen-decomposition for every window and the clamp S > eps and
  // nothing else (as avm_options::marg_noise_rel = 0).  AVM_PRIOR_FORCE_EIG=1: the eigen-decomposition for every window, the clamp as
  // the options say (A/B tests of the two forms of the square root).  Read per call: the tests flip them inside one process.
  const char* lit = getenv("AVM_PRIOR_LITERAL");
  const char* fe = getenv("AVM_PRIOR_FORCE_EIG");
  const bool lit1 = lit && lit[0] == '1';
  const int literal = (lit1 || (fe && fe[0] == '1')) ? 1 : 0;
  if (lit1) noise_rel = 0.0;
  // (the LDS attribute once per process, a failure to set it remembered: kernels.hpp; the occupancy query below needs it set)
  const hipError_t e = lds_attr_once<pe::prior_eig_kernel>(pe::P_END * 8);
  if (e != hipSuccess) return e;
  if (prof) {
    static const bool printed = pe::print_occupancy();  // (by the first profiled call)
    (void)printed;
  }
  // the well-conditioned windows on one wavefront each; what that kernel leaves (done[w] == 0) goes through the pivoted path
  // (AVM_PRIOR_LITERAL=1 / AVM_PRIOR_FORCE_EIG=1 / AVM_PRIOR_NO_FAST=1: everything through the pivoted path, for A/B tests)
  const char* nf = getenv("AVM_PRIOR_NO_FAST");
  const bool fast = done && !literal && !(nf && nf[0] == '1');
  if (fast) hipLaunchKernelGGL(pe::prior_chol_kernel, dim3(n_windows), dim3(64), 0, stream, po, n_windows, eps, noise_rel, scale, done);
  return launch_lds<pe::prior_eig_kernel>(n_windows, pe::NT, pe::P_END * 8, stream, po, n_windows, eps, noise_rel, scale, prof, literal,
                                          fast ? (const int*)done : (const int*)nullptr);
}

}  // namespace avm
