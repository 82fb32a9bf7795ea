// fsel/logdet4.hpp - fs_log, fsel_logdet4 (four candidates per wavefront, LDL^T in registers), fsel_ub4
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

// Natural logarithm of a positive, normal, finite double (every argument here is a pivot or a diagonal entry that has already
// passed `> 0`; anything else gives finite junk or NaN, which the callers discard): the fdlibm reduction - x = 2^k (1 + f),
// sqrt(1/2) <= 1 + f < sqrt(2), s = f / (2 + f), log(1 + f) = f - f^2/2 + s (f^2/2 + R(s^2)) with the degree-14 minimax R - with
// the quotient from v_rcp_f64 + two Newton steps + a residual correction.  < 1 ulp like the library's, in 45 instead of ~80
// instructions: the evaluation takes five logarithms per candidate and round.
AVM_DEV double fs_log(double x) {
  int k = __builtin_amdgcn_frexp_exp(x);           // x = m 2^k, 1/2 <= m < 1
  double m = __builtin_amdgcn_frexp_mant(x);
  const bool lo = m < 0.70710678118654752440;
  m = lo ? m + m : m;
  k = lo ? k - 1 : k;
  const double f = m - 1.0, d = 2.0 + f;
  const double r = fast_rcp(d);
  double sq = f * r;
  sq = fma(fma(-d, sq, f), r, sq);                  // s = f / (2 + f)
  const double z = sq * sq, w = z * z;
  const double t1 = w * fma(w, fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), 3.999999999940941908e-01);
  const double t2 = z * fma(w, fma(w, fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01), 2.857142874366239149e-01), 6.666666666666735130e-01);
  const double R = t2 + t1, hfsq = 0.5 * f * f, dk = (double)k;
  return dk * 6.93147180369123816490e-01 - ((hfsq - (sq * (hfsq + R) + dk * 1.90821492927058770002e-10)) - f);
}

// logdet(C + pr D) and the Hadamard bound for the candidate of this lane's 16-lane row (see the comment above fs_rowbcast_k, dpp.hpp):
// *ld_out = sum_j log(sqrt(d_j)) in pivot order, *ub_out = sum_i log((dpp + pr D)_ii); returns false on a non-positive pivot.
// sC / sdpp: the frame's current reduced information and position diagonal (LDS), D: the candidate's Delta (global).
// PHASED (the single-frame kernel, one wavefront per SIMD): the phases are kept apart in the schedule; the compiler's own
// interleaving of the loads, the logarithms and the elimination was measured 10 % slower there - and 6 % faster on the batched
// path, where a second wavefront fills the gaps.
#ifdef FS_TRACE_EVAL
#define FS_TK(i) { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); __builtin_amdgcn_sched_barrier(0); const long long n__ = clock64(); if (tk) tk[i] += n__ - tkp; tkp = n__; __builtin_amdgcn_sched_barrier(0); }
#else
#define FS_TK(i) if (PHASED) __builtin_amdgcn_sched_barrier(0);
#endif
// (Measured and dropped: the multipliers as LDS broadcasts - a column written once, one ds_read per gk instead of two DPP moves
//  per pair, the round trip hidden by look-ahead - made the evaluation 10-17 % slower.)
// PACKED: D is the packed lower triangle (row R at R (R + 1) / 2, the single-frame kernel's LDS copy) instead of the full
// T x T block; an entry past the diagonal of a diagonal block - never used, see above - then reads into the next row.
// PACKED == 2: D is the lower triangle BY COLUMNS (FselDev::delta_pk): the 15 lanes of a candidate still read consecutive doubles.
template <int T, int BS, int NB, bool PHASED = false, int PACKED = 0>
AVM_DEV bool fsel_logdet4(const double* sC, const double* sdpp, const double* D, double pr, double* ld_out, double* ub_out, long long* tk = nullptr) {
#ifdef FS_TRACE_EVAL
  long long tkp = clock64();
#endif
  const int lane = threadIdx.x & 63;
  const int r = min(lane & 15, BS - 1);  // this lane's row inside every block row
  // m[bi][c] = (C + p Delta)[bi BS + r][c], c < (bi + 1) BS.  Both matrices are symmetric, so the entry is fetched as
  // [c][bi BS + r]: the 15 lanes of a candidate then read 15 consecutive doubles instead of 15 different cache lines
  double m[NB][T];
  double ddg[NB];  // the candidate's diagonal entries of this lane's rows (the Hadamard bound)
  if constexpr (PACKED == 2) {
    // D comes from MEMORY here (fsel_solo_kernel): a block row's entries are all requested before the first one is used.  Left to itself the
    // compiler pairs each load with its multiply-add and keeps one or two in flight - 45 dependent trips to the L2, 15.3 K of an
    // evaluation's 23.2 K cycles (round 5, profiles/r05_fsel_single_frame_floor.md).  One block row at a time (15 + 30 entries at 3 H = 30,
    // 13 + 26 + 39 at 39): every entry of the candidate at once costs registers the elimination needs (49 spilled at 30, 6 % slower at 39).
#pragma unroll
    for (int bi = 0; bi < NB; bi++) {
#pragma unroll
      for (int c = 0; c < (bi + 1) * BS; c++) {
        const int R = bi * BS + r;
        m[bi][c] = D[c <= R ? c * T - c * (c - 1) / 2 + (R - c) : R * T - R * (R - 1) / 2];  // (an entry past the diagonal is never used)
      }
      const int dgi = bi * BS + r;
      ddg[bi] = D[dgi * T - dgi * (dgi - 1) / 2];
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int c = 0; c < (bi + 1) * BS; c++) m[bi][c] = sC[c * T + bi * BS + r] + pr * m[bi][c];
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
#pragma unroll
    for (int bi = 0; bi < NB; bi++)
#pragma unroll
      for (int c = 0; c < (bi + 1) * BS; c++) {
        const int idx = c * T + bi * BS + r, R = bi * BS + r;
        m[bi][c] = sC[idx] + pr * D[PACKED == 1 ? R * (R + 1) / 2 + c : idx];
      }
#pragma unroll
    for (int bi = 0; bi < NB; bi++) {
      const int dgi = bi * BS + r;
      ddg[bi] = D[PACKED == 1 ? dgi * (dgi + 1) / 2 + dgi : dgi * T + dgi];
    }
  }
  FS_TK(0)
  // Hadamard upper bound: sum over the rows, block row by block row, then across the 16 lanes in lane order
  double ubl = 0.0;
#pragma unroll
  for (int bi = 0; bi < NB; bi++) {
    const int dgi = bi * BS + r;
    ubl += fs_log(sdpp[dgi] + pr * ddg[bi]);
  }
  const double ubt = fs_row_sum((lane & 15) < BS ? ubl : 0.0);
  FS_TK(1)
  double dkeep[NB];  // lane j keeps the pivot of row bj BS + j
  bool bad = false;
  // m[bi][gk] += A[gk][gj] * (-mult[bi]) with A[gk][gj] = lane k of m[bk][gj], taken by the multiply-add itself (fs_fmac_bcast): one instruction per
  // (pivot, column, block row) where it was two 32-bit DPP moves per (pivot, column) and a multiply-add per block row - the same product, the same rounding
  sfor<NB>([&](auto BJ) {
    constexpr int bj = BJ;
    dkeep[bj] = 1.0;
    sfor<BS>([&](auto J) {
      constexpr int j = J, gj = bj * BS + j;
      const double djj = fs_rowbcast_k<j>(m[bj][gj]);
      if (!(djj > 0.0)) bad = true;
      dkeep[bj] = (lane & 15) == j ? djj : dkeep[bj];
      double y = __builtin_amdgcn_rcp(djj), e = fma(-djj, y, 1.0);
      y = fma(y, e, y);
      e = fma(-djj, y, 1.0);
      y = fma(y, e, y);
      double nmult[NB];
#pragma unroll
      for (int bi = bj; bi < NB; bi++) nmult[bi] = -(m[bi][gj] * y);
      fs_dpp_fence();
      sfor<NB - bj>([&](auto BKK) {
        constexpr int bk = bj + BKK, k0 = bk == bj ? j + 1 : 0;
        sfor<BS - k0>([&](auto KK) {
          constexpr int k = k0 + KK, gk = bk * BS + k;
          sfor<NB - bk>([&](auto BII) {
            constexpr int bi = bk + BII;
            fs_fmac_bcast<k>(m[bi][gk], m[bk][gj], nmult[bi]);
          });
        });
      });
      fs_dpp_fence();  // (the next pivot's broadcast reads an entry this run has written)
    });
  });
  FS_TK(2)
  // log(sqrt(d)): per lane over its block rows, then across the candidate's lanes
  double ldl = 0;
#pragma unroll
  for (int bj = 0; bj < NB; bj++) ldl += dkeep[bj] > 0.0 ? 0.5 * fs_log(dkeep[bj]) : 0.0;
  const double ld = fs_row_sum((lane & 15) < BS ? ldl : 0.0);
  FS_TK(3)
  *ld_out = ld, *ub_out = ubt;
  return !bad;
}


// The Hadamard bound alone, for the candidate of this lane's 16-lane row: the same expression, in the same order, as the bound
// inside fsel_logdet4.  dd[d * stride]: the T diagonal entries of the candidate's Delta (fsel_solo_kernel takes every candidate's bound from
// here, scored or not, so the equal-key rule and the (fValue, bound, id) order of the pick see one function).
template <int T, int BS, int NB>
AVM_DEV double fsel_ub4(const double* sdpp, const double* dd, int stride, double pr) {
  const int lane = threadIdx.x & 63;
  const int r = min(lane & 15, BS - 1);
  double ubl = 0.0;
#pragma unroll
  for (int bi = 0; bi < NB; bi++) {
    const int dgi = bi * BS + r;
    ubl += fs_log(sdpp[dgi] + pr * dd[dgi * stride]);
  }
  return fs_row_sum((lane & 15) < BS ? ubl : 0.0);
}
