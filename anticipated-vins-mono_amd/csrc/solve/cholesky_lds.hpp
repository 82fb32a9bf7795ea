// solve/cholesky_lds.hpp - left-looking factorization of the packed system in LDS and its solve (latency and extended builds)
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// Scratch of the factorization inside the tile at L_WCH (dead while S is being factored): L^-T of the current and of the
// next diagonal block, and a per-lane dump slot for the masked-out stores.
constexpr int L_CLT = L_WCH /* two buffers of 256: block j's L^-T in buffer j & 1 */, L_CDUMP = L_WCH + 512;

// ---- tiles of the factorization, 16x16 on v_mfma_f64_16x16x4 --------------------------------------------------------
// Everything is unconditional (a predicated LDS access compiles to a branch with its own s_waitcnt): operand rows are
// clamped to the last valid row (the duplicates only reach outputs that are not stored), destination loads are clamped to
// a valid address and masked-out stores go to a per-lane dump slot.  The k index of a product is a summation index, so
// lane group lk takes columns 4 lk + {0..3} of a 16-column block: two 16-byte loads per operand instead of four 8-byte ones.
struct CholTile {
  double d[4];
  int o[4];  // destination offsets (doubles from lds[0]); masked-out entries point at the dump slot
};

// Factor the nb x nb diagonal block at c0 in the registers of the calling wavefront (lane = row, register = column).
//  * Select-free: lanes / columns outside the block (and the upper triangle) just carry finite junk that is never stored.
//  * Lanes 16..31 carry the rows of the identity through the same eliminations: lane 16+i ends with row i of L^-T, which the
//    MFMA panel solve multiplies the rows below with (zero extra instructions in the pivot chain).
//  * Square-root free: column j is divided by its pivot with v_rcp_f64 + two Newton steps; rows and L^-T are stored
//    unscaled (times sqrt(d_c) per column c, the pivot d_c itself on the diagonal) and the consumers apply rsqrt(d_c):
//    the panel solve (which also raises the non-positive-pivot flag) and chol_solve_lds.
//  * The wavefront is instruction-issue bound (~4.5 cycles per FP64 / v_readlane instruction, 3 instructions per
//    (pivot, column) pair), so everything else is kept out of it: no pivot bookkeeping, stores by address select, and the
//    rank-1 update of pivot j-1 is software-pipelined by hand into the latency shadows of pivot j's reciprocal chain.
AVM_NOINL void chol_diag_block(int c0, int nb, int buf) {
  constexpr int NB = CNB;
  double* S = LDS() + L_S;
  const int r = threadIdx.x & 63;
  __builtin_amdgcn_s_setprio(3);  // this wavefront is the critical path of the factorization: win issue arbitration
  double a[NB];
  const bool idl = (r & 48) == 16;
  const int rc = min(r, nb - 1);
  double* row = S + roff(c0 + rc) + c0;
  {
#pragma unroll
    for (int k = 0; k < NB; k++) a[k] = row[k];  // 16 reads in flight at immediate offsets; past the diagonal they run into the
                                                 // next packed rows (still inside the factor's LDS region + slack): junk, never stored
#pragma unroll
    for (int k = 0; k < NB; k++) a[k] = idl ? ((r & 15) == k ? 1.0 : 0.0) : a[k];  // lanes 16..31: the identity's rows
  }
  double uprev = 0.0;
#pragma unroll
  for (int j = 0; j < NB; j++) {
    if (j > 0) a[j] = fma(-uprev, readlane_d(a[j - 1], j), a[j]);
    const double djj = readlane_d(a[j], j);
    double y = __builtin_amdgcn_rcp(djj), e = 0;
    AVM_PIVOT_TAIL(0, true)
    e = fma(-djj, y, 1.0);
    AVM_PIVOT_TAIL(1, true)
    y = fma(y, e, y);
    AVM_PIVOT_TAIL(2, true)
    e = fma(-djj, y, 1.0);
    AVM_PIVOT_TAIL(3, true)
    y = fma(y, e, y);
    AVM_PIVOT_TAIL(4, true)
    uprev = a[j] * y;
  }
  {
    double* dst = idl ? LDS() + L_CLT + buf * (NB * NB) + (r & 15) * NB : row;
    double* dump = LDS() + L_CDUMP + r;
    const int kmax = idl ? NB - 1 : (r < nb ? r : -1);
#pragma unroll
    for (int k = 0; k < NB; k++) *(k <= kmax ? dst + k : dump) = a[k];
  }
  __builtin_amdgcn_s_setprio(0);
}

// U_ij = A_ij - sum_{p < j} X_ip X_jp^T: the update of tile (ti, tj) by the panels [p_begin, p_end) at once (LEFT-looking),
// accumulated in registers over the solved panels - 4 tj MFMAs on four independent chains - and ONE read-modify-write of the destination
// (right-looking costs a destination round trip per panel, and the LDS write path is the slow one: ~70 B/clk).
AVM_DEV void chol_left_tile(int ti, int tj, int p_begin, int p_end) {
  constexpr int NR = NF + 1;
  double* S = LDS() + L_S;
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  const dv2* pa = reinterpret_cast<const dv2*>(S + roff(min(16 * ti + lr, NR - 1)) + 4 * lk);
  const dv2* pb = reinterpret_cast<const dv2*>(S + roff(min(16 * tj + lr, NF - 1)) + 4 * lk);
  CholTile T;  // (destination part only)
  {
    const int gj = 16 * tj + lr;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int gi = 16 * ti + lk + 4 * r;
      const bool ok = gi < NR && gj < NF && gj <= gi;
      const int gic = min(gi, NR - 1);
      const int ol = L_S + roff(gic) + min(gj, min(gic, NF - 1));
      T.d[r] = LDS()[ol];
      T.o[r] = ok ? ol : L_CDUMP + lane;
    }
  }
  d4 D0 = {0, 0, 0, 0}, D1 = {0, 0, 0, 0}, D2 = {0, 0, 0, 0}, D3 = {0, 0, 0, 0};
  const bool diag = ti == tj;
#pragma unroll 1
  for (int p = p_begin; p < p_end; p++) {
    const dv2 a0 = pa[8 * p], a1 = pa[8 * p + 1];
    dv2 b0 = a0, b1 = a1;
    if (!diag) b0 = pb[8 * p], b1 = pb[8 * p + 1];
    D0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[0], b0[0], D0, 0, 0, 0);
    D1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[1], b0[1], D1, 0, 0, 0);
    D2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[0], b1[0], D2, 0, 0, 0);
    D3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[1], b1[1], D3, 0, 0, 0);
  }
  const d4 D = (D0 + D1) + (D2 + D3);
#pragma unroll
  for (int r = 0; r < 4; r++) LDS()[T.o[r]] = T.d[r] - D[r];
}

// X_ij = (A_ij - X_{i,j-1} X_{j,j-1}^T) L_jj^-T: the tile of row block ti in block column j (c0 = 16 j, nb columns), for the
// rows >= c0 + nb.  `upd`: the tile still lacks the update of the last solved panel (j - 1); that product is computed
// TRANSPOSED - X_{j,j-1} X_{i,j-1}^T - because the accumulator layout of the transposed tile is exactly the A operand
// layout of the solve: the update costs no round trip through LDS.  bop = L_jj^-T (B operand), isq = rsqrt(d_c) of the
// lane's column (see chol_diag_block).
AVM_DEV void chol_panel_tile(int ti, int c0, int nb, const double (&bop)[CNB / 4], double isq, bool upd) {
  constexpr int NB = CNB, NR = NF + 1;
  double* lds = LDS();
  double* S = lds + L_S;
  const int lane = threadIdx.x & 63, lr = lane & 15, lk = lane >> 4;
  const int c1 = c0 + nb;
  const int row = 16 * ti + lr;
  const double* pa = S + roff(min(row, NR - 1)) + c0 + lk;
  const bool va = row < NR && row >= c1;
  double aop[NB / 4];
#pragma unroll
  for (int m = 0; m < NB / 4; m++) aop[m] = pa[4 * m];  // past-the-row reads stay inside the LDS carve and are masked below
  if (upd) {
    const dv2* pj = reinterpret_cast<const dv2*>(S + roff(min(c0 + lr, NF - 1)) + (c0 - NB) + 4 * lk);
    const dv2* pi = reinterpret_cast<const dv2*>(S + roff(min(row, NR - 1)) + (c0 - NB) + 4 * lk);
    const dv2 a0 = pj[0], a1 = pj[1], b0 = pi[0], b1 = pi[1];
    d4 C0 = {0, 0, 0, 0}, C1 = {0, 0, 0, 0}, C2 = {0, 0, 0, 0}, C3 = {0, 0, 0, 0};
    C0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[0], b0[0], C0, 0, 0, 0);
    C1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[1], b0[1], C1, 0, 0, 0);
    C2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[0], b1[0], C2, 0, 0, 0);
    C3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[1], b1[1], C3, 0, 0, 0);
    const d4 C = (C0 + C1) + (C2 + C3);  // C[m] = (X_{i,j-1} X_{j,j-1}^T)[row lr][column lk + 4 m]
#pragma unroll
    for (int m = 0; m < NB / 4; m++) aop[m] -= C[m];
  }
#pragma unroll
  for (int m = 0; m < NB / 4; m++) aop[m] = (va && lk + 4 * m < nb) ? aop[m] : 0.0;
  d4 Da = {0, 0, 0, 0}, Db = {0, 0, 0, 0};
  Da = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[0], bop[0], Da, 0, 0, 0);
  Db = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[1], bop[1], Db, 0, 0, 0);
  Da = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[2], bop[2], Da, 0, 0, 0);
  Db = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[3], bop[3], Db, 0, 0, 0);
  const d4 D = (Da + Db) * isq;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int gi = 16 * ti + lk + 4 * r;
    lds[(gi < NR && gi >= c1 && lr < nb) ? L_S + roff(gi) + c0 + lr : L_CDUMP + lane] = D[r];
  }
}

// In-place lower Cholesky of the packed NFxNF matrix in lds[L_S]; returns false on a non-positive pivot.
// The right-hand side rides along as row NF of the packed storage, so the forward substitution L z = b happens as part of
// the factorization (z ends up in that row).  LEFT-looking by 16-column blocks, ONE workgroup barrier per block column,
// everything lagging one panel behind the diagonal.  At the barrier that opens phase j: the panels p < j are solved, the
// diagonal block j is factored (L_jj^-T in buffer j & 1), the tiles of block column j carry the updates of the panels
// p <= j - 2 and the diagonal tile (j + 1, j + 1) those of the panels p <= j - 1.  Phase j:
//   wavefront 0  (the critical path): tile (j + 1, j) = [last panel's update, solve]; diagonal tile (j + 1, j + 1) -= panel
//                j; then its 16-pivot chain (chol_diag_block).  It reads nothing the others write in this phase.
//   the helpers  (wavefronts 1-3, 5-7; wavefront 4 shares wavefront 0's SIMD and FP64 pipe and stays idle): the other
//                tiles (i, j) = [last panel's update, solve]; block column j + 1 receives the panels p < j (solved before
//                the phase began); the diagonal tile (j + 2, j + 2) receives the panels p <= j from the helper that
//                solves tile (j + 2, j).
// Every tile is read-modify-written once for all its early panels and once more, fused with its solve, for the last one.
AVM_NOINL bool cholesky_lds(long long* prof) {
  struct { long long* prof; } c{prof};
  double* lds = LDS();
  double* S = lds + L_S;
  const int t = threadIdx.x, wv = t >> 6, lane = t & 63, lr = lane & 15, lk = lane >> 4;
  constexpr int NB = CNB;
  constexpr int NHELP = NT / 64 - 2;
  const int hslot = wv < 4 ? wv - 1 : wv - 5 + 3;  // helpers 1 2 3 5 6 7 -> 0..5 (wavefronts 0 and 4: not helpers)
  const bool helper = wv != 0 && wv != 4;
  int* s_fail = reinterpret_cast<int*>(lds + L_INT) + I_FAIL;
  if (t == 0) *s_fail = 0;
  PROF_T0();
  if (wv == 0) chol_diag_block(0, NB, 0);
  __syncthreads();
  PROF(c, 4);
  for (int j = 0, c0 = 0; c0 < NF; j++, c0 += NB) {
    const int nb = min(NB, NF - c0), c1 = c0 + nb;
    const int t0 = c1 >> 4;  // first tile row with rows below the block (the block's own tile row when nb < 16)
    // B operand of the solves = L_jj^-T (left in buffer j & 1 by chol_diag_block, stored times sqrt(d_c) per column: the
    // pivots sit on the diagonal of the block)
    double bop[NB / 4];
    {
      const double* LT = lds + L_CLT + (j & 1) * (NB * NB);
#pragma unroll
      for (int m = 0; m < NB / 4; m++) bop[m] = LT[(lk + 4 * m) * NB + lr];
    }
    const int cc = c0 + min(lr, nb - 1);
    const double dc = S[roff(cc) + cc];
    if (!(dc > 0.0)) *s_fail = 1;  // non-positive (or NaN) pivot: every wavefront sees the same values
    const double isq = fast_rsqrt(dc);  // applied to the product's columns: its latency hides under the loads and MFMAs
#pragma unroll
    for (int m = 0; m < NB / 4; m++) bop[m] = (lk + 4 * m < nb && lr < nb) ? bop[m] : 0.0;
    const bool last = c1 >= NF;
    if (wv == 0) {
      const long long q0 = clock64();
      chol_panel_tile(t0, c0, nb, bop, isq, j > 0 && t0 > j);
      if (!last) {
        wave_lds_sync();
        chol_left_tile(j + 1, j + 1, j, j + 1);  // (the panels before were applied a phase ago by the first helper)
        wave_lds_sync();
        chol_diag_block(c1, min(NB, NF - c1), (j + 1) & 1);
      }
      if (c.prof && t == 0) c.prof[28] += clock64() - q0;
    } else if (helper) {
      const long long q0 = clock64();
      for (int ti = t0 + 1 + hslot; ti <= TLAST; ti += NHELP) chol_panel_tile(ti, c0, nb, bop, isq, j > 0 && ti > j);
      // the diagonal tile (j + 2, j + 2) only needs its own row block's panels: the helper that has just solved tile
      // (j + 2, j) applies all of them, panel j included, so that wavefront 0 adds a single panel next phase
      if (!last && hslot == 0 && j + 2 <= TLAST) {
        wave_lds_sync();
        chol_left_tile(j + 2, j + 2, 0, j + 1);
      }
      if (!last && j > 0) {
        // tiles (j + 2 .. TLAST, j + 1) receive the panels p < j; dealt in the opposite order of the panel tiles above
        const int ntile = TLAST - (j + 1);
        for (int k = NHELP - 1 - hslot; k < ntile; k += NHELP) chol_left_tile(j + 2 + k, j + 1, 0, j);
      }
      if (c.prof && t == 64) c.prof[27] += clock64() - q0;
    }
    __syncthreads();
    PROF(c, 5);
    if (*s_fail) return false;
    if (last) break;
  }
  return true;
}

// Backward substitution L^T x = z with z in the augmented row of lds[L_S] (left there by cholesky_lds), result to
// lds[vec..vec+NF).  13.6K multiply-adds on an 11-block serial chain: all of it runs in wavefront 0 with no workgroup
// barrier (a barrier costs ~250 cycles, two per block were most of the old version's time).  Per 16-column block, last
// to first:  lane r (mod 16) holds column r of the block triangle scaled so that x_r comes straight out of v_readlane
// (x_r = d_r^-1/2 z_r - d_r^-1 sum_i raw[i][r] x_i; the diagonal blocks are stored unscaled, see chol_diag_block) and
// the 16 steps are readlane -> fma; entries at or above the diagonal are finite junk that only reaches values that
// have already been consumed.  The finished x_i stay in SGPRs and are applied to the remaining b[j], j < c0, by all
// 64 lanes (loads issued ahead of the chain).
template <int NBV>
AVM_DEV void chol_solve_block(double* S, double* b, int c0, int lane) {
  const int rr = min(lane & 15, NBV - 1);
  const double* col = S + c0 + rr;  // + roff(row): column c0+rr
  const double dr = col[roff(c0 + rr)];
  double colv[NBV];
#pragma unroll
  for (int i = 0; i < NBV; i++) colv[i] = col[roff(c0 + i)];  // uniform row offset; i < rr reads (finite) entries of the next rows
  double bv = b[c0 + rr];
  // rows of the block for all (<= 160 = 3 x 64) remaining columns: in flight during the chain (clamped addresses; a
  // segment beyond c0 is simply not stored)
  const int jc = max(c0 - 1, 0);
  double v0[3][NBV], acc[3];
#pragma unroll
  for (int sgm = 0; sgm < 3; sgm++) {
    const int j = min(64 * sgm + lane, jc);
    acc[sgm] = b[j];
#pragma unroll
    for (int i = 0; i < NBV; i++) v0[sgm][i] = S[roff(c0 + i) + j];
  }
  const double isq = fast_rsqrt(dr), di2 = isq * isq;
  bv *= isq;
#pragma unroll
  for (int i = 0; i < NBV; i++) colv[i] *= di2;
  double xs[NBV], xout = 0.0;
#pragma unroll
  for (int jj = NBV - 1; jj >= 0; jj--) {
    xs[jj] = readlane_d(bv, jj);
    bv = fma(-colv[jj], xs[jj], bv);
    xout = lane == jj ? xs[jj] : xout;
  }
  if (lane < NBV) b[c0 + lane] = xout;
#pragma unroll
  for (int sgm = 0; sgm < 3; sgm++) {
    if (64 * sgm >= c0) break;  // (uniform)
    double a0 = acc[sgm], a1 = 0.0;
#pragma unroll
    for (int i = 0; i < NBV; i++) {
      if (i & 1) a1 = fma(-v0[sgm][i], xs[i], a1); else a0 = fma(-v0[sgm][i], xs[i], a0);
    }
    if (64 * sgm + lane < c0) b[64 * sgm + lane] = a0 + a1;
  }
  wave_lds_sync();
}

AVM_NOINL void chol_solve_lds(int vec) {
  double* lds = LDS();
  double* S = lds + L_S;
  double* b = lds + vec;
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  constexpr int NB = 16;
  if (wv == 0) {
#pragma unroll
    for (int q = 0; q < 3; q++)
      if (lane + 64 * q < NF) b[lane + 64 * q] = S[roff(NF) + lane + 64 * q];
    wave_lds_sync();
    if (NF % NB) chol_solve_block<(NF % NB) ? (NF % NB) : NB>(S, b, (NF / NB) * NB, lane);
    // (unrolled: every block's row offsets become immediates of its LDS reads)
#pragma unroll
    for (int blk = NF / NB - 1; blk >= 0; blk--) chol_solve_block<NB>(S, b, blk << 4, lane);
  }
  __syncthreads();
}
