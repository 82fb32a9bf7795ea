// solve/chol_regs_tables.hpp - chol_regs' elimination order and its compile-time tables: tp_perm, tp_off_c, TpPattern, steps / owners / W slots, tp_offsets
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// =====================================================================================================================
// Throughput build, and the latency / extended builds for every window whose prior fits (I_CRFIT): the factorization on REGISTER tiles,
// distributed over four wavefronts (the latency build's other four only keep the barriers company; the extended build, with 13 more dense
// columns = one more tile column, spreads them over all eight), in an elimination order that keeps the factor SPARSE and lets TWO pivot
// chains run at a time (round 6).
//
// Order of elimination - a nested dissection of the speed-bias chain with frame 5's block as the separator:
//     B: the speed-bias blocks of frames 10, 9, .. 6   (45 columns + 3 of padding = tile columns 0, 1, 2)
//     F: the speed-bias blocks of frames 4, 3, .. 0    (45 columns + 3 of padding = tile columns 3, 4, 5)
//     then frame 5's block, the poses and the right-hand side (9 + 66 + 1 = 76 positions = tile columns 6 .. 10).
// Speed-bias block b couples to blocks b - 1 / b + 1 and to the poses b - 1 .. b + 1 (one IMU factor each side).  Eliminated from the
// window's end, B hands each next block the poses b .. 10 as fill and nothing else; F is eliminated from the separator outwards, so
// that the prior's speed-bias block (frame 0: the one block the prior couples to EVERY pose - the strip) comes last of it and its
// dense row fills nothing.  B and F never meet (no factor joins them, and neither does the fill: what joins them is eliminated
// later), so the 16-pivot chains of tile columns t and 3 + t, t = 0, 1, 2, run at the same time on two wavefronts: a factorization is
// EIGHT chain times long (3 + 5) instead of eleven, and the chain - one wavefront, 4.5 K cycles - is what a step lasts.  Of the 66
// upper tiles of the 11 x 11 grid 47 can be nonzero and a factorization takes 91 tile updates (364 MFMAs) where the order poses |
// speed-biases takes 220 (880): with the poses first every speed-bias row fills in completely.  The padding positions are rows of the
// identity.  The rest of the kernel keeps its layout; the permutation happens when the tiles are loaded (tp_offsets) and when the
// solution is written back.
//
// The augmented system [H' + mu D^2, g'; g'^T, .] in that order is cut into 11 x 11 tiles of 16 x 16 and held as its UPPER tiles
// U(k, i), k <= i (U(k, i) = L(i, k)^T once factored), in the accumulator layout of v_mfma_f64_16x16x4: register r of lane
// (lk = lane / 16, lr = lane % 16) is entry (lk + 4 r, lr).  With the k index of a product running as lk + 4 r such a tile IS a B
// operand and, read as an A operand, its transpose (the scheme of prior_chol_kernel, prior_eig.hip), so nothing is transposed or
// moved between lanes.  The right-hand side is position TP_RHS (tile column 10, local column 11): the forward substitution rides along.
//   * which tiles exist is a compile-time table (TPP: the system's tile pattern closed under the elimination's fill); a tile outside
//     it is never loaded, solved, published or updated;
//   * ownership by tile COLUMN (tp_owner): wavefront 3 holds B's columns, wavefront 2 F's - their tiles only ever meet each other, the two
//     chains of chains run there -, the other columns are spread so that a chain's owner has little else to do: at most 13 tiles;
//   * step t (tp_step_piv: the pivot columns {t, 3 + t} for t < 3, then {t + 3}):
//              [owner of a pivot column k] 16-pivot chain on the diagonal tile (through a 2 KB LDS patch into lane = row form: the
//              square-root-free chain of chol_diag_block, L_kk^-T riding along in lanes 16..31) ...................... barrier
//              [every wavefront] W(k, i) = L_kk^-1 U(k, i) for its columns i > k, published to LDS; the owner of a pivot column q of
//              step t + 1 then updates tile (q, q) - it needs its own W(k, q) only -, stages it and starts the chain ... counted
//              [every other wavefront] waits for the four counts, then U(j, i) -= W(k, j)^T W(k, i) for its columns while the chains run
//   * backward substitution L^T x = z by the same steps, last to first: the owner of column i solves x_i from z_i minus the four
//     wavefronts' partial sums, folds x_i into element-wise accumulators E_k += U(k, i) .* x_i (k < i, no reduction), and every
//     wavefront that holds a tile of the next step's rows reduces its E over the 16-lane rows (DPP) into its partial vector: one barrier per step.
// Nothing of the factor ever goes to memory; the LDS traffic is the published rows of W (<= 18 KB per step).
static_assert(NFR == 11 && NF == NPOSE + 99 && (TPT == 11 || TPT == 12), "the elimination order below is written for eleven frames");
constexpr int TP_PAD = -1;
// (TP_M0, TP_P0, TP_RHS - first position of frame 5's block / of the dense columns (poses [, relo_Pose, ex_pose, td]) / the right-hand side - and TPT: at the LDS carve)
constexpr int TP_NBL = TP_RHS - 16 * (TPT - 1);       // state columns in the last tile column: 11 (+ the right-hand side at local column 11)
static_assert(TP_NBL >= 1 && TP_NBL < 16, "the right-hand side fits the last tile column");
// position n of the elimination order -> column of the assembled system (poses | speed-biases; NF = the right-hand side), TP_PAD for padding
__host__ __device__ constexpr int tp_perm(int n) {
  if (n < 45) return NPOSE + 9 * (10 - n / 9) + n % 9;             // B: frames 10 .. 6
  if (n < 48) return TP_PAD;
  if (n < 93) return NPOSE + 9 * (4 - (n - 48) / 9) + (n - 48) % 9;  // F: frames 4 .. 0
  if (n < TP_M0) return TP_PAD;
  if (n < TP_P0) return NPOSE + 45 + (n - TP_M0);                   // frame 5's block
  if (n < TP_RHS) return n - TP_P0;                                 // poses
  return n == TP_RHS ? NF : TP_PAD;
}

// Where the tiles are loaded from: for a pair of positions the LDS offset (in doubles) of the entry - s_off() of the two columns with the
// prior's speed-bias block at frame 0 (the host sends every other prior to the latency form), the right-hand side for position TP_RHS -,
// TP_NONE for a structural zero, TP_ONE for the diagonal of a padding position: the places of the constants 0.0 and 1.0 (with codes to be masked
// the compiler built a branch per entry: 10 K cycles per factorization).
constexpr int TP_NONE = L_ZERO, TP_ONE = L_ONE;
constexpr int tp_off_c(int Rn, int Cn) {
  const int R = tp_perm(Rn), C = tp_perm(Cn);
  if (R == TP_PAD || C == TP_PAD) return Rn == Cn ? TP_ONE : TP_NONE;
  const int hi = R > C ? R : C, lo = R > C ? C : R;
  if (hi == NF) return lo < NF ? L_RHS + lo : TP_NONE;
  if (hi < NPOSE) return L_S + croff(hi) + lo;
  const int q = hi - NPOSE, b = q / 9;
#ifdef AVM_TP
  if (lo < NPOSE) {
    if (b == 0) return L_STRIP + (q - 9 * b) * NPOSE + lo;
    const int p = lo - 6 * (b - 1);
    return p >= 0 && p < 18 ? L_SBC + q * SBW + p : TP_NONE;
  }
  const int p = lo - (NPOSE + 9 * (b - 1));
  return p >= 0 && p < 18 ? L_SBC + q * SBW + 18 + p : TP_NONE;
#else
  // (latency build: the same structure, the places are those of the packed triangle)
  const int p = lo < NPOSE ? lo - 6 * (b - 1) : lo - (NPOSE + 9 * (b - 1));
  return (lo < NPOSE && b == 0) || (p >= 0 && p < 18) ? L_S + croff(hi) + lo : TP_NONE;
#endif
}

// Tile pattern of the system in elimination order, [k][i] with k <= i: h = the assembled system can be nonzero there (tp_off_c names a place),
// nz = h closed under the fill of the tile-level elimination (which is what the scalar elimination fills, aggregated:
// tests/test_tp_pattern.py states both in numpy).
struct TpPattern {
  bool h[TPT][TPT], nz[TPT][TPT];
};
constexpr TpPattern tp_make_pattern() {
  TpPattern P{};
  for (int k = 0; k < TPT; k++)
    for (int i = k; i < TPT; i++) {
      bool any = false;
      for (int a = 0; a < 16 && !any; a++)
        for (int b = 0; b < 16 && !any; b++) any = tp_off_c(16 * k + a, 16 * i + b) != TP_NONE;
      P.h[k][i] = P.nz[k][i] = any;
    }
  for (int k = 0; k < TPT; k++)
    for (int j = k + 1; j < TPT; j++)
      if (P.nz[k][j])
        for (int i = j; i < TPT; i++)
          if (P.nz[k][i]) P.nz[j][i] = true;
  return P;
}
constexpr TpPattern TPP = tp_make_pattern();
__host__ __device__ constexpr bool tp_nz(int k, int i) { return k <= i && TPP.nz[k][i]; }
// the steps of the factorization: pivot columns {t, 3 + t} for t < 3 (B and F side by side), then one column per step
constexpr int TP_NSTEP = TPT - 3;  // 8 (9)
__host__ __device__ constexpr int tp_step_np(int t) { return t < 3 ? 2 : 1; }
__host__ __device__ constexpr int tp_step_piv(int t, int a) { return t < 3 ? (a == 0 ? t : t + 3) : t + 3; }
__host__ __device__ constexpr int tp_step_of(int k) { return k < 3 ? k : k - 3; }
__host__ __device__ constexpr int tp_slot_of(int k) { return k >= 3 && k < 6 ? 1 : 0; }           // which of its step's pivot columns (the patch it uses)
__host__ __device__ constexpr int tp_buf(int k) { return 2 * (tp_step_of(k) & 1) + tp_slot_of(k); }  // its L^-T buffer: the next step's chains write the other pair
__host__ __device__ constexpr bool tp_is_piv(int t, int q) {  // is q a pivot column of step t ?
  return t >= 0 && t < TP_NSTEP && (tp_step_piv(t, 0) == q || (tp_step_np(t) == 2 && tp_step_piv(t, 1) == q));
}
__host__ __device__ constexpr bool tp_steps_ok() {  // the two pivot columns of a step share no tile, and a column's rows all belong to earlier steps
  for (int t = 0; t < 3; t++)
    if (tp_nz(t, t + 3)) return false;
  for (int i = 0; i < TPT; i++)
    for (int k = 0; k < i; k++)
      if (tp_nz(k, i) && tp_step_of(k) >= tp_step_of(i)) return false;
  return true;
}
static_assert(tp_steps_ok(), "B and F must not meet");
__host__ __device__ constexpr int tp_owner(int i) {
#ifdef AVM_X
  // eight wavefronts: B and F as below, every later column a wavefront of its own (a chain's owner has nothing else in the rows of the step before)
  return i < 3 ? 3 : (i < 6 ? 2 : (i == 6 ? 0 : (i == 7 ? 1 : i - 4)));
#else
  // (build/dev: the assignment that leaves the owner of a step's pivot columns the least other work in the step before)
  return i < 3 ? 3 : (i < 7 ? 2 : (i < 9 ? 0 : (i == 9 ? 3 : 1)));
#endif
}
__host__ __device__ constexpr int tp_ncol(int i) {  // tiles of column i
  int n = 0;
  for (int k = 0; k <= i; k++) n += tp_nz(k, i) ? 1 : 0;
  return n;
}
__host__ __device__ constexpr int tp_idx(int wv, int k, int i) {  // index of tile (k, i) in wavefront wv's array
  int n = 0;
  for (int c = 0; c < i; c++) n += tp_owner(c) == wv ? tp_ncol(c) : 0;
  for (int q = 0; q < k; q++) n += tp_nz(q, i) ? 1 : 0;
  return n;
}
__host__ __device__ constexpr int tp_ntiles(int wv) { return tp_idx(wv, 0, TPT); }
__host__ __device__ constexpr int tp_nrow(int k) {  // tiles of row k beside the diagonal
  int n = 0;
  for (int c = k + 1; c < TPT; c++) n += tp_nz(k, c) ? 1 : 0;
  return n;
}
__host__ __device__ constexpr int tp_wslot(int k, int i) {  // slot of W(k, i) among its step's published tiles
  int n = tp_slot_of(k) == 1 ? tp_nrow(tp_step_piv(tp_step_of(k), 0)) : 0;
  for (int c = k + 1; c < i; c++) n += tp_nz(k, c) ? 1 : 0;
  return n;
}
__host__ __device__ constexpr int tp_max_wslots() {
  int m = 0;
  for (int t = 0; t < TP_NSTEP; t++) {
    int n = 0;
    for (int a = 0; a < tp_step_np(t); a++) n += tp_nrow(tp_step_piv(t, a));
    m = n > m ? n : m;
  }
  return m;
}
static_assert(tp_max_wslots() <= TP_WSLOTS, "the published rows of W fit their LDS slots");
__host__ __device__ constexpr bool tp_row_held(int wv, int k) {  // does wavefront wv hold a tile (k, i), i > k ?
  for (int i = k + 1; i < TPT; i++)
    if (tp_owner(i) == wv && tp_nz(k, i)) return true;
  return false;
}
__host__ __device__ constexpr bool tp_owns_piv(int wv, int t) {  // does wavefront wv own a pivot column of step t ?
  for (int a = 0; t >= 0 && t < TP_NSTEP && a < tp_step_np(t); a++)
    if (tp_owner(tp_step_piv(t, a)) == wv) return true;
  return false;
}
__host__ __device__ constexpr bool tp_owners_ok() {  // a wavefront runs one chain at a time
  for (int t = 0; t < 3; t++)
    if (tp_owner(tp_step_piv(t, 0)) == tp_owner(tp_step_piv(t, 1))) return false;
  return true;
}
static_assert(tp_owners_ok(), "the two chains of a step run on two wavefronts");

AVM_DEV int tp_perm_dev(int n) {
  const int m = n - 48;
  const int b = NPOSE + 9 * 10 - 9 * (n / 9) + n % 9, f = NPOSE + 9 * 4 - 9 * (m / 9) + m % 9;
  return n < 45 ? b : (n < 48 ? TP_PAD : (n < 93 ? f : (n < TP_M0 ? TP_PAD : (n < TP_P0 ? NPOSE + 45 + (n - TP_M0) : (n < TP_RHS ? n - TP_P0 : (n == TP_RHS ? NF : TP_PAD))))));
}

// The offsets as a table in the code object's constant data, evaluated at compile time ([tile][lane][register]: one 8-byte load per lane and
// tile).  The generic form - position -> column, s_off with its division and branches, an LDS read behind each - was 28 K cycles per factorization.
__host__ __device__ constexpr int tp_h_ord(int k, int i) {  // ordinal of tile (k, i) among the tiles with TPP.h, column by column
  int n = 0;
  for (int c = 0; c < TPT; c++)
    for (int q = 0; q <= c; q++) {
      if (c == i && q == k) return n;
      n += TPP.h[q][c] ? 1 : 0;
    }
  return n;
}
constexpr int TP_NH = tp_h_ord(TPT, TPT);
struct TpOffsets {
  unsigned short o[TP_NH][64][4];
};
constexpr TpOffsets tp_make_offsets() {
  TpOffsets t{};
  for (int i = 0; i < TPT; i++)
    for (int k = 0; k <= i; k++)
      if (TPP.h[k][i])
        for (int lane = 0; lane < 64; lane++)
          for (int r = 0; r < 4; r++) t.o[tp_h_ord(k, i)][lane][r] = (unsigned short)tp_off_c(16 * k + (lane >> 4) + 4 * r, 16 * i + (lane & 15));
  return t;
}
__device__ const TpOffsets tp_offsets = tp_make_offsets();
