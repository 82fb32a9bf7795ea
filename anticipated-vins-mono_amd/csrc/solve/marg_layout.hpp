// solve/marg_layout.hpp - marginalization: what it computes, its LDS layout (namespace mg), mg_col
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
// =====================================================================================
// Post-solve marginalization: MarginalizationInfo::addResidualBlockInfo / preMarginalize /
// marginalize / getParameterBlocks (vins_estimator/src/factor/marginalization_factor.cpp:89-319)
// as driven by Estimator::optimization() (estimator.cpp:817-990), one workgroup per window.
//
// Variable layout of the joint system: poses 0..65 | speed-bias 66..164 | ex_pose 165..170 (171 dims,
// packed lower triangle in LDS).  Factors: old prior, IMU factor 0, every projection factor of the
// features that start in frame 0 (with their ex_pose Jacobians) — assembled with the same MFMA X^T X
// scheme as the solve (X row = Jj | Ji | r | Jex).  The inverse depths of those features are
// eliminated first as scalar pivots (they are mutually independent; identical to the reference's joint
// eigen-pseudo-inverse of Amm whenever no eigenvalue is clamped), then pose0/speedbias0 through the
// eigen-decomposition of their 15x15 block with the reference's 1e-8 clamp, and the kept block is
// square-rooted through a second eigen-decomposition (parallel cyclic Jacobi in LDS).
// Deterministic block order (the reference's is address-hash order): kept = poses by frame,
// speed-bias by frame, ex_pose.
namespace mg {
constexpr int MXRS = 68;                              // rows per staged column: HALF a chunk (32 factors x 2 residual rows) + 4 (bank spread)
constexpr int MXSTG = 20 * MXRS;                      // column-major staging tile: Jj 0-5 | Ji 6-11 | r 12 | Jex 13-18 | Jtd 19
#ifdef AVM_TP
// THROUGHPUT form of the marginalization (marginalize_tp_kernel in window_solve_tp.o, round 5): the same phases as a 256-thread
// workgroup inside the throughput build's 80 KB of LDS, so that TWO windows are resident per CU - the kernel is a sequence of short
// latency-bound phases (62 % of its wavefront cycles waiting), and a second window fills them.  What makes it fit: the joint system
// only holds the variables a marginalization can touch - poses | speed-bias 0, 1 | ex_pose | td = 91 instead of 172 (packed 33 KB
// instead of 117): IMU factor 0 reaches speed-biases 0 and 1, the projection factors the poses and ex_pose / td, and the old prior
// whatever it kept last time, which for a prior the reference can build is a subset of these (estimator.cpp:904-916 keeps
// para_SpeedBias[1], shifted to frame 0).  A prior with a speed-bias block of a later frame takes the other kernel (the host checks:
// window_prior_fits_marg_tp).  Speed-biases 0 and 1 keep their indices (66 .. 83), so imu_col() and SB0 + 9 fr hold unchanged.
constexpr int MEX0 = 84, MTD = 90, MVARS = 91;
constexpr int MASM = 4;                               // every wavefront assembles (frames 1 8 9 | 2 7 10 | 3 6 + raw IMU, prior | 4 5 + prior)
#else
constexpr int MEX0 = 165, MTD = 171, MVARS = 172;     // 172 variables: poses | speed-biases | ex_pose | td
constexpr int MASM = 7;                               // assembling wavefronts (staging must stay below row 165: half tiles let seven fit)
#endif
constexpr int MROWS = croff(MVARS);
#ifdef AVM_TP
// LDS of the throughput form: S (4232) | EA EV EB / IMU factor rows (2048) | T (1536) | g_e (152) ... b in the scaling vector's place;
// the staging tiles of phase A lie over everything from row 66 of S to 7684, all of it written after phase A only
constexpr int M_WCH = MROWS;                          // Amm, its eigenvectors / inverse factor, Arm (n x 16); before: the IMU factor's rows
constexpr int M_GT = M_WCH + 2048;                    // T = Arm Amm^+ (n x 16)
constexpr int M_GE = M_GT + 96 * 16;                  // g_e (152)
constexpr int M_G = L_SC;                             // b over the 91 variables (the Jacobi scaling is the solve's)
static_assert(M_GE + 152 <= M_G && MVARS <= VEC && M_G + VEC <= L_X, "marg layout (throughput form)");
static_assert(L_S + SPP + MASM * MXSTG <= M_G, "marg staging must not reach b");
#else
constexpr int M_G = MROWS;                            // b over the 171 variables (176)
constexpr int M_GE = M_G + 176;                       // g_e (152)
constexpr int M_WCH = M_GE + 152;                     // [24][80] Schur staging / IMU factor rows
constexpr int M_GT = L_G;                             // T = Arm Amm^+ in the range of the solve's gradient / scaling vectors (unused here)
constexpr int MWCH = 24;
static_assert(M_WCH + MWCH * WLD <= L_G, "marg layout");
static_assert(SPP + MASM * MXSTG <= 13778, "marg staging must not reach the ex_pose rows (roff(165))");
#endif
}  // namespace mg

// column of the joint system for W column c (0..71): poses, then ex_pose
AVM_DEV int mg_col(int c) { return c < NPOSE ? c : mg::MEX0 + (c - NPOSE); }  // (td: W column 72 -> variable 171)
