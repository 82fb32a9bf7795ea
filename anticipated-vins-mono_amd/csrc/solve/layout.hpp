// solve/layout.hpp - limits, the LDS carve of the three builds, the int carve, tuning constants
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
//
// Order: what the three builds share; then ONE block per build (throughput, extended, latency) with that build's workgroup size, staging
// tiles and its map of LDS from L_S up to L_DD, no conditional inside; then the tail of the carve that all three share, the int carve
// and the tuning constants.

constexpr int croff(int i) { return 2 * ((i >> 1) + 1) * ((i >> 1) + (i & 1)); }  // roff() at compile time
constexpr int SROWS = croff(NF + 1);  // padded packed lower triangle of the NF x NF matrix + one augmented row (the RHS): 13944 (16200)
constexpr int VEC = (NCOL + 7) & ~7;  // padded NCOL: 320 (328)
constexpr int XSB = 7 * NFRP, XLAM = XSB + 99;  // state vector: poses (relo_Pose as frame 11) | speedbias 99 | inv depth 150 [| ex_pose 7 | td]

// LDS carve (offsets in doubles).  Everything between L_S + SPP (end of the pose-pose rows of S) and
// L_G is dead while the projection factors are being assembled, so that range doubles as the per-wave
// staging area of the MFMA X^T X products (ASM_WAVES x XSTG doubles).
constexpr int SPP = croff(NPOSE);  // packed rows 0..NPOSE-1 = the dense pose(-like) block: 2244 (3200)
constexpr int WLD = 80;
constexpr int XRS = 132;           // column stride of the frame tasks' column-major staging tile: 128 rows + 4 (bank spread)
// positions of chol_regs' elimination order (see there): [0, 48) B, [48, 96) F, frame 5's speed-bias block, the dense columns, the right-hand side
constexpr int TP_M0 = 96, TP_P0 = 105, TP_RHS = TP_P0 + NPOSE;  // 171 (184)
constexpr int TPT = TP_RHS / 16 + 1;                            // tile columns: 11 (12)
constexpr int TP_NPOS = 16 * TPT;                               // 176 (192)
constexpr int CNB = 16;            // Cholesky panel width (pivot chain per diagonal block); trailing tiles stay 16x16
constexpr int TLAST = NF / 16;     // last 16-row tile of the packed matrix incl. the augmented row NF: 10 (11)
constexpr int FRS = 18 * NFRP;     // one frames slot: R (NFRP x 9) then A = ric^T R^T (NFRP x 9)
constexpr int L_S = 0;
constexpr int TP_PS = 17;         // row stride of the 16 x 16 blocks of the factorization's scratch: lane = row accesses of a stride-16 block put sixteen lanes on two LDS banks

// Latency and extended blocks, from L_RHS to L_ZV: the factorization on register tiles (chol_regs, the throughput build's; latency: on wavefronts 0..3, extended: on all
// eight) reads the packed system once; from then on the range of S is its scratch - same carve as the throughput build's union region, and the
// right-hand side is row NF of S.
#if defined(AVM_TP)
// THROUGHPUT build (window_solve_tp.o, -DAVM_TP): the same minimizer as a 256-thread workgroup (four wavefronts, one per SIMD) with at most
// 80 KB of LDS, so that TWO windows are resident per CU and the dependent chains of one overlap the other's.  What makes it fit:
//   * only the dense pose-pose rows of S (66 packed rows, 18 KB) stay in LDS as they are; the speed-bias rows are kept in their
//     structural form (per 9-row block the 18 pose and 18 speed-bias columns an IMU factor can reach, plus the prior's speed-bias x pose
//     strip), in the range the frame tasks' staging occupies during phase A;
//   * the factorization runs on REGISTER tiles distributed over the four wavefronts (chol_regs below), fed from those two forms;
//   * the frame tasks stage half a chunk (32 factors) at a time.
constexpr int NT = 256;
constexpr int XN = XLAM + MAXE + 2;  // 328
constexpr int XRS_H = 68;          // column stride of the HALF-chunk staging tile: 32 factors x 2 residual rows + 4 (bank spread)
constexpr int XSTG = 13 * XRS_H;   // 884
constexpr int ASM_WAVES = 4;       // every wavefront assembles; wavefront 2 then takes the raw IMU Jacobians, wavefront 3 the prior
constexpr int TP_NWO = 4;          // wavefronts that hold tiles of the factorization
// rows 0..65 of S packed as in the other builds, then the union region U: phase A: 4 staging tiles; from phase D on: the speed-bias
// rows in structural form + the prior's strip; during the factorization: diagonal patch, L_kk^-T (two buffers), the published row of W
constexpr int SBW = 36;                       // compact speed-bias row: 18 pose columns (poses i-1, i, i+1) | 18 speed-bias columns (i-1, i)
constexpr int L_U = L_S + SPP;
constexpr int L_SBC = L_U;                    // [99][SBW]
constexpr int L_STRIP = L_SBC + 99 * SBW;     // [9][66]: rows of the prior's speed-bias block x every pose column
constexpr int USZ = 99 * SBW + 9 * NPOSE + 2; // 4160; its last two doubles hold the constants 0.0 and 1.0 for chol_regs' tile load (set by schur_reduce)
constexpr int L_ZERO = L_U + USZ - 2, L_ONE = L_U + USZ - 1;
static_assert(ASM_WAVES * XSTG <= USZ, "staging fits the union region");
constexpr int L_PATCH = L_U;                  // factorization: [2][16][TP_PS] diagonal blocks of the (up to two) pivot columns of a step in lane = row form
constexpr int L_LINV = L_PATCH + 2 * 16 * TP_PS;  // [4][16][TP_PS]: L_kk^-T (unscaled, see chol_diag_block), 1 / sqrt(pivot) of column r in the padding word of row r (tp_buf)
constexpr int TP_WSLOTS = 9;                  // tiles of a step's rows of W that exist beside the diagonal (tp_wslot: the factor is sparse in the order chol_regs eliminates in)
constexpr int L_WROW = L_LINV + 4 * 16 * TP_PS;      // [TP_WSLOTS][256]: the step's rows of W, the tiles that exist in column order, in the accumulator layout [r][lane]
constexpr int L_PARTV = L_WROW;               // back substitution (the rows of W are dead by then): [4][176] partial sums of the four wavefronts
constexpr int L_ZV = L_WROW + TP_WSLOTS * 256;  // [176] z = L^-1 b, then x, in elimination order (lds[L_Y] keeps the right-hand side until x replaces it, in the system's order)
static_assert(L_ZV + TP_NPOS <= L_ZERO && TP_NWO * TP_NPOS <= TP_WSLOTS * 256, "factorization scratch fits the union region");
static_assert(ASM_WAVES * XSTG <= USZ - 2, "staging leaves the two constants alone");
constexpr int L_Y = L_U + USZ;                // Gauss-Newton solution y; until the solve writes it: the right-hand side (row NF of the other builds)
constexpr int L_RHS = L_Y;
constexpr int WCH_TP = 224;                   // doubles: ys of back_substitute / rvb of jac_times_vec_sq (<= 150), then 64 dump slots
constexpr int L_ST = L_Y + VEC;
constexpr int L_XC = L_ST + VEC;
constexpr int L_WCH = L_XC + XN;
constexpr int L_DUMP = L_WCH + 160;
constexpr int L_G = L_WCH + WCH_TP;
constexpr int L_DD = L_G + VEC;               // (g / D is recomputed where it is needed, as in the extended build)
// Per-wavefront accumulators of the two per-feature sums that end in LDS anyway (E^T E -> lds[L_HEE], E^T r -> lds[L_G + NF]), over the range the
// Gauss-Newton step, the dogleg step and the candidate state occupy between evaluations (all three are dead or parked while eval_jac runs: the
// minimizer recomputes them, and a speculative evaluation parks y in the slot).  Wavefront 0 accumulates in the destinations themselves, wavefronts
// 1..3 in [3][2][152] here; the per-feature sums add the four in a fixed order.  Round 5: every 8 bytes per factor the frame tasks write to the slot
// cost 0.1 ms per 4096 windows (profiles/r05e_experiments.md section 10); these two were sixteen of them.
constexpr int L_ACC = L_Y, ACCW = 152;
static_assert(L_ACC + 6 * ACCW <= L_WCH, "the accumulators stay inside y | step | candidate state");
constexpr int RICW = 20;           // lds[L_RIC]: ric 9, tic 3, current ex_pose 7 (+1 pad)
constexpr int NPRIW = 2;           // wavefronts that share the prior: the second one's dx / J0^T r_p at L_DX2
constexpr int IMUW = 2;            // eval_jac, phase A: the wavefront of the raw IMU Jacobians (every wavefront assembles; wavefronts 2 and 3 get fewer frames and take
                                   // the raw IMU Jacobians and the prior afterwards)
constexpr int NQB = 6;             // eval_jac, phase B: per-factor quantities summed per feature (E^T E and E^T r come out of the frame tasks' accumulators in LDS)
constexpr int PT0 = 160;           // jac_times_vec_sq: first thread of the prior's rows (256 threads: they sit right behind the 150 IMU rows)
constexpr int PBT0 = 160;          // window load: first thread that reads the prior's block table
constexpr int L_GF = L_Y;          // rot_diff / origin_P0 of the gauge fix (the Gauss-Newton step is dead after the loop)
constexpr int LDS_BUDGET = 81920;  // two workgroups per CU: 80 KB each
#elif defined(AVM_X)
// EXTENDED build (window_solve_x.o, -DAVM_X): every optional member of the problem (ex_pose / td / relocalization), 512 threads, one window per CU.
constexpr int NT = 512;          // threads per workgroup (8 wavefronts)
constexpr int XEX = XLAM + MAXE, XTD = XEX + 7;
constexpr int XN = (XTD + 2) & ~1;  // 342
constexpr int WCH = 8;             // rows of the scratch tile at L_WCH (x 80 columns): diag-block temporaries, back-substitution vector
constexpr int XCOLS = 20;          // staged factor row: Jj(6) | Ji(6) | r | Jex(6) | Jtd
constexpr int XRS_X = 68;          // column stride of the HALF-chunk staging tile (round 5): 32 factors x 2 residual rows + 4 (bank spread)
constexpr int XSTG = XCOLS * XRS_X;
constexpr int ASM_WAVES = 7;       // wavefronts assembling projection factors (round 5: seven half-chunk tiles fit where five whole ones did; eleven
                                   // frames deal 2 2 2 2 1 1 1 instead of 3 2 2 2 2, and wavefront 7 takes the raw IMU Jacobians AND the prior)
constexpr int TP_NWO = 8;          // wavefronts that hold tiles of the factorization
constexpr int L_Y = L_S + SROWS;   // Gauss-Newton solution y of (H + mu D^2) y = g
constexpr int L_ST = L_Y + VEC;    // trust region step (scaled space)
constexpr int L_XC = L_ST + VEC;   // candidate state
constexpr int L_WCH = L_XC + XN;   // [WCH][80] scratch tile
constexpr int L_DUMP = L_WCH + 512;     // per-lane dump slots of the masked-out stores
constexpr int L_G = L_WCH + WCH * WLD;  // scaled gradient g (f | e)
constexpr int L_RHS = L_S + croff(NF);
constexpr int L_PATCH = L_S;
constexpr int L_LINV = L_PATCH + 2 * 16 * TP_PS;
constexpr int TP_WSLOTS = 14;
constexpr int L_WROW = L_LINV + 4 * 16 * TP_PS;
constexpr int L_PARTV = L_WROW;
constexpr int L_ZV = L_WROW + TP_WSLOTS * 256;
static_assert(L_ZV + TP_NPOS <= L_S + SROWS && TP_NWO * TP_NPOS <= TP_WSLOTS * 256, "factorization scratch fits the range of S");
constexpr int L_DD = L_G + VEC;    // D   (g / D is recomputed where it is needed: no room for a fourth vector next to the 178 x 178 system)
constexpr int RICW = 24;           // lds[L_RIC]: [2][12]: ric 9, tic 3 of the current point / of the candidate
constexpr int NPRIW = 1;           // the extended build keeps the prior on one wavefront
constexpr int IMUW = ASM_WAVES;    // eval_jac, phase A: the wavefront of the raw IMU Jacobians, the first one that does not assemble
constexpr int NQB = 15;            // eval_jac, phase B: per-factor quantities summed per feature, all NQ of them
constexpr int PT0 = 192;           // jac_times_vec_sq: first thread of the prior's rows
constexpr int PBT0 = 256;          // window load: first thread that reads the prior's block table
constexpr int L_GF = L_Y;          // rot_diff / origin_P0 of the gauge fix (the Gauss-Newton step is dead after the loop)
constexpr int LDS_BUDGET = 163840;
#else
// LATENCY build (window_solve.o): 512 threads, one window per CU.
constexpr int NT = 512;          // threads per workgroup (8 wavefronts)
constexpr int XN = XLAM + MAXE + 2;  // 328
constexpr int WCH = 32;
constexpr int XLD = 14;            // staged factor row: Jj(6) | Ji(6) | r (+1 pad)
constexpr int XSTG = 128 * XLD;    // 64 factors x 2 residual rows (>= 13 * XRS)
static_assert(13 * XRS <= XSTG, "column-major staging tile fits");
constexpr int ASM_WAVES = 6;       // wavefronts assembling projection factors (wavefront 6: the raw IMU Jacobians, 7: the prior)
constexpr int TP_NWO = 4;          // wavefronts that hold tiles of the factorization
constexpr int L_Y = L_S + SROWS;   // Gauss-Newton solution y of (H + mu D^2) y = g
constexpr int L_ST = L_Y + VEC;    // trust region step (scaled space)
constexpr int L_XC = L_ST + VEC;   // candidate state
constexpr int L_WCH = L_XC + XN;   // [WCH][80] scratch tile
constexpr int L_DUMP = L_WCH + 512;     // per-lane dump slots of the masked-out stores
constexpr int L_G = L_WCH + WCH * WLD;  // scaled gradient g (f | e)
constexpr int L_RHS = L_S + croff(NF);
constexpr int L_PATCH = L_S;
constexpr int L_LINV = L_PATCH + 2 * 16 * TP_PS;
constexpr int TP_WSLOTS = 9;
constexpr int L_WROW = L_LINV + 4 * 16 * TP_PS;
constexpr int L_PARTV = L_WROW;
constexpr int L_ZV = L_WROW + TP_WSLOTS * 256;
static_assert(L_ZV + TP_NPOS <= L_S + SROWS && TP_NWO * TP_NPOS <= TP_WSLOTS * 256, "factorization scratch fits the range of S");
constexpr int L_DG = L_G + VEC;    // g / D
constexpr int L_DD = L_DG + VEC;   // D
constexpr int RICW = 20;           // lds[L_RIC]: ric 9, tic 3, current ex_pose 7 (+1 pad)
constexpr int NPRIW = 2;           // wavefronts that share the prior: the second one's dx / J0^T r_p at L_DX2
constexpr int IMUW = ASM_WAVES;    // eval_jac, phase A: the wavefront of the raw IMU Jacobians, the first one that does not assemble
constexpr int NQB = 8;             // eval_jac, phase B: per-factor quantities summed per feature, all NQ of them
constexpr int PT0 = 192;           // jac_times_vec_sq: first thread of the prior's rows
constexpr int PBT0 = 256;          // window load: first thread that reads the prior's block table
constexpr int L_GF = L_DG;         // rot_diff / origin_P0 of the gauge fix (g / D is dead after the loop)
constexpr int LDS_BUDGET = 163840;
#endif

// the tail all three builds share
constexpr int ST_XE = 152;         // schur_reduce: f_e at lds[L_ST + e] and x_e beside it at lds[L_ST + ST_XE + e] (L_ST is dead during the Schur update)
static_assert(MAXE + 2 <= ST_XE && 2 * ST_XE <= VEC, "f_e and x_e (MAXE + 2 each, the tiles' clamp included) share the step vector");
constexpr int L_SC = L_DD + VEC;   // Jacobi scaling
constexpr int L_X = L_SC + VEC;
constexpr int L_FR = L_X + XN;     // [2][FRS]
constexpr int L_RIC = L_FR + 2 * FRS;
constexpr int L_HEE = L_RIC + RICW;    // E^T E (150) padded
constexpr int L_DXP = L_HEE + 152;
constexpr int L_RP = L_DXP + MAXPRIOR;
constexpr int L_DX2 = NPRIW == 2 ? L_RP + MAXPRIOR : L_DXP;
constexpr int L_RED = L_RP + NPRIW * MAXPRIOR;
constexpr int L_RED_B = L_RED + 16, L_RED_CNT = L_RED + 32;  // second value of a paired reduction; the wavefronts' reduction counters (8 ints)
constexpr int L_INT = L_RED + 36;  // int region (as doubles): 360 doubles = 720 ints
constexpr int L_SUM = L_INT + 360;  // cost_trace[16], radius_trace[16]
constexpr int L_CTX = L_SUM + 32;   // WinCtx of the window being solved (32 doubles)
constexpr int L_OPT = L_CTX + 32;   // avm_options (copied from the kernel arguments)
constexpr int L_END = L_OPT + (int)((sizeof(avm_options) + 7) / 8);
static_assert(L_END * 8 <= LDS_BUDGET, "LDS budget exceeded (throughput build: two workgroups per CU, 80 KB each; the others: one CU's 160 KB)");
static_assert(L_S + SPP + ASM_WAVES * XSTG <= L_G, "assembly staging overlaps live data");
// int carve (offsets in ints from L_INT)
constexpr int I_FSTART = 0, I_FNOBS = 150, I_FOBS = 300, I_PIDX = 450, I_FS = 546, I_PBLK = 560 /* kind,frame,off x16 */, I_FAIL = 620,
              I_NCOV = 624 /* [12] factors observed in frame b */, I_FRW = 636 /* [12] assembling wave of frame b */,
              I_PMASK = 648 /* [12] start frames flushed by frame b */, I_TIMEUP = 660 /* max_solver_time reached (set by thread 0) */,
              I_NRUN = 661 /* [12] distinct start frames among the factors observed in frame b */,
              I_PSB = 673 /* throughput build: frame of the prior's speed-bias block (its rows x every pose column: the strip) */,
              I_CNT = 674 /* wavefronts x rows of W published so far in this factorization (chol_regs) */,
              I_CRFIT = 675 /* latency build: the window's prior fits the sparse factorization (chol_regs), else cholesky_lds */, I_END = 676;
static_assert(I_END <= 720, "int carve");
#ifndef AVM_TP
constexpr int L_ZERO = L_INT + 340, L_ONE = L_INT + 341;  // the constants 0.0 and 1.0 of chol_regs' tile load, in the unused tail of the int carve (set by schur_reduce)
static_assert(2 * 340 >= I_END, "the constants sit behind the int carve");
#endif

// Issue priority of the calling wavefront (throughput build only).  Two windows share every SIMD there, one wavefront each: while one
// of them streams MFMAs / factor arithmetic (the frame tasks, the Schur tiles, the trailing updates of the factorization: AVM_PRIO_BULK)
// and the other walks a dependent chain or one of the short barrier-separated vector phases of the trust-region loop (AVM_PRIO_LIGHT),
// the arbiter should hand the next free issue slot to the latter - its instructions are the window's critical path, the bulk work
// fills whatever is left.  (The pivot chains have run at priority 3 since round 4.)
// Settled tuning constants (each was a -D knob while it was being measured)
constexpr int PRIO_LIGHT = 2;       // dependent chains and the short vector phases of the trust-region loop
constexpr int PRIO_CHOL = 1;        // trailing updates of the factorization (the pivot chains themselves run at 3)
constexpr int PRIO_SCHUR = 1;       // Schur tiles
constexpr int LPT_RUNW = 16;        // frame deal of the solve kernel: what one more distinct start frame among a frame's factors weighs, in factors
constexpr int TP_WIMU = 60, TP_WPRI = 300;  // throughput frame deal: the raw IMU Jacobians' and the prior's weight, in factors (see the deal in the solve kernel)
#ifdef AVM_TP
#define AVM_PRIO_BULK() __builtin_amdgcn_s_setprio(0)
#define AVM_PRIO_BULK_CHOL() __builtin_amdgcn_s_setprio(PRIO_CHOL)
#define AVM_PRIO_BULK_SCHUR() __builtin_amdgcn_s_setprio(PRIO_SCHUR)
#define AVM_PRIO_LIGHT() __builtin_amdgcn_s_setprio(PRIO_LIGHT)
#else
#define AVM_PRIO_BULK() ((void)0)
#define AVM_PRIO_BULK_CHOL() ((void)0)
#define AVM_PRIO_BULK_SCHUR() ((void)0)
#define AVM_PRIO_LIGHT() ((void)0)
#endif
