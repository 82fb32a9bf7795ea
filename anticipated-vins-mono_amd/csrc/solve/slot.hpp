// solve/slot.hpp - the map of the per-workgroup global scratch slot: what lies inside each region of kernels.hpp's Scratch, for the solve and the marginalization
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.
//
// kernels.hpp's Scratch has the regions (PF | PART | IJRAW | W | HP) and their sizes, because the host sizes the slots from them.  Every
// index INTO a region is named here, once, for the three builds of the solve and for the marginalization, which share the slots; the
// static_asserts at the end hold every layout of every build against its region.
//
// ---- W and PF: the per-factor products, feature-major.  The FEATURE index runs fastest, so the frame tasks (lane = feature) write, and
// the per-feature sums / Schur tiles / back substitution read, whole lines:
//   Wt [columns][WLE]         E^T F transposed: Wt[c][e] = (E^T F)[e][c]; NPOSE columns in the solve, MNW in the marginalization
//   PFt[quantity][frame][WLE] per (quantity q, observing frame b, feature e) the factor's product with Je; NQ quantities x NFRP frames in
//                             the solve, PQ_JTD + 1 quantities x NFR frames in the marginalization (these features start in frame 0)
// WLE leaves room for the 8-feature granularity of the Schur tiles' operand loads (150 features -> 152).
constexpr int WLE = 152;
constexpr int PQ_JI = 0;    // .. 5: Ji^T Je (q < 3, Ji_t^T Je, is minus the observing frame's Wt entry and is not stored: the sums read it out of Wt)
constexpr int PQ_HEE = 6;   // Je^T Je
constexpr int PQ_GE = 7;    // Je^T r
constexpr int PQ_JEX = 8;   // .. 13: Jex^T Je (extended build, marginalization)
constexpr int PQ_JTD = 14;  // Jtd^T Je (extended build, marginalization)
#ifdef AVM_X
constexpr int NQ = PQ_JTD + 1;  // 15 per-factor quantities
#else
constexpr int NQ = PQ_JEX;      // 8: the latency and throughput builds of the solve stop in front of Jex^T Je
#endif
static_assert(NQB == NQ || NQB == 6, "eval_jac's phase B sums every per-factor quantity, or (throughput build) the first six");
// (What follows for the marginalization - MPF2, MNW, the MP_* row, PARTW - is defined in the extended build too, which has no marginalization, on purpose:
//  the slots are shared, so its layouts are held against the regions in every build.)
// The marginalization reads its quantities from PQ_JEX on as a table of its own ([7][NFR][WLE]: Jex^T Je (6), Jtd^T Je), at this offset in PF:
constexpr size_t MPF2 = (size_t)PQ_JEX * NFR * WLE;
constexpr int MNW = 73;     // columns of Wt in the marginalization: 66 pose | 6 ex_pose | 1 td

// ---- PART: the partial blocks the frame tasks own, summed per start frame / per variable in a fixed order afterwards.
// The solve: one row per (observing frame b, start frame a), PART[(b * NFR + a) * SPARTW + ..]
constexpr int SP_AA = 0;    // Ji^T Ji, packed lower triangle (21)
constexpr int SP_GA = 21;   // Ji^T r (6)
constexpr int SP_XA = 27;   // [Jex; Jtd]^T Ji (7 x 6), extended build only
#ifdef AVM_X
constexpr int SPARTW = SP_XA + 42;  // 69
constexpr int PARTX = 35;   // then one row per frame b: [Jex; Jtd]^T [Jex; Jtd] lower (28) | [Jex; Jtd]^T r (7)
constexpr int PARTX0 = NFRP * NFR * SPARTW;
static_assert(PARTX0 + NFRP * PARTX <= Scratch::PART_N, "partial blocks fit the PART region");
#else
constexpr int SPARTW = SP_XA;       // 27
static_assert(NFR * NFR * SPARTW <= Scratch::PART_N, "partial blocks fit the PART region");
#endif
// The marginalization: one row per observing frame b (the start frame is 0), PART[b * PARTW + ..]; written by marg_frame_task's end_frame, read by
// phase B of the kernel
constexpr int MP_AA = 0;    // Ji^T Ji of pose 0, packed lower triangle (21)
constexpr int MP_GA = 21;   // Ji^T r: g of pose 0 (6)
constexpr int MP_XA = 27;   // [Jex; Jtd]^T Ji: [ex td] x pose 0 (7 x 6)
constexpr int MP_XX = 69;   // [Jex; Jtd]^T [Jex; Jtd], packed lower triangle (28)
constexpr int MP_GX = 97;   // [Jex; Jtd]^T r: g of [ex td] (7)
constexpr int MP_XB = 104;  // [Jex; Jtd]^T Jj: [ex td] x pose b (7 x 6)
constexpr int PARTW = 146;

// ---- IJRAW: per IMU factor i the residual and Jacobian before sqrt_info, [15][31] (column 0 = residual, 1..30 = Jacobian) at IJRAW + i * IJBLK
constexpr int IJBLK = 15 * 31;  // 465

// ---- HP: the prior's J0^T J0, lower triangle packed by idx = p (p + 1) / 2 + q (HPK_MAX doubles), then every entry's destination inside the packed S
// (HPK_MAX ints); behind them, at HP_SPEC, what a speculative evaluation parks: the current point (XN) and the Gauss-Newton step (VEC)
constexpr int HPK_MAX = MAXPRIOR * (MAXPRIOR + 1) / 2;  // 4656
constexpr int HP_SPEC = HPK_MAX + HPK_MAX / 2 + 8;

static_assert(MAXE <= WLE && WLE % 8 == 0, "a column of Wt holds every feature, in whole 8-feature groups");
static_assert(NPOSE * WLE <= Scratch::W_N && NQ * NFRP * WLE <= Scratch::PF_N, "transposed layouts fit the W / PF regions");
static_assert(MNW * WLE <= Scratch::W_N && (PQ_JTD + 1) * NFR * WLE <= Scratch::PF_N && NFR * PARTW <= Scratch::PART_N, "the marginalization's layouts fit the W / PF / PART regions");
static_assert((NFR - 1) * IJBLK <= Scratch::IJRAW_N, "raw IMU blocks fit the IJRAW region");
static_assert(HPK_MAX + HPK_MAX / 2 <= Scratch::HP_N, "packed Hp + destinations fit the HP scratch region");
static_assert(HP_SPEC + XN + VEC <= Scratch::HP_N, "speculation backup fits the slot");
