// window_solve.hip — Estimator::optimization() for a batch of independent sliding windows
// on gfx950, one 512-thread workgroup per window, the whole trust-region loop on device.
//
// What it replaces (reference, all CPU):
//   problem assembly            vins_estimator/src/estimator.cpp:663-755
//   ceres::Solve (DENSE_SCHUR + DOGLEG, <= 8 iterations)          estimator.cpp:794-809
//     = per-factor Evaluate     factor/imu_factor.h:19-179, factor/projection_factor.cpp:21-121,
//                               factor/marginalization_factor.cpp:333-381
//     + CauchyLoss/Corrector    (Ceres; in-tree copy factor/marginalization_factor.cpp:37-68)
//     + Jacobi scaling, J^T J, Schur elimination of the inverse depths, dense Cholesky,
//       traditional dogleg, step acceptance                       (Ceres 1.14)
//   double2vector + vector2double gauge fix                       estimator.cpp:477-587
//
// Data placement (solve/layout.hpp has the map, DESIGN.md §2.2 the reasons): the reduced 165x165 system lives in LDS for the
// whole solve - row-packed lower triangle, rows padded to even length, the right-hand side as an augmented row 165: 13944
// doubles = 111 KB (the throughput build keeps the 66 pose rows packed and the speed-bias rows in structural form) - together
// with the states, gradient, dogleg vectors, Jacobi scaling, per-frame rotation blocks, E^T E, the prior's dx / residual, the
// window's context and the options: about 162.5 KB of the CU's 160 KiB, one workgroup per CU (throughput build: <= 80 KB, two).
// The range between the pose-pose rows of S and the live vectors is dead while the projection factors are assembled and is the
// wavefronts' MFMA staging area.  E^T F and the per-factor products (feature-major: Wt[column][feature],
// PFt[quantity][frame][feature]), the partial Ji^T Ji blocks, the raw IMU Jacobians and the prior's packed J0^T J0 are streamed
// through a per-workgroup global scratch slot that stays L2 / Infinity Cache resident.
// All arithmetic FP64.  Every reduction has a fixed order, so results are bit-reproducible
// run to run and independent of how windows are sharded over ranks.
//
// csrc/Makefile compiles this file three ways:
//   window_solve.o      latency build: 512 threads and the whole CU's LDS per window, the reference's default problem;
//                       also marginalize_kernel and eval_factors_kernel
//   window_solve_x.o    -DAVM_X, extended build: the same with ex_pose / td / relo_Pose as variables (178 x 178 system); the solve only
//   window_solve_tp.o   -DAVM_TP, throughput build: 256 threads and <= 80 KB of LDS, two windows per CU; solve and marginalization
//   window_solve_mm.o, window_solve_tp_mm.o   -DAVM_MARG_MIXED [-DAVM_TP]: the marginalization kernel of the latency / throughput build once
//                       more, with the marginalization flag per window (solve/marg_kernel.hpp); no solve kernel
//   window_solve_list.o, window_solve_x_list.o, window_solve_tp_list.o   -DAVM_WIN_LIST [-DAVM_X | -DAVM_TP]: the solve kernel of each of the three
//                       builds once more over a list of windows (solve/solve_kernel.hpp); nothing else
// This file is the table of contents: every function and kernel is in a part under solve/, included below in DEFINITION ORDER, which
// is the order the compiler emits the functions in - moving an include moves code.  A part that all three builds share carries their
// differences inside its functions under #ifdef AVM_X / AVM_TP; a part that only some builds have sits behind a conditional include
// here.  solve/layout.hpp (included by solve/lds.hpp) has each build's map of LDS and the constants that are a plain number per build.
#include <cfloat>
#include <utility>

#include "devmath.hpp"
#include "kernels.hpp"

namespace avm {

extern __shared__ __attribute__((aligned(16))) char avm_smem[];

namespace {

#include "solve/lds.hpp"              // LDS(), the profiling stopwatches, layout.hpp, workgroup reductions, roff / s_off
#include "solve/factors.hpp"          // proj_eval, imu_raw, imu_col, prior_block_dx: the factors, one thread each
#include "solve/context.hpp"          // address-space typedefs, WinCtx and the options in LDS, build_frames, ric_of, td_shift
#include "solve/prior_residual.hpp"   // prior_residual_dev, prior_wave
#include "solve/eval_cost.hpp"        // eval_cost: residual-only cost of a candidate state
#include "solve/slot.hpp"             // the map of the scratch slot: Wt / PFt, the PART rows, the raw IMU blocks, the HP region
#include "solve/prior_jtj.hpp"        // prior_jtj_add_lds, prior_jtj_packed
#ifndef AVM_X
#include "solve/frame_task.hpp"       // frame_task: a wavefront's projection factors -> X^T X on the matrix cores
#else
#include "solve/frame_task_x.hpp"     // ... with every optional member of the problem
#endif
#include "solve/imu_mfma.hpp"         // ImuOperands, imu_factor_load, imu_factor_mfma: one IMU factor on the matrix cores
#include "solve/eval_jac.hpp"         // eval_jac: the full evaluation, phases A to E
#include "solve/jac_times_vec.hpp"    // jac_times_vec_sq (the Cauchy point's |J' u|^2)
#include "solve/chol_regs_tables.hpp" // chol_regs' elimination order and compile-time tables (tests/test_tp_pattern.py states them in numpy)
#include "solve/chol_regs.hpp"        // chol_regs<WV>: the factorization on register tiles, both triangular solves; tp_pattern_export
#ifndef AVM_TP  // the other builds (the latency build: for a prior chol_regs' pattern does not hold)
#include "solve/cholesky_lds.hpp"     // left-looking factorization of the packed system in LDS and its solve
#endif
#include "solve/schur.hpp"            // mfma4, schur_macro_tile, [schur_strip4.hpp,] schur_reduce
#include "solve/step.hpp"             // back_substitute, scale_system, state_plus

}  // namespace

#ifndef AVM_MARG_MIXED
#include "solve/gauge.hpp"            // gauge_rot_diff: rot_diff / origin_P0 of the gauge fix
#include "solve/solve_kernel.hpp"     // the kernel: load, frame deal, TrustRegionMinimizer, gauge fix
#endif

#if !defined(AVM_X) && !defined(AVM_WIN_LIST)  // marginalization: latency and throughput builds
#include "solve/marg_layout.hpp"        // what the marginalization computes, its map of LDS (namespace mg), mg_col
#include "solve/marg_imu0.hpp"          // marg_imu0_raw, marg_prior_wave (phase A beside the frame tasks), marg_imu0_gram (phase D)
#include "solve/marg_feature_sums.hpp"  // marg_feature_sums: phase B, the per-feature sums
#include "solve/marg_schur.hpp"         // marg_schur_macro_tile, marg_schur_phase: phase F, the start-0 inverse depths eliminated
#include "solve/marg_frame_task.hpp"    // marg_frame_task: phase A, a wavefront's projection factors -> X^T X on the matrix cores
#include "solve/jacobi_eig_lds.hpp"     // jacobi_eig_lds<NTH>: cyclic Jacobi eigen-decomposition in LDS
#include "solve/pinv16.hpp"             // pinv16_cholesky: the 16 x 16 pseudo-inverse when no eigenvalue is clamped
#include "solve/marg_kernel.hpp"        // the marginalization kernel: one function, phases A to G and the output
#endif

#if defined(AVM_WIN_LIST)  // each build's launchers and test exports
#include "solve/launch_list.hpp"
#elif defined(AVM_MARG_MIXED)
#include "solve/launch_mm.hpp"
#elif defined(AVM_TP)
#include "solve/launch_tp.hpp"
#elif defined(AVM_X)
#include "solve/launch_x.hpp"
#else
#include "solve/eval_factors_kernel.hpp"  // per-factor evaluation kernel (parity-test surface)
#include "solve/launch.hpp"
#endif

}  // namespace avm
