// fsel.hip — FeatureSelector::select() (initialized branch) for a batch of frames on gfx950.
//
// reference: vins_estimator/src/feature_selector.cpp
//   calcInfoFromRobotMotion :463-527, createLinearImuMatrices :531-598, addOmegaPrior :602-609,
//   calcInfoFromFeatures :239-365 (+ inFOV :369-376, findNNDepth :437-459, PinholeCamera
//   spaceToPlane/distortion camera_model/src/camera_models/PinholeCamera.cc:520-542,646-662),
//   selectInformativeFeatures :613-686, sortedlogDetUB :690-728, Utility::logdet utility.h:144-167.
//
// MI355X mapping.  Delta_ell only touches the 3H position rows of horizon states 1..H
// (feature_selector.cpp:349-355), while Omega's other 6H+9 rows never change during a
// select() call.  So the Cholesky pivots of those rows are hoisted: setup eliminates them once
// per frame (partial Cholesky in LDS) leaving C0 = Omega_pp - Omega_pn Omega_nn^-1 Omega_np and
// logdet(Omega_nn); every candidate evaluation logdet(Omega + OmegaS + p*Delta) is then
// logdet(Omega_nn) + logdet(C + p*Delta_pp) with a 3H x 3H factorisation held entirely in
// registers (four candidates per wavefront, one per 16-lane DPP row; one launch per greedy round).
// This is the same Cholesky with the constant leading pivots factored once — the same kind of
// hoist as IMUFactor's sqrt_info.  All FP64; selection order is deterministic.
// This file is the table of contents: every function and kernel is in a part under fsel/, included below in DEFINITION ORDER, which is
// the order the compiler emits the kernels in - moving an include moves code (scripts/isa_same.py tells).  fsel/dpp.hpp comes before
// fsel/kdtree.hpp because the kd-tree's reductions use its lane exchanges; everything in it is inlined.
#include <algorithm>
#include <type_traits>
#include <cfloat>
#include <cstdlib>

#include "devmath.hpp"
#include "kernels.hpp"

namespace avm {

namespace {

#include "fsel/args.hpp"           // FS_NT, FS_CPW, FS_TABLES_GUARD, FselDev: the argument block of every kernel
#include "fsel/dpp.hpp"            // fs_rowbcast_k, fs_dpp_fence, fs_fmac_bcast, fs_row_sum, fs_wave_max
#include "fsel/kdtree.hpp"         // findNNDepth: KdNode, fsel_kdtree_kernel (nanoflann's build), kd_depth (its search, stackless)
#include "fsel/feature_delta.hpp"  // feature_front, feature_front4, feature_pair, feature_delta: Delta_ell of one feature
#include "fsel/setup_kernel.hpp"   // slerp_eigen, fsel_setup_kernel: Omega, its partial Cholesky, every feature's Delta
#include "fsel/pick.hpp"           // FS_CPWG, FselPar / fsel_par (the double-buffered round state), fsel_pick_local, fsel_pick_frame
#include "fsel/logdet4.hpp"        // fs_log, fsel_logdet4 (four candidates per wavefront, LDL^T in registers), fsel_ub4
#include "fsel/round_kernel.hpp"   // fsel_round_kernel: one launch per greedy round; fsel_live_init_kernel
#include "fsel/frame_kernel.hpp"   // fsel_frame_kernel / _mf: all rounds of a frame in one launch, a team of workgroups per frame
#include "fsel/solo_kernel.hpp"    // fsel_solo_kernel: one workgroup per frame, lazy evaluation

}  // namespace

#include "fsel/launch.hpp"         // LDS sizes, the table of instantiated sizes, launch_fsel (host only)
#include "fsel/aux_kernels.hpp"    // horizon from the IMU, depth cloud, findNNDepth parity surface: kernels and launchers

}  // namespace avm
