// select_image.hpp — avm_fsel_select_image_batch: the argument block and the launchers of its three kernels (tracks.hip), shared with the
// host C-ABI layer (avm_api.hip).  They are declared here and not in kernels.hpp: kernels.hpp is one of the sources the committed
// rocprof summary is tied to (bench.py, kernel_source_sha256), and nothing here is seen by a kernel that summary measures.
#pragma once
#include "kernels.hpp"

namespace avm {

struct SelectImageArgs {
  avm_image_batch image;       // in
  const double* prob;          // [B][image.max_pts]
  const int32_t* initialized;  // [B], or null: every window is initialized
  int init_thresh, prune_lost;
  avm_select_state state;      // in; written by select_merge_kernel only
  avm_fsel_batch problem;      // n_cand, cand_*, n_used, used_* are written by select_split_kernel
  avm_fsel_out out;            // the selection's result, read by select_merge_kernel
  avm_image_batch image_out;   // written by select_merge_kernel
};

// The rules of select_image_check_kernel; first_bad as in the other checks of tracks.hip: min over the failing windows of (window * 8 + rule)
enum { SEL_BAD_NPTS = 1, SEL_BAD_IDS = 2, SEL_BAD_NTRACKED = 3, SEL_CAP_CAND = 4, SEL_CAP_USED = 5, SEL_CAP_IMAGE = 6, SEL_CAP_TRACKED = 7 };

hipError_t launch_select_image_check(const SelectImageArgs& a, int* first_bad, hipStream_t stream);
hipError_t launch_select_split(const SelectImageArgs& a, hipStream_t stream);
hipError_t launch_select_merge(const SelectImageArgs& a, hipStream_t stream);

}  // namespace avm
