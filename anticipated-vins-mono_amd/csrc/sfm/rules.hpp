// sfm/rules.hpp - the table check of avm_global_sfm_batch: one rule function per unit (a stream's scalars, one frame of a stream), run
// on the host for AVM_MEM_HOST tables and by validate_sfm_kernel for device-resident ones.  No HIP in here: a host program compiles it
// with -DSFM_HD=inline.
#pragma once
#include "../../../include/avm_init.h"

#ifndef SFM_HD
#define SFM_HD __host__ __device__ inline
#endif

namespace avm {
enum { BAD_SFM_L = 1, BAD_SFM_FRAMES = 2, BAD_SFM_KEYS = 3, BAD_SFM_NPTS = 4, BAD_SFM_IDS = 5 };

// 0 = fine; otherwise the first violated rule among the scalars and key_index of stream b
SFM_HD int check_sfm_stream(const avm_sfm_batch& s, int b) {
  if (s.l[b] < 0 || s.l[b] > 9) return BAD_SFM_L;
  const int F = s.n_frames[b];
  if (F < 11 || F > s.max_frames) return BAD_SFM_FRAMES;
  for (int i = 0; i < 11; i++) {
    const int k = s.key_index[(size_t)b * 11 + i];
    if (k < 0 || k >= F || (i > 0 && k <= s.key_index[(size_t)b * 11 + i - 1])) return BAD_SFM_KEYS;
  }
  return 0;
}
// ... of frame k of stream b (frames at and beyond n_frames are never read: fine)
SFM_HD int check_sfm_frame(const avm_sfm_batch& s, int b, int k) {
  if (k >= s.n_frames[b]) return 0;
  const int n = s.frame_n_pts[(size_t)b * s.max_frames + k];
  if (n < 0 || n > s.max_pts) return BAD_SFM_NPTS;
  const int32_t* id = s.frame_pt_id + ((size_t)b * s.max_frames + k) * s.max_pts;
  for (int i = 1; i < n; i++)
    if (id[i] <= id[i - 1]) return BAD_SFM_IDS;
  return 0;
}
// the whole stream, as the host runs it: the lowest rule number over its units (what atomicMin leaves on the device)
SFM_HD int check_sfm_tables(const avm_sfm_batch& s, int b) {
  int rule = check_sfm_stream(s, b);
  const int F = s.n_frames[b] < s.max_frames ? s.n_frames[b] : s.max_frames;
  for (int k = 0; k < F; k++) {
    const int r = check_sfm_frame(s, b, k);
    if (r && (!rule || r < rule)) rule = r;
  }
  return rule;
}
}  // namespace avm
