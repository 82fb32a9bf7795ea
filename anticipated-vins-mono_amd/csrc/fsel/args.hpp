// fsel/args.hpp - FS_NT, FS_CPW, the table-validation guard, FselDev: the argument block of every selector kernel
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

constexpr int FS_NT = 256;
constexpr int FS_CPW = 4;  // candidates per wavefront in the Delta slices of the setup kernel
constexpr int FS_TABLES_OK = 0x7f7f7f7f;  // (what launch_validate_fsel leaves in the flag when every frame passes)
#define FS_TABLES_GUARD(A) if ((A).vflag && *(A).vflag != FS_TABLES_OK) return

struct FselDev {
  avm_fsel_batch b;  // device pointers
  int no_key_rule;   // test switch (AVM_FSEL_NO_KEY_RULE=1): skip the std::map equal-key rule of sortedlogDetUB
  int lazy_stats;    // development (AVM_FSEL_LAZY_STATS=1): workgroup 0 of fsel_solo_kernel leaves its counters and phase clocks in sync[32..]
  double lazy_tau;   // fsel_solo_kernel: a candidate is scored in a round's first pass when its gain bound reaches lazy_tau x the last winner's gain
  const int* vflag;  // result of the table validation that runs ahead on the same stream (null: already checked by the host): any
                     // value but FS_TABLES_OK means a malformed table - no kernel of the select may index with the tables then
  // work buffers
  double* C;        // [P][T*T] current reduced position information (C0 + used + OmegaS)
  double* dpp;      // [P][T]   un-reduced diagonal of the position rows (for the Hadamard bound)
  double* consts;   // [P][4]   ld_nn, Kn
  double* delta;    // [P][max_cand][T*T]
  double* delta_pk; // [P][max_cand][T(T+1)/2] the same, lower triangle by columns (entry (R, c), c <= R, at c T - c (c - 1) / 2 + R - c): what
                    // fsel_solo_kernel scores from - half the bytes per evaluation; null unless the solo form runs
  double* delta_u;  // [P][max_used][T*T]
  double* ddiag;    // [P][max_cand][T] every candidate's Delta diagonal (fsel_solo_kernel at 3 H = 39, where its LDS copy is single precision)
  int32_t* valid;   // [P][max_cand] 1 = triangulable (numVisible > 1)
  int32_t* valid_u; // [P][max_used]
  int32_t* black;   // [P][max_cand]
  double* fval;     // [P][max_cand]
  double* ub;       // [P][max_cand]
  int32_t* nsel;    // [P] number selected so far
  int32_t* done;    // [P] 1 when a round found no winner (state is then frozen)
  int32_t* live;    // [P][max_cand] indices of the candidates still in the race (valid, not yet selected), any order
  int32_t* pos;     // [P][max_cand] position of candidate l in live[]
  int32_t* nlive;   // [P]
  double* omega_out;  // optional [P][N*N] (tests)
  avm_fsel_out out;
  double* kd;         // [P][kd_stride(max_cloud)] the frame's kd-tree over its depth cloud (fsel_kdtree_kernel; searched by kd_depth)
};
