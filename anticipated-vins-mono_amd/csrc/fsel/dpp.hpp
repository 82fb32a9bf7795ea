// fsel/dpp.hpp - the selector's own lane exchange: the row broadcast and the v_fmac_f64_dpp run with its fence, row sum, wave maximum
// (written with devmath.hpp's dpp_d / readlane_d / sfor)
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

// FOUR candidates per wavefront: candidate g lives in the 16-lane DPP row g of the wave.  The T x T matrix is cut into NB block
// rows of BS <= 16 rows (T = 30: 2 x 15, T = 39: 3 x 13); lane r of the row holds row r of EVERY block row in registers
// (block row bi: columns 0 .. (bi + 1) BS - 1), so an entry A[gk][gj] is broadcast to the whole candidate with a DPP
// row_newbcast of lane gk % BS - since round 6 as the DPP operand of the multiply-add itself (fs_fmac_bcast below: v_fmac_f64_dpp, one instruction per
// update; before: two 32-bit DPP moves feeding the updates of all block rows).  The factorization is the same right-looking, square-root-free
// LDL^T as before (column j divided by its pivot with v_rcp_f64 + two Newton steps; junk above the diagonal of the diagonal
// blocks is computed and never read), only the lanes are used four times as densely and there are no SGPR round trips:
// 1-3 DPP multiply-adds per (pivot, column) pair for four candidates instead of 2 v_readlane + 1 FMA for one.
// logdet = sum_j log(d_j) and the Hadamard bound (sortedlogDetUB) are summed in one fixed association for every candidate, so
// mirror-image candidates still get bit-identical bounds (the std::map rule of the pick depends on that).
template <int K>
AVM_DEV double fs_rowbcast_k(double v) { return dpp_d<0x150 + K>(v); }  // lane K of every 16-lane row -> the whole row (row_newbcast:K = dpp_ctrl 0x150 + K)

// acc += (lane k of src's 16-lane row) * nmul in ONE instruction: v_fmac_f64_dpp with row_newbcast (the FP64 ALU of gfx90a+ takes a DPP operand
// of that one kind).  Round 6, scripts/ubench/dpp2.hip: 5.8 cycles an issue against 4.8 for a plain v_fmac_f64.  (The pre-round-6 form - two 32-bit
// DPP moves per (pivot, column) feeding a plain multiply-add per block row - was removed; commit 24fd667 is the last that has it.)
// The wait-state rule: a DPP instruction reads its DPP source (its first source operand) correctly only if no VALU instruction has written that
// VGPR within the two wait states before it (the round-3 probe, scripts/ubench/dpp.hip, broke it and read as "does not accumulate").  The
// compiler's hazard recognizer does not look inside inline assembly, so the caller keeps those two wait states itself (fs_dpp_fence: s_nop 1)
// between the last write of any operand and the first instruction of a run, and after the run before the next broadcast; inside a run nothing
// reads what a neighbour writes.  The scheduler may still move independent instructions between a fence and its run:
// tests/test_isa_dpp_hazards.py checks every DPP instruction of the compiled code object against the rule.
AVM_DEV void fs_dpp_fence() { asm volatile("s_nop 1"); }
template <int K>
AVM_DEV void fs_fmac_bcast(double& acc, double src, double nmul) {
  asm volatile("v_fmac_f64_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(src), "v"(nmul), "n"(K));
}
// Sum over the 16 lanes of a DPP row, in every lane of the row: the same four exchange steps as fs_wave_max (a fixed
// association, the same for every candidate - mirror-image candidates keep bit-identical Hadamard bounds): pairs, quads, the two
// quads of a half (mirrored), the two halves (mirrored).
AVM_DEV double fs_row_sum(double v) {
  v += dpp_d<0xB1>(v);   // quad_perm [1,0,3,2]
  v += dpp_d<0x4E>(v);   // quad_perm [2,3,0,1]
  v += dpp_d<0x141>(v);  // row_half_mirror
  v += dpp_d<0x140>(v);  // row_mirror
  return v;
}
// Maximum over the wavefront, in every lane: four DPP exchange steps inside the 16-lane rows (lane ^ 1, lane ^ 2, mirror of 8,
// mirror of 16 - any pairing of already-reduced groups will do for a maximum), then the four row results through SGPRs: uniform.
// (__shfl_xor is a ds_bpermute per 32 bits and step: the lexicographic argmax of the pick took 30 of them, 2 K cycles.)
AVM_DEV double fs_wave_max(double v) {
  v = fmax(v, dpp_d<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmax(v, dpp_d<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmax(v, dpp_d<0x141>(v));  // row_half_mirror
  v = fmax(v, dpp_d<0x140>(v));  // row_mirror
  const double r0 = readlane_d(v, 0), r1 = readlane_d(v, 16), r2 = readlane_d(v, 32), r3 = readlane_d(v, 48);
  return fmax(fmax(r0, r1), fmax(r2, r3));
}
AVM_DEV int fs_wave_max(int v) {
  v = max(v, dpp_mov<0xB1>(v));
  v = max(v, dpp_mov<0x4E>(v));
  v = max(v, dpp_mov<0x141>(v));
  v = max(v, dpp_mov<0x140>(v));
  return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
             max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}
