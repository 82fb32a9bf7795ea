// solve/lds.hpp - the workgroup's LDS and what every phase uses: LDS(), the profiling stopwatches, each build's layout, workgroup reductions, roff / s_off
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// the workgroup's dynamic LDS, always reached through the shared symbol (never through a generic pointer that
// crosses a function boundary), so the compiler keeps ds_* addressing inside outlined functions
//
// None of the kernels of this translation unit has static LDS, so the dynamic segment starts at LDS address 0 (checked once per
// workgroup by lds_base_check()).  Spelling the base as the constant instead of the symbol matters: outside a
// kernel body the symbol's address is a load from llvm.amdgcn.dynlds.offset.table, which the compiler happily
// re-issues (s_load + s_waitcnt) in front of every predicated LDS access of the outlined phases.
typedef __attribute__((address_space(3))) double lds_double_t;
typedef __attribute__((address_space(3))) char lds_char_t;
AVM_DEV double* LDS() {
  // (integer -> pointer keeps this the LDS address 0; a literal null would become the address-space's null, -1)
  return (double*)reinterpret_cast<lds_double_t*>((uintptr_t)__builtin_amdgcn_readfirstlane(0));
}
AVM_DEV void lds_base_check() {
  if ((unsigned)(uintptr_t)(lds_char_t*)avm_smem != 0u) __builtin_trap();
}

#define AVM_NOINL __device__ __noinline__
#define PROF_T0() long long pt__ = clock64()
#define PROF(c, k) do { if ((c).prof && threadIdx.x == 0) { long long n__ = clock64(); (c).prof[k] += n__ - pt__; pt__ = n__; } } while (0)
// second, independent stopwatch for the trust-region loop's own segments (slots 32..)
#define PROFQ_T0() pq__ = clock64()
#define PROFQ(c, k) do { if ((c).prof && threadIdx.x == 0) { long long n__ = clock64(); (c).prof[k] += n__ - pq__; pq__ = n__; } } while (0)

#include "layout.hpp"  // (a part includes a part by its name inside solve/)

// A value every lane of the wavefront holds alike, moved to scalar registers.  The trust-region loop's own scalars (radius, mu, norms,
// costs) are live across every outlined phase; as vector registers the compiler parks them in scratch memory around the calls and each
// use after a call starts with a reload, as scalar registers they are parked in lanes of a vector register (v_readlane, no memory).
AVM_DEV double uni(double v) {
  return __hiloint2double(__builtin_amdgcn_readfirstlane(__double2hiint(v)), __builtin_amdgcn_readfirstlane(__double2loint(v)));
}
// A loop-carried uniform double, held as its two 32-bit halves.  Where a uni() value is merged at a loop head or behind a branch, the
// compiler weighs the merged 64-bit value's uses - FP64 arithmetic, all of it vector instructions - and moves the whole chain back to
// vector registers; the halves are integers, merge in scalar registers, and become a double again (a register pair, no instruction
// of its own) at the use.
struct unid {
  int hi, lo;
  AVM_DEV unid(double v = 0) { *this = v; }
  AVM_DEV unid& operator=(double v) {
    hi = __builtin_amdgcn_readfirstlane(__double2hiint(v)), lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
    return *this;
  }
  AVM_DEV operator double() const { return __hiloint2double(hi, lo); }
};
// ... and a flag or count every lane holds alike (what an outlined phase returns, what LDS holds): a branch on it is a scalar branch, and
// the loop scalars assigned behind it stay in scalar registers.
AVM_DEV int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
AVM_DEV bool uni(bool v) { return __builtin_amdgcn_readfirstlane((int)v) != 0; }

// A fresh copy of the thread index (and of the lane / wavefront index), opaque to the compiler.  The kernel bodies use the whole register
// file; whatever they derive from threadIdx.x once (t >> 6, lds + L_X + t, the start address of a strided loop) the compiler hoists out of
// the trust-region loop and the window loop, keeps live across every outlined phase, spills, and reloads at the use: one dependent round
// trip to scratch memory per value.  Behind the empty asm there is nothing to hoist or to share with an earlier copy: a value derived from
// a fresh index is recomputed where it is used (a v_and / v_lshrrev or two) and dies with the segment that asked for it.  Every phase of a
// kernel body takes its own at its head (`const int t = fresh_tid();`); none lives across an outlined call or a loop iteration.
AVM_DEV int fresh_tid() {
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}
AVM_DEV int fresh_lane() { return fresh_tid() & 63; }
AVM_DEV int fresh_wave() { return fresh_tid() >> 6; }  // (per lane; __builtin_amdgcn_readfirstlane makes it a scalar)

// Workgroup reductions of the solve kernel with ONE barrier each.  The partial sums of consecutive reductions go to alternating
// halves of lds[L_RED]: a wavefront can only overwrite a half two reductions later, i.e. after a barrier that every wavefront
// reaches with its reads of that half done.  Which half is next is a counter every wavefront keeps for itself in LDS (all
// wavefronts run the same sequence of reductions, so the counters agree); red_init() zeroes it at kernel entry.
// (The address from fresh_wave(): the compiler cannot hoist it, so every reduction computes it with two VALU instructions.  Computed
//  once it was kept for the whole kernel, spilled, and every reduction began by reloading it from scratch memory.)
AVM_DEV int* red_counter() {
  return reinterpret_cast<int*>(LDS() + L_RED_CNT) + fresh_wave();
}
AVM_DEV void red_init() {
  if ((threadIdx.x & 63) == 0) *red_counter() = 0;
}
template <class Op>
AVM_DEV double block_reduce1(double v, Op op) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int* cnt = red_counter();
  const int k = *cnt;
  double* red = LDS() + L_RED + 8 * (k & 1);
  if (lane == 0) red[wv] = v, *cnt = k + 1;
  __syncthreads();
  double s = red[0];
#pragma unroll
  for (int i = 1; i < NT / 64; i++) s = op(s, red[i]);
  return s;
}
AVM_DEV double block_sum1(double v) {
  return block_reduce1(wave_sum(v), [](double a, double b) { return a + b; });
}
AVM_DEV double block_max1(double v) {
  return block_reduce1(wave_max(v), [](double a, double b) { return fmax(a, b); });
}
// two sums at once (one barrier, both halves of the pair in the same half of lds[L_RED])
AVM_DEV void block_sum1x2(double& a, double& b) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double wa = wave_sum(a), wb = wave_sum(b);
  int* cnt = red_counter();
  const int k = *cnt;
  double* red = LDS() + L_RED + 8 * (k & 1);
  double* redb = LDS() + L_RED_B + 8 * (k & 1);
  if (lane == 0) red[wv] = wa, redb[wv] = wb, *cnt = k + 1;
  __syncthreads();
  double sa = red[0], sb = redb[0];
#pragma unroll
  for (int i = 1; i < NT / 64; i++) sa += red[i], sb += redb[i];
  a = sa, b = sb;
}

AVM_DEV int roff(int i) {  // even i = 2q: 2q(q+1); odd i = 2q+1: 2(q+1)^2 -> every row starts 16-byte aligned
  const int q = i >> 1;
  return 2 * __mul24(q + 1, q + (i & 1));  // 24-bit multiply: full rate (v_mul_lo_u32 is quarter rate)
}

#ifdef AVM_TP
// Throughput build: offset (doubles from lds[0]) of entry (r, c), c <= r < NF, of the assembled system, or -1 where the entry is
// structurally zero.  Pose rows: the packed triangle; speed-bias rows: the compact row [poses i-1, i, i+1 | speed-biases i-1, i] of
// block i, except that the pose columns of the prior's speed-bias block live in the strip (the prior couples it to every pose).
AVM_DEV int s_off(int r, int c) {
  if (r < NPOSE) return L_S + roff(r) + c;
  const int q = r - NPOSE, i = q / 9;
  if (c < NPOSE) {
    if (i == reinterpret_cast<const int*>(LDS() + L_INT)[I_PSB]) return L_STRIP + (q - 9 * i) * NPOSE + c;
    const int p = c - 6 * (i - 1);
    return (p >= 0 && p < 18) ? L_SBC + q * SBW + p : -1;
  }
  const int p = c - (NPOSE + 9 * (i - 1));
  return (p >= 0 && p < 18) ? L_SBC + q * SBW + 18 + p : -1;
}
#define S_OFF(r, c) s_off(r, c)
#else
#define S_OFF(r, c) (L_S + roff(r) + (c))
#endif
