// track_prims.hpp — what the one-workgroup-per-window kernels that walk a list share (tracks.hip, relo.hip): the workgroup's shape,
// ranking by ballot (block_compact), the lookup in an ascending id list (find_id) and the verdict of a check kernel (report).
// Integer bookkeeping only: no floating-point operation in this file.
#pragma once
#include "devmath.hpp"
#include "kernels.hpp"

namespace avm {
namespace {

constexpr int TRK_NT = 256;
constexpr int TRK_WAVES = TRK_NT / 64;
constexpr int TRK_MAX_CHUNKS = AVM_MAX_IMAGE_PTS / 64;               // 16 (the rows of a window: 6)

// The items i < n with pred(i), ranked in index order: emit(i, rank) for each, the count returned to every thread.  Ballot / popcount per
// 64-item chunk, the chunk totals through `tot` (TRK_MAX_CHUNKS ints of LDS).  pred is evaluated twice; ends with a workgroup barrier.
template <class Pred, class Emit>
AVM_DEV int block_compact(int n, int* tot, Pred pred, Emit emit) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = wave; c * 64 < n; c += TRK_WAVES) {
    const int i = c * 64 + lane;
    const unsigned long long m = __ballot(i < n && pred(i));
    if (lane == 0) tot[c] = __popcll(m);
  }
  __syncthreads();
  int total = 0;
  for (int c = 0; c * 64 < n; c++) total += tot[c];
  for (int c = wave; c * 64 < n; c += TRK_WAVES) {
    const int i = c * 64 + lane;
    const bool f = i < n && pred(i);
    const unsigned long long m = __ballot(f);
    int base = 0;
    for (int k = 0; k < c; k++) base += tot[k];
    if (f) emit(i, base + __popcll(m & ((1ull << lane) - 1ull)));
  }
  __syncthreads();
  return total;
}

// position of `id` in the ascending ids[0 .. n), or -1 (memory-safe on any input)
AVM_DEV int find_id(const int* ids, int n, int id) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (ids[mid] < id) lo = mid + 1;
    else hi = mid;
  }
  return (lo < n && ids[lo] == id) ? lo : -1;
}

AVM_DEV void report(int* first_bad, int w, int rule) { atomicMin(first_bad, w * 8 + rule); }

}  // namespace
}  // namespace avm
