// solve_split.hip - avm_window_solve_batch_relo's split of a batch into the windows without and with a pending relocalization:
// two ascending lists of window indices for the list builds of the solve kernel (solve/solve_kernel.hpp, AVM_WIN_LIST).
// Integer bookkeeping only.  Positions come from ballots and a running offset: the order never depends on which wavefront ran first.
#include "track_prims.hpp"

namespace avm {
namespace {
constexpr int SPLIT_CHUNK = TRK_NT;  // windows per block_compact: one ballot per wavefront (its chunk totals: TRK_WAVES <= TRK_MAX_CHUNKS ints of LDS)

// One workgroup.  list[0 .. B): the windows with relo_active == 0, list[B .. 2 B): the others; counts[0] = the number of the others.
__global__ __launch_bounds__(TRK_NT) void solve_partition_kernel(int n_windows, const int32_t* relo_active, int32_t* list, int* counts) {
  __shared__ int tot[TRK_MAX_CHUNKS];
  int n_plain = 0, n_ext = 0;
  for (int base = 0; base < n_windows; base += SPLIT_CHUNK) {
    const int n = min(SPLIT_CHUNK, n_windows - base);
    n_plain += block_compact(n, tot, [&](int i) { return relo_active[base + i] == 0; }, [&](int i, int rank) { list[n_plain + rank] = base + i; });
    n_ext += block_compact(n, tot, [&](int i) { return relo_active[base + i] != 0; },
                           [&](int i, int rank) { list[(size_t)n_windows + n_ext + rank] = base + i; });
  }
  if (threadIdx.x == 0) counts[0] = n_ext;
}
}  // namespace

hipError_t launch_solve_partition(int n_windows, const int32_t* relo_active, int32_t* list, int* counts, hipStream_t stream) {
  hipLaunchKernelGGL(solve_partition_kernel, dim3(1), dim3(TRK_NT), 0, stream, n_windows, relo_active, list, counts);
  return hipGetLastError();
}
}  // namespace avm
