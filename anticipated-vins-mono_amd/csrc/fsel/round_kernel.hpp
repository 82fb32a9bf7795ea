// fsel/round_kernel.hpp - one launch per greedy round: fsel_round_kernel, and fsel_live_init_kernel that starts its live list
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

// ---- one greedy round: f_l = logdet(Omega + OmegaS + p_l Delta_l) for every live candidate ----

// One greedy step of workgroup `bx` of problem p: settle round k - 1, evaluate round k.  Returns true when the problem is
// finished (the same answer in every workgroup of the problem: it depends on the shared state only).
template <int T, int BS, int NB>
AVM_DEV bool fsel_round_body(const FselDev& A, int p, int k, int bx) {
  static_assert(BS * NB == T && BS <= 16, "block rows of at most 16 lanes");
  const avm_fsel_batch& b = A.b;
  const int t = threadIdx.x;
  const int kappa = max(0, b.max_features - (b.n_used ? b.n_used[p] : 0));
  if (A.done[p]) return true;  // (set by an earlier round: the state is frozen)
  const bool has_pick = k >= 1 && k <= kappa, has_eval = k < kappa;
  if (!has_pick && !has_eval) return true;
  const FselPar S = fsel_par(A, p, k);
  // ---- 1. the previous round's winner
  int win = -1;
  double fwin = 0.0, frun = -HUGE_VAL;
  if (has_pick) {
    win = fsel_pick_local(A, S, &fwin, &frun);
    if (win < 0) {
      if (bx == 0 && t == 0) A.done[p] = 1;  // lMax == -1: nothing is added; later rounds would repeat the same state
      return true;
    }
  }
  const bool won = win >= 0;
  const int wc = max(win, 0);
  const int nl = S.nl, nln = won ? nl - 1 : nl;
  const int at = won ? S.pos[wc] : -1, lastc = S.live[max(nl - 1, 0)];  // swap-remove: the last candidate takes the winner's slot
  const double prw = b.cand_prob[(size_t)p * b.max_cand + wc];
  const double* Dw = A.delta + ((size_t)p * b.max_cand + wc) * T * T;
  if (bx == 0) {  // this problem's recorder: outputs and the next buffers
    if (won && t == 0) {
      const int ks = A.nsel[p];
      A.out.selected_ids[(size_t)p * b.max_features + ks] = b.cand_id[(size_t)p * b.max_cand + win];
      if (A.out.fvalues) A.out.fvalues[(size_t)p * b.max_features + ks] = fwin;
      if (A.out.min_gap) A.out.min_gap[(size_t)p * b.max_features + ks] = fwin - frun;
      A.nsel[p] = ks + 1;
      A.out.n_selected[p] = ks + 1;
      A.black[(size_t)p * b.max_cand + win] = 1;
    }
    for (int idx = t; idx < T * T; idx += FS_NT) {
      const double c = won ? S.C[idx] + prw * Dw[idx] : S.C[idx];
      S.Cn[idx] = c;
      if (idx / T == idx % T) S.dppn[idx / T] = won ? S.dpp[idx / T] + prw * Dw[idx] : S.dpp[idx / T];
    }
    for (int s = t; s < nln; s += FS_NT) {
      const int l = s == at ? lastc : S.live[s];
      S.liven[s] = l, S.posn[l] = s;
    }
    if (t == 0) *S.nliven = nln;
  }
  if (!has_eval) return true;
  // ---- 2. this round's candidates against the state with the winner folded in: every workgroup builds it in LDS (the same
  //         expressions workgroup 0 stores), and the candidates' matrices take their C part from there
  __shared__ double sC[T * T], sdpp[T];
  for (int idx = t; idx < T * T; idx += FS_NT) {
    const double c = won ? S.C[idx] + prw * Dw[idx] : S.C[idx];
    sC[idx] = c;
    if (idx / T == idx % T) sdpp[idx / T] = won ? S.dpp[idx / T] + prw * Dw[idx] : S.dpp[idx / T];
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = lane >> 4;  // candidate slot of this lane
  // the candidates still in the race are kept compact (the winner is swap-removed), so late rounds do not pay for
  // the slots of the features already selected
  const int slot = (bx * (FS_NT / 64) + wv) * 4 + g;
  const bool live = slot < nln;
  if (!__any(live)) return false;  // (wave-uniform; no workgroup barrier follows in this function)
  const int sc = min(slot, max(nln - 1, 0));
  const int l = sc == at ? lastc : S.live[sc];
  const int lc = l;  // a slot past the end factors the last live candidate's matrix again and throws the result away
  const double pr = b.cand_prob[(size_t)p * b.max_cand + lc];
  const double* D = A.delta + ((size_t)p * b.max_cand + lc) * T * T;
  const double ld_nn = A.consts[(size_t)p * 4], ub_nn = A.consts[(size_t)p * 4 + 1];  // (requested before the evaluation, not after it)
  double ld, ubt;
  const bool bad = !fsel_logdet4<T, BS, NB>(sC, sdpp, D, pr, &ld, &ubt);
  if (live && (lane & 15) == 0) {
    const double f = bad ? __builtin_nan("") : (ld_nn + 2.0 * ld);
    S.fvaln[sc] = f;  // (by slot of the next live list: see fsel_pick_local)
    S.ubn[sc] = ub_nn + ubt;
  }
  return false;
}

// (amdgpu_waves_per_eu(2, 2): a batch puts two of these wavefronts on a SIMD; left to itself the scheduler trades the
//  evaluation's instruction-level parallelism for an occupancy the launch never reaches - measured 0.22 -> 0.30 ms per frame)
template <int T, int BS, int NB>
__global__ __launch_bounds__(FS_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void fsel_round_kernel(FselDev A, int k) {
  FS_TABLES_GUARD(A);
  (void)fsel_round_body<T, BS, NB>(A, blockIdx.y, k, blockIdx.x);
}

// the compact list of the candidates that take part in the greedy rounds: the valid ones, in ascending index (= id) order
__global__ __launch_bounds__(64) void fsel_live_init_kernel(FselDev A) {
  FS_TABLES_GUARD(A);
  const avm_fsel_batch& b = A.b;
  const int p = blockIdx.x, lane = threadIdx.x;
  const int nc = b.n_cand[p];
  int n = 0;
  for (int base = 0; base < nc; base += 64) {
    const int l = base + lane;
    const bool ok = l < nc && A.valid[(size_t)p * b.max_cand + l] != 0;
    const unsigned long long m = __ballot(ok);
    if (ok) {
      const int at = n + __popcll(m & ((1ull << lane) - 1));
      A.live[(size_t)p * b.max_cand + at] = l, A.pos[(size_t)p * b.max_cand + l] = at;
    }
    n += __popcll(m);
  }
  if (lane == 0) A.nlive[p] = n;
}
