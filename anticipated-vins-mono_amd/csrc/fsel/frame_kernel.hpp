// fsel/frame_kernel.hpp - all rounds of a frame in one launch: records, teams, fsel_frame_body, fsel_frame_kernel and fsel_frame_kernel_mf
// Part of fsel.hip, which includes it inside namespace avm; no translation unit of its own.

// ---- all rounds of a frame in ONE launch (a select() is 151 dependent steps) ----------------------------------------------------
// Measured on the launch-per-round path: a step is bound by its chain of dependent trips to memory (state, live list, values,
// the winner's Delta, the candidates' Delta: each a miss, because a kernel boundary invalidates the caches), not by the launch.
// Here the frame's state never leaves the compute unit: every workgroup keeps its own copy of C, of the position diagonal and
// of the candidates' alive flags in LDS and applies the same deterministic update (winner out, C += p Delta_winner) to it.  The
// only thing exchanged per round is (fValue, ub) of each workgroup's 16 candidates - a fixed assignment by candidate index, no
// live list.
// There is no barrier and no fence.  A value travels as a 16-byte record {value, round tag, check word} written with ONE store
// and read with ONE device-scope load (a single request each, never served by the vector L1; two parity buffers): a reader spins
// until the records of all candidates still in the race carry the round's tag, and then it has the values - one trip after the
// last writer, nothing to order, no cache maintenance.  Everything else the kernel reads from global memory was written before
// the launch.  The workgroups that exchange records sit on ONE XCD (a team, see fsel_frame_kernel): the records never leave
// that XCD's L2 - a trip is ~0.5 us instead of a trip across the fabric.
// A spin longer than FS_SPIN_TICKS of the 100 MHz clock raises sync[2], every participant leaves, and the host runs the call
// again one mode down (and stays there).
constexpr long long FS_SPIN_TICKS = 20 * 100000;  // 20 ms
constexpr int FS_FRAME_MAXC = 512;                // candidates of a frame on the single-launch path (32 slots of 16)
// {value, round tag, check}: `check` = the value's two halves xor-ed with the tag.  The 16 bytes travel as one request, but
// nothing in the ISA promises that a concurrent reader cannot see them half-written: a record counts as arrived only when its
// tag is the round's AND its check matches its value.
struct alignas(16) FselRec {
  double v;
  int32_t tag, chk;
};
AVM_DEV int fsel_rec_check(int lo, int hi, int tag) { return lo ^ hi ^ (tag * 0x9E3779B1); }
template <bool SC1>
AVM_DEV void fsel_rec_load2(const FselRec* pa, const FselRec* pb, FselRec* a, FselRec* b) {  // device-scope loads
  typedef int v4i __attribute__((ext_vector_type(4)));
  v4i va, vb;
  asm volatile("global_load_dwordx4 %0, %2, off sc1\n\tglobal_load_dwordx4 %1, %3, off sc1\n\ts_waitcnt vmcnt(0)"
               : "=&v"(va), "=&v"(vb)
               : "v"(pa), "v"(pb)
               : "memory");
  a->v = __hiloint2double(va[1], va[0]), a->tag = va[3] == fsel_rec_check(va[0], va[1], va[2]) ? va[2] : -1;
  b->v = __hiloint2double(vb[1], vb[0]), b->tag = vb[3] == fsel_rec_check(vb[0], vb[1], vb[2]) ? vb[2] : -1;
}
template <bool SC1>
AVM_DEV void fsel_rec_store(FselRec* p, double v, int tag) {
  typedef int v4i __attribute__((ext_vector_type(4)));
  const v4i x = {__double2loint(v), __double2hiint(v), tag, fsel_rec_check(__double2loint(v), __double2hiint(v), tag)};
  if (SC1) asm volatile("global_store_dwordx4 %0, %1, off sc1" ::"v"(p), "v"(x) : "memory");
  else asm volatile("global_store_dwordx4 %0, %1, off" ::"v"(p), "v"(x) : "memory");
}

// TEAMS: the workgroups of every XCD form a team of `nslots` (first come, first slot; the rest exit), and a team takes frames from
// a queue until it is empty - a batch of P frames runs as up to eight independent selects side by side, each inside one L2.
// A team's leader (slot 0) hands out the frame: it waits for the team to be complete (first frame) or for everybody's `done`
// (later frames: nobody may still be reading the last frame's records), takes the next frame number and publishes it as a tagged
// record; a team that does not fill up within FS_TEAM_TICKS (its XCD is busy with something else) dissolves and leaves the frames
// to the others.  The host checks that every frame was finished (sync[4]) and runs the launch-per-round path otherwise.
// !TEAMS: one team over the whole device (blockIdx.x = slot, records written through to memory), one frame: the first fallback.
constexpr long long FS_TEAM_TICKS = 2 * 100000;  // 2 ms
constexpr int FS_TEAM_HDR = 32;                   // ints per team header: [0] members [1] done [4..7] the frame assignment record
constexpr int FS_SYNC_HDR = 64;                   // ints: [2] failure [3] frame queue [4] frames finished [8..15] arrivals per XCD [16..17] evaluations executed (solo form, 64-bit) [32..] trace
constexpr int FS_MAX_TEAMS = 16;
// TPX = 2 (batches of more than eight frames, 3H <= 30): TWO teams per XCD, i.e. two wavefronts per SIMD - the second one fills the
// latency gaps of the first (a team alone is bound by dependent latencies, not by issue).  Two workgroups then share a compute
// unit's LDS, so the Delta copies are packed lower triangles (16 x 3.7 KB).
template <int T, int BS, int NB, int TPX>
AVM_DEV void fsel_frame_body(const FselDev& A, int32_t* sync, int nslots, int test_drop) {
  FS_TABLES_GUARD(A);
  constexpr bool TEAMS = TPX > 0;
  // the workgroup's 16 Delta matrices stay in LDS for the whole select: full blocks while they fit (3H <= 30: 16 x 7.2 KB), packed
  // lower triangles beyond (3H = 39: 16 x 6.2 KB; the packed indexing costs 3 % at 3H = 30) or when two workgroups share the LDS
  constexpr bool PACKD = T > 30 || TPX > 1;
  constexpr int PK = PACKD ? T * (T + 1) / 2 : T * T;
  __shared__ int s_slot, s_fail, s_frame;
  __shared__ double sC[T * T], sdpp[T];
  __shared__ int32_t s_alive[FS_FRAME_MAXC];
  extern __shared__ double s_delta[];
  const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const int g = lane >> 4;  // this lane's candidate slot: its 16-lane DPP row
  const bool rec_lane = (lane & 15) == 0;  // one lane per candidate writes the records
  int bx = blockIdx.x, team = 0;
  if (TEAMS) {
    unsigned xcc;
    asm volatile("s_getreg_b32 %0, hwreg(20, 0, 4)" : "=s"(xcc));  // HW_REG_XCC_ID[3:0]
    xcc &= 7;
    if (t == 0) s_slot = __hip_atomic_fetch_add(&sync[8 + xcc], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    const int arrival = s_slot;  // order of arrival on this XCD: the first nslots are its first team, ...
    if (arrival >= TPX * nslots) return;
    team = xcc * TPX + arrival / nslots, bx = arrival % nslots;
    __syncthreads();
  }
  int32_t* th = sync + FS_SYNC_HDR + team * FS_TEAM_HDR;
  if (TEAMS && t == 0) __hip_atomic_fetch_add(&th[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (t == 0) s_fail = 0;
  FselRec* recF = reinterpret_cast<FselRec*>(sync + FS_SYNC_HDR + FS_MAX_TEAMS * FS_TEAM_HDR) + (size_t)team * 4 * FS_FRAME_MAXC;  // [2][MAXC] fValues
  FselRec* recU = recF + 2 * FS_FRAME_MAXC;                                                                      // [2][MAXC] bounds
  FselRec* assign = reinterpret_cast<FselRec*>(th + 4);
  const avm_fsel_batch& b = A.b;
  const int mc = b.max_cand, P = b.n_problems;
  const int l = (bx * (FS_NT / 64) + wv) * 4 + g;  // this block's candidate index, in every frame
  const int lc = min(l, mc - 1);
  auto give_up = [&]() { __hip_atomic_store(&sync[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); };
#ifdef FS_TRACE_EVAL
  long long tk_body = 0, tk_wait = 0, tk_pick = 0, tk_upd = 0, tk0 = clock64();
  long long tke[4] = {0, 0, 0, 0};
#define FS_SEG(acc) { const long long n__ = clock64(); acc += n__ - tk0; tk0 = n__; }
#else
#define FS_SEG(acc)
#endif
  for (int seq = 1;; seq++) {
    // ---- which frame
    int p = 0;
    if (TEAMS) {
      __syncthreads();  // (s_frame / s_fail of the previous frame have been read)
      if (t == 0) {
        const long long t0 = wall_clock64();
        if (bx == 0) {  // the leader
          int f = -2;   // (-2: the team never filled up)
          for (;;) {
            const int have = seq == 1 ? __hip_atomic_load(&th[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)
                                      : __hip_atomic_load(&th[1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) / (seq - 1);
            if (have >= nslots) {
              f = __hip_atomic_fetch_add(&sync[3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
              if (f >= P) f = -1;
              break;
            }
            if (wall_clock64() - t0 > (seq == 1 ? FS_TEAM_TICKS : FS_SPIN_TICKS)) {
              if (seq > 1) give_up();  // (a member got lost in the middle of the batch)
              break;
            }
            __builtin_amdgcn_s_sleep(2);
          }
          fsel_rec_store<false>(assign, (double)f, seq);
        }
        FselRec ra, rb;
        for (;;) {
          fsel_rec_load2<true>(assign, assign, &ra, &rb);
          if (ra.tag == seq) break;
          if (__hip_atomic_load(&sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 || wall_clock64() - t0 > 2 * FS_SPIN_TICKS) {
            give_up();
            ra.v = -3.0;
            break;
          }
          __builtin_amdgcn_s_sleep(2);
        }
        s_frame = (int)ra.v;
      }
      __syncthreads();
      p = s_frame;
      if (p < 0) return;
    } else if (seq > 1) {
      return;
    }
    // ---- the frame's state, this workgroup's copy
    const int nc = b.n_cand[p];
    const int kappa = max(0, b.max_features - (b.n_used ? b.n_used[p] : 0));
    const size_t pc = (size_t)p * mc;
    for (int idx = t; idx < T * T; idx += FS_NT) sC[idx] = A.C[(size_t)p * T * T + idx];
    for (int idx = t; idx < T; idx += FS_NT) sdpp[idx] = A.dpp[(size_t)p * T + idx];
    for (int c = t; c < FS_FRAME_MAXC; c += FS_NT) s_alive[c] = (c < nc && A.valid[pc + min(c, mc - 1)] != 0) ? 1 : 0;
    for (int q = 0; q < FS_CPWG; q++) {
      const double* src = A.delta + (pc + min(bx * FS_CPWG + q, mc - 1)) * T * T;
      for (int idx = t; idx < T * T; idx += FS_NT) {
        const int R = idx / T, c = idx % T;
        if (!PACKD) s_delta[q * PK + idx] = src[idx];
        else if (c >= R) s_delta[q * PK + c * (c + 1) / 2 + R] = src[idx];  // (slot (c, R) <- entry [R][c]: the entry the full form reads for it)
      }
    }
    const double pr = b.cand_prob[pc + lc];
    const double* D = s_delta + (wv * 4 + g) * PK;
    const double ld_nn = A.consts[(size_t)p * 4], ub_nn = A.consts[(size_t)p * 4 + 1];  // logdet of the hoisted pivots / their share of the bound
    const int tag0 = seq << 12;  // (round tags of different frames never meet: max_features < 4096 on this path)
    __syncthreads();
    int nsel = 0;
    for (int k = 0; k <= kappa; k++) {
      // ---- 1. the previous round's winner (its values are in parity buffer (k - 1) & 1, tagged k)
      if (k >= 1) {
        const int par = (k - 1) & 1;
        int cl[2];
        double cf[2], cu[2];
#pragma unroll
        for (int q = 0; q < 2; q++) {  // this thread's candidates: t and t + FS_NT
          const int sq = t + q * FS_NT;
          cl[q] = (sq < nc && s_alive[sq]) ? sq : -1;
          const FselRec *pf = recF + par * FS_FRAME_MAXC + sq, *pu = recU + par * FS_FRAME_MAXC + sq;
          FselRec rf, ru;
          const long long t0 = wall_clock64();
          for (;;) {
            fsel_rec_load2<true>(pf, pu, &rf, &ru);
            if (__all(cl[q] < 0 || (rf.tag == tag0 + k && ru.tag == tag0 + k))) break;
            // A record of THIS frame that already carries a later round's tag: its writer is two rounds ahead and has overwritten the
            // value this workgroup still needed.  That can only happen to a workgroup none of whose own candidates is alive (nobody
            // waits for its records, so nobody is held back by it); the value is gone - leave at once instead of spinning into the
            // time-out (the host runs the call again one mode down, avm_fsel_fallback_stats counts it).
            const bool overtaken = cl[q] >= 0 && (((rf.tag >> 12) == seq && rf.tag > tag0 + k) || ((ru.tag >> 12) == seq && ru.tag > tag0 + k));
            if (__any(overtaken) || __hip_atomic_load(&sync[2], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0 || wall_clock64() - t0 > FS_SPIN_TICKS) {
              give_up();
              s_fail = 1;
              break;
            }
            __builtin_amdgcn_s_sleep(1);
          }
          cf[q] = rf.v, cu[q] = ru.v;
        }
        FS_SEG(tk_wait)
        double fwin, frun = -HUGE_VAL;
        const int win = fsel_pick_frame(A, cl, cf, cu, &fwin, &frun);  // (a workgroup barrier inside: s_fail is settled after it)
        FS_SEG(tk_pick)
        if (s_fail) return;
        if (win < 0) break;  // lMax == -1: nothing is added; later rounds would repeat the same state
        if (bx == 0 && t == 0) {  // this frame's recorder
          A.out.selected_ids[(size_t)p * b.max_features + nsel] = b.cand_id[pc + win];
          if (A.out.fvalues) A.out.fvalues[(size_t)p * b.max_features + nsel] = fwin;
          if (A.out.min_gap) A.out.min_gap[(size_t)p * b.max_features + nsel] = fwin - frun;
          A.out.n_selected[p] = nsel + 1;
          A.black[pc + win] = 1;
        }
        nsel++;
        const double* Dw = A.delta + (pc + win) * T * T;
        // (all of the thread's entries of the winner's Delta - and its probability - requested before the first is used: one trip to memory,
        //  not one per entry; round 5)
        constexpr int NFOLD = (T * T + FS_NT - 1) / FS_NT;
        double dwv[NFOLD];
#pragma unroll
        for (int q = 0; q < NFOLD; q++) dwv[q] = Dw[min(t + q * FS_NT, T * T - 1)];
        const double prw = b.cand_prob[pc + win];
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < NFOLD; q++) {
          const int idx = t + q * FS_NT;
          if (idx < T * T) {
            sC[idx] = sC[idx] + prw * dwv[q];
            if (idx / T == idx % T) sdpp[idx / T] = sdpp[idx / T] + prw * dwv[q];
          }
        }
        if (t == 0) s_alive[win] = 0;
        __syncthreads();
        FS_SEG(tk_upd)
      }
      if (k >= kappa) break;
      // ---- 2. this round's values of this workgroup's candidates, published with tag k + 1
      const bool live = l < nc && s_alive[min(l, FS_FRAME_MAXC - 1)] != 0;
      if (__any(live)) {
        double ld, ubt;
#ifdef FS_TRACE_EVAL
        const bool ok = fsel_logdet4<T, BS, NB, true, PACKD>(sC, sdpp, D, pr, &ld, &ubt, tke);
#else
        const bool ok = fsel_logdet4<T, BS, NB, true, PACKD>(sC, sdpp, D, pr, &ld, &ubt);
#endif
        if (live && rec_lane && l != test_drop) {  // (test_drop: a record that never arrives, tests only; -1 otherwise)
          fsel_rec_store<!TEAMS>(recF + (k & 1) * FS_FRAME_MAXC + l, ok ? (ld_nn + 2.0 * ld) : __builtin_nan(""), tag0 + k + 1);
          fsel_rec_store<!TEAMS>(recU + (k & 1) * FS_FRAME_MAXC + l, ub_nn + ubt, tag0 + k + 1);
        }
      }
      __syncthreads();  // (sC / s_alive are read by the evaluation above and written by the next round's update)
      FS_SEG(tk_body)
    }
#ifdef FS_TRACE_EVAL  // (development: cycles per phase of workgroup 0 of the team that took frame 0, printed with AVM_FSEL_TRACE=1)
    if (t == 0 && bx == 0 && p == 0) {
      long long* o = reinterpret_cast<long long*>(sync + 32);
      o[0] = tk_pick, o[1] = tk_upd, o[2] = tk_body, o[3] = (long long)A.consts[2], o[4] = tk_wait;
      o[9] = (long long)A.consts[3];
      o[5] = tke[0], o[6] = tke[1], o[7] = tke[2], o[8] = tke[3];
    }
#endif
    if (t == 0) {
      if (bx == 0) {
        A.nsel[p] = nsel;
        __hip_atomic_fetch_add(&sync[4], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // frames finished
      }
      if (TEAMS) __hip_atomic_fetch_add(&th[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // done with this frame's records
    }
  }
#undef FS_SEG
}

// The kernel proper.  fsel_frame_kernel_mf is the instance for two teams per XCD (3 H <= 30), pinned to the two wavefronts per SIMD that
// two teams run at.  The pin came with the matrix-core evaluation (round 3: left alone the allocator took 334 registers for it, one
// wavefront per SIMD, and the second team of an XCD never became resident); that form was removed after round 6 (commit 24fd667 is the
// last that has it).  The instance keeps its name, which the profile records use, and its attribute, without which its code changes.
// The instances with a SIMD per wavefront are left to the scheduler - the attribute costs them 3-4 %.
template <int T, int BS, int NB, int TPX>
__global__ __launch_bounds__(FS_NT) void fsel_frame_kernel(FselDev A, int32_t* sync, int nslots, int test_drop) {
  fsel_frame_body<T, BS, NB, TPX>(A, sync, nslots, test_drop);
}
template <int T, int BS, int NB>
__global__ __launch_bounds__(FS_NT) __attribute__((amdgpu_waves_per_eu(2, 2))) void fsel_frame_kernel_mf(FselDev A, int32_t* sync, int nslots, int test_drop) {
  fsel_frame_body<T, BS, NB, 2>(A, sync, nslots, test_drop);
}
