// solve/chol_regs.hpp - chol_regs<WV>: the factorization on register tiles and both triangular solves; pivot chains, row sums, tp_pattern_export
// Part of window_solve.hip, which includes it inside namespace avm; no translation unit of its own.

// One of the five latency shadows of the 16-pivot elimination chains (tp_diag_chain, chol_diag_block, pinv16_cholesky: the one definition for
// the three).  Pivot j's reciprocal is a dependent chain - v_rcp_f64, then two Newton steps - and the rank-1 update of pivot j - 1 (columns
// j + 1 .. NB - 1 of the caller's row a[NB], factor uprev) is dealt over the shadows before, between and after its four steps, three columns
// per shadow: AVM_PIVOT_TAIL(0 .. 4, FENCE) around the caller's e / y updates.  Uses the caller's a, NB, j, uprev.  FENCE (a constant):
// scheduling barriers around the shadow, so that the compiler keeps the hand-made interleaving.
#define AVM_PIVOT_TAIL(slot, FENCE)                                                                                    \
  if (FENCE) __builtin_amdgcn_sched_barrier(0);                                                                        \
  if (j > 0) {                                                                                                         \
    double sk[3];                                                                                                      \
    _Pragma("unroll") for (int q = 0; q < 3; q++) sk[q] = readlane_d(a[j - 1], min(j + 1 + (slot) + 5 * q, NB - 1));   \
    if (FENCE) __builtin_amdgcn_sched_barrier(0);                                                                      \
    _Pragma("unroll") for (int q = 0; q < 3; q++)                                                                      \
      if (j + 1 + (slot) + 5 * q < NB) a[j + 1 + (slot) + 5 * q] = fma(-uprev, sk[q], a[j + 1 + (slot) + 5 * q]);      \
  }                                                                                                                    \
  if (FENCE) __builtin_amdgcn_sched_barrier(0);

// 16-pivot chain on the diagonal block in LDS patch `patch` ([row][16], symmetric): chol_diag_block with the patch as its source and
// destination.  Leaves L~ (lower, unscaled: times sqrt(d_c) per column c, the pivot d_c on the diagonal) in the patch and
// L~^-T with 1 / sqrt(d_c) behind it in buffer `buf`.
AVM_DEV void tp_diag_chain(int nb, int patch, int buf, int stamp) {
  constexpr int NB = 16;
  double* lds = LDS();
  const int r = threadIdx.x & 63;
  __builtin_amdgcn_s_setprio(3);
  double a[NB];
  const bool idl = (r & 48) == 16;
  const int rc = min(r, nb - 1);
  double* row = lds + L_PATCH + patch * (16 * TP_PS) + (rc & 15) * TP_PS;
  {
#pragma unroll
    for (int k = 0; k < NB; k++) a[k] = row[k];
#pragma unroll
    for (int k = 0; k < NB; k++) a[k] = idl ? ((r & 15) == k ? 1.0 : 0.0) : a[k];  // lanes 16..31: the identity's rows
  }
  wave_lds_sync();  // (every lane holds its row: the stores below go to the same patch)
  double uprev = 0.0;
#pragma unroll
  for (int j = 0; j < NB; j++) {
    if (j > 0) a[j] = fma(-uprev, readlane_d(a[j - 1], j), a[j]);
    const double djj = readlane_d(a[j], j);
    double y = __builtin_amdgcn_rcp(djj), e = 0;
    AVM_PIVOT_TAIL(0, true)
    e = fma(-djj, y, 1.0);
    AVM_PIVOT_TAIL(1, true)
    y = fma(y, e, y);
    AVM_PIVOT_TAIL(2, true)
    e = fma(-djj, y, 1.0);
    AVM_PIVOT_TAIL(3, true)
    y = fma(y, e, y);
    AVM_PIVOT_TAIL(4, true)
    uprev = a[j] * y;
  }
  {
    double* dst = idl ? lds + L_LINV + buf * (16 * TP_PS) + (r & 15) * TP_PS : row;
    double* dump = lds + L_DUMP + r;
    const int kmax = idl ? NB - 1 : (r < nb ? r : -1);
#pragma unroll
    for (int k = 0; k < NB; k++) *(k <= kmax ? dst + k : dump) = a[k];
  }
  // 1 / sqrt(d_c) of the block's columns beside L~^-T (every wavefront's solves scale their rows with it: computed here once, not four times
  // behind the barrier), and the verdict on the pivots
  wave_lds_sync();
  if (r < NB) {
    const double dc = lds[L_PATCH + patch * (16 * TP_PS) + min(r, nb - 1) * (TP_PS + 1)];
    if (!(dc > 0.0)) reinterpret_cast<int*>(lds + L_INT)[I_FAIL] = stamp;  // non-positive (or NaN) pivot in a pivot column of step stamp - 1
    lds[L_LINV + buf * (16 * TP_PS) + r * TP_PS + 16] = fast_rsqrt(dc);
  }
#ifdef AVM_TP
  AVM_PRIO_BULK_CHOL();
#else
  __builtin_amdgcn_s_setprio(0);
#endif
}

// Sum over the 16 lanes of a DPP row: lane i adds lane i - 1, - 2, - 4, - 8 in that order; the result is valid in lane 15 of every row
// (row_shr with bound_ctrl: a lane without a source adds 0).  wave_sum_shr's (devmath.hpp) first four steps.
AVM_DEV double tp_row_sum(double v) {
  v += dpp_d<0x111>(v);
  v += dpp_d<0x112>(v);
  v += dpp_d<0x114>(v);
  v += dpp_d<0x118>(v);
  return v;
}

// Factor the assembled system and solve it: (H' + mu D^2) y = g', y -> lds[L_Y .. L_Y + NF).  Returns false on a non-positive pivot
// (uniform over the workgroup).  Called by every wavefront of the workgroup, WV = the caller's wavefront; the tiles live on wavefronts 0..3
// (tp_owner) - the latency build's wavefronts 4..7 hold none and only take part in the barriers and the count.
// (tile indices and LDS slots as constants of the instantiation: left to the optimizer, one of the four wavefronts' tile arrays ended up in scratch memory)
#ifdef AVM_PROF_CHOL  // (development: where a factorization's time goes, per wavefront; slots 56.. of the profile: chain, wait b, solve, wait d, update, rest)
#define CPROF_T0() long long cp__ = clock64()
#define CPROF(slot) do { if (c.prof && lane == 0 && WV == AVM_PROF_CHOL) { long long n__ = clock64(); c.prof[56 + (slot)] += n__ - cp__; cp__ = n__; } } while (0)
#else
#define CPROF_T0() ((void)0)
#define CPROF(slot) ((void)0)
#endif
#define TPI(k, i) (std::integral_constant<int, tp_idx(WV, k, i)>::value)
#define TPW(k, i) (std::integral_constant<int, tp_wslot(k, i)>::value)
template <int WV>
AVM_NOINL bool chol_regs() {
  double* lds = LDS();
  const int lane = threadIdx.x & 63, lk = lane >> 4, lr = lane & 15;
  int* s_fail = reinterpret_cast<int*>(lds + L_INT) + I_FAIL;
  constexpr int NTL = tp_ntiles(WV) > 0 ? tp_ntiles(WV) : 1;
  d4 T[NTL];
#ifdef AVM_PROF_CHOL
  const long long cp_in__ = clock64();
#endif
  // ---- load, in elimination order (structural zeros included; a tile of the pattern the assembled system cannot reach starts as zero: it is fill).
  // Two passes, each with all its memory operations in flight: the offsets of every tile (left alone the compiler waited for one 8-byte load
  // per tile before the next: 13 trips to the L2 in a row), then the entries.
  typedef unsigned short us4 __attribute__((ext_vector_type(4)));
  us4 off[NTL];
  sfor<TPT>([&](auto I) {
    constexpr int i = I;
    if constexpr (tp_owner(i) == WV) {
      sfor<i + 1>([&](auto K) {
        constexpr int k = K;
        if constexpr (tp_nz(k, i) && TPP.h[k][i])
          off[TPI(k, i)] = *reinterpret_cast<const __attribute__((address_space(1))) us4*>(
              (const __attribute__((address_space(1))) unsigned short*)&tp_offsets.o[tp_h_ord(k, i)][0][0] + 4 * lane);
      });
    }
  });
  __builtin_amdgcn_sched_barrier(0);
  sfor<TPT>([&](auto I) {
    constexpr int i = I;
    if constexpr (tp_owner(i) == WV) {
      sfor<i + 1>([&](auto K) {
        constexpr int k = K;
        if constexpr (tp_nz(k, i)) {
          d4& t = T[TPI(k, i)];
          if constexpr (TPP.h[k][i]) {
#pragma unroll
            for (int r = 0; r < 4; r++) t[r] = lds[off[TPI(k, i)][r]];
          } else {
            t = d4{0, 0, 0, 0};
          }
        }
      });
    }
  });
  typedef __attribute__((address_space(3))) int lds_int_t;
  lds_int_t* s_cnt = reinterpret_cast<lds_int_t*>((uintptr_t)(L_INT * 8 + I_CNT * 4));
  if (threadIdx.x == 0) *s_fail = 0, *s_cnt = 0;
  const WinCtx& c = lds_ctx();
#ifdef AVM_PROF_CHOL
  if (c.prof && lane == 0 && WV == AVM_PROF_CHOL) c.prof[61] += clock64() - cp_in__;  // the load
#endif
  PROF_T0();
  __syncthreads();  // every tile is in registers: the union region becomes the factorization's scratch
  PROF(c, 4);
  CPROF_T0();
  // by the owner of pivot column k: diagonal tile (staged in its step's patch) -> chain -> L~_kk^T back into the tile, L~_kk^-T in buffer tp_buf(k)
  d4 Dlast = {0, 0, 0, 0};  // the last diagonal tile as it was before its chain (its column TP_NBL is the right-hand side)
  auto run_chain = [&](auto K) {
    constexpr int k = K;
    CPROF(4);
    d4& D = T[TPI(k, k)];
    if constexpr (tp_step_of(k) == 0) {  // (the later ones were staged by the step before)
#pragma unroll
      for (int r = 0; r < 4; r++) lds[L_PATCH + tp_slot_of(k) * (16 * TP_PS) + (lk + 4 * r) * TP_PS + lr] = D[r];
    }
    wave_lds_sync();
    tp_diag_chain(k == TPT - 1 ? TP_NBL : 16, tp_slot_of(k), tp_buf(k), tp_step_of(k) + 1);
    wave_lds_sync();
    // the diagonal tile becomes L~_kk^T (entry (a, b) = L~[b][a]); the patch is free for the next step's chain
#pragma unroll
    for (int r = 0; r < 4; r++) D[r] = lds[L_PATCH + tp_slot_of(k) * (16 * TP_PS) + lr * TP_PS + lk + 4 * r];
    CPROF(0);
  };
  sfor<2>([&](auto A) {
    constexpr int k = tp_step_piv(0, A);
    if constexpr (tp_owner(k) == WV) run_chain(std::integral_constant<int, k>{});
  });
  bool failed = false;
  sfor<TP_NSTEP>([&](auto TT) {
    constexpr int t = TT;
    if (failed) return;  // (uniform)
    CPROF(4);
    __syncthreads();  // (b) L~_kk^-T of this step's pivot columns are published; every wavefront is done with step t - 1
    CPROF(1);
    // (a chain stamps a non-positive pivot with its step + 1: the next chains may already run while a slow wavefront reads this, and
    //  all four have to take the same way out)
    {
      const int f = *s_fail;
      if (f != 0 && f <= t + 1) {
        failed = true;
        return;
      }
    }
    // (c) W(k, i) = L_kk^-1 U(k, i) for this wavefront's columns i > k: the final factor tiles, published for the others' updates
    sfor<tp_step_np(t)>([&](auto A) {
      constexpr int k = tp_step_piv(t, A);
      constexpr int nb = k == TPT - 1 ? TP_NBL : 16;
      if constexpr (tp_row_held(WV, k) || (k == TPT - 1 && tp_owner(k) == WV)) {
        // A operand of the solves: L_kk^-1[i' = lr][k' = lk + 4 m] = L~^-T[k'][i'] / sqrt(d_i'); the row scaling is applied to the product
        double aop[4], isq4[4];
        const double* LT = lds + L_LINV + tp_buf(k) * (16 * TP_PS);
#pragma unroll
        for (int m = 0; m < 4; m++) {
          const double v = LT[(lk + 4 * m) * TP_PS + lr];
          aop[m] = (lk + 4 * m < nb && lr < nb) ? v : 0.0;
          isq4[m] = LT[min(lk + 4 * m, nb - 1) * TP_PS + 16];
        }
        if constexpr (k == TPT - 1 && tp_owner(k) == WV) {  // the last diagonal tile gives up the right-hand side: z_10 = L^-1 b
          d4 Za = {0, 0, 0, 0}, Zb = {0, 0, 0, 0};
          Za = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[0], Dlast[0], Za, 0, 0, 0);
          Zb = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[1], Dlast[1], Zb, 0, 0, 0);
          Za = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[2], Dlast[2], Za, 0, 0, 0);
          Zb = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[3], Dlast[3], Zb, 0, 0, 0);
#pragma unroll
          for (int r = 0; r < 4; r++)
            if (lr == TP_NBL && lk + 4 * r < TP_NBL) lds[L_ZV + 16 * k + lk + 4 * r] = (Za[r] + Zb[r]) * isq4[r];
        }
        sfor<TPT - 1 - k>([&](auto II) {
          constexpr int i = k + 1 + II;
          if constexpr (tp_owner(i) == WV && tp_nz(k, i)) {
            d4& U = T[TPI(k, i)];
            d4 Wa = {0, 0, 0, 0}, Wb = {0, 0, 0, 0};
            Wa = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[0], U[0], Wa, 0, 0, 0);
            Wb = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[1], U[1], Wb, 0, 0, 0);
            Wa = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[2], U[2], Wa, 0, 0, 0);
            Wb = __builtin_amdgcn_mfma_f64_16x16x4f64(aop[3], U[3], Wb, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; r++) {
              U[r] = (Wa[r] + Wb[r]) * isq4[r];
              lds[L_WROW + TPW(k, i) * 256 + r * 64 + lane] = U[r];
            }
            if constexpr (i == TPT - 1) {  // the right-hand side column of tile column 10 is z_k
#pragma unroll
              for (int r = 0; r < 4; r++)
                if (lr == TP_NBL) lds[L_ZV + 16 * k + lk + 4 * r] = U[r];
            }
          }
        });
      }
    });
    if constexpr (t < TP_NSTEP - 1) {
      // the owner of a pivot column q of the next step needs nothing but its own W(k, q) for tile (q, q): it is updated and staged in the
      // patch before the count, while the wavefronts with more tiles in this step's rows still solve; the chain starts right behind it
      sfor<tp_step_np(t + 1)>([&](auto B) {
        constexpr int q = tp_step_piv(t + 1, B);
        if constexpr (tp_owner(q) == WV) {
          d4& U = T[TPI(q, q)];
          sfor<tp_step_np(t)>([&](auto A) {
            constexpr int k = tp_step_piv(t, A);
            if constexpr (tp_nz(k, q)) {
              const d4& Wd = T[TPI(k, q)];
#pragma unroll
              for (int r = 0; r < 4; r++) U = __builtin_amdgcn_mfma_f64_16x16x4f64(-Wd[r], Wd[r], U, 0, 0, 0);
            }
          });
          if constexpr (q == TPT - 1) Dlast = U;
#pragma unroll
          for (int r = 0; r < 4; r++) lds[L_PATCH + tp_slot_of(q) * (16 * TP_PS) + (lk + 4 * r) * TP_PS + lr] = U[r];
        }
      });
      CPROF(2);
      // (d) this step's rows of W are published - counted, not a barrier: the owner of a next pivot column needs nobody's tiles for its chain
      // and does not wait (1 K cycles per step it spent at a barrier for the wavefronts with more tiles to solve); everybody else waits for all four counts
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
      if (lane == 0) __hip_atomic_fetch_add(s_cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      auto wait_rows = [&]() {
        while (__hip_atomic_load(s_cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < (NT / 64) * (t + 1)) __builtin_amdgcn_s_sleep(1);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
      };
      if constexpr (tp_owns_piv(WV, t + 1)) {
        sfor<tp_step_np(t + 1)>([&](auto B) {
          constexpr int q = tp_step_piv(t + 1, B);
          if constexpr (tp_owner(q) == WV) run_chain(std::integral_constant<int, q>{});
        });
      }
      if constexpr (tp_ntiles(WV) > 0) wait_rows();
      CPROF(3);
      // (e) trailing update U(j, i) -= W(k, j)^T W(k, i), k < j <= i, over the tiles of this step's rows that exist (the next step's diagonal
      // tiles have theirs already), while the next chains run on their owners
      sfor<tp_step_np(t)>([&](auto A) {
        constexpr int k = tp_step_piv(t, A);
        sfor<TPT - 1 - k>([&](auto II) {
          constexpr int i = k + 1 + II;
          if constexpr (tp_owner(i) == WV && tp_nz(k, i)) {
            const d4& Wi = T[TPI(k, i)];
            sfor<i - k>([&](auto JJ) {
              constexpr int j = k + 1 + JJ;
              if constexpr (tp_nz(k, j) && !(j == i && tp_is_piv(t + 1, i))) {
                static_assert(tp_nz(j, i), "the pattern is closed under the elimination's fill");
                d4 Wj;
                if constexpr (tp_owner(j) == WV) {
                  Wj = T[TPI(k, j)];
                } else {
#pragma unroll
                  for (int r = 0; r < 4; r++) Wj[r] = lds[L_WROW + TPW(k, j) * 256 + r * 64 + lane];
                }
                d4& U = T[TPI(j, i)];
#pragma unroll
                for (int r = 0; r < 4; r++) U = __builtin_amdgcn_mfma_f64_16x16x4f64(-Wj[r], Wi[r], U, 0, 0, 0);
              }
            });
          }
        });
      });
    }
  });
  if (failed) return false;
  // (every wavefront is past the last step's barrier: nobody reads a row of W any more, and the partial sums of the back substitution live there)
  if constexpr (WV < TP_NWO)
    for (int q = lane; q < TP_NPOS; q += 64) lds[L_PARTV + WV * TP_NPOS + q] = 0.0;
  __syncthreads();  // z is complete in lds[L_ZV]
  PROF(c, 5);
  if (*s_fail) return false;
  // ---- backward substitution L^T x = z by the same steps, last to first; x_i replaces z_i (elimination order) and goes to lds[L_Y] (the system's order)
  d4 E[TPT - 1];  // E[k] += U(k, i) .* x_i over this wavefront's columns i > k (element-wise: reduced once, when block k is due)
#pragma unroll
  for (int k = 0; k < TPT - 1; k++) E[k] = d4{0, 0, 0, 0};
  sfor<TP_NSTEP>([&](auto TR) {
    constexpr int t = TP_NSTEP - 1 - TR;
    sfor<tp_step_np(t)>([&](auto A) {
      constexpr int i = tp_step_piv(t, A);
      constexpr int nb = i == TPT - 1 ? TP_NBL : 16;
      constexpr int PB = L_PATCH + tp_slot_of(i) * (16 * TP_PS);
      if constexpr (tp_owner(i) == WV) {
        // v = z_i - the four partial sums; L~_ii back into the patch in [row][column] form; the 16-step chain of chol_solve_block
        const d4& D = T[TPI(i, i)];
#pragma unroll
        for (int r = 0; r < 4; r++) lds[PB + lr * TP_PS + lk + 4 * r] = D[r];
        const int rr = min(lr, nb - 1);
        double bv = lds[L_ZV + 16 * i + rr];
#pragma unroll
        for (int w = 0; w < TP_NWO; w++) bv -= lds[L_PARTV + w * TP_NPOS + 16 * i + rr];
        wave_lds_sync();
        double colv[16];
#pragma unroll
        for (int q = 0; q < 16; q++) colv[q] = lds[PB + q * TP_PS + rr];
        const double isq = fast_rsqrt(lds[PB + rr * (TP_PS + 1)]), di2 = isq * isq;
        bv *= isq;
#pragma unroll
        for (int q = 0; q < 16; q++) colv[q] *= di2;
        double xout = 0.0;
        // x_jj is lane jj's bv; every lane subtracts colv[jj] x_jj - the broadcast as the multiply-add's own DPP operand (v_fmac_f64_dpp row_newbcast: no trip
        // through the scalar registers; the s_nop is the two wait states a DPP read needs behind the VALU write of the same register).  Round 6: bit-identical
        // to the 2 v_readlane_b32 + v_fma_f64 per step it replaced, solve 9.29 -> 9.21 ms; commit 24fd667 is the last that has that form.
        sfor<nb>([&](auto JR) {
          constexpr int jj = nb - 1 - JR;
          xout = lr == jj ? bv : xout;
          const double nc = -colv[jj];
          asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, %0, %1 row_newbcast:%2 row_mask:0xf bank_mask:0xf" : "+v"(bv) : "v"(nc), "n"(jj));
        });
        if (lane < nb) {
          lds[L_ZV + 16 * i + lane] = xout;
          const int col = tp_perm_dev(16 * i + lane);
          if (col != TP_PAD) lds[L_Y + col] = xout;
        }
        wave_lds_sync();
        // fold x_i into the element-wise accumulators of the blocks above (lane (lk, lr): column lr of every tile)
        const double xl = lr < nb ? lds[L_ZV + 16 * i + min(lr, nb - 1)] : 0.0;
        sfor<i>([&](auto K) {
          constexpr int k = K;
          if constexpr (tp_nz(k, i)) {
            const d4& U = T[TPI(k, i)];
#pragma unroll
            for (int r = 0; r < 4; r++) E[k][r] = fma(U[r], xl, E[k][r]);
          }
        });
      }
    });
    if constexpr (t > 0) {
      // every wavefront that holds a tile of a row the next step solves: its share of that block is complete (all its columns beyond it have been
      // folded in); the others' partial sums stay the zeros they were set to
      sfor<tp_step_np(t - 1)>([&](auto B) {
        constexpr int p = tp_step_piv(t - 1, B);
        if constexpr (tp_row_held(WV, p)) {
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const double sacc = tp_row_sum(E[p][r]);
            if (lr == 15) lds[L_PARTV + WV * TP_NPOS + 16 * p + lk + 4 * r] = sacc;
          }
        }
      });
      __syncthreads();
    }
  });
  __syncthreads();
  PROF(c, 6);
  return true;
}
#undef TPI
#undef TPW
// the factorization's compile-time tables of this build for the tests (tests/test_tp_pattern.py states them in numpy): T = TPT tile columns,
// out[0 .. T T) = TPP.h, [T T .. 2 T T) = TPP.nz (both [k][i]), then tp_owner [T], then tp_perm of the 16 T positions (-1: padding)
int tp_pattern_export(int* out) {
  for (int k = 0; k < TPT; k++)
    for (int i = 0; i < TPT; i++) out[k * TPT + i] = TPP.h[k][i], out[TPT * TPT + k * TPT + i] = TPP.nz[k][i];
  for (int i = 0; i < TPT; i++) out[2 * TPT * TPT + i] = tp_owner(i);
  for (int n = 0; n < 16 * TPT; n++) out[2 * TPT * TPT + TPT + n] = tp_perm(n);
  return 2 * TPT * TPT + TPT + 16 * TPT;
}
