// Fused posterior sweep for gfx950 -- the hot kernel of the engine: one uniform 16-wave workgroup per
// compute unit.  Included once per kernel kind (TGP_SWEEP_KIND) by tgp_kernels_sweep_k*.hip so the four
// kinds compile in parallel.
//
// For a block of 128 candidates x_j one workgroup computes, without ever writing an [N, M] intermediate
// to HBM as a product,
//     k*_j   = k(X, x_j)                      (generated once per block, tile by tile)
//     c_j    = W k*_j,  W = L^-1              (f64 MFMA triangular GEMM)
//     var_j  = clip(variance - |c_j|^2)       (fused column norms)
//     mean_j = k*_j . alpha + c               (fused dot with alpha = K^-1 (Y - c))
//     acq_j  = EI / PI / -LCB / AEI           (fused tail)
//     block (max, first index)                (wave shuffles + LDS)
// Replaces the arithmetic of (reference): GPflowPredictor.predict_encoded / predict_joint_encoded
// (trieste/models/gpflow/interface.py:119-133, i.e. gpflow base_conditional_with_lm: A = L^-1 Kmn;
// fvar = Knn - sum A^2; fmean = (L^-T A)^T err), expected_improvement.__call__
// (acquisition/function/function.py:215-223) and the arg-max of _get_max_discrete_points
// (acquisition/optimizer.py:124-150).
//
// Data layout: Wt [Npad][Npad] holds W transposed (Wt[k][i] = W[i][k]) so that a [16 x 256] operand tile
// is 16 contiguous 2 KiB rows in HBM and lands in LDS k-major, which is the layout a
// v_mfma_f64_16x16x4_f64 A-fragment read wants (16 consecutive i per k).  Rows are padded by 16 doubles
// in LDS so the 4 k-rows of a fragment read hit disjoint bank halves.
//
// What the measurements on MI355X say (profiles/r01_ubench_fp64.txt, DESIGN.md section 4):
//   * one wave issues an f64 MFMA at most every 128 cycles, the pipe retires one per 64: a SIMD needs
//     at least two MFMA-ready waves at every moment, and with exactly two (the wave-specialised
//     kernel, tools/legacy_kernels/sweep_ws.inc) every stall of either wave is pipe time lost for good;
//   * every workgroup barrier is dead pipe time for the whole workgroup (halving the k-step, i.e.
//     doubling the barriers, cost 7 %), and fp64 VALU work steals MFMA issue time.
// So: FOUR identical waves per SIMD (1024 threads), wave tile 64 x 32 (8 accumulator fragments = 64
// VGPR inside a 128-VGPR budget), workgroup tile 256 rows of W x 128 candidates, 16-row k-steps,
// double-buffered LDS, one __syncthreads per k-step.  Every thread stages 2 x 16 B of the Wt tile
// and 2 doubles of the K* tile per step: global -> registers while the MFMAs of the current tile
// run -> LDS for the next tile.
//
// K* is generated once per candidate block in the diagonal block-steps and kept in a per-workgroup
// HBM slab (8 bytes of HBM traffic per entry and row block are free; ~60 fp64 VALU instructions per
// entry and row block were 25 % of the sweep).  The scaled candidate coordinates live in LDS so the
// generating steps need no long-lived registers.
#include "tgp_dev.hpp"
#include "tgp_internal.hpp"

#ifndef TGP_EXP
#define TGP_EXP 0  // timing experiments of tools/build_exp.sh (wrong results): 1 no step barrier, 2 no LDS staging
                   // stores, 4 no global loads, 8 no LDS operand reads, 16 no K* generation, 32 stage tile t+1 at the start of step t, 64 (with 2) loads stay live, 128 no Wt loads, 256 no slab loads, 512 compiler-merged ds_read2_b64 operand loads
#endif

namespace tgp {
namespace {

constexpr int UBM = 256, UBN = 128, UBK = 16;
constexpr int ULDA = UBM + 16, ULDB = UBN + 16;
constexpr int UKSTEPS = UBM / UBK;
constexpr int U_STAGE = UBK * ULDA + UBK * ULDB;  // doubles per stage

// JOINT: the 128 columns are two halves of 64; each half packs floor(64 / q) groups of q candidates.
// Every completed 256-row block of C = W K* is also written to a per-workgroup slab in HBM; after the
// sweep the 16 waves compute the 64 x 64 Gram S = C^T C of each half from the slab (2 fragments per
// wave, MFMA, operands straight from L2) and cov = K** - S is emitted for the q x q diagonal blocks
// (== GPflowPredictor.predict_joint_encoded, interface.py:126-133).  The extra MFMA work is
// 2 * 64 * 64 * N per block against 128 * N^2: about 6 % at N = 2048.
//
// SPLIT (launches with few candidate blocks, e.g. EGO's default 8000-candidate sweep): the work item is
// (candidate block, row group) instead of a whole block -- the group walks only its row blocks of W,
// generates the K* rows it meets for the first time, and leaves partial (k*.alpha, sum c^2) for
// sweep_combine_kernel (tgp_kernels_misc.hip), which runs the common tail.
//
// WIDE inputs (DP == DP_WIDE: dp > MAX_D, a multiple of WIDE_CHUNK, DESIGN.md 4.7): [dp][128] candidate coordinates would not fit
// beside the two stages (2 x 52 KiB + 64 KiB at dp = 64 > 160 KiB), so they go to a per-workgroup tile in device scratch (a.xqw,
// written once per candidate block, read back from L2 / L1 coalesced over the 128 columns) and the generating steps walk the
// coordinates in a run-time loop.  Nothing else changes: every other step already reads K* back from the slab.
template <int KIND, int DP, bool JOINT, bool SPLIT>
__global__ __launch_bounds__(1024, 4) void sweep_kernel(const SweepArgs a) {
  constexpr bool WIDE = DP == DP_WIDE;
  __shared__ __attribute__((aligned(16))) double smem[2 * U_STAGE + UBN * DP];
  const int dpr = WIDE ? a.m.dp : DP;   // the padded dimension (a constant unless WIDE)
  // [DP][128] scaled candidate coordinates
  double* const xqs = WIDE ? a.xqw + (size_t)blockIdx.x * (size_t)dpr * UBN : smem + 2 * U_STAGE;

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;  // 4 (M) x 4 (N) waves, wave tile 64 x 32
  const int64_t Npad = a.m.Npad;
  const int nb = (int)(Npad / UBM);
  const int d = a.m.d;
  const double variance = a.m.variance;
  const double* __restrict__ Wt = a.m.Wt;

  // staging coordinates
  const int wrow0 = tid >> 7, wcol = (tid & 127) * 2;         // Wt tile: rows wrow0, wrow0 + 8; 2 doubles
  const int kcol = tid & 127;                                  // K* tile: candidate column
  const int krg = __builtin_amdgcn_readfirstlane(tid >> 7);   // row group 0..7 -> rows 2 krg, 2 krg + 1

  double* const mred = smem;         // [8][128]   reduction scratch (aliases stage 0 after the sweep)
  double* const sred = smem + 1024;  // [4][128]
  double* const bvs = smem + 1536;
  int64_t* const bis = (int64_t*)(smem + 1540);

  double* const kc = a.kcache + (size_t)blockIdx.x * (size_t)Npad * UBN;
  // SPLIT only: the candidate count may live on the device (the repair pass of the split-precision sweep)
  const int64_t Mrun = (SPLIT && a.M_dev) ? *a.M_dev : a.M;
  const int64_t nblk = JOINT ? (a.G + 2 * (64 / a.q) - 1) / (2 * (64 / a.q)) : (Mrun + UBN - 1) / UBN;
  double* const aslab = JOINT ? a.aslab + (size_t)blockIdx.x * (size_t)Npad * UBN : nullptr;
  // SPLIT (few candidate blocks): work item = (block, row group); the group walks only its row blocks
  // [ib0, ib1) of W, generates the K* rows it meets for the first time, and leaves partial sums.
  const int ngrp = SPLIT ? a.split_g : 1;

  for (int64_t wk = blockIdx.x; wk < nblk * ngrp; wk += gridDim.x) {
    const int64_t blk = SPLIT ? wk / ngrp : wk;
    // the groups differ in work (whole row blocks); a workgroup's items alternate heavy-first / light-first
    // (the flip depends on the block alone, so (block, group) stays a bijection for any grid size)
    const int gsel = SPLIT ? (int)(wk % ngrp) : 0;
    const int64_t per_round = SPLIT ? ((int64_t)gridDim.x / ngrp > 0 ? (int64_t)gridDim.x / ngrp : 1) : 1;
    const int grp = (SPLIT && ((blk / per_round) & 1)) ? ngrp - 1 - gsel : gsel;
    const int ib0 = SPLIT ? a.split_ib[grp] : 0, ib1 = SPLIT ? a.split_ib[grp + 1] : nb;
    const int T = (ib1 * (ib1 + 1) - ib0 * (ib0 + 1)) / 2 * UKSTEPS;
    for (int e = tid; e < UBN * dpr; e += 1024) {  // scale the block's candidates once (c-major)
      const int j = e / dpr, c = e % dpr;
      int64_t cand;
      if constexpr (!JOINT) {
        cand = blk * UBN + j;
      } else {
        const int q = a.q, gp = 64 / q, cc = j & 63;
        const int64_t g = (blk * 2 + (j >> 6)) * gp + cc / q;
        cand = (cc < gp * q && g < a.G) ? g * q + cc % q : Mrun;
      }
      const int64_t src = cand < Mrun ? cand : 0;
      xqs[c * UBN + j] = (c < d) ? a.Xq[src * d + c] / as_const(a.m.ls)[c] : 0.0;
    }
    v4d acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    double ssq0 = 0.0, ssq1 = 0.0, macc = 0.0;
    v2d wreg0, wreg1;
    double kv[2];
    __syncthreads();  // xqs is read by other threads below

    // K* rows of block kb are generated at their first use by this work item: the diagonal step when the
    // item starts at row block 0, otherwise everything below ib0 is met for the first time at ib == ib0
    auto first_use = [&](int ib, int kb) { return SPLIT ? ib == (kb > ib0 ? kb : ib0) : kb == ib; };
    auto issue_loads = [&](int ib, int kb, int ks) {
      const int64_t krow = (int64_t)kb * UBM + ks * UBK;
      const double* src = Wt + (krow + wrow0) * Npad + (int64_t)ib * UBM + wcol;
      if (!(TGP_EXP & (4 | 128))) {
        wreg0 = *(const v2d*)src;
        wreg1 = *(const v2d*)(src + 8 * Npad);
      }
      if (!first_use(ib, kb) && !(TGP_EXP & (4 | 256))) {
        const double* kcp = kc + (krow + 2 * krg) * UBN + kcol;
#pragma unroll
        for (int r = 0; r < 2; ++r) kv[r] = kcp[r * UBN];
      }
    };
    auto finish_tile = [&](int buf, int ib, int kb, int ks) {
      const int64_t krow0 = (int64_t)kb * UBM + ks * UBK + 2 * krg;
      if (first_use(ib, kb) && !(TGP_EXP & 16)) {  // generate this thread's two entries (first use of the rows)
        const cptr xs = as_const(a.m.Xs + krow0 * dpr);
        const cptr al = as_const(a.m.alpha + krow0);
        double r2[2] = {0.0, 0.0};
        if constexpr (WIDE) {
          // chunks of 8 coordinates: eight coalesced loads of the tile in flight, the two training rows by scalar loads
          const double* const xw = xqs + kcol;
          for (int c0 = 0; c0 < dpr; c0 += 8) {
            double x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = xw[(c0 + u) * UBN];
#pragma unroll
            for (int u = 0; u < 8; ++u)
#pragma unroll
              for (int r = 0; r < 2; ++r) {
                const double t0 = x[u] - xs[r * dpr + c0 + u];
                r2[r] = fma(t0, t0, r2[r]);
              }
          }
        } else {
#pragma unroll
          for (int c = 0; c < DP; ++c) {
            const double x = xqs[c * UBN + kcol];
#pragma unroll
            for (int r = 0; r < 2; ++r) {
              const double t0 = x - xs[r * DP + c];
              r2[r] = fma(t0, t0, r2[r]);
            }
          }
        }
#pragma unroll
        for (int r = 0; r < 2; ++r) kv[r] = kernel_from_r2<KIND>(r2[r], variance);
        double* kcp = kc + krow0 * UBN + kcol;
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          if (!SPLIT || kb == ib) macc = fma(kv[r], al[r], macc);  // the mean term belongs to the diagonal owner
          if (ib1 - ib0 > 1 || SPLIT) kcp[r * UBN] = kv[r];
        }
      }
      double* sA = smem + buf * U_STAGE;
      double* sB = sA + UBK * ULDA + (2 * krg) * ULDB + kcol;
      if (TGP_EXP & 64) {  // keep the loads (and their wait) alive without the LDS stores
        asm volatile("" ::"v"(wreg0), "v"(wreg1), "v"(kv[0]), "v"(kv[1]));
      }
      if (!(TGP_EXP & 2)) {
        *(v2d*)(sA + wrow0 * ULDA + wcol) = wreg0;
        *(v2d*)(sA + (wrow0 + 8) * ULDA + wcol) = wreg1;
#pragma unroll
        for (int r = 0; r < 2; ++r) sB[r * ULDB] = kv[r];
      }
    };

    // Staging schedule.  Default: the loads of tile t+1 are issued at the start of step t and written to LDS at its
    // END, before the barrier.  TGP_EXP bit 5 (development builds) selects the other textbook order -- tile t+1
    // written at the START of step t, loads of tile t+2 re-issued at once -- which measured 1.5 % SLOWER here
    // (0.795 vs 0.807 of peak on the headline, profiles/r02_sweep_knockout.txt): the knock-out runs there show that
    // what the staging costs is the Wt loads themselves (3.3 points), not where the stores sit (2.5 points).
    auto advance = [&](int& i_b, int& k_b, int& k_s) {
      if (++k_s == UKSTEPS) {
        k_s = 0;
        if (++k_b > i_b) {
          k_b = 0;
          ++i_b;
        }
      }
    };
    constexpr bool STAGE_EARLY = (TGP_EXP & 32) != 0;
    int ib = ib0, kb = 0, ks = 0, buf = 0;
    int nib = ib0, nkb = 0, nks = 0;  // tile t + 1
    issue_loads(ib0, 0, 0);
    finish_tile(0, ib0, 0, 0);
    advance(nib, nkb, nks);
    if (STAGE_EARLY && T > 1) issue_loads(nib, nkb, nks);  // the registers hold tile 1
    __syncthreads();
    for (int t = 0; t < T; ++t) {
      const bool has_next = t + 1 < T;
      int n2ib = nib, n2kb = nkb, n2ks = nks;  // tile t + 2
      advance(n2ib, n2kb, n2ks);
      if (STAGE_EARLY) {
        if (has_next) finish_tile(buf ^ 1, nib, nkb, nks);
        if (t + 2 < T) issue_loads(n2ib, n2kb, n2ks);
      } else {
        if (has_next) issue_loads(nib, nkb, nks);
      }
      {
        // In a diagonal block-step (kb == ib) Wt[k][i] = 0 for i < k: when all 64 rows of this wave's
        // row quarter lie above the 16-row k-slab its A operand is all zero and the wave skips the
        // step's MFMAs (6 of the 16 steps of a diagonal block on average; the four waves of a SIMD own
        // the four row quarters, so the saving is SIMD-balanced).  Deliberately NOT per fragment row:
        // a per-fragment predicate inside the unrolled loop made the compiler move half the MFMAs out
        // of line behind taken branches and full LDS waits (or, as two code paths, spill 116 VGPRs);
        // the extra 1.5 steps per diagonal block it saved are not worth a branchy hot loop.
        const bool all_zero = kb == ib && ks * UBK >= wm * 64 + 64;
        const double* sA = smem + buf * U_STAGE;
        const double* ab = sA + (lane >> 4) * ULDA + wm * 64 + (lane & 15);
        const double* bb = sA + UBK * ULDA + (lane >> 4) * ULDB + wn * 32 + (lane & 15);
        __builtin_amdgcn_s_setprio(2);  // MFMA-ready waves issue ahead of staging waves (+1.5 %)
        if (!all_zero) {
#pragma unroll
          for (int k4 = 0; k4 < UBK / 4; ++k4) {
            double av[4], bv[2];
            if constexpr ((TGP_EXP & (8 | 512)) == 0) {
              // six single ds_read_b64 (2 LDS-array cycles each) instead of the three ds_read2_b64 (8 cycles each, half
              // the LDS rate) the compiler merges the plain loads into: +1 % (0.812 -> 0.821 of peak at 2^18
              // candidates; TGP_EXP bit 9 = the compiler's form)
              const uint32_t la = (uint32_t)(size_t)(__attribute__((address_space(3))) const double*)ab;
              const uint32_t lb = (uint32_t)(size_t)(__attribute__((address_space(3))) const double*)bb;
              asm volatile(
                  "ds_read_b64 %0, %6 offset:%c8\n\t"
                  "ds_read_b64 %1, %6 offset:%c9\n\t"
                  "ds_read_b64 %4, %7 offset:%c12\n\t"
                  "ds_read_b64 %2, %6 offset:%c10\n\t"
                  "ds_read_b64 %3, %6 offset:%c11\n\t"
                  "ds_read_b64 %5, %7 offset:%c13\n\t"
                  "s_waitcnt lgkmcnt(0)"
                  : "=&v"(av[0]), "=&v"(av[1]), "=&v"(av[2]), "=&v"(av[3]), "=&v"(bv[0]), "=&v"(bv[1])
                  : "v"(la), "v"(lb), "n"(k4 * 4 * ULDA * 8), "n"(k4 * 4 * ULDA * 8 + 128), "n"(k4 * 4 * ULDA * 8 + 256),
                    "n"(k4 * 4 * ULDA * 8 + 384), "n"(k4 * 4 * ULDB * 8), "n"(k4 * 4 * ULDB * 8 + 128)
                  : "memory");
            } else {
#pragma unroll
              for (int f = 0; f < 4; ++f) av[f] = (TGP_EXP & 8) ? (double)(lane + f + k4) : ab[k4 * 4 * ULDA + f * 16];
#pragma unroll
              for (int f = 0; f < 2; ++f) bv[f] = (TGP_EXP & 8) ? (double)(lane - f) : bb[k4 * 4 * ULDB + f * 16];
            }
#pragma unroll
            for (int fm = 0; fm < 4; ++fm)
#pragma unroll
              for (int fn = 0; fn < 2; ++fn) acc[fm][fn] = mfma_f64(av[fm], bv[fn], acc[fm][fn]);
          }
        }
      }
      __builtin_amdgcn_s_setprio(0);
      if (!STAGE_EARLY && has_next) finish_tile(buf ^ 1, nib, nkb, nks);
      if (ks == UKSTEPS - 1 && kb == ib) {  // row block ib complete: fold into the column norms
        if constexpr (JOINT) {
          double* dst = aslab + ((int64_t)ib * UBM + wm * 64 + (lane >> 4)) * UBN + wn * 32 + (lane & 15);
#pragma unroll
          for (int fm = 0; fm < 4; ++fm)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              dst[(fm * 16 + 4 * r) * UBN] = acc[fm][0][r];
              dst[(fm * 16 + 4 * r) * UBN + 16] = acc[fm][1][r];
            }
        }
#pragma unroll
        for (int fm = 0; fm < 4; ++fm)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            ssq0 = fma(acc[fm][0][r], acc[fm][0][r], ssq0);
            ssq1 = fma(acc[fm][1][r], acc[fm][1][r], ssq1);
          }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
      }
      if (!(TGP_EXP & 1)) __syncthreads();
      buf ^= 1;
      ib = nib;
      kb = nkb;
      ks = nks;
      nib = n2ib;
      nkb = n2kb;
      nks = n2ks;
    }
    if constexpr (JOINT) {
      // ---- Gram phase: S_h = C_h^T C_h for the two 64-column halves, from the slab -----------------
      __syncthreads();  // the slab stores of every wave are visible to the workgroup
      const int h = w >> 3, f0 = (w & 7) * 2;      // this wave: half h, Gram fragments f0, f0 + 1
      const int fa = f0 >> 2, fb = f0 & 3;         // fragment (fa, fb) and (fa, fb + 1)
      v4d g0 = (v4d){0.0, 0.0, 0.0, 0.0}, g1 = (v4d){0.0, 0.0, 0.0, 0.0};
      const double* pa = aslab + (int64_t)(lane >> 4) * UBN + h * 64 + fa * 16 + (lane & 15);
      const double* pb = aslab + (int64_t)(lane >> 4) * UBN + h * 64 + fb * 16 + (lane & 15);
      for (int64_t r0 = 0; r0 < Npad; r0 += 32) {
        double xa[8], xb0[8], xb1[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          xa[u] = pa[(r0 + 4 * u) * UBN];
          xb0[u] = pb[(r0 + 4 * u) * UBN];
          xb1[u] = pb[(r0 + 4 * u) * UBN + 16];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          g0 = mfma_f64(xa[u], xb0[u], g0);
          g1 = mfma_f64(xa[u], xb1[u], g1);
        }
      }
      double* const Sg = smem + 2048;  // [2][64][64] after the reduction scratch
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int aa = fa * 16 + (lane >> 4) + 4 * r, bb = fb * 16 + (lane & 15);
        Sg[h * 4096 + aa * 64 + bb] = g0[r];
        Sg[h * 4096 + aa * 64 + bb + 16] = g1[r];
      }
    }
    // ---- reductions (LDS is free after the last barrier) ---------------------------------------
    mred[krg * 128 + kcol] = macc;
    {  // (colnorm_reduce / colnorm_read of tgp_dev.hpp, written out: as calls they reorder this kernel's machine code)
      double s0 = ssq0, s1 = ssq1;
      s0 += __shfl_xor(s0, 16, 64);
      s0 += __shfl_xor(s0, 32, 64);
      s1 += __shfl_xor(s1, 16, 64);
      s1 += __shfl_xor(s1, 32, 64);
      if (lane < 16) {
        sred[wm * 128 + wn * 32 + lane] = s0;
        sred[wm * 128 + wn * 32 + 16 + lane] = s1;
      }
    }
    __syncthreads();
    if constexpr (SPLIT) {
      if (tid < 128) {
        double m = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) m += mred[g * 128 + tid];
        double* pp = a.part + ((size_t)blk * ngrp + grp) * 256;
        pp[tid] = m;
        pp[128 + tid] = (sred[tid] + sred[128 + tid]) + (sred[256 + tid] + sred[384 + tid]);
      }
      __syncthreads();  // scratch / xqs are rewritten by the next work item
      continue;
    }
    double val = -INFINITY;
    int64_t gidx = INT64_MAX;
    if constexpr (JOINT) {
      const int q = a.q, gp = 64 / q;
      if (tid < 128 && a.mean_out) {
        const int cc = tid & 63;
        const int64_t g = (blk * 2 + (tid >> 6)) * gp + cc / q;
        if (cc < gp * q && g < a.G) {
          double m = 0.0;
#pragma unroll
          for (int gg = 0; gg < 8; ++gg) m += mred[gg * 128 + tid];
          a.mean_out[g * q + cc % q] = m + a.m.mean_const;
        }
      }
      if (a.cov_out) {
        const double* const Sg = smem + 2048;
        const int per_half = gp * q * q;
        for (int e = tid; e < 2 * per_half; e += 1024) {
          const int hh = e / per_half, rem = e % per_half;
          const int gi = rem / (q * q), ab = rem % (q * q);
          const int aa = ab / q, bb = ab % q;
          const int64_t g = (blk * 2 + hh) * gp + gi;
          if (g >= a.G) continue;
          const int ca = gi * q + aa, cb = gi * q + bb;  // columns inside the half
          double r2 = 0.0;
          if constexpr (WIDE) {
            for (int c = 0; c < dpr; ++c) {
              const double tt = xqs[c * UBN + hh * 64 + ca] - xqs[c * UBN + hh * 64 + cb];
              r2 = fma(tt, tt, r2);
            }
          } else {
#pragma unroll
            for (int c = 0; c < DP; ++c) {
              const double tt = xqs[c * UBN + hh * 64 + ca] - xqs[c * UBN + hh * 64 + cb];
              r2 = fma(tt, tt, r2);
            }
          }
          double cv = kernel_from_r2<KIND>(r2, variance) - Sg[hh * 4096 + ca * 64 + cb];
          if (aa == bb) cv = fmax(cv, VAR_FLOOR);  // reference interface.py:130-132
          a.cov_out[(g * q + aa) * q + bb] = cv;
        }
      }
    }
    if (!JOINT && tid < 128) {
      const int64_t cj = blk * UBN + tid;
      if (cj < Mrun) {
        const double mean = mean_reduce(a, mred, tid);
        const double s = (sred[tid] + sred[128 + tid]) + (sred[256 + tid] + sred[384 + tid]);
        sweep_tail(a, cj, mean, fmax(variance - s, VAR_FLOOR), val, gidx);
      }
    }
    if (a.blk_val) block_winner(a, blk, val, gidx, bvs, bis, tid, w);
    __syncthreads();  // scratch / xqs are rewritten by the next block
  }
}

template <int KIND, bool JOINT, bool SPLIT>
hipError_t launch_sweep_dp(hipStream_t s, const SweepArgs& a, int64_t grid) {
  dim3 g((unsigned)grid), b(1024);
  if (a.m.dp <= MAX_D)
    return with_dp<MAX_D>(a.m.dp, [&](auto DP) {
      hipLaunchKernelGGL((sweep_kernel<KIND, DP(), JOINT, SPLIT>), g, b, 0, s, a);
      return hipGetLastError();
    });
  if (a.m.dp % WIDE_CHUNK != 0 || !a.xqw) return hipErrorInvalidValue;
  hipLaunchKernelGGL((sweep_kernel<KIND, DP_WIDE, JOINT, SPLIT>), g, b, 0, s, a);
  return hipGetLastError();
}

}  // namespace

#define TGP_CAT2(a, b) a##b
#define TGP_CAT(a, b) TGP_CAT2(a, b)
hipError_t TGP_CAT(launch_sweep_kind, TGP_SWEEP_KIND)(hipStream_t s, const SweepArgs& a, bool joint,
                                                          int64_t grid) {
  if (joint) return launch_sweep_dp<TGP_SWEEP_KIND, true, false>(s, a, grid);
  // (a device-side count forces the SPLIT instantiation even with one row group: its combine kernel runs the tail)
  return (a.split_g > 1 || (a.split_g == 1 && a.M_dev)) ? launch_sweep_dp<TGP_SWEEP_KIND, false, true>(s, a, grid)
                       : launch_sweep_dp<TGP_SWEEP_KIND, false, false>(s, a, grid);
}

}  // namespace tgp
