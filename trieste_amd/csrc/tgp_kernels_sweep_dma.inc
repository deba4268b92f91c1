// Fused posterior sweep, LDS-DMA staging form: the kernel of the large plain launches (>= 4 x #CU candidate blocks,
// dp <= 16).  Same tile (256 rows of W x 128 candidates, 16 waves, wave tile 64 x 32, 16-row k-steps), same
// arithmetic and summation order as sweep_kernel<KIND, DP, false, false> (tgp_kernels_sweep.inc) -- bit-identical
// results -- but nothing is staged through registers any more:
//   * the Wt tile of step t+2 and the K* tile of step t+1 (when it comes from the slab) travel global -> LDS
//     directly (global_load_lds_dwordx4: one 1 KiB row half / row per wave-instruction, written lane-linearly, which
//     a padded row-major tile is as long as one instruction stays inside a row);
//   * the A operand has THREE stages, so its loads have two steps of lead instead of one and are never waited for
//     with the data still in flight (knock-out runs, profiles/r02_sweep_knockout.txt: the Wt loads + staging stores
//     cost 6 points of MFMA utilisation in the register-staged kernel); the K* tile keeps two stages (LDS is full);
//   * no staging VGPRs (12 fewer live registers in a kernel at the 128-VGPR cap), no ds_write on the Wt path.
// hipcc does not count inline-asm memory operations: every wait on the DMA is an explicit counted s_waitcnt here,
// barriers are raw s_barrier.  Per step and wave the order of VMEM issue is  [K* row DMA (tile t+1)]
// [2 x Wt row-half DMA (tile t+2)] ... and the step ends with  s_waitcnt vmcnt(2): everything but the two newest
// operations (the Wt DMA of tile t+2) has landed -- tile t+1's operands are complete before the barrier that
// publishes them.  Generated K* tiles (diagonal block-steps) are written with ordinary ds_write / global stores; those
// stores are younger than the step's DMA, so vmcnt(2) in such a step also drains the Wt DMA (one step in 8.5).
// Round 4 (profiles/r04_defer_ab.txt, bit-identical outputs):
//   * TGP_DMA_DEFER: the MFMAs of a step's LAST k4-round run at the top of the NEXT step, from operands read before the
//     barrier -- every wave leaves the barrier with eight MFMAs in hand while the first operand reads of the new tile are
//     in flight (otherwise all 16 waves wait for LDS there with the matrix pipe idle).  Same MFMAs in the same order per
//     accumulator.  Headline 267.4 -> 265.3 ms, C2 18.68 -> 18.19 ms.
//   * TGP_DMA_SADDR: every DMA addressed as (uniform base in SGPRs) + (one shared 32-bit lane offset), the two LDS
//     operand addresses rebuilt from the lane offset in every step behind an opaque asm.  On its own this is SLOWER
//     (271.6 ms); it is what keeps the deferred form free of scratch reloads in the every-step path (with 64-bit per-lane
//     pointers the compiler spills one and reloads it in front of the DMA: 283 ms -- a scratch reload is an
//     s_waitcnt vmcnt(0) on everything in flight).
#include <type_traits>

#include "tgp_dev.hpp"
#include "tgp_internal.hpp"

namespace tgp {
namespace {

constexpr int DBM = 256, DBN = 128, DBK = 16;
constexpr int DLDA = DBM + 16, DLDB = DBN + 16;
constexpr int DKSTEPS = DBM / DBK;
constexpr int D_ASTAGE = DBK * DLDA;   // 4352 doubles
constexpr int D_BSTAGE = DBK * DLDB;   // 2304 doubles

// one wave-instruction: lane l copies 16 bytes from its own global address to LDS byte address lds_dst + 16 l
__device__ __forceinline__ void glds16(const void* gsrc, uint32_t lds_dst_uniform) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst_uniform)
      : "memory");
}

// the same with the global address as (uniform 64-bit base in SGPRs) + (32-bit per-lane byte offset): one loop-invariant
// VGPR serves every DMA of the kernel instead of a 64-bit per-lane pointer each (TGP_DMA_SADDR)
__device__ __forceinline__ void glds16s(const double* sbase_uniform, uint32_t voff, uint32_t lds_dst_uniform) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase_uniform), "s"(lds_dst_uniform)
      : "memory");
}

#ifndef TGP_DMA_SADDR
#define TGP_DMA_SADDR 1
#endif
#ifndef TGP_DMA_LADDR
#define TGP_DMA_LADDR TGP_DMA_SADDR
#endif

// One 16-row k-step of a wave: per k4-step six operand reads (single ds_read_b64: the compiler merges plain loads into
// half-rate ds_read2_b64) and the MFMAs of the live A fragments FM_LO..3.
#ifndef TGP_DMA_DEFER
#define TGP_DMA_DEFER 1
#endif
template <int FM_LO>
__device__ __forceinline__ void dma_kstep(v4d (&acc)[4][2], uint32_t la, uint32_t lb, double (&dav)[4], double (&dbv)[2]) {
#pragma unroll
  for (int k4 = 0; k4 < DBK / 4; ++k4) {
    double av[4], bv[2];
    asm volatile(
        "ds_read_b64 %0, %6 offset:%c8\n\t"
        "ds_read_b64 %1, %6 offset:%c9\n\t"
        "ds_read_b64 %4, %7 offset:%c12\n\t"
        "ds_read_b64 %2, %6 offset:%c10\n\t"
        "ds_read_b64 %3, %6 offset:%c11\n\t"
        "ds_read_b64 %5, %7 offset:%c13\n\t"
        "s_waitcnt lgkmcnt(0)"
        : "=&v"(av[0]), "=&v"(av[1]), "=&v"(av[2]), "=&v"(av[3]), "=&v"(bv[0]), "=&v"(bv[1])
        : "v"(la), "v"(lb), "n"(k4 * 4 * DLDA * 8), "n"(k4 * 4 * DLDA * 8 + 128), "n"(k4 * 4 * DLDA * 8 + 256),
          "n"(k4 * 4 * DLDA * 8 + 384), "n"(k4 * 4 * DLDB * 8), "n"(k4 * 4 * DLDB * 8 + 128)
        : "memory");
    if (TGP_DMA_DEFER && k4 == DBK / 4 - 1) {   // the last round's MFMAs run at the top of the next step (see the kernel)
#pragma unroll
      for (int fm = 0; fm < 4; ++fm) dav[fm] = av[fm];
      dbv[0] = bv[0];
      dbv[1] = bv[1];
    } else {
#pragma unroll
      for (int fm = FM_LO; fm < 4; ++fm)
#pragma unroll
        for (int fn = 0; fn < 2; ++fn) acc[fm][fn] = mfma_f64(av[fm], bv[fn], acc[fm][fn]);
    }
  }
}

// PRUNE (tgp_kernels_sweep_prune_k*.hip, the EI arg-max alone): a candidate block is given up at a row-block boundary once
// no candidate of it can still win.  The column norms only grow, so `variance - partial norm` bounds the variance from
// above and EI, increasing in the variance, from above with it; the bound is compared with the launch's best word
// (SweepArgs::prune).  For that the block's mean is formed BEFORE the step loop by a pass that generates every K* entry
// and stores none (same thread -> entry mapping and order as generate_B: the mean is bit-identical and known before the
// first MFMA).  With the mean two things are known that need no MFMA at all:
//   * the SEED: EI(mean, var) >= eta - mean for every var > 0, so the block's largest eta - mean raises the best word
//     before any block has finished;
//   * the MEAN SCREEN (nb > 1): the checkpoint's rule at the prior variance (empty partial norm).  A block that fails it
//     for every candidate is reported as given up and costs no slab store, no DMA and no row block.
// Why a seed can stand where a finished maximum stood: the seed is eta - mean to one rounding, and the tail holds
// RTOL = 1e-5, so the device EI of the candidate that supplied it is >= seed (1 - 1e-5).  A candidate given up under
// ub MARGIN < best has device EI <= ub (1 + 1e-5)^2 < best (1 + 1e-5)^2 / (1 + 2^-14) < seed (1 - 1e-5): strictly below
// that candidate's value -- neither the winner nor a tie.  The best word only ever decides giving up; results come from
// blk_val / blk_idx.  A block that survives the screen generates its K* a second time, into the slab, and every B tile
// comes from the slab by DMA (generating in the diagonal block-steps as the plain kernel does was measured slower in
// this instantiation, DESIGN.md 4.1).  Candidate blocks behind a workgroup's first are drawn from a counter: the
// winner's block runs all its block-steps, a screened one a mean pass.
// The instantiations without PRUNE compile to what they were.
constexpr int D_PRUNE_LDS = 5 * DBN + 3;   // [4][128] checkpoint norms, [128] means, two vote words, the drawn block
constexpr double PRUNE_MIN_BEST = 1e-280, PRUNE_MARGIN = 1.0 + 0x1p-14;
constexpr int PRUNE_NO_SCREEN = 1, PRUNE_STATIC_BLOCKS = 2;   // SweepArgs::prune_flags (tgp_set_variant bits 12, 13)
// Models of more than one row block run the pruned arg-max in THREE PHASES on one stream (DESIGN.md 4.1):
//   0 prune_prescreen_kernel: every block's mean in float32 with a bound that holds by construction; phase 1 skips what
//     that dismisses (below; tgp_set_variant bit 14 runs without it);
//   1 prune_mean_kernel: the mean pass of every block -- means, seed, and the block's largest bound at the prior variance;
//     prune_list_kernel then applies the give-up rule per block against the best word that holds EVERY seed and writes the
//     survivors in block order (S and the order of the work are deterministic), the regime and the ranges;
//   2 sweep_dma_kernel<.., PRUNE>: the survivors.  Whole-block regime: drawn from the list and run as ever (slab, row blocks,
//     checkpoints, fold, tail).  Split regime (S small): one workgroup per (survivor, range of row blocks); at the end of a
//     row block the 32 accumulator doubles of every thread go to the dump area instead of into the column norms;
//   3 prune_fold_kernel: per split survivor the folds replayed over the dump in the fused order, then the fused tail.
// No workgroup waits for another.  Models of one row block keep the single launch.
constexpr int GEN_MEAN = 1, GEN_SLAB = 2;

// Every K* entry of k-steps [g0, gmax) of a block, entry for entry the arithmetic of generate_B, k-steps in the order the
// sweep meets them -- folded into the mean (GEN_MEAN: nothing is stored), written to the slab (GEN_SLAB) or both.  One
// function for the mean kernel and the sweep: the thread -> entry mapping and the order of the fma chain fix the mean's bits.
template <int KIND, int DP, int WHAT>
__device__ __forceinline__ void prune_generate(const SweepArgs& a, const double* xqs, int kcol, int krg, int gmax, double* kc,
                                               double variance, double& macc, int g0 = 0) {
  double xr[DP];
#pragma unroll
  for (int c = 0; c < DP; ++c) xr[c] = xqs[c * DBN + kcol];
  for (int g = g0; g < gmax; ++g) {
    const int64_t krow0 = (int64_t)g * DBK + 2 * krg;
    const cptr xs = as_const(a.m.Xs + krow0 * DP);
    const cptr al = as_const(a.m.alpha + krow0);
    double r2[2] = {0.0, 0.0};
#pragma unroll
    for (int c = 0; c < DP; ++c) {
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const double t0 = xr[c] - xs[r * DP + c];
        r2[r] = fma(t0, t0, r2[r]);
      }
    }
    double* kcp = kc + krow0 * DBN + kcol;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const double kv = kernel_from_r2<KIND>(r2[r], variance);
      if constexpr (WHAT & GEN_MEAN) macc = fma(kv, al[r], macc);
      if constexpr (WHAT & GEN_SLAB) kcp[r * DBN] = kv;
    }
  }
}

// coordinate c of column j of block blk, scaled by its lengthscale, into xqs [DP][128] (c-major); columns past M repeat
// candidate 0.  (One entry, the caller keeps the loop `e = tid, tid + 1024, ..; j = e / DP, c = e % DP`: with the loop or the
// division in here the plain instantiations of sweep_dma_kernel compile to other machine code.)
__device__ __forceinline__ void scale_entry(double* xqs, const double* Xq, int64_t M, int d, const double* ls, int64_t blk,
                                            int j, int c) {
  const int64_t cand = blk * DBN + j;
  const int64_t src = cand < M ? cand : 0;
  xqs[c * DBN + j] = (c < d) ? Xq[src * d + c] / as_const(ls)[c] : 0.0;
}

// PRUNE, the seed (threads 0 .. 127, column `valid` with mean pm): the block's largest eta - mean over its valid columns
// raises the best word (a NaN mean posts nothing)
__device__ __forceinline__ void post_seed(const SweepArgs& a, bool valid, double pm, int lane) {
  double seed = valid ? a.acq_param - pm : 0.0;
  if (!(seed > 0.0)) seed = 0.0;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) seed = fmax(seed, __shfl_xor(seed, o, 64));
  if (lane == 0 && seed > 0.0) atomicMax(a.prune + PRUNE_W_BEST, (unsigned long long)__double_as_longlong(seed));
}

template <int KIND, int DP, bool PRUNE>
__global__ __launch_bounds__(1024, 4) void sweep_dma_kernel(const SweepArgs a) {
  static_assert(!PRUNE || TGP_DMA_DEFER, "the checkpoint sits behind the deferred MFMAs");
  __shared__ __attribute__((aligned(16))) double smem[3 * D_ASTAGE + 2 * D_BSTAGE + DBN * DP + (PRUNE ? D_PRUNE_LDS : 0)];
  double* const sAbase = smem;                       // three A stages
  double* const sBbase = smem + 3 * D_ASTAGE;        // two B stages
  double* const xqs = smem + 3 * D_ASTAGE + 2 * D_BSTAGE;  // [DP][128] scaled candidate coordinates

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;  // 4 (M) x 4 (N) waves, wave tile 64 x 32
  const int64_t Npad = a.m.Npad;
  const int nb = (int)(Npad / DBM);
  const int d = a.m.d;
  const double variance = a.m.variance;
  const double* __restrict__ Wt = a.m.Wt;
  const uint32_t lds0 = (uint32_t)(size_t)(__attribute__((address_space(3))) double*)smem;
  const uint32_t lane16 = (uint32_t)lane * 16u;   // per-lane byte offset of every DMA (TGP_DMA_SADDR)

  const int kcol = tid & 127;                                  // generated K* entries: candidate column
  const int krg = __builtin_amdgcn_readfirstlane(tid >> 7);   // row group 0..7 -> rows 2 krg, 2 krg + 1

  double* const mred = smem;         // [8][128]   reduction scratch (aliases A stage 0 after the sweep)
  double* const sred = smem + 1024;  // [4][128]
  double* const bvs = smem + 1536;
  int64_t* const bis = (int64_t*)(smem + 1540);
  // PRUNE: areas of their own behind xqs (mred / sred alias A stage 0, which is in use at a checkpoint)
  double* const psred = xqs + DBN * DP;         // [4][128]
  double* const pmean = psred + 4 * DBN;        // [128]
  int* const pvote = (int*)(pmean + DBN);       // [2]
  int64_t* const pdraw = (int64_t*)(pmean + DBN + 1);

  double* const kc = a.kcache + (size_t)blockIdx.x * (size_t)Npad * DBN;
  const int64_t nblk = (a.M + DBN - 1) / DBN;
  const int T = nb * (nb + 1) / 2 * DKSTEPS;
  // PRUNE only; a view per use: a named one, captured by the lambdas below, costs this instantiation 16 bytes of scratch
  auto pv = [&]() { return PruneView{a.prune, nblk}; };

  // PRUNE, phase 2 (nb > 1): the blocks are the entries of the survivor list.  Split regime (items > 0): this workgroup
  // is work item blockIdx.x = (survivor, range), row blocks [ib_lo, ib_hi) of the one block, and nothing else.
  const bool listed = PRUNE && nb > 1;
  int64_t nsurv = 0, li = blockIdx.x, blk_first = blockIdx.x;
  int srv = 0, ib_lo = 0, ib_hi = nb;
  bool split = false;
  if constexpr (PRUNE) {
    if (listed) {
      const unsigned long long* hdr = a.prune;
      if (hdr[PRUNE_W_FEW]) return;   // the few-blocks path: the survivors are prune_tile_kernel's
      const int64_t* list = pv().list();
      nsurv = (int64_t)hdr[PRUNE_W_SURVIVORS];
      const int items = (int)hdr[PRUNE_W_ITEMS], groups = (int)hdr[PRUNE_W_GROUPS];
      split = items > 0;
      if (split) {
        if ((int)blockIdx.x >= items) return;
        srv = (int)blockIdx.x / groups;
        const int g = (int)blockIdx.x % groups;
        ib_lo = (int)hdr[PRUNE_W_IB + g];
        ib_hi = (int)hdr[PRUNE_W_IB + g + 1];
        blk_first = list[srv];
      } else {
        blk_first = li < nsurv ? list[li] : nblk;
      }
    }
  }
  const int Tb = PRUNE ? (ib_hi * (ib_hi + 1) / 2 - ib_lo * (ib_lo + 1) / 2) * DKSTEPS : T;   // tiles of this workgroup's block

  for (int64_t blk = PRUNE ? blk_first : (int64_t)blockIdx.x, blk_next = 0; blk < nblk; blk = PRUNE ? blk_next : blk + gridDim.x) {
    // PRUNE, the end of a block: the next one is drawn by one thread and handed round through LDS (static order under
    // PRUNE_STATIC_BLOCKS); the barrier is the one behind which LDS is rewritten.  Phase 2 draws list positions.
    auto draw_next = [&]() {
      if (split) {
        blk_next = nblk;   // a work item is all this workgroup does
        __syncthreads();
        return;
      }
      int64_t pos;
      if (a.prune_flags & PRUNE_STATIC_BLOCKS) {
        pos = (listed ? li : blk) + gridDim.x;
        __syncthreads();
      } else {
        if (tid == 0) *pdraw = (int64_t)gridDim.x + (int64_t)atomicAdd(a.prune + PRUNE_W_DRAW, 1ull);
        __syncthreads();
        pos = *pdraw;   // (rewritten at the next draw, behind this block's barriers)
      }
      if (listed) {
        li = pos;
        blk_next = pos < nsurv ? pv().list()[pos] : nblk;
      } else {
        blk_next = pos;
      }
    };
    for (int e = tid; e < DBN * DP; e += 1024) scale_entry(xqs, a.Xq, a.M, d, a.m.ls, blk, e / DP, e % DP);   // once per block
    v4d acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    double ssq0 = 0.0, ssq1 = 0.0, macc = 0.0;
    __syncthreads();  // xqs is read by other threads below; every DMA of the previous block has been waited for

    // PRUNE: the block's means are known before its first MFMA.  Phase 2 (nb > 1) reads what the mean kernel stored;
    // a model of one row block generates its K* here, into the mean and the slab at once (there is no screen to wait for)
    if constexpr (PRUNE) {
      if (listed) {   // (read behind the barriers that follow the slab generation)
        if (tid < 128) pmean[tid] = pv().means()[blk * DBN + tid];
      }
    }
    if constexpr (PRUNE) if (!listed) {   // (one row block)
      prune_generate<KIND, DP, GEN_MEAN | GEN_SLAB>(a, xqs, kcol, krg, nb * DKSTEPS, kc, variance, macc);
      mred[krg * 128 + kcol] = macc;   // (no DMA is in flight: A stage 0 is free)
      __syncthreads();
      if (tid < 128) {
        const double pm = pmean[tid] = mean_reduce(a, mred, tid);
        if (!(a.prune_flags & PRUNE_NO_SCREEN)) post_seed(a, blk * DBN + tid < a.M, pm, lane);
      }
      __syncthreads();   // mred is A stage 0 again
    }

    // wave w moves row w of a tile: the two 1 KiB halves of the Wt row, the whole 1 KiB K* row
    auto dma_A = [&](int stage, int ib, int kb, int ks) {
      const int64_t krow = (int64_t)kb * DBM + ks * DBK + w;
      const uint32_t dst = lds0 + (uint32_t)((stage * D_ASTAGE + w * DLDA) * 8);
      if (TGP_DMA_SADDR) {
        const double* src = Wt + krow * Npad + (int64_t)ib * DBM;
        glds16s(src, lane16, __builtin_amdgcn_readfirstlane(dst));
        glds16s(src + 128, lane16, __builtin_amdgcn_readfirstlane(dst + 1024));
      } else {
        const double* src = Wt + krow * Npad + (int64_t)ib * DBM + lane * 2;
        glds16(src, __builtin_amdgcn_readfirstlane(dst));
        glds16(src + 128, __builtin_amdgcn_readfirstlane(dst + 1024));
      }
    };
    auto dma_B = [&](int stage, int kb, int ks) {
      const int64_t krow = (int64_t)kb * DBM + ks * DBK + w;
      const uint32_t dst = lds0 + (uint32_t)((3 * D_ASTAGE + stage * D_BSTAGE + w * DLDB) * 8);
      if (TGP_DMA_SADDR) glds16s(kc + krow * DBN, lane16, __builtin_amdgcn_readfirstlane(dst));
      else glds16(kc + krow * DBN + lane * 2, __builtin_amdgcn_readfirstlane(dst));
    };
    // first use of the K* rows of k-step (kb, ks): generate this thread's two entries, fold them into the mean,
    // keep them in the slab for the later row blocks, write them to the B stage
    auto generate_B = [&](int stage, int kb, int ks) {
      const int64_t krow0 = (int64_t)kb * DBM + ks * DBK + 2 * krg;
      const cptr xs = as_const(a.m.Xs + krow0 * DP);
      const cptr al = as_const(a.m.alpha + krow0);
      double r2[2] = {0.0, 0.0};
#pragma unroll
      for (int c = 0; c < DP; ++c) {
        const double x = xqs[c * DBN + kcol];
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const double t0 = x - xs[r * DP + c];
          r2[r] = fma(t0, t0, r2[r]);
        }
      }
      double* kcp = kc + krow0 * DBN + kcol;
      double* sB = sBbase + stage * D_BSTAGE + (2 * krg) * DLDB + kcol;
#pragma unroll
      for (int r = 0; r < 2; ++r) {
        const double kv = kernel_from_r2<KIND>(r2[r], variance);
        macc = fma(kv, al[r], macc);
        if (nb > 1) kcp[r * DBN] = kv;
        sB[r * DLDB] = kv;
      }
    };
    auto advance = [&](int& i_b, int& k_b, int& k_s) {
      if (++k_s == DKSTEPS) {
        k_s = 0;
        if (++k_b > i_b) {
          k_b = 0;
          ++i_b;
        }
      }
    };

    bool pend_fold = false;
    auto fold_block = [&]() {   // a complete row block of C: into the column norms, accumulators cleared
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
    };
    // PRUNE checkpoint (all accumulators have just been folded and cleared): true when every candidate's EI bound lies
    // below the best finished block maximum by more than the tail's own resolution -- one decision per workgroup
    auto cannot_win = [&]() -> bool {
      colnorm_reduce(psred, ssq0, ssq1, wn, wm, lane);
      __syncthreads();
      if (tid < 128) {
        bool out = true;   // (columns past M have nothing to lose)
        if (blk * DBN + tid < a.M) {
          const double s = colnorm_read(psred + tid);
          const double ub = acq_tail(ACQ_EI, a.acq_param, pmean[tid], fmax(variance - s, VAR_FLOOR), a.m.noise);
          const double best = __longlong_as_double(
              (long long)__hip_atomic_load(a.prune + PRUNE_W_BEST, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
          out = best > PRUNE_MIN_BEST && ub * PRUNE_MARGIN < best;   // (a NaN bound compares false: never given up)
        }
        const int all_out = __all(out);
        if (lane == 0) pvote[w] = all_out;
      }
      __syncthreads();
      return __builtin_amdgcn_readfirstlane(pvote[0] & pvote[1]) != 0;
    };
    // PRUNE, split regime: a complete row block of C goes to the dump area as it stands, [survivor][row block][32][1024]
    // (thread-linear: coalesced); prune_fold_kernel folds it in fold_block's order.  Accumulators cleared.
    auto dump_block = [&](int ibd) {
      double* dp = pv().dump(srv, ibd, nb) + tid;
#pragma unroll
      for (int fm = 0; fm < 4; ++fm)
#pragma unroll
        for (int fn = 0; fn < 2; ++fn)
#pragma unroll
          for (int r = 0; r < 4; ++r) dp[((fm * 2 + fn) * 4 + r) * 1024] = acc[fm][fn][r];
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the stores, and the Wt DMA in flight: the steps count what they issue)
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    };
    if constexpr (PRUNE) {
      // phase 2: the K* rows this workgroup's row blocks meet go into the slab, every B tile comes from there by DMA
      // (the mean screen, today's rule at the prior variance, has run over the whole list in prune_list_kernel)
      if (listed) prune_generate<KIND, DP, GEN_SLAB>(a, xqs, kcol, krg, ib_hi * DKSTEPS, kc, variance, macc);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the slab stores, before the barrier that lets the DMA read them
      __syncthreads();
    }
    bool given_up = false;
    int ib = PRUNE ? ib_lo : 0, kb = 0, ks = 0;        // tile t
    int ib1 = ib, kb1 = 0, ks1 = 0;                    // tile t + 1
    advance(ib1, kb1, ks1);
    // prologue: Wt tiles 0 and 1 in flight, K* tile 0 generated (k-step (0, 0) is always a first use)
    dma_A(0, ib, 0, 0);
    if constexpr (PRUNE) dma_B(0, 0, 0);
    if (Tb > 1) dma_A(1, ib1, kb1, ks1);
    if constexpr (!PRUNE) generate_B(0, 0, 0);
    if (Tb > 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // TGP_DMA_DEFER: the MFMAs of a step's last k4-round run at the top of the next step, from operands read before the
    // barrier: every wave leaves the barrier with matrix work in hand while the first operand reads of the new tile fly
    double dav[4] = {0.0, 0.0, 0.0, 0.0}, dbv[2] = {0.0, 0.0};
    bool dpend = false;
    auto flush_deferred = [&]() {
      if (TGP_DMA_DEFER && dpend) {
#pragma unroll
        for (int fm = 0; fm < 4; ++fm)
#pragma unroll
          for (int fn = 0; fn < 2; ++fn) acc[fm][fn] = mfma_f64(dav[fm], dbv[fn], acc[fm][fn]);
        dpend = false;
      }
    };
    for (int t = 0; t < Tb; ++t) {
      int ib2 = ib1, kb2 = kb1, ks2 = ks1;  // tile t + 2
      advance(ib2, kb2, ks2);
      const bool has1 = t + 1 < Tb, has2 = t + 2 < Tb;
      const bool gen1 = !PRUNE && has1 && kb1 == ib1;  // tile t + 1 brings K* rows seen for the first time
      if (TGP_DMA_DEFER) {
        __builtin_amdgcn_s_setprio(2);
        flush_deferred();
        __builtin_amdgcn_s_setprio(0);
        if (pend_fold) {
          bool dumped = false;
          if constexpr (PRUNE) {
            if (split) {   // row block ib - 1 is complete
              dump_block(ib - 1);
              dumped = true;
            }
          }
          if (!dumped) fold_block();
          pend_fold = false;
          if constexpr (PRUNE) {
            if (!split && cannot_win()) {   // row blocks ib .. nb - 1 are not needed
              given_up = true;
              break;
            }
          }
        }
      }
      if (has1 && !gen1) dma_B((t + 1) & 1, kb1, ks1);
      if (has2) dma_A((t + 2) % 3, ib2, kb2, ks2);
      {
        // W is lower triangular: in a diagonal block-step (kb == ib) this wave's 64-row quarter multiplies zeros when all
        // its rows lie above the 16-row k-slab: the step is skipped (6 of the 16 steps of a diagonal block on average).
        // Skipping per 16-row FRAGMENT instead (five forms of the k-step behind a wave-uniform switch) would cut a
        // diagonal block from 62.5 % to 53 % of a full one -- measured: the extra code paths push accumulators to
        // scratch inside the hot loop (138 spilled VGPRs), 0.847 -> 0.608 of peak.  Whole quarters it stays.
        const bool all_zero = kb == ib && ks * DBK >= wm * 64 + 64;
#if TGP_DMA_LADDR
        // operand addresses rebuilt from the lane offset in every step: as loop invariants they are what the compiler
        // spills first at the 128-VGPR cap, and a scratch reload is an s_waitcnt vmcnt(0) on the DMA just issued
        uint32_t l16 = lane16;
        asm volatile("" : "+v"(l16));
        const uint32_t lrow = l16 >> 8, lcol8 = (l16 & 0xF0u) >> 1;   // lane >> 4, 8 (lane & 15)
        const uint32_t la = lds0 + (uint32_t)(((t % 3) * D_ASTAGE + wm * 64) * 8) + lrow * (DLDA * 8) + lcol8;
        const uint32_t lb = lds0 + (uint32_t)((3 * D_ASTAGE + (t & 1) * D_BSTAGE + wn * 32) * 8) + lrow * (DLDB * 8) + lcol8;
#else
        const double* ab = sAbase + (t % 3) * D_ASTAGE + (lane >> 4) * DLDA + wm * 64 + (lane & 15);
        const double* bb = sBbase + (t & 1) * D_BSTAGE + (lane >> 4) * DLDB + wn * 32 + (lane & 15);
        const uint32_t la = (uint32_t)(size_t)(__attribute__((address_space(3))) const double*)ab;
        const uint32_t lb = (uint32_t)(size_t)(__attribute__((address_space(3))) const double*)bb;
#endif
        __builtin_amdgcn_s_setprio(2);
        if (!all_zero) {
          dma_kstep<0>(acc, la, lb, dav, dbv);
          if (TGP_DMA_DEFER) dpend = true;
        }
        __builtin_amdgcn_s_setprio(0);
      }
      if (gen1) generate_B((t + 1) & 1, kb1, ks1);
      if (ks == DKSTEPS - 1 && kb == ib) {  // row block ib complete: fold into the column norms
        if (TGP_DMA_DEFER) pend_fold = true;   // ... behind the deferred MFMAs, at the top of the next step
        else fold_block();
      }
      // tile t + 1 complete in LDS (its DMA is older than the two Wt instructions of tile t + 2), then publish
      if (has2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
      else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      ib = ib1;
      kb = kb1;
      ks = ks1;
      ib1 = ib2;
      kb1 = kb2;
      ks1 = ks2;
    }
    if (TGP_DMA_DEFER) {
      flush_deferred();
      if constexpr (PRUNE) {
        if (split) {   // the item's last row block; fold and tail are prune_fold_kernel's
          dump_block(ib - 1);
          draw_next();
          continue;
        }
      }
      if (pend_fold) fold_block();
    }
    if constexpr (PRUNE) {
      if (given_up) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the Wt DMA of the next tile is still in flight
        if (tid == 0) {
          a.blk_val[blk] = -INFINITY;   // as a block without a valid candidate
          a.blk_idx[blk] = INT64_MAX;
          atomicAdd(a.prune + PRUNE_W_GIVEN_UP, 1ull);
          atomicAdd(a.prune + PRUNE_W_SKIPPED, (unsigned long long)(nb - ib));
        }
        draw_next();  // LDS is rewritten by the next block
        continue;
      }
    }
    // ---- reductions (LDS is free after the last barrier; no DMA is outstanding) --------------------------
    if constexpr (!PRUNE) mred[krg * 128 + kcol] = macc;
    colnorm_reduce(sred, ssq0, ssq1, wn, wm, lane);
    __syncthreads();
    double val = -INFINITY;
    int64_t gidx = INT64_MAX;
    if (tid < 128) {
      const int64_t cj = blk * DBN + tid;
      if (cj < a.M) {
        double mean;
        if constexpr (PRUNE) mean = pmean[tid];
        else mean = mean_reduce(a, mred, tid);
        sweep_tail(a, cj, mean, fmax(variance - colnorm_read(sred + tid), VAR_FLOOR), val, gidx);
      }
    }
    if (a.blk_val) {
      const double v0 = block_winner(a, blk, val, gidx, bvs, bis, tid, w);
      if constexpr (PRUNE) {   // EI >= 0: the bit patterns order like the values (a -0.0 or a rounded-negative value stays out)
        if (tid == 0 && v0 > 0.0) atomicMax(a.prune + PRUNE_W_BEST, (unsigned long long)__double_as_longlong(v0));
      }
    }
    if constexpr (PRUNE) draw_next();
    else __syncthreads();  // scratch / xqs are rewritten by the next block
  }
}

#ifdef TGP_SWEEP_PRUNE_TU
// ---- Phase 0: the float32 pre-screen (nb > 1; DESIGN.md 4.1 has the derivation) ----------------------------------------------
// Phase 1 spends its time (float64 distance, software sqrt and exp per K* entry) on blocks of which all but a handful are
// given up by the mean screen; all the screen needs of their means is a bound.  Phase 0 forms every candidate's mean in
// float32 kernel arithmetic, mean32, with a bound |mean32 - mean| <= E that holds by construction, and leaves per block
//   bounds()[blk] = ub32: the largest tail at (mean32 - E, prior variance), inflated past the tail's own resolution -- never
//                   below the bound phase 1 would store (EI falls with the mean; +inf where mean32 or E is not finite);
//   PRUNE_W_PREBEST: the largest eta - mean32 - E, rounded down -- never above the top seed eta - mean.
// Phase 1 skips a block whose ub32 MARGIN < prebest.  Why results, S and every counter keep their bits:
//   * the block B* of the top seed has ub32 >= ub >= seed (1 - 1e-5) (the seed argument above), so
//     ub32 MARGIN > seed >= prebest: it is never skipped and PRUNE_W_BEST ends at the value it had without phase 0;
//   * a skipped block has ub MARGIN <= ub32 MARGIN < prebest <= best: prune_list_kernel drops it (it reads ub32 where the
//     exact bound stood) exactly as it dropped it on the exact bound -- same list, same S, same counters;
//   * the means of a skipped block are never read: only listed blocks' are.
// Per entry: q = SCALE r^2 by the difference form on float32 copies of the centred, sqrt(SCALE)-scaled coordinates (centred
// and scaled in float64, then rounded: a shift of the whole box costs nothing), the shape by v_sqrt_f32 / v_exp_f32 (the
// square root IS the base-2 exponent, TrajShape), the value converted and folded by a float64 fma against alpha (the sum
// adds no term that grows with N).  The bound, with u = 2^-24, S = |a|_2 + max_k |b_k|_2 (a, b the scaled centred
// candidate and rows) and G1 = sup 2 sqrt(q) |f'(q)|, G2 = sup q |f'(q)| of the shape f:
//   |q32 - q| <= 2 u sqrt(q) S + (2 DP + 2) u q      (two conversions and the subtraction; DP fmas or 2 DP mul / adds)
//   |f32 - f| <= u [G1 S + G2 (2 DP + 10) + 10]      (+ 8 u q: v_sqrt_f32 at 2 ulp; 10 u: v_exp_f32 at 2 ulp, the
//                                                     polynomial's two constants and two fmas, the product)
//   E = |alpha|_1 variance (1.0625 u [..] + 2^-53 [2 G1 (|Xs_0| + S) + 256 + Npad] + 2^-60) + 2^-50 (|mean32| + |eta|)
// (1/16 for the second-order terms; the 2^-53 term for the float64 side -- centring, the exact pass's own rounding; 2^-60
// for flushed float32 denormals: at most DP squares below 2^-126 are lost, 2^-61 on sqrt(q); the last term for the
// roundings of mean32 - E and eta - mean32).  A block with a candidate whose E is not finite or exceeds the prior standard
// deviation (E * E > variance: E is a length in output units, the variance its square, so the cap must compare like with
// like -- E <= variance switched phase 0 off for every model whose outputs are scaled down), or whose mean32 is not
// finite, gets +inf and posts no lower seed.
template <int KIND>
struct PreShape {
  static constexpr double G1 = KIND == KIND_RBF ? 0.72 : KIND == KIND_M12 ? 0.70 : KIND == KIND_M32 ? 0.26 : 0.20;
  static constexpr double G2 = KIND == KIND_RBF ? 0.37 : KIND == KIND_M12 ? 0.19 : KIND == KIND_M32 ? 0.28 : 0.31;
};
constexpr double PRE_TAIL_INFLATE = 1.0 + 4e-5, PRE_MIN_BOUND = 1e-290;   // (below PRUNE_MIN_BEST: a floor skips nothing new)

template <int KIND>
__device__ __forceinline__ float prescreen_shape(float q) {   // q = SCALE r^2 >= 0 (difference form)
  if constexpr (KIND == KIND_RBF) {
    return __builtin_amdgcn_exp2f(-q);
  } else {
    constexpr float IL = (float)(1.0 / TrajShape<KIND>::L2E), IL2 = (float)(1.0 / (3.0 * TrajShape<KIND>::L2E * TrajShape<KIND>::L2E));
    const float qc = fmaxf(q, (float)TrajShape<KIND>::FLOOR);
    const float v = __builtin_amdgcn_sqrtf(qc);
    const float e = __builtin_amdgcn_exp2f(-v);
    if constexpr (KIND == KIND_M12) return e;
    else if constexpr (KIND == KIND_M32) return fmaf(IL, v, 1.0f) * e;
    else return fmaf(IL2, qc, fmaf(IL, v, 1.0f)) * e;
  }
}

// the bound E of a candidate whose scaled centred norm is `an` and whose float32 mean is m32
template <int KIND, int DP>
__device__ __forceinline__ double prescreen_bound(const SweepArgs& a, const double* pre, double an, double m32) {
  const double S = an + pre[PRE_XC_MAX];
  const double c32 = 1.0625 * 0x1p-24 * (PreShape<KIND>::G1 * S + PreShape<KIND>::G2 * (2 * DP + 10) + 10.0);
  const double c64 = 0x1p-53 * (2.0 * PreShape<KIND>::G1 * (pre[PRE_X0] + S) + 256.0 + (double)a.m.Npad);
  return pre[PRE_ALPHA_L1] * a.m.variance * (c32 + c64 + 0x1p-60) + 0x1p-50 * (fabs(m32) + fabs(a.acq_param));
}

template <int KIND, int DP>
__global__ __launch_bounds__(1024, 8) void prune_prescreen_kernel(const SweepArgs a, const PruneLaunch pl) {
  __shared__ float xqs[DP * DBN];     // [DP][128] centred, scaled candidate coordinates
  __shared__ double mred[8 * DBN];    // [8][128]
  __shared__ double ubw[2], sdw[2];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kcol = tid & 127;
  const int krg = __builtin_amdgcn_readfirstlane(tid >> 7);   // row group: rows 32 g + 4 krg .. + 3
  const int d = a.m.d;
  const int ng = (int)(a.m.Npad / 32);
  const double variance = a.m.variance;
  const int64_t nblk = (a.M + DBN - 1) / DBN;
  const PruneView pv{a.prune, nblk};
  const double rs = pl.pre[PRE_RS];
  typedef const __attribute__((address_space(4))) float* cfptr;
  const cfptr xc32 = (cfptr)(const __attribute__((address_space(1))) float*)(pl.xc32);
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    for (int e = tid; e < DBN * DP; e += 1024) {
      const int j = e / DP, c = e % DP;
      const int64_t cand = blk * DBN + j;
      const int64_t src = cand < a.M ? cand : 0;
      // centred in float64 FIRST (Xs_0 is row 0 of Xs), then rounded
      xqs[c * DBN + j] = (c < d) ? (float)(rs * (a.Xq[src * d + c] / as_const(a.m.ls)[c] - as_const(a.m.Xs)[c])) : 0.0f;
    }
    __syncthreads();
    float xr[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) xr[c] = xqs[c * DBN + kcol];
    double macc = 0.0;
    for (int g = 0; g < ng; ++g) {
      const int64_t krow0 = (int64_t)g * 32 + 4 * krg;
      const cfptr xs = xc32 + krow0 * DP;
      const cptr al = as_const(a.m.alpha + krow0);
      float q[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int c = 0; c < DP; ++c) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float t0 = xr[c] - xs[r * DP + c];
          q[r] = fmaf(t0, t0, q[r]);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) macc = fma((double)prescreen_shape<KIND>(q[r]), al[r], macc);
    }
    mred[krg * 128 + kcol] = macc;
    __syncthreads();
    if (tid < 128) {
      double sum = 0.0;
#pragma unroll
      for (int g = 0; g < 8; ++g) sum += mred[g * 128 + tid];
      const double m32 = fma(variance, sum, a.m.mean_const);
      const int64_t cand = blk * DBN + tid;
      const bool valid = cand < a.M;
      double ub = -INFINITY, seed = 0.0;   // columns past M have nothing to lose
      if (valid) {
        double an = 0.0;
        for (int c = 0; c < d; ++c) {
          const double v = rs * (a.Xq[cand * d + c] / as_const(a.m.ls)[c] - as_const(a.m.Xs)[c]);
          an = fma(v, v, an);
        }
        const double E = prescreen_bound<KIND, DP>(a, pl.pre, sqrt(an), m32);
        if (pl.m32_out) {
          pl.m32_out[cand] = m32;
          pl.e_out[cand] = E;
        }
        ub = INFINITY;
        if (E * E <= variance && fabs(m32) < INFINITY) {   // (a NaN compares false; an overflowing square is +inf)
          const double t = acq_tail(ACQ_EI, a.acq_param, m32 - E, fmax(variance, VAR_FLOOR), a.m.noise);
          if (!(t != t)) ub = fmax(t * PRE_TAIL_INFLATE, PRE_MIN_BOUND);
          seed = ((a.acq_param - m32) - E) * (1.0 - 0x1p-50);   // rounded down
          if (!(seed > 0.0)) seed = 0.0;
        }
      }
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        ub = fmax(ub, __shfl_xor(ub, o, 64));
        seed = fmax(seed, __shfl_xor(seed, o, 64));
      }
      if (lane == 0) {
        ubw[w] = ub;
        sdw[w] = seed;
      }
    }
    __syncthreads();   // xqs and mred are rewritten by the next block
    if (tid == 0) {
      const double ub = fmax(ubw[0], ubw[1]);
      pv.bounds()[blk] = ub;
      const double seed = fmax(sdw[0], sdw[1]);
      // (one candidate without a finite bound takes the block's lower seed with it)
      if (ub < INFINITY && seed > 0.0) atomicMax(a.prune + PRUNE_W_PREBEST, (unsigned long long)__double_as_longlong(seed));
    }
  }
}
#endif

#ifdef TGP_SWEEP_PRUNE_TU
// The end of a block's mean pass, thread (kcol, krg) holding its fma chain `macc`: the 128 means stored, the seed posted, the
// block's largest EI tail at the prior variance stored as its bound (a NaN bound as +inf: never screened).  mred [8][128] and
// ubw [2] are LDS; the last barrier frees them, and whatever the caller read before the call, for the next block.
__device__ __forceinline__ void prune_mean_epilogue(const SweepArgs& a, const PruneView& pv, int64_t blk, double macc, double* mred,
                                                    double* ubw, bool screen) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  mred[(tid >> 7) * 128 + (tid & 127)] = macc;
  __syncthreads();
  if (tid < 128) {
    const double pm = pv.means()[blk * DBN + tid] = mean_reduce(a, mred, tid);
    const bool valid = blk * DBN + tid < a.M;
    if (screen) post_seed(a, valid, pm, lane);
    // the checkpoint's bound with an empty partial norm; columns past M have nothing to lose
    double ub = -INFINITY;
    if (valid) {
      ub = acq_tail(ACQ_EI, a.acq_param, pm, fmax(a.m.variance, VAR_FLOOR), a.m.noise);
      if (ub != ub) ub = INFINITY;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) ub = fmax(ub, __shfl_xor(ub, o, 64));
    if (lane == 0) ubw[w] = ub;
  }
  __syncthreads();   // xqs and mred are rewritten by the next block
  if (tid == 0) pv.bounds()[blk] = fmax(ubw[0], ubw[1]);
}

// Phase 1: the mean pass of every candidate block, blocks i, i + #WG, ... (a pass costs the same for every block).  Leaves
// the block's 128 means, posts its seed as the fused kernel did and stores the largest EI tail at the prior variance over
// its valid candidates (a NaN bound as +inf: never screened).  Gives nothing up.  No A / B stages, no accumulators, no
// slab: WAVES per SIMD is 8 (two workgroups per compute unit) or 4.
template <int KIND, int DP, int WAVES>
__global__ __launch_bounds__(1024, WAVES) void prune_mean_kernel(const SweepArgs a) {
  __shared__ double smem[DBN * DP + 8 * DBN + 2];
  double* const xqs = smem;              // [DP][128]
  double* const mred = smem + DBN * DP;  // [8][128]
  double* const ubw = mred + 8 * DBN;    // [2]
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int kcol = tid & 127;
  const int krg = __builtin_amdgcn_readfirstlane(tid >> 7);
  const int nb = (int)(a.m.Npad / DBM);
  const double variance = a.m.variance;
  const int64_t nblk = (a.M + DBN - 1) / DBN;
  const PruneView pv{a.prune, nblk};
  const bool screen = !(a.prune_flags & PRUNE_NO_SCREEN);
  if (a.prune[PRUNE_W_FEW]) return;   // the few-blocks path: the means come from the slabs (prune_mean_slab_kernel)
  // phase 0 (zero when it did not run): written by the launch in front of this one, stable during this one
  const double prebest = __longlong_as_double((long long)a.prune[PRUNE_W_PREBEST]);
  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    // a block the pre-screen dismissed keeps its float32 bound and costs nothing here (one decision per workgroup; thread 0
    // rewrites the word only at the end of a block that was not skipped)
    if (prebest > PRUNE_MIN_BEST && pv.bounds()[blk] * PRUNE_MARGIN < prebest) {
      if (tid == 0) atomicAdd(a.prune + PRUNE_W_PRESCREENED, 1ull);
      continue;
    }
    for (int e = tid; e < DBN * DP; e += 1024) scale_entry(xqs, a.Xq, a.M, a.m.d, a.m.ls, blk, e / DP, e % DP);
    __syncthreads();
    double macc = 0.0;
    prune_generate<KIND, DP, GEN_MEAN>(a, xqs, kcol, krg, nb * DKSTEPS, nullptr, variance, macc);
    prune_mean_epilogue(a, pv, blk, macc, mred, ubw, screen);
  }
}

// Between phases 1 and 2, one workgroup: the give-up rule per block on the stored bound against the best word, which now
// holds every seed -- best > PRUNE_MIN_BEST and ub_max MARGIN < best.  Rounding a product with a constant is monotone, so
// the largest bound fails the test exactly when every candidate's does: the per-candidate vote of the fused screen.
// Screened blocks get (-inf, INT64_MAX) and are counted; the survivors are listed in block order; then the regime.
__global__ __launch_bounds__(1024) void prune_list_kernel(const SweepArgs a, const PruneLaunch pl, int wg) {
  __shared__ int wcnt[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int nb = (int)(a.m.Npad / DBM);
  const int64_t nblk = (a.M + DBN - 1) / DBN;
  const PruneView pv{a.prune, nblk};
  const double* ubs = pv.bounds();
  int64_t* list = pv.list();
  // (the pre-screen's lower seed never exceeds the best word -- phase 0 above; the larger of the two is the best word)
  const double best = fmax(__longlong_as_double((long long)a.prune[PRUNE_W_BEST]),
                           __longlong_as_double((long long)a.prune[PRUNE_W_PREBEST]));
  const bool screen = !(a.prune_flags & PRUNE_NO_SCREEN) && best > PRUNE_MIN_BEST;
  int64_t base = 0;
  for (int64_t c0 = 0; c0 < nblk; c0 += 1024) {
    const int64_t blk = c0 + tid;
    bool live = false;
    if (blk < nblk) {
      live = !(screen && ubs[blk] * PRUNE_MARGIN < best);
      if (!live) {
        a.blk_val[blk] = -INFINITY;   // as a block without a valid candidate
        a.blk_idx[blk] = INT64_MAX;
      }
    }
    const unsigned long long vote = __ballot(live);
    if (lane == 0) wcnt[w] = __popcll(vote);
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < 16; ++i) {
      if (i < w) before += wcnt[i];
      total += wcnt[i];
    }
    if (live) list[base + before + __popcll(vote & ((1ull << lane) - 1ull))] = blk;
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    const int64_t S = base, out = nblk - S;
    a.prune[PRUNE_W_GIVEN_UP] += (unsigned long long)out;
    a.prune[PRUNE_W_SKIPPED] += (unsigned long long)(out * (nb - 1));   // row blocks behind the first that are not computed
    a.prune[PRUNE_W_SCREENED] += (unsigned long long)out;               // ... and the first is not either
    a.prune[PRUNE_W_SURVIVORS] = (unsigned long long)S;
    int groups = 0;
    if (S >= 1 && S <= (int64_t)pl.max_survivors && S <= (int64_t)wg) {   // split regime
      groups = (int)((int64_t)wg / S);
      if (groups > nb) groups = nb;
      if (groups > PRUNE_MAX_GROUPS) groups = PRUNE_MAX_GROUPS;
      if (pl.max_groups > 0 && groups > pl.max_groups) groups = pl.max_groups;
      while (!plan_row_split(a.prune + PRUNE_W_IB, nb, groups, true)) --groups;   // (one range always works)
    }
    a.prune[PRUNE_W_GROUPS] = (unsigned long long)groups;
    a.prune[PRUNE_W_ITEMS] = (unsigned long long)(S * groups);
    // the few-blocks path (S <= P <= few_max <= max_survivors: the split regime above, so the fold runs and the dump fits)
    if (a.prune[PRUNE_W_FEW]) a.prune[PRUNE_W_TILE_ITEMS] = (unsigned long long)(S * nb * 16);
  }
}

// ---- The few-blocks path (nb > 1; DESIGN.md 4.1) ----------------------------------------------------------------------------
// When phase 0 leaves P <= few_max blocks, phases 1 and 2 concern a handful of 128-candidate blocks, and the kernels above
// spend their time on one workgroup each: the mean pass of a block is one workgroup's 0.3 ms, every split item generates the
// K* rows it meets again, and the longest item is one compute unit's matrix rate.  Here instead
//   prune_prelist_kernel   lists the P blocks phase 1 would not skip and raises PRUNE_W_FEW;
//   prune_kstar_kernel     generates the K* of pre-listed block p ONCE, into slab p, one k-step per work item;
//   prune_mean_slab_kernel replays the mean's fma chain over the slab (same values, same order: same bits);
//   prune_list_kernel      runs as ever;
//   prune_tile_kernel      forms a survivor's row blocks one 64 x 32 wave tile per work item: every accumulator sees the fused
//                          kernel's MFMAs in the fused order and goes to the dump word the split item writes;
//   prune_fold_kernel      runs as ever.
// prune_mean_kernel and the PRUNE sweep_dma_kernel return at once.  Every kernel has a fixed grid and reads P, S and the
// flag from the header: no host synchronisation, no kernel waits for another.

// One workgroup, behind phase 0: the blocks phase 1 would not skip (prune_mean_kernel's rule), compacted in block order.
// Without phase 0 prebest is zero and every block is listed.
__global__ __launch_bounds__(1024) void prune_prelist_kernel(const SweepArgs a, const PruneLaunch pl) {
  __shared__ int wcnt[16];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int64_t nblk = (a.M + DBN - 1) / DBN;
  const PruneView pv{a.prune, nblk};
  int64_t* prelist = pv.prelist();
  const double prebest = __longlong_as_double((long long)a.prune[PRUNE_W_PREBEST]);
  int64_t base = 0;
  for (int64_t c0 = 0; c0 < nblk; c0 += 1024) {
    const int64_t blk = c0 + tid;
    const bool live = blk < nblk && !(prebest > PRUNE_MIN_BEST && pv.bounds()[blk] * PRUNE_MARGIN < prebest);
    const unsigned long long vote = __ballot(live);
    if (lane == 0) wcnt[w] = __popcll(vote);
    __syncthreads();
    int before = 0, total = 0;
    for (int i = 0; i < 16; ++i) {
      if (i < w) before += wcnt[i];
      total += wcnt[i];
    }
    const int64_t pos = base + before + __popcll(vote & ((1ull << lane) - 1ull));
    if (live && pos < (int64_t)pl.few_max) prelist[pos] = blk;
    base += total;
    __syncthreads();
  }
  if (tid == 0) {
    a.prune[PRUNE_W_PRELISTED] = (unsigned long long)base;
    if (base >= 1 && base <= (int64_t)pl.few_max) {
      a.prune[PRUNE_W_FEW] = 1ull;
      a.prune[PRUNE_W_PRESCREENED] = (unsigned long long)(nblk - base);   // what prune_mean_kernel's skips would have counted
    }
  }
}

// Work item (pre-listed block p, k-step g): the 16 x 128 K* entries of the k-step into slab p -- one iteration of
// prune_generate's loop, entry for entry what the sweep's own generation stores.
template <int KIND, int DP>
__global__ __launch_bounds__(1024) void prune_kstar_kernel(const SweepArgs a) {
  __shared__ double xqs[DBN * DP];
  if (!a.prune[PRUNE_W_FEW]) return;
  const int tid = threadIdx.x;
  const int kcol = tid & 127;
  const int krg = __builtin_amdgcn_readfirstlane(tid >> 7);
  const int64_t Npad = a.m.Npad;
  const int ng = (int)(Npad / DBK);
  const int64_t nblk = (a.M + DBN - 1) / DBN;
  const PruneView pv{a.prune, nblk};
  const int64_t items = (int64_t)a.prune[PRUNE_W_PRELISTED] * ng;
  for (int64_t item = blockIdx.x; item < items; item += gridDim.x) {
    const int64_t p = item / ng;
    const int g = (int)(item % ng);
    const int64_t blk = pv.prelist()[p];
    for (int e = tid; e < DBN * DP; e += 1024) scale_entry(xqs, a.Xq, a.M, a.m.d, a.m.ls, blk, e / DP, e % DP);
    __syncthreads();
    double macc = 0.0;
    prune_generate<KIND, DP, GEN_SLAB>(a, xqs, kcol, krg, g + 1, a.kcache + (size_t)p * (size_t)Npad * DBN, a.m.variance, macc, g);
    __syncthreads();   // xqs is rewritten by the next item
  }
}

// One workgroup per pre-listed block: thread (kcol, krg) replays prune_generate's chain macc = fma(kv, alpha[row], macc) over
// g = 0 .. and r = 0, 1 with kv read from the slab, then the mean pass's own epilogue.
__global__ __launch_bounds__(1024) void prune_mean_slab_kernel(const SweepArgs a) {
  __shared__ double mred[8 * DBN];
  __shared__ double ubw[2];
  if (!a.prune[PRUNE_W_FEW] || (unsigned long long)blockIdx.x >= a.prune[PRUNE_W_PRELISTED]) return;
  const int tid = threadIdx.x;
  const int kcol = tid & 127;
  const int krg = __builtin_amdgcn_readfirstlane(tid >> 7);
  const int64_t Npad = a.m.Npad;
  const int ng = (int)(Npad / DBK);
  const int64_t nblk = (a.M + DBN - 1) / DBN;
  const PruneView pv{a.prune, nblk};
  const double* __restrict__ kc = a.kcache + (size_t)blockIdx.x * (size_t)Npad * DBN + (size_t)(2 * krg) * DBN + kcol;
  double macc = 0.0;
#pragma unroll 8
  for (int g = 0; g < ng; ++g) {
    const cptr al = as_const(a.m.alpha + (int64_t)g * DBK + 2 * krg);
    const double k0 = kc[(size_t)g * DBK * DBN], k1 = kc[(size_t)g * DBK * DBN + DBN];
    macc = fma(k0, al[0], macc);
    macc = fma(k1, al[1], macc);
  }
  prune_mean_epilogue(a, pv, pv.prelist()[blockIdx.x], macc, mred, ubw, !(a.prune_flags & PRUNE_NO_SCREEN));
}

// Work item (survivor, row block ib, wave tile (wm, wn)), one wave: the 64 x 32 tile of C = W K* the fused kernel's wave
// (wm, wn) holds at the end of row block ib.  Per accumulator one mfma_f64(av, bv, acc) per k4 round, k-steps in the order
// (kb = 0 .. ib, ks = 0 .. 15) from zero -- the rows of step s = 16 kb + ks are 16 s .. 16 s + 15 -- and the fused kernel's
// whole-quarter skip (kb == ib and 16 ks >= 64 wm + 64), which cuts the tail of the order: steps [0, 16 ib + 4 wm + 4).
// The operands come straight from Wt and the survivor's slab, lane for lane what dma_kstep reads from LDS, four k-steps
// of them in registers at a time (a wave has the SIMD's registers to itself).  What the compiled loop does with them: the
// hardware counts 63 loads in flight and a step is 24, and the compiler waits ONCE per four steps, with vmcnt(24) at the
// top of the body -- there steps s .. s + 2 have landed and only the loads of s + 3, just issued, are out.  The loads of
// s + 4, s + 5, s + 6 go out behind the MFMAs of s, s + 1, s + 2, so the youngest has one step of MFMAs (32 x 64 cycles)
// of lead before that wait, the others two and three.  Measured: SQ_WAIT_ANY is 9 % of the wave cycles at the headline
// (profiles/r29_prune_tiles.txt).  Items are ordered longest row block first.
constexpr int TILE_DEPTH = 4;
__device__ __forceinline__ void tile_load(double (&av)[16], double (&bv)[8], const double* ap, const double* bp, int64_t Npad, int s) {
  const double* a0 = ap + (int64_t)s * DBK * Npad;
  const double* b0 = bp + (int64_t)s * DBK * DBN;
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4) {
#pragma unroll
    for (int fm = 0; fm < 4; ++fm) av[k4 * 4 + fm] = a0[(int64_t)k4 * 4 * Npad + fm * 16];
#pragma unroll
    for (int fn = 0; fn < 2; ++fn) bv[k4 * 2 + fn] = b0[k4 * 4 * DBN + fn * 16];
  }
}
__device__ __forceinline__ void tile_step(v4d (&acc)[4][2], const double (&av)[16], const double (&bv)[8]) {
#pragma unroll
  for (int k4 = 0; k4 < 4; ++k4)
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int fn = 0; fn < 2; ++fn) acc[fm][fn] = mfma_f64(av[k4 * 4 + fm], bv[k4 * 2 + fn], acc[fm][fn]);
}
__global__ __launch_bounds__(64) void prune_tile_kernel(const SweepArgs a) {
  if (!a.prune[PRUNE_W_FEW]) return;
  const int64_t Npad = a.m.Npad;
  const int nb = (int)(Npad / DBM);
  const int64_t S = (int64_t)a.prune[PRUNE_W_SURVIVORS];
  if ((int64_t)blockIdx.x >= S * nb * 16) return;
  const int lane = threadIdx.x;
  const int wt = (int)(blockIdx.x & 15u), wm = wt >> 2, wn = wt & 3;
  const int64_t q = blockIdx.x >> 4;
  const int srv = (int)(q % S), ib = nb - 1 - (int)(q / S);
  const int64_t nblk = (a.M + DBN - 1) / DBN;
  const PruneView pv{a.prune, nblk};
  // the survivor's slab: its position in the pre-list (every survivor is pre-listed)
  const int64_t blk = pv.list()[srv];
  const int P = (int)a.prune[PRUNE_W_PRELISTED];
  const unsigned long long hit = __ballot(lane < P && pv.prelist()[lane < P ? lane : 0] == blk);
  const int p = __builtin_amdgcn_readfirstlane(hit ? __ffsll((long long)hit) - 1 : 0);
  const double* ap = a.m.Wt + (int64_t)(lane >> 4) * Npad + (int64_t)ib * DBM + wm * 64 + (lane & 15);
  const double* bp = a.kcache + (size_t)p * (size_t)Npad * DBN + (lane >> 4) * DBN + wn * 32 + (lane & 15);
  const int steps = ib * DKSTEPS + wm * 4 + 4;
  v4d acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
  // (loads past the last step repeat it: in bounds, unused, and the loop body has no branch)
  auto at = [&](int s) { return s < steps ? s : steps - 1; };
  double av0[16], bv0[8], av1[16], bv1[8], av2[16], bv2[8], av3[16], bv3[8];
  // The step count is a multiple of four: the loop body is four steps and one basic block.  The scheduling barriers keep
  // every step's loads in front of the MFMAs they overlap (left alone, the compiler sinks them behind the MFMAs and waits
  // for memory with nothing in flight).
  tile_load(av0, bv0, ap, bp, Npad, 0);
  tile_load(av1, bv1, ap, bp, Npad, 1);
  tile_load(av2, bv2, ap, bp, Npad, 2);
  for (int s = 0; s < steps; s += TILE_DEPTH) {
    tile_load(av3, bv3, ap, bp, Npad, s + 3);
    __builtin_amdgcn_sched_barrier(0);
    tile_step(acc, av0, bv0);
    __builtin_amdgcn_sched_barrier(0);
    tile_load(av0, bv0, ap, bp, Npad, at(s + 4));
    __builtin_amdgcn_sched_barrier(0);
    tile_step(acc, av1, bv1);
    __builtin_amdgcn_sched_barrier(0);
    tile_load(av1, bv1, ap, bp, Npad, at(s + 5));
    __builtin_amdgcn_sched_barrier(0);
    tile_step(acc, av2, bv2);
    __builtin_amdgcn_sched_barrier(0);
    tile_load(av2, bv2, ap, bp, Npad, at(s + 6));
    __builtin_amdgcn_sched_barrier(0);
    tile_step(acc, av3, bv3);
    __builtin_amdgcn_sched_barrier(0);
  }
  double* dp = pv.dump(srv, ib, nb) + wt * 64 + lane;
#pragma unroll
  for (int fm = 0; fm < 4; ++fm)
#pragma unroll
    for (int fn = 0; fn < 2; ++fn)
#pragma unroll
      for (int r = 0; r < 4; ++r) dp[((fm * 2 + fn) * 4 + r) * 1024] = acc[fm][fn][r];
}

// Phase 3, one workgroup per split survivor: thread (wave, lane) replays fold_block over its dumped accumulators for
// ib = 0 .. nb - 1 in the fused order (fm, r; explicit fma), then the fused kernel's reduction and tail on the stored means.
// The accumulators of a row block do not depend on where a work item started: the variance has the fused kernel's bits.
__global__ __launch_bounds__(1024) void prune_fold_kernel(const SweepArgs a) {
  __shared__ double sred[4 * DBN];
  __shared__ double bvs[2];
  __shared__ int64_t bis[2];
  const int64_t nblk = (a.M + DBN - 1) / DBN;
  if (a.prune[PRUNE_W_ITEMS] == 0 || (unsigned long long)blockIdx.x >= a.prune[PRUNE_W_SURVIVORS]) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;
  const int nb = (int)(a.m.Npad / DBM);
  const PruneView pv{a.prune, nblk};
  const int64_t blk = pv.list()[blockIdx.x];
  const double* dp = pv.dump(blockIdx.x, 0, nb) + tid;
  double ssq0 = 0.0, ssq1 = 0.0;
  for (int ib = 0; ib < nb; ++ib, dp += PRUNE_DUMP_BLOCK) {
#pragma unroll
    for (int fm = 0; fm < 4; ++fm)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double c0 = dp[((fm * 2 + 0) * 4 + r) * 1024], c1 = dp[((fm * 2 + 1) * 4 + r) * 1024];
        ssq0 = fma(c0, c0, ssq0);
        ssq1 = fma(c1, c1, ssq1);
      }
  }
  colnorm_reduce(sred, ssq0, ssq1, wn, wm, lane);
  __syncthreads();
  double val = -INFINITY;
  int64_t gidx = INT64_MAX;
  const int64_t cj = blk * DBN + tid;
  if (tid < 128 && cj < a.M)
    sweep_tail(a, cj, pv.means()[cj], fmax(a.m.variance - colnorm_read(sred + tid), VAR_FLOOR), val, gidx);
  block_winner(a, blk, val, gidx, bvs, bis, tid, w);
}

template <int KIND, int DP>
void launch_prune_prescreen(hipStream_t s, const SweepArgs& a, int64_t wg, const PruneLaunch& pl) {
  hipLaunchKernelGGL((prune_prescreen_kernel<KIND, DP>), dim3((unsigned)wg), dim3(1024), 0, s, a, pl);
}
template <int KIND, int DP>
void launch_prune_mean(hipStream_t s, const SweepArgs& a, int64_t wg, int waves) {
  if (waves >= 8) hipLaunchKernelGGL((prune_mean_kernel<KIND, DP, 8>), dim3((unsigned)(2 * wg)), dim3(1024), 0, s, a);
  else hipLaunchKernelGGL((prune_mean_kernel<KIND, DP, 4>), dim3((unsigned)wg), dim3(1024), 0, s, a);
}
#endif

template <int KIND, bool PRUNE>
hipError_t launch_sweep_dma_dp(hipStream_t s, const SweepArgs& a, int64_t grid) {
  dim3 g((unsigned)grid), b(1024);
  return with_dp<16>(a.m.dp, [&](auto DP) {
    hipLaunchKernelGGL((sweep_dma_kernel<KIND, DP(), PRUNE>), g, b, 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace

#ifndef TGP_CAT
#define TGP_CAT2(a, b) a##b
#define TGP_CAT(a, b) TGP_CAT2(a, b)
#endif
// one translation unit holds either the plain instantiations or the PRUNE ones (tgp_kernels_sweep_prune_k*.hip)
#ifdef TGP_SWEEP_PRUNE_TU
// `a.prune`'s header is zero.  Models of one row block: the single launch.  Otherwise means, list, survivors, fold -- in
// stream order, no host synchronisation; what depends on the number of survivors is decided on the device.
hipError_t TGP_CAT(launch_sweep_prune_kind, TGP_SWEEP_KIND)(hipStream_t s, const SweepArgs& a, int64_t grid, const PruneLaunch& pl) {
  if (a.m.Npad / DBM <= 1) return launch_sweep_dma_dp<TGP_SWEEP_KIND, true>(s, a, grid);
  const int nb = (int)(a.m.Npad / DBM), ng = nb * DKSTEPS;
  hipError_t e = with_dp<16>(a.m.dp, [&](auto DP) {
    if (pl.xc32) launch_prune_prescreen<TGP_SWEEP_KIND, DP()>(s, a, 2 * grid, pl);   // two workgroups per compute unit
    if (pl.few_max > 0) {   // the few-blocks path: taken or not on the device
      hipLaunchKernelGGL(prune_prelist_kernel, dim3(1), dim3(1024), 0, s, a, pl);
      hipLaunchKernelGGL((prune_kstar_kernel<TGP_SWEEP_KIND, DP()>), dim3((unsigned)std::min<int64_t>((int64_t)pl.few_max * ng, 8 * grid)),
                         dim3(1024), 0, s, a);
      hipLaunchKernelGGL(prune_mean_slab_kernel, dim3((unsigned)pl.few_max), dim3(1024), 0, s, a);
    }
    launch_prune_mean<TGP_SWEEP_KIND, DP()>(s, a, grid, pl.mean_waves);
    return hipSuccess;
  });
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(prune_list_kernel, dim3(1), dim3(1024), 0, s, a, pl, (int)grid);
  e = launch_sweep_dma_dp<TGP_SWEEP_KIND, true>(s, a, grid);
  if (e != hipSuccess) return e;
  if (pl.few_max > 0) hipLaunchKernelGGL(prune_tile_kernel, dim3((unsigned)(pl.few_max * nb * 16)), dim3(64), 0, s, a);
  if (pl.max_survivors > 0) hipLaunchKernelGGL(prune_fold_kernel, dim3((unsigned)pl.max_survivors), dim3(1024), 0, s, a);
  return hipGetLastError();
}
hipError_t TGP_CAT(launch_prescreen_kind, TGP_SWEEP_KIND)(hipStream_t s, const SweepArgs& a, int64_t grid, const PruneLaunch& pl) {
  return with_dp<16>(a.m.dp, [&](auto DP) {
    launch_prune_prescreen<TGP_SWEEP_KIND, DP()>(s, a, grid, pl);
    return hipGetLastError();
  });
}
#else
hipError_t TGP_CAT(launch_sweep_dma_kind, TGP_SWEEP_KIND)(hipStream_t s, const SweepArgs& a, int64_t grid) {
  return launch_sweep_dma_dp<TGP_SWEEP_KIND, false>(s, a, grid);
}
#endif

}  // namespace tgp
