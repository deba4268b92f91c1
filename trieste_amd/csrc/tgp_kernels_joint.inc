// Joint-mode posterior sweep (predict_joint / batch Monte-Carlo EI), dp <= 16: groups of q <= 64 query points,
//   mean [G, q] and cov [G, q, q] = K** - (W K*)^T (W K*)   with the diagonal clipped to >= 1e-12
// == GPflowPredictor.predict_joint_encoded (trieste/models/gpflow/interface.py:126-133).
//
// Tile: the groups are packed CONTIGUOUSLY into a 128-row x 256-column workgroup tile (floor(256 / q) whole groups:
// 250 of 256 columns at q = 50, BASELINE config C4); 16 waves as 4 (M) x 4 (N), wave tile 32 x 64 (8 accumulator
// fragments); 16-row k-steps.  C = W K* goes to a per-workgroup slab, K* is generated once per block in the diagonal
// block-steps (fused mean k* . alpha) and kept in a second slab for the later row blocks.
//
// Main loop, LDS-DMA staging (the form of tgp_kernels_sweep_dma.inc): nothing is staged through registers.  Wave w
// moves row w of a tile with global_load_lds_dwordx4: the W tile of step t + 2 (one 1 KiB row, three stages) and the K*
// tile of step t + 1 (two 1 KiB row halves, two stages) when it comes from the slab.  Per step and wave the VMEM order
// is [K* DMA x 2 (tile t+1)] [W DMA (tile t+2)] and the step ends with s_waitcnt vmcnt(1).  The register-staged form
// this replaces kept the W row in VGPRs across the step -- at the 128-VGPR cap the compiler spilled it, which put an
// s_waitcnt vmcnt(0) right behind the load in every step (round 4 knock-out runs, profiles/r04_joint_knockout.txt).
//
// Gram phase S_g = C_g^T C_g out of LDS: the C slab is re-streamed in 16-row chunks by DMA (three chunk buffers, two
// chunks in flight), every wave accumulates up to four 16 x 16 fragments of its groups per pass.  S_g is symmetric and
// the two halves are bit-identical (same products, same order over k), so only the fragments (fa <= fb) are computed
// (10 of 16 per group at q = 50: one pass of 50 fragments instead of two passes of 80) and written to both places.
// Groups are not aligned to fragment boundaries: fragment (g, fa, fb) starts at columns g q + 16 fa / g q + 16 fb and
// entries beyond q are computed and dropped.  Operand reads are single ds_read_b64 in asm blocks (the compiler's
// merged ds_read2st64_b64 runs at half rate), MFMAs of one k4-step are independent (fragment-inner order).
#include "tgp_dev.hpp"
#include "tgp_internal.hpp"

namespace tgp {
namespace {

constexpr int JBM = 128, JBN = 256, JBK = 16;
constexpr int JLDA = JBM + 16, JLDB = JBN + 16;
constexpr int JKSTEPS = JBM / JBK;                      // 8
constexpr int J_ASTAGE = JBK * JLDA;                    // 2304 doubles (W tile)
constexpr int J_BSTAGE = JBK * JLDB;                    // 4352 doubles (K* tile; also one chunk of the Gram phase)
constexpr int J_STAGES = 3 * J_ASTAGE + 2 * J_BSTAGE;   // 15616 doubles = 122 KiB; >= 3 chunk buffers
constexpr int J_GRAM_PER_PASS = 4;                      // Gram fragments per wave and pass (4 x 8 VGPRs)

#ifndef TGP_J_KO
#define TGP_J_KO 0   // timing knock-outs, WRONG results (tools/build_exp.sh): 4 no Gram phase, 64 no main loop,
                     // 128 Gram chunks always the same three (cache-resident), 256 Gram phase without MFMAs
#endif

// one wave-instruction: lane l copies 16 bytes from sbase + voff(l) to LDS byte address lds_dst + 16 l.  The global
// address is (uniform 64-bit base in SGPRs) + (32-bit per-lane offset): one loop-invariant VGPR (16 l) serves every DMA
// of the kernel -- 64-bit per-lane pointers would be spilled at the 128-VGPR cap, and every reload of a spilled value is
// an s_waitcnt vmcnt(0) that also waits for the DMA in flight.
__device__ __forceinline__ void jglds16(const double* sbase_uniform, uint32_t voff, uint32_t lds_dst_uniform) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase_uniform), "s"(lds_dst_uniform)
      : "memory");
}

template <int N>
struct JTag {
  static constexpr int value = N;
};

// One 16-row chunk of the Gram phase for a wave with NF live fragments: per k4-step 2 NF operand reads, then NF
// independent MFMAs.  la[u] / lb[u]: LDS byte addresses of the fragment's A / B operand in chunk buffer 0, row lane>>4.
template <int NF>
__device__ __forceinline__ void gram_chunk(v4d (&g)[J_GRAM_PER_PASS], const uint32_t (&la)[J_GRAM_PER_PASS],
                                           const uint32_t (&lb)[J_GRAM_PER_PASS], uint32_t boff) {
#pragma unroll
  for (int k4 = 0; k4 < JBK / 4; ++k4) {
    double pa[NF], pb[NF];
#pragma unroll
    for (int u = 0; u < NF; ++u) {
      if (TGP_J_KO & 512) {   // half the operand reads (is the phase bound by LDS throughput?)
        asm volatile("ds_read_b64 %0, %1 offset:%c2" : "=&v"(pa[u]) : "v"(la[u] + boff), "n"(k4 * 4 * JLDB * 8) : "memory");
        pb[u] = pa[u];
      } else {
      asm volatile("ds_read_b64 %0, %2 offset:%c4\n\tds_read_b64 %1, %3 offset:%c4"
                   : "=&v"(pa[u]), "=&v"(pb[u])
                   : "v"(la[u] + boff), "v"(lb[u] + boff), "n"(k4 * 4 * JLDB * 8)
                   : "memory");
      }
    }
    if constexpr (NF == 1) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pa[0]), "+v"(pb[0])::"memory");
    if constexpr (NF == 2)
      asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(pa[0]), "+v"(pb[0]), "+v"(pa[1]), "+v"(pb[1])::"memory");
    if constexpr (NF == 3)
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(pa[0]), "+v"(pb[0]), "+v"(pa[1]), "+v"(pb[1]), "+v"(pa[2]), "+v"(pb[2])::"memory");
    if constexpr (NF == 4)
      asm volatile("s_waitcnt lgkmcnt(0)"
                   : "+v"(pa[0]), "+v"(pb[0]), "+v"(pa[1]), "+v"(pb[1]), "+v"(pa[2]), "+v"(pb[2]), "+v"(pa[3]),
                     "+v"(pb[3])::"memory");
#pragma unroll
    for (int u = 0; u < NF; ++u) g[u] = mfma_f64(pa[u], pb[u], g[u]);
  }
}

template <int KIND, int DP>
__global__ __launch_bounds__(1024, 4) void joint_kernel(const SweepArgs a) {
  __shared__ __attribute__((aligned(16))) double smem[J_STAGES + JBN * DP];
  double* const sAbase = smem;                      // three W stages
  double* const sBbase = smem + 3 * J_ASTAGE;       // two K* stages
  double* const xqs = smem + J_STAGES;              // [DP][256] scaled candidate coordinates

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = w >> 2, wn = w & 3;  // 4 (M) x 4 (N) waves, wave tile 32 x 64
  const int64_t Npad = a.m.Npad;
  const int nb = (int)(Npad / JBM);
  const int d = a.m.d;
  const double variance = a.m.variance;
  const double* __restrict__ Wt = a.m.Wt;
  const uint32_t lds0 = (uint32_t)(size_t)(__attribute__((address_space(3))) double*)smem;
  const uint32_t lane16 = (uint32_t)lane * 16u;               // per-lane byte offset of every DMA
  const int q = a.q, gpb = JBN / q;                       // groups per block
  const int ncol = gpb * q;                               // live columns of a block

  const int kcol = tid & 255;                                 // generated K* entries: candidate column
  const int krg = __builtin_amdgcn_readfirstlane(tid >> 8);  // row group 0..3 -> rows 4 krg .. 4 krg + 3

  double* const kc = a.kcache + (size_t)blockIdx.x * (size_t)Npad * JBN;
  double* const cs = a.aslab + (size_t)blockIdx.x * (size_t)Npad * JBN;
  const int64_t nblk = (a.G + gpb - 1) / gpb;
  const int T = nb * (nb + 1) / 2 * JKSTEPS;

  for (int64_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int64_t cand0 = blk * ncol;                      // flat index of the block's first candidate
    for (int e = tid; e < JBN * DP; e += 1024) {
      const int j = e / DP, c = e % DP;
      const int64_t cand = cand0 + j;
      const int64_t src = (j < ncol && cand < a.M) ? cand : 0;
      xqs[c * JBN + j] = (c < d) ? a.Xq[src * d + c] / as_const(a.m.ls)[c] : 0.0;
    }
    v4d acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    double macc = 0.0;
    __syncthreads();  // xqs is read by other threads below; every DMA of the previous block has been waited for

    // wave w moves row w of a tile: the 1 KiB W row, the two 1 KiB halves of the K* row
    auto dma_A = [&](int stage, int ib, int kb, int ks) {
      const int64_t krow = (int64_t)kb * JBM + ks * JBK + w;
      const uint32_t dst = lds0 + (uint32_t)((stage * J_ASTAGE + w * JLDA) * 8);
      jglds16(Wt + krow * Npad + (int64_t)ib * JBM, lane16, __builtin_amdgcn_readfirstlane(dst));
    };
    auto dma_B = [&](int stage, int kb, int ks) {
      const int64_t krow = (int64_t)kb * JBM + ks * JBK + w;
      const double* src = kc + krow * JBN;
      const uint32_t dst = lds0 + (uint32_t)((3 * J_ASTAGE + stage * J_BSTAGE + w * JLDB) * 8);
      jglds16(src, lane16, __builtin_amdgcn_readfirstlane(dst));
      jglds16(src + 128, lane16, __builtin_amdgcn_readfirstlane(dst + 1024));
    };
    // first use of the K* rows of k-step (kb, ks): generate this thread's four entries, fold them into the mean,
    // keep them in the slab for the later row blocks, write them to the B stage
    auto generate_B = [&](int stage, int kb, int ks) {
      const int64_t krow0 = (int64_t)kb * JBM + ks * JBK + 4 * krg;
      const cptr al = as_const(a.m.alpha + krow0);
      double* const kcrow = kc + krow0 * JBN;                                   // uniform
      double* const sBrow = sBbase + stage * J_BSTAGE + (4 * krg) * JLDB;      // uniform
      // one entry at a time (not unrolled): four interleaved evaluations of the kernel function do not fit beside the
      // 64 accumulator registers, and a spill inside this loop costs an s_waitcnt vmcnt(0) on the DMA in flight
#pragma clang loop unroll(disable)
      for (int r = 0; r < 4; ++r) {
        const cptr xs = as_const(a.m.Xs + (krow0 + r) * DP);
        double r2 = 0.0;
#pragma unroll
        for (int c = 0; c < DP; ++c) {
          const double t0 = xqs[c * JBN + kcol] - xs[c];
          r2 = fma(t0, t0, r2);
        }
        const double kv = kernel_from_r2<KIND>(r2, variance);
        macc = fma(kv, al[r], macc);
        if (nb > 1) kcrow[r * JBN + kcol] = kv;
        sBrow[r * JLDB + kcol] = kv;
      }
    };
    auto advance = [&](int& i_b, int& k_b, int& k_s) {
      if (++k_s == JKSTEPS) {
        k_s = 0;
        if (++k_b > i_b) {
          k_b = 0;
          ++i_b;
        }
      }
    };

    auto store_C = [&](int ibs) {   // row block ibs of C: accumulators to the slab, cleared
      double* dst = cs + ((int64_t)ibs * JBM + wm * 32 + (lane >> 4)) * JBN + wn * 64 + (lane & 15);
#pragma unroll
      for (int fm = 0; fm < 2; ++fm)
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int fn = 0; fn < 4; ++fn) dst[(fm * 16 + 4 * r) * JBN + fn * 16] = acc[fm][fn][r];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = (v4d){0.0, 0.0, 0.0, 0.0};
    };
    if (!(TGP_J_KO & 64)) {
    bool cpend = false;
    int cpend_ib = 0;
    int ib = 0, kb = 0, ks = 0;        // tile t
    int ib1 = 0, kb1 = 0, ks1 = 0;     // tile t + 1
    advance(ib1, kb1, ks1);
    // prologue: W tiles 0 and 1 in flight, K* tile 0 generated (k-step (0, 0) is always a first use); T >= 8
    dma_A(0, 0, 0, 0);
    dma_A(1, ib1, kb1, ks1);
    generate_B(0, 0, 0);
    asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    for (int t = 0; t < T; ++t) {
      int ib2 = ib1, kb2 = kb1, ks2 = ks1;  // tile t + 2
      advance(ib2, kb2, ks2);
      const bool has1 = t + 1 < T, has2 = t + 2 < T;
      const bool gen1 = has1 && kb1 == ib1;  // tile t + 1 brings K* rows seen for the first time
      // ordinary stores go out BEFORE the step's DMA, so that vmcnt(1) at the end of the step leaves only the newest
      // DMA in flight and the stores have had the whole step to complete: the C rows finished in the previous step,
      // then the generated K* rows of tile t + 1 (their B stage was last read in step t - 1)
      if (cpend) {
        store_C(cpend_ib);
        cpend = false;
      }
      if (gen1) generate_B((t + 1) & 1, kb1, ks1);
      if (has1 && !gen1) dma_B((t + 1) & 1, kb1, ks1);
      if (has2) dma_A((t + 2) % 3, ib2, kb2, ks2);
      {
        // diagonal block-step: this wave's 32 rows all lie above the 16-row k-slab -> its A operand is zero
        const bool all_zero = kb == ib && ks * JBK >= wm * 32 + 32;
        // operand addresses rebuilt from the lane offset in every step (a handful of integer instructions): as
        // loop invariants they are the registers the compiler spills at the 128-VGPR cap, and the reload is an
        // s_waitcnt vmcnt(0) right behind the DMA issued above
        uint32_t l16 = lane16;
        asm volatile("" : "+v"(l16));
        const uint32_t lrow = l16 >> 8, lcol8 = (l16 & 0xF0u) >> 1;   // lane >> 4, 8 (lane & 15)
        const uint32_t la = lds0 + (uint32_t)(((t % 3) * J_ASTAGE + wm * 32) * 8) + lrow * (JLDA * 8) + lcol8;
        const uint32_t lb = lds0 + (uint32_t)((3 * J_ASTAGE + (t & 1) * J_BSTAGE + wn * 64) * 8) + lrow * (JLDB * 8) + lcol8;
        __builtin_amdgcn_s_setprio(2);
        if (!all_zero) {
#pragma unroll
          for (int k4 = 0; k4 < JBK / 4; ++k4) {
            double av[2], bv[4];
            // six single ds_read_b64 instead of the compiler's three half-rate ds_read2_b64 (see tgp_kernels_sweep.inc)
            asm volatile(
                "ds_read_b64 %0, %6 offset:%c8\n\t"
                "ds_read_b64 %2, %7 offset:%c10\n\t"
                "ds_read_b64 %3, %7 offset:%c11\n\t"
                "ds_read_b64 %1, %6 offset:%c9\n\t"
                "ds_read_b64 %4, %7 offset:%c12\n\t"
                "ds_read_b64 %5, %7 offset:%c13\n\t"
                "s_waitcnt lgkmcnt(0)"
                : "=&v"(av[0]), "=&v"(av[1]), "=&v"(bv[0]), "=&v"(bv[1]), "=&v"(bv[2]), "=&v"(bv[3])
                : "v"(la), "v"(lb), "n"(k4 * 4 * JLDA * 8), "n"(k4 * 4 * JLDA * 8 + 128), "n"(k4 * 4 * JLDB * 8),
                  "n"(k4 * 4 * JLDB * 8 + 128), "n"(k4 * 4 * JLDB * 8 + 256), "n"(k4 * 4 * JLDB * 8 + 384)
                : "memory");
#pragma unroll
            for (int fm = 0; fm < 2; ++fm)
#pragma unroll
              for (int fn = 0; fn < 4; ++fn) acc[fm][fn] = mfma_f64(av[fm], bv[fn], acc[fm][fn]);
          }
        }
        __builtin_amdgcn_s_setprio(0);
      }
      if (ks == JKSTEPS - 1 && kb == ib) {  // row block ib of C complete: stored at the top of the next step
        cpend = true;
        cpend_ib = ib;
      }
      // tile t + 1 complete in LDS (its DMA is older than the W instruction of tile t + 2), then publish
      if (has2) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
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
    if (cpend) store_C(cpend_ib);   // the last row block: complete before the barriers of the mean reduction below,
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // behind which other waves read it back by DMA
    }
    // ---- mean: the four row-group partials of every column (LDS is free: no DMA is outstanding) -------------------
    {
      double* const mred = smem;  // [4][256]
      mred[krg * JBN + kcol] = macc;
      __syncthreads();
      if (tid < JBN && tid < ncol && a.mean_out) {
        const int64_t cand = cand0 + tid;
        if (cand < a.M)
          a.mean_out[cand] = (mred[tid] + mred[JBN + tid]) + (mred[2 * JBN + tid] + mred[3 * JBN + tid]) + a.m.mean_const;
      }
      __syncthreads();
    }
    // ---- Gram phase: S_g = C_g^T C_g for every group of the block, fragments fa <= fb, operands from LDS ----------
    if (a.cov_out && !(TGP_J_KO & 4)) {
      const int nf = (q + 15) >> 4;                 // fragments per side of a group
      const int per_group = nf * (nf + 1) / 2;      // upper triangle, diagonal included
      const int nfrag = gpb * per_group;
      const int nchunk = (int)(Npad / JBK);
      auto dma_chunk = [&](int buf, int ch) {        // wave w moves row w of chunk ch (two 1 KiB halves)
        const double* src = cs + ((int64_t)((TGP_J_KO & 128) ? (ch % 3) : ch) * JBK + w) * JBN;
        const uint32_t dst = lds0 + (uint32_t)((buf * J_BSTAGE + w * JLDB) * 8);
        jglds16(src, lane16, __builtin_amdgcn_readfirstlane(dst));
        jglds16(src + 128, lane16, __builtin_amdgcn_readfirstlane(dst + 1024));
      };
      for (int pass0 = 0; pass0 < nfrag; pass0 += 16 * J_GRAM_PER_PASS) {
        v4d g[J_GRAM_PER_PASS];
        uint32_t la[J_GRAM_PER_PASS], lb[J_GRAM_PER_PASS];   // LDS byte address of the fragment's operands, buffer 0
        int nlive = 0;
#pragma unroll
        for (int u = 0; u < J_GRAM_PER_PASS; ++u) {
          g[u] = (v4d){0.0, 0.0, 0.0, 0.0};
          const int f = pass0 + u * 16 + w;
          if (f < nfrag) nlive = u + 1;
          const int ff = f < nfrag ? f : 0;
          const int gi = ff / per_group;
          int fa = 0, fb = ff % per_group;
          while (fb >= nf - fa) {
            fb -= nf - fa;
            ++fa;
          }
          fb += fa;
          la[u] = lds0 + (uint32_t)(((lane >> 4) * JLDB + gi * q + fa * 16 + (lane & 15)) * 8);
          lb[u] = lds0 + (uint32_t)(((lane >> 4) * JLDB + gi * q + fb * 16 + (lane & 15)) * 8);
        }
        nlive = __builtin_amdgcn_readfirstlane(nlive);
        // chunks 0 and 1 in flight; chunk ch + 2 is issued in iteration ch into the buffer iteration ch - 1 read
        dma_chunk(0, 0);
        if (nchunk > 1) dma_chunk(1, 1);
        if (nchunk > 1) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        // the chunk loop once per fragment count (wave-uniform switch OUTSIDE the loop: inside it the arms exchange
        // the accumulators through register copies in every iteration)
        auto chunk_loop = [&](auto nf_tag) {
          constexpr int NF = decltype(nf_tag)::value;
          for (int ch = 0; ch < nchunk; ++ch) {
            const bool more2 = ch + 2 < nchunk;
            if (more2) dma_chunk((ch + 2) % 3, ch + 2);
            if constexpr (NF > 0)
              if (!(TGP_J_KO & 256)) gram_chunk<NF>(g, la, lb, (uint32_t)((ch % 3) * J_BSTAGE * 8));
            // chunk ch + 1 landed (older than the two instructions of chunk ch + 2); all reads of chunk ch are done
            if (more2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
          }
        };
        switch (nlive) {
          case 4: chunk_loop(JTag<4>{}); break;
          case 3: chunk_loop(JTag<3>{}); break;
          case 2: chunk_loop(JTag<2>{}); break;
          case 1: chunk_loop(JTag<1>{}); break;
          default: chunk_loop(JTag<0>{}); break;
        }
        // cov = K** - S on the q x q block of each group; the diagonal is clipped (interface.py:130-132)
#pragma unroll
        for (int u = 0; u < J_GRAM_PER_PASS; ++u) {
          if (u >= nlive) continue;
          const int f = pass0 + u * 16 + w;
          const int gi = f / per_group;
          int fa = 0, fb = f % per_group;
          while (fb >= nf - fa) {
            fb -= nf - fa;
            ++fa;
          }
          fb += fa;
          const int64_t gg = blk * gpb + gi;
          if (gg >= a.G) continue;
          const int bcol = fb * 16 + (lane & 15);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int arow = fa * 16 + (lane >> 4) + 4 * r;
            if (arow < q && bcol < q) {
              double r2 = 0.0;
#pragma unroll
              for (int c = 0; c < DP; ++c) {
                const double tt = xqs[c * JBN + gi * q + arow] - xqs[c * JBN + gi * q + bcol];
                r2 = fma(tt, tt, r2);
              }
              double cv = kernel_from_r2<KIND>(r2, variance) - g[u][r];
              if (arow == bcol) cv = fmax(cv, VAR_FLOOR);
              a.cov_out[(gg * q + arow) * q + bcol] = cv;
              if (fa != fb) a.cov_out[(gg * q + bcol) * q + arow] = cv;   // the mirror fragment, bit-identical
            }
          }
        }
      }
    }
    __syncthreads();  // LDS (xqs, stage buffers) is rewritten by the next block
  }
}

template <int KIND>
hipError_t launch_joint_dp(hipStream_t s, const SweepArgs& a, int64_t grid) {
  dim3 g((unsigned)grid), b(1024);
  return with_dp<16>(a.m.dp, [&](auto DP) {
    hipLaunchKernelGGL((joint_kernel<KIND, DP()>), g, b, 0, s, a);
    return hipGetLastError();
  });
}

}  // namespace

hipError_t TGP_CAT(launch_joint_kind, TGP_SWEEP_KIND)(hipStream_t s, const SweepArgs& a, int64_t grid) {
  return launch_joint_dp<TGP_SWEEP_KIND>(s, a, grid);
}

}  // namespace tgp
