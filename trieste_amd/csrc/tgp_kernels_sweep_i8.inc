// Split-precision form of the fused posterior sweep (tgp_set_precision(h, TGP_PREC_I8X4)): the product
// C = W K* runs on the int8 matrix cores (v_mfma_i32_32x32x32_i8: ~50x the f64 MFMA rate) with BOTH
// operands split error-free into four signed 8-bit digit planes (the Ozaki scheme), everything else --
// K* generation, the mean, the column norms, the acquisition tail, the arg-max -- stays in float64.
//
//   W_ik  = S_i  * sum_s a_s[i][k] 2^(-7-8s),   S_i  = (1 + 2^-7) max_k |W_ik|   (a_s: balanced base-256 digits of
//   K*_kj = S'   * sum_s b_s[k][j] 2^(-7-8s),   S'   = (1 + 2^-7) variance         rint(x / S * 2^31), int8 each;
//   C_ij  = S_i S' sum_{s+s' <= 3} 2^(-14-8(s+s')) (sum_k a_s[i][k] b_s'[k][j])     |q| <= 0x7f7f7f7f = 0.99609 2^31)
//
// The inner sums are EXACT (int32 accumulation: <= 4 pairs * 2^14 * N fits for N <= 2^15); what is lost are the digit
// pairs s + s' >= 4 -- an error of rms 2^-32.8 S_i S' sqrt(i + 1) on c_i, independent over i (tools/ozaki_tight.py:
// observed / model = 0.95 .. 0.97) -- and the rounding of each operand at 2^-32 of its scale, an order below.  The scales
// are TIGHT since round 4 (rounds 2 / 3: 2 max, 2 variance): the error is proportional to S_i S', a quarter of what it
// was.  The four "diagonals" s + s' = 0..3 have their own int32 accumulators (10 MFMAs per 32-deep k-step and fragment
// pair) and are combined in float64 once per 256-row block; there the kernel also accumulates the candidate's own error
// model sum_i c_i^2 S_i^2 (i + 1) (a 32-row fragment at its largest row weight), from which the tail prices THIS
// candidate's truncation error on the variance.  With SweepArgs::rep_ub (TGP_PREC_AUTO) it flags what exceeds the parity
// tolerance and brackets the acquisition value for the exact arg-max (tgp_api.hip launch_sweep_i8_timed recomputes the
// flagged candidates in float64).  Without it this is the plain EMULATED-precision sweep (TGP_PREC_I8X4 / I8X5): no
// per-result guarantee, never the default, its own bench line.
//
// Structure (one persistent 8-wave workgroup per CU, tile = 256 rows of W x 64 candidates, 32-deep k-steps,
// double-buffered LDS, one barrier per step; 2 waves per SIMD with 256 VGPRs each -- the four diagonals of a
// 64 x 32 wave tile are 128 accumulator registers):
//   * W digit planes are prepared once per `update` in the tile-blocked layout Wq[s][k/32][i][32 B]: a
//     [256 rows x 32 k] operand tile of one plane is 8 KiB contiguous (tgp_kernels_misc.hip, w_digits_kernel);
//   * K* is generated once per candidate block in the diagonal block-steps (float64, same kernel function as the
//     f64 sweep, folded into the mean k*.alpha), split into digits with integer arithmetic, and kept in a
//     per-workgroup slab of 4 B per entry (half the f64 slab) for the later row blocks;
//   * staging is LDS-DMA only (global_load_lds_dwordx4, counted vmcnt, raw barriers -- see tgp_kernels_sweep_dma.inc):
//     THREE stages for both operands (40 KiB each), so every tile has two steps of lead; at 2 waves per SIMD and
//     ~1300-cycle steps the register-staged first form (tools/legacy_kernels/sweep_i8_regstage.inc) lost 14 points
//     of int8-pipe utilisation to exposed load latency (profiles/r02_i8_knockout.txt);
//   * LDS rows are the bare 32 B of digits (an LDS-DMA image is lane-linear, it cannot be padded); the two 16-byte
//     halves of row r are swapped when bit 3 of r is set -- applied to the SOURCE address of the DMA and to the
//     reader's address -- which makes every 32x32x32 operand fragment one conflict-free ds_read_b128.
#include "tgp_dev.hpp"
#include "tgp_internal.hpp"

namespace tgp {
namespace {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));

#ifndef TGP_I8_TRACE
#define TGP_I8_TRACE 0  // development aid (tools/build_exp.sh + tools/i8_trace.py): shader-clock stamps of the phases of a step
#endif
#if TGP_I8_TRACE
constexpr int I8_TR_T0 = 300, I8_TR_N = 128, I8_TR_S = 12;   // steps [T0, T0 + N) of the first block of workgroups 0 and 97
__device__ unsigned long long g_i8_trace[2][I8_TR_N][8][I8_TR_S];
#define I8_STAMP(i) do { __builtin_amdgcn_sched_barrier(0); tr_s[i] = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define I8_STAMP(i) do { } while (0)
#endif
constexpr int I8_BM = 256, I8_BN = 64, I8_BK = 32;
constexpr int I8_KSTEPS = I8_BM / I8_BK;                      // 8 k-steps per 256-row block
// NS digit planes per operand (4: TGP_PREC_I8X4, 5: TGP_PREC_I8X5); one LDS stage = NS x (256 + 64) rows of 32 B
constexpr int i8_a_bytes(int ns) { return ns * I8_BM * 32; }
// The training rows a generating step needs (32 rows of Xs, their alpha, their squared norms) staged in LDS: tile k-step of
// the image w_digits builds beside the digit planes, [32][dp] rows + [32] alpha + [32] |row|^2, padded to whole KiB (one DMA
// instruction each)
constexpr int i8_xt_doubles(int dp) { return i8_xs_tile_doubles(dp); }   // rows, alpha, |row|^2 (tgp_internal.hpp)
constexpr int i8_stage(int ns) { return ns * (I8_BM + I8_BN) * 32; }

// x / scale (|.| <= 1/2) -> q = rint(. * 2^(8 NS - 1)) -> its NS balanced base-256 digits (each in [-128, 127],
// q = sum_b digit_b 256^b), as the BYTES of one word: adding 128 at every byte position below the top one turns
// the balanced digits into the ordinary unsigned bytes of the sum, and flipping bit 7 of those bytes (x - 128 = x ^ 0x80
// on a byte) turns them back into the digits' two's-complement bytes; the top byte already is the top digit.
// Two integer operations per value instead of a shift / mask / subtract chain per digit.
__device__ __forceinline__ uint32_t digit_bytes4(double tfix) {  // NS = 4: byte b = the digit of weight 256^b
  const uint32_t u = (uint32_t)(int)rint(tfix) + 0x00808080u;
  return u ^ 0x00808080u;
}
__device__ __forceinline__ void digit_bytes5(double tfix, uint32_t& lo, uint32_t& top) {  // NS = 5: 4 bytes + the top digit
  const unsigned long long u = (unsigned long long)(long long)rint(tfix) + 0x0080808080ull;
  lo = (uint32_t)u ^ 0x80808080u;
  top = (uint32_t)(u >> 32) & 255u;
}
// bytes b of four words, one per output word: out[b] = (p0.b, p1.b, p2.b, p3.b) -- a 4 x 4 byte transpose, 8 v_perm_b32
__device__ __forceinline__ void transpose_bytes4(uint32_t p0, uint32_t p1, uint32_t p2, uint32_t p3, uint32_t (&out)[4]) {
  // v_perm_b32 D, S0, S1, sel: selector byte i picks byte sel_i of the eight bytes {S0 (4..7), S1 (0..3)}
  const uint32_t x_lo = __builtin_amdgcn_perm(p1, p0, 0x05010400u);  // p0.b0 p1.b0 p0.b1 p1.b1
  const uint32_t x_hi = __builtin_amdgcn_perm(p1, p0, 0x07030602u);  // p0.b2 p1.b2 p0.b3 p1.b3
  const uint32_t y_lo = __builtin_amdgcn_perm(p3, p2, 0x05010400u);
  const uint32_t y_hi = __builtin_amdgcn_perm(p3, p2, 0x07030602u);
  out[0] = __builtin_amdgcn_perm(y_lo, x_lo, 0x05040100u);
  out[1] = __builtin_amdgcn_perm(y_lo, x_lo, 0x07060302u);
  out[2] = __builtin_amdgcn_perm(y_hi, x_hi, 0x05040100u);
  out[3] = __builtin_amdgcn_perm(y_hi, x_hi, 0x07060302u);
}

// one wave-instruction: lane l copies 16 bytes from its own global address to LDS byte address lds_dst + 16 l
__device__ __forceinline__ void i8_glds16(const void* gsrc, uint32_t lds_dst_uniform) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(gsrc), "s"(lds_dst_uniform)
      : "memory");
}

// byte offset of the 16-byte half h of row r inside a [rows][32 B] plane image (halves swapped when bit 3 of r is set)
__device__ __forceinline__ int i8_off(int r, int h) { return (r * 2 + (h ^ ((r >> 3) & 1))) * 16; }

template <int N>
__device__ __forceinline__ void i8_wait_vm() {
  static_assert(N >= 0 && N <= 8, "counted waits of the DMA pipeline");
  if constexpr (N == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  else if constexpr (N == 1) asm volatile("s_waitcnt vmcnt(1)" ::: "memory");
  else if constexpr (N == 2) asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
  else if constexpr (N == 3) asm volatile("s_waitcnt vmcnt(3)" ::: "memory");
  else if constexpr (N == 4) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  else if constexpr (N == 5) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
  else if constexpr (N == 6) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
  else if constexpr (N == 7) asm volatile("s_waitcnt vmcnt(7)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
}

// one wave-instruction, address = uniform 64-bit base (SGPRs) + 32-bit per-lane byte offset: no 64-bit lane arithmetic
__device__ __forceinline__ void i8_glds16s(const unsigned char* sbase_uniform, uint32_t voff, uint32_t lds_dst_uniform) {
  unsigned keep;
  asm volatile(
      "s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2\n\ts_mov_b32 m0, %0"
      : "=&s"(keep)
      : "v"(voff), "s"(sbase_uniform), "s"(lds_dst_uniform)
      : "memory");
}

// the same for the K* slab: a per-workgroup stream (1 MiB per candidate block, re-read once per row block: no reuse any cache
// level could serve) next to the W tiles, which every workgroup of an XCD reads and which live on L2 hits
#ifndef TGP_I8_SLAB_POLICY
#define TGP_I8_SLAB_POLICY 0  // 0 default policy, 1 nt, 2 sc1 nt, 3 sc0 sc1, 4 sc0 sc1 nt, 5 sc1
#endif
__device__ __forceinline__ void i8_glds16s_slab(const unsigned char* sbase_uniform, uint32_t voff, uint32_t lds_dst_uniform) {
  unsigned keep;
#define TGP_I8_SLAB_ASM(POL)                                                                                            \
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2" POL "\n\ts_mov_b32 m0, %0" \
               : "=&s"(keep)                                                                                            \
               : "v"(voff), "s"(sbase_uniform), "s"(lds_dst_uniform)                                                    \
               : "memory")
  if constexpr (TGP_I8_SLAB_POLICY == 1) TGP_I8_SLAB_ASM(" nt");
  else if constexpr (TGP_I8_SLAB_POLICY == 2) TGP_I8_SLAB_ASM(" sc1 nt");
  else if constexpr (TGP_I8_SLAB_POLICY == 3) TGP_I8_SLAB_ASM(" sc0 sc1");
  else if constexpr (TGP_I8_SLAB_POLICY == 4) TGP_I8_SLAB_ASM(" sc0 sc1 nt");
  else if constexpr (TGP_I8_SLAB_POLICY == 5) TGP_I8_SLAB_ASM(" sc1");
  else TGP_I8_SLAB_ASM("");
#undef TGP_I8_SLAB_ASM
}

#ifndef TGP_I8_SLAB_NT_STORE
#define TGP_I8_SLAB_NT_STORE 0
#endif
#ifndef TGP_I8_PRIO
#define TGP_I8_PRIO 1  // s_setprio 1 around the MFMAs: 1 always, 0 never, 2 not in generating steps
#endif
#ifndef TGP_I8_GENFIRST
#define TGP_I8_GENFIRST 0  // round 6 experiment, measured and NOT the default (profiles/r06_i8_genfirst.txt, r06_i8_trace.txt): in a
                           // generating step the waves 0-3 generate their K* entries BEFORE their MFMAs, the waves 4-7 after
                           // theirs, so that one wave's float64 VALU work runs under its SIMD partner's int8 MFMAs.  In the kernel
                           // the partner's MFMA phase stretches from 1300 to 2050 cycles under that VALU stream and the step is
                           // as long as before (4470 against 4370 cycles): 80.8 against 80.0 ms.
#endif
#ifndef TGP_I8_GENMFMA
#define TGP_I8_GENMFMA 1   // round 6: the squared distances of a generating step as a float64 MFMA product (dot-product form
                           // |x|^2 + |X_k|^2 - 2 x . X_k, two v_mfma_f64_16x16x4 per wave at d <= 8) instead of 16 d difference /
                           // fma instructions per thread fed by ~24 dependent LDS reads: the in-kernel trace showed that phase at
                           // 950 - 1600 cycles per wave for 64 FMAs (LDS round trips in sequence at the 256-VGPR cap), half of a
                           // generating step's excess over a plain one.  Needs the staged training rows (four planes, d <= 16);
                           // Matern-1/2 keeps the difference form (kink at r = 0, see tgp_kernels_traj.hip).
#endif
#ifndef TGP_I8_SHORTK
#define TGP_I8_SHORTK 1    // round 6: the generating steps evaluate the kernel function in the SHORT forms of the trajectory kernel
                           // (tgp_dev.hpp traj_shape: log2(e) and sqrt(c) folded into the distance scale, one coupled Goldschmidt
                           // step for the square root, 2^t with an exact fractional part; the exponential at 1 - 2 ulp, the square
                           // root as far as traj_sqrt's comment says) -- ~27 instead of ~34 float64
                           // instructions per Matern-5/2 entry.  Round 5 measured a (less accurate) short form at 0.35 %: generation
                           // was bound by its scalar-load / LDS round trips then, not by its instruction count.
#endif
#ifndef TGP_I8_WMMAP
#define TGP_I8_WMMAP 1     // round 6: which 64-row quarter of the 256-row tile a wave owns.  In a diagonal block-step the quarters
                           // carry 3 / 7 / 11 / 15 live 32-row fragments over its eight k-steps; waves w and w + 4 share a SIMD:
                           // 1 pairs quarter 0 with 3 and 1 with 2 (18 fragments per SIMD), 0 = rounds 2-5 (0 with 2, 1 with 3: 14 / 22)
#endif
#ifndef TGP_I8_KO
#define TGP_I8_KO 0  // development aid, timing only (WRONG results): 1 no DMA, 2 K* DMA from an L2-resident corner of the slab,
                     // 4 no K* generation, 8 no row-block fold (and with it no MFMAs, no operand reads), 16 no step barrier, 32 no W DMA
#endif

template <int KIND, int DP, int NS>
__global__ __launch_bounds__(512, 2) void sweep_i8_kernel(const SweepArgs a) {
  constexpr int I8_NS = NS, I8_A_BYTES = i8_a_bytes(NS), I8_STAGE = i8_stage(NS);
  constexpr double FIX = NS == 4 ? 2147483648.0 : 549755813888.0;  // 2^(8 NS - 1)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  double* const xqs = (double*)(smem_raw + 3 * I8_STAGE);  // [DP][64] scaled candidate coordinates
  // generation reads its training rows from LDS when the launch staged them (SweepArgs::i8_xsa; DP <= 16 and room in LDS):
  // three tile buffers behind the coordinates, filled by DMA two steps ahead.  Through scalar loads -- the other form -- a
  // generating step began with ~500 cycles of s_load latency that nothing overlapped (in-kernel trace, profiles/r05_i8_h.txt:
  // "distances" 700 - 1100 cycles for 64 FMAs)
  constexpr int XT = i8_xt_doubles(DP), XT_DMA = XT / 128, XT_USED = 32 * DP + 64;
  // three tile buffers beside four planes (rows requested two steps ahead), TWO beside five (round 6: requested one step
  // ahead, first among the step's DMA instructions, complete at the step's own wait); tgp_api.hip hands the tile image over
  // under the same condition (tgp_internal.hpp i8_tiles_fit)
  constexpr bool xs_lds = i8_tiles_fit(NS, DP);
  constexpr int NXB = i8_tile_buffers(NS);
  constexpr bool gen_mfma = TGP_I8_GENMFMA && xs_lds && KIND != KIND_M12;
  const uint32_t xsl0 = 3 * I8_STAGE + I8_BN * DP * 8;     // byte offset of the first tile buffer
  // [64] squared norms of the scaled candidates (gen_mfma), times the kernel's distance scale: in the padding of tile buffer 0
  // where a tile has 64 spare doubles (the tile DMA masks the lanes of the padding: dma_X), else behind the buffers
  double* const qn = (double*)(smem_raw + xsl0 + (i8_qn_in_pad(DP) ? XT_USED : NXB * XT) * 8);
  constexpr double KSC = TGP_I8_SHORTK ? TrajShape<KIND>::SCALE : 1.0;   // q = KSC r^2 is what the kernel function takes
  double* const red = (double*)(smem_raw);                 // reduction scratch (aliases stage 0 after the sweep)

  const int tid = threadIdx.x, lane = tid & 63;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  // 4 (M) x 2 (N) waves, wave tile 64 x 32; quarters 0, 1 (light in diagonal block-steps) on the waves 0-3
  const int wm = (TGP_I8_WMMAP && w >= 4) ? 3 - ((w - 4) >> 1) : (w >> 1), wn = w & 1;
  const int64_t Npad = a.m.Npad;
  const int nb = (int)(Npad / I8_BM);
  const int d = a.m.d;
  const double variance = a.m.variance;
  const double colscale = I8_TIGHT * variance;                  // S' (k <= variance: the digits stay inside 0x7f7f7f7f)
  const double to_fixed = FIX / colscale;                       // 2^(8 NS - 1) / S'
  const unsigned char* const Wq = (const unsigned char*)a.i8_wq;
  const size_t plane = (size_t)Npad * (size_t)Npad;             // bytes per digit plane
  unsigned char* const slab = (unsigned char*)a.kcache + (size_t)blockIdx.x * (size_t)Npad * (I8_BN * I8_NS);
  const uint32_t lds0 = (uint32_t)(size_t)(__attribute__((address_space(3))) unsigned char*)smem_raw;
  const uint32_t row_bytes = (uint32_t)Npad * 32u;              // one k-step image of a plane: [Npad rows][32 B] (< 2^19)

  // DMA lane roles: lane l moves the half (l & 1) ^ bit3(row) of row (l >> 1) of a 32-row group to LDS position l.
  // Every source address is (uniform 64-bit base) + (32-bit lane offset): offsets inside a plane stay below 2^28
  // (N <= 16384), inside a slab below 2^23.
  const int dr = lane >> 1;                                       // row inside the group (bit 3 of the tile row = bit 3 of dr)
  const int dh = (lane & 1) ^ ((dr >> 3) & 1);                    // source half
  const uint32_t a_lane = (uint32_t)((w * 32 + dr) * 32 + dh * 16);                  // + kstep * row_bytes + ib * 8192
  const uint32_t b_lane = (uint32_t)(((w >> 1) * I8_BN + (w & 1) * 32 + dr) * 32 + dh * 16);   // item w: plane w >> 1, half w & 1
  const uint32_t a_dst = lds0 + (uint32_t)(w * 1024);                                // + stage + s * 8192
  const uint32_t b_dst = lds0 + (uint32_t)(I8_A_BYTES + ((w >> 1) * I8_BN + (w & 1) * 32) * 32);  // + stage
  // operand reads: lane l holds row / candidate l & 31, k half l >> 5 of a fragment
  const uint32_t l_off = (uint32_t)i8_off(lane & 31, lane >> 5);
  const uint32_t a_rd = l_off + (uint32_t)(wm * 2048);                               // + stage + f * 1024 + s * 8192
  const uint32_t b_rd = l_off + (uint32_t)(I8_A_BYTES + wn * 1024);                  // + stage + s * 2048
  // slab write-out of a generated tile (logical layout): plane, candidate, half
  const int b_col = (tid >> 1) & 63, b_half = tid & 1;   // + plane (tid >> 7) + 4 j: NS x 64 x 2 items over 512 threads
  // generation: this thread's candidate column and k quad (4 consecutive k of the 32-row tile).  Difference form: column =
  // lane, quad = wave.  MFMA form: wave w owns the 16 x 16 tile (k half w >> 2, candidate group w & 3) of the cross products;
  // the accumulator of lane l holds rows (l >> 4) + 4 r of column l & 15, and the A operand's rows are permuted so that
  // these ARE four consecutive k: quad 4 (w >> 2) + (l >> 4)
  const int g_col = gen_mfma ? 16 * (w & 3) + (lane & 15) : (tid & 63);
  const int g_kq = gen_mfma ? 4 * (w >> 2) + (lane >> 4) : w;

  const int64_t nblk = (a.M + I8_BN - 1) / I8_BN;
  // candidate blocks: the first one by workgroup index, every later one drawn from a counter (SweepArgs::blk_ctr) -- the
  // workgroups of a launch do not run at one speed (XCDs, clocks), and a static 64-blocks-each split ends with the slowest
  for (int64_t blk = blockIdx.x; blk < nblk;) {
    for (int e = tid; e < I8_BN * DP; e += 512) {
      const int j = e / DP, c = e % DP;
      const int64_t cand = blk * I8_BN + j;
      const int64_t src = cand < a.M ? cand : 0;
      // with the staged tiles (ModelDev::xc) the coordinates are centred at the first training input, Xs_0
      xqs[c * I8_BN + j] = (c < d) ? a.Xq[src * d + c] / as_const(a.m.ls)[c] - (xs_lds ? as_const(a.m.Xs)[c] : 0.0) : 0.0;
    }
    v16i acc[2][I8_NS];
#pragma unroll
    for (int f = 0; f < 2; ++f)
#pragma unroll
      for (int g = 0; g < I8_NS; ++g)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[f][g][r] = 0;
#ifndef TGP_I8_ESQ
#define TGP_I8_ESQ 2  // development aid (tools/build_exp.sh): 0 = no error model (timing only), 2 = per 32-row fragment
#endif
    double ssq = 0.0, macc = 0.0;
    float esq = 0.f;  // sum_i c_i^2 S_i^2 (i + 1), a 32-row fragment at its largest row weight: the candidate's own
                      // error model (three digits are plenty: single precision, one register)
    __syncthreads();  // xqs is read by other threads below; no DMA of the previous block is outstanding
    if constexpr (gen_mfma) {
      if (tid < I8_BN) {
        double s2 = 0.0;
#pragma unroll
        for (int c = 0; c < DP; ++c) s2 = fma(xqs[c * I8_BN + tid], xqs[c * I8_BN + tid], s2);
        qn[tid] = KSC * s2;
      }
      __syncthreads();
    }

    // step t -> (row block ib, k block kb <= ib, k-step ks): k range [(kb*8 + ks)*32, +32)
    // wave w moves the 32-row group w of all W planes (NS instructions) ...
    auto dma_A = [&](uint32_t st, uint32_t a_off) {   // a_off = kstep * row_bytes + ib * 8192
      const uint32_t voff = a_lane + a_off;
      const uint32_t dst = a_dst + st;
#pragma unroll
      for (int s = 0; s < I8_NS; ++s) i8_glds16s(Wq + s * plane, voff, dst + s * (I8_BM * 32));
    };
    // ... and the 32-candidate halves of the K* planes from the slab: 2 NS instructions over the 8 waves (one each for
    // NS = 4; for NS = 5 waves 0 and 1 take a second one)
    auto dma_B = [&](uint32_t st, uint32_t b_off) {   // b_off = kstep * NS * 2048
      const uint32_t voff = b_lane + ((TGP_I8_KO & 2) ? (b_off & (8 * I8_NS * I8_BN * 32 - 1)) : b_off);
      i8_glds16s_slab(slab, voff, b_dst + st);
      if (I8_NS == 5 && w < 2) i8_glds16s_slab(slab + 4 * (I8_BN * 32), voff, b_dst + st + 4 * (I8_BN * 32));
    };
    const int n_dma_b = 1 + ((w + 8 < 2 * I8_NS) ? 1 : 0);   // this wave's K* DMA instructions per step
    // the training-row tile of k-step `kstep` into tile buffer xb (byte offset): waves 0 .. XT_DMA - 1, one KiB each
    const int n_dma_x = (w < XT_DMA) ? 1 : 0;
    auto dma_X = [&](uint32_t xb, int kstep) {   // (the lanes of a tile's zero padding stay off: qn may live there)
      if (w < XT_DMA && w * 128 + lane * 2 < XT_USED)
        i8_glds16s((const unsigned char*)a.i8_xsa, (uint32_t)lane * 16u + (uint32_t)(kstep * XT + w * 128) * 8u,
                   lds0 + xb + (uint32_t)(w * 1024));
    };
    // first use of these 32 rows of K*: generate this thread's 4 entries (rows 4 kq .. 4 kq + 3), digits to the B stage
#if TGP_I8_TRACE
    unsigned long long* tr_g = nullptr;
#define I8_GSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); if (tr_g) tr_g[i] = __builtin_readcyclecounter(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define I8_GSTAMP(i) do { } while (0)
#endif
    auto generate_B = [&](uint32_t st, int kstep, uint32_t xb) {
      I8_GSTAMP(0);
      const int64_t k0 = (int64_t)kstep * I8_BK + 4 * g_kq;
      double r2[4] = {0.0, 0.0, 0.0, 0.0};
      double al[4];
      if constexpr (gen_mfma) {
        // r^2 = |x|^2 + |X_k|^2 - 2 x . X_k, the cross products on the float64 matrix core: D[i][j] = sum_c A[i][c] B[c][j],
        // A[i][c] = tile row rowmap(i), coordinate c; B[c][j] = candidate 16 (w & 3) + j, coordinate c
        const double* xt = (const double*)(smem_raw + xb);
        const int gl = lane & 15, gq = lane >> 4;
        const int arow = 16 * (w >> 2) + 4 * (gl & 3) + (gl >> 2);   // rowmap: accumulator row q + 4 r <-> k = 4 q + r
        v4d dd = (v4d){0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k4 = 0; k4 < (DP + 3) / 4; ++k4) {
          const int dim = gq + 4 * k4;
          const bool in = (DP % 4 == 0) || dim < DP;
          const double av = in ? xt[arow * DP + dim] : 0.0;
          const double bv = in ? xqs[dim * I8_BN + g_col] : 0.0;
          dd = mfma_f64(av, bv, dd);
        }
        const double* all = xt + 32 * DP + 4 * g_kq;     // this lane's four consecutive rows: alpha, |row|^2
        const double qnj = qn[g_col];                      // (KSC |x|^2)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          al[r] = all[r];
          r2[r] = fmax(fma(-2.0 * KSC, dd[r], fma(KSC, all[32 + r], qnj)), 0.0);   // KSC r^2
        }
      } else if constexpr (xs_lds) {   // rows 4 kq .. 4 kq + 3 of the staged tile: wave-uniform LDS addresses (broadcast reads)
        const double* xl = (const double*)(smem_raw + xb) + 4 * g_kq * DP;
        const double* all = (const double*)(smem_raw + xb) + 32 * DP + 4 * g_kq;
#pragma unroll
        for (int r = 0; r < 4; ++r) al[r] = all[r];
#pragma unroll
        for (int c = 0; c < DP; ++c) {
          const double x = xqs[c * I8_BN + g_col];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double t0 = x - xl[r * DP + c];
            r2[r] = fma(t0, t0, r2[r]);
          }
        }
      } else {
        const cptr xs = as_const(a.m.Xs + k0 * DP);
        const cptr als = as_const(a.m.alpha + k0);
#pragma unroll
        for (int r = 0; r < 4; ++r) al[r] = als[r];
#pragma unroll
        for (int c = 0; c < DP; ++c) {
          const double x = xqs[c * I8_BN + g_col];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double t0 = x - xs[r * DP + c];
            r2[r] = fma(t0, t0, r2[r]);
          }
        }
      }
      if constexpr (TGP_I8_SHORTK && !gen_mfma) {
#pragma unroll
        for (int r = 0; r < 4; ++r) r2[r] *= KSC;
      }
      I8_GSTAMP(1);
      // this thread's four entries as digit planes: pk[s] = the bytes (entry 0 .. 3) of plane s, most significant first
      uint32_t pk[I8_NS], pw[4], ptop = 0u;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const double kv = TGP_I8_SHORTK ? variance * traj_shape<KIND>(r2[r]) : kernel_from_r2<KIND>(r2[r], variance);
        macc = fma(kv, al[r], macc);
        if constexpr (I8_NS == 4) {
          pw[r] = digit_bytes4(kv * to_fixed);
        } else {
          uint32_t top;
          digit_bytes5(kv * to_fixed, pw[r], top);
          ptop |= top << (8 * r);
        }
      }
      {
        uint32_t byw[4];  // byw[b]: the digits of weight 256^b
        transpose_bytes4(pw[0], pw[1], pw[2], pw[3], byw);
        if constexpr (I8_NS == 4) {
#pragma unroll
          for (int s = 0; s < 4; ++s) pk[s] = byw[3 - s];
        } else {
          pk[0] = ptop;
#pragma unroll
          for (int s = 1; s < 5; ++s) pk[s] = byw[4 - s];
        }
      }
      // bytes 4 kq .. 4 kq + 3 of candidate row g_col: half kq >> 2, offset (4 kq) & 15 inside it
      unsigned char* dst = smem_raw + st + I8_A_BYTES + i8_off(g_col, g_kq >> 2) + ((4 * g_kq) & 15);
#pragma unroll
      for (int s = 0; s < I8_NS; ++s) *(uint32_t*)(dst + s * I8_BN * 32) = pk[s];
      I8_GSTAMP(2);
    };

    // The T = 8 P steps of a candidate block are walked as P = nb (nb + 1) / 2 block-steps (ib, kb <= ib) of eight k-steps.
    // Per step the scalar bookkeeping is a handful of adds: what a step needs about tiles t + 1 and t + 2 is loop-invariant
    // inside a block-step except in its last two k-steps, which look into the NEXT block-step -- three inlined copies of the
    // step body (k-steps 0..5, 6, 7) instead of one generic body that re-derives everything from (ib, kb, ks) (round 4:
    // ~120 scalar instructions per step and wave, most of them between the barrier and the first operand read).
    uint32_t st0 = 0, st1 = I8_STAGE, st2 = 2 * I8_STAGE;   // LDS byte offsets of the stages of tiles t, t + 1, t + 2
    // prologue: W tiles 0 and 1 in flight (k-steps (0,0) and (0,1) are first uses of their K* rows: no slab DMA),
    // K* tile 0 generated
    // tile buffers.  Three: of tiles t + 1, t + 2, t + 3 (requested in step t, two steps of lead).  Two: of tile t + 1 and the
    // target of tile t + 2's rows (requested in step t into the buffer step t - 1 generated from, complete at step t's wait)
    uint32_t xb1 = xsl0 + XT * 8, xb2 = NXB == 3 ? xsl0 + 2 * XT * 8 : xsl0, xb3 = xsl0;
    if constexpr (xs_lds) {   // the rows of tiles 0, 1 (, 2) (all of row block 0 is generated): in LDS before anything reads them
      dma_X(xsl0, 0);
      dma_X(xb1, 1);
      if constexpr (NXB == 3) dma_X(xb2, 2);
      i8_wait_vm<0>();
      __builtin_amdgcn_s_barrier();
    }
    dma_A(st0, 0);
    dma_A(st1, row_bytes);
    generate_B(st0, 0, xsl0);
    i8_wait_vm<I8_NS>();
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    // one k-step: tile t = (ib, kb, ks) in stage st0.  diag: kb == ib.  gen1: tile t + 1 is generated in this step
    // (kstep1 = its k-step).  has2 / dmab2 / a_off2 / b_off2: tile t + 2's DMA.  fold: the row block is complete.
    // gen3 / kstep3: tile t + 3 (three tile buffers; t + 2 with two) will be generated: its training rows are requested in this step.
    auto step = [&](const int ks, const bool diag, const int kstep, const bool gen1, const int kstep1, const bool has2,
                    const bool dmab2, const uint32_t a_off2, const uint32_t b_off2, const bool fold, const int ib,
                    const int t, const bool gen3, const int kstep3) {
      const bool xdma = xs_lds && gen3;
#if TGP_I8_TRACE
      unsigned long long tr_s[I8_TR_S] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
      tr_g = tr_s + 8;
#endif
      I8_STAMP(0);
      const bool gen_early = TGP_I8_GENFIRST && gen1 && w < 4 && !(TGP_I8_KO & 4);
      if (gen_early) generate_B(st1, kstep1, xb1);
      if (diag && nb > 1) {  // tile t was generated: keep its digits for the later row blocks (logical layout)
#pragma unroll
        for (int it = 0; it < (I8_NS + 3) / 4; ++it) {
          const int b_s = (tid >> 7) + 4 * it;
          if (b_s < I8_NS)
            *(v4i*)(slab + ((size_t)kstep * I8_NS + b_s) * (I8_BN * 32) + b_col * 32 + b_half * 16) =
                *(const v4i*)(smem_raw + st0 + I8_A_BYTES + b_s * (I8_BN * 32) + i8_off(b_col, b_half));
        }
      }
      I8_STAMP(1);
      {
        // W is lower triangular: in a diagonal block-step a 32-row fragment whose rows all lie above the
        // k-step's columns multiplies zeros (wave-uniform predicate, one branch per fragment)
        const int kofs = ks * I8_BK;
        const unsigned char* bp = smem_raw + (st0 + b_rd);
        const unsigned char* ap = smem_raw + (st0 + a_rd);
        v4i bv[I8_NS];
#pragma unroll
        for (int s = 0; s < I8_NS; ++s) bv[s] = *(const v4i*)(bp + s * (I8_BN * 32));
        const bool prio = TGP_I8_PRIO == 1 || (TGP_I8_PRIO == 2 && !gen1);
        if (prio) __builtin_amdgcn_s_setprio(1);
        const bool live0 = !(diag && kofs >= wm * 64 + 32), live1 = !(diag && kofs >= wm * 64 + 64);
        v4i av[I8_NS];
        if (live0) {
#pragma unroll
          for (int s = 0; s < I8_NS; ++s) av[s] = *(const v4i*)(ap + s * (I8_BM * 32));
#pragma unroll
          for (int g = 0; g < I8_NS; ++g)
#pragma unroll
            for (int s = 0; s <= g; ++s)
              acc[0][g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[s], bv[g - s], acc[0][g], 0, 0, 0);
        }
        I8_STAMP(2);
        // the step's DMA (tile t + 2) goes out BETWEEN the two row fragments: issued before the MFMAs (rounds 2-4) all
        // eight waves queue ~1350 cycles at the memory pipeline with the matrix pipe idle; after them the same queue
        // forms in front of the barrier (profiles/r05_i8_trace_ko.txt, r05_i8_c.txt: 91.7 / 88.4 / 91.5 ms)
        if (prio) __builtin_amdgcn_s_setprio(0);
        if (!(TGP_I8_KO & 1)) {
          if (NXB == 2 && xdma) dma_X(xb2, kstep3);   // FIRST: older than this step's A / B instructions, so the step's wait covers it
          if (dmab2) dma_B(st2, b_off2);
          if (has2 && !(TGP_I8_KO & 32)) dma_A(st2, a_off2);
          if (NXB == 3 && xdma) dma_X(xb3, kstep3);
        }
        if (prio) __builtin_amdgcn_s_setprio(1);
        if (live1) {
#pragma unroll
          for (int s = 0; s < I8_NS; ++s) av[s] = *(const v4i*)(ap + 1024 + s * (I8_BM * 32));
#pragma unroll
          for (int g = 0; g < I8_NS; ++g)
#pragma unroll
            for (int s = 0; s <= g; ++s)
              acc[1][g] = __builtin_amdgcn_mfma_i32_32x32x32_i8(av[s], bv[g - s], acc[1][g], 0, 0, 0);
        }
        if (prio) __builtin_amdgcn_s_setprio(0);
      }
      I8_STAMP(3);
      if (gen1 && !gen_early && !(TGP_I8_KO & 4)) generate_B(st1, kstep1, xb1);
      if (fold && !(TGP_I8_KO & 8)) {  // row block ib complete: digits -> float64, fold into the column norms
        const double k0s = colscale * 6.103515625e-05;  // S' 2^-14: the weight of diagonal 0 (digits carry 2^(-7-8s))
#pragma unroll
        for (int f = 0; f < 2; ++f) {
          const double* rsp = a.i8_rs + (int64_t)ib * I8_BM + wm * 64 + f * 32 + 4 * (lane >> 5);
          const double ssq_in = ssq;
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            // D layout of the 32x32 forms: col = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
            double tsum = (double)acc[f][I8_NS - 1][r];
#pragma unroll
            for (int g = I8_NS - 2; g >= 0; --g) tsum = fma(tsum, 0.00390625, (double)acc[f][g][r]);
            const double cv = rsp[(r & 3) + 8 * (r >> 2)] * k0s * tsum;
            ssq = fma(cv, cv, ssq);
#pragma unroll
            for (int g = 0; g < I8_NS; ++g) acc[f][g][r] = 0;
          }
          if (TGP_I8_ESQ)  // this fragment's share of |c|^2 at the fragment's weight (rs[Npad + row / 32])
            esq = fmaf((float)(ssq - ssq_in), (float)a.i8_rs[Npad + (int64_t)ib * (I8_BM / 32) + wm * 2 + f], esq);
        }
      }
      I8_STAMP(4);
      // tile t + 1 complete in LDS: everything older than this step's DMA (tile t + 2) has landed; then publish.
      // (compiler-issued VMEM of this step -- the slab write-out, the row scales -- is older or already waited for:
      // it can only make these waits stronger)
      if (TGP_I8_KO & 1) {
      } else if (TGP_I8_KO & 32) {
        i8_wait_vm<2>();
      } else {
        // this step's own DMA instructions of this wave stay in flight, everything older has landed
        const int mine = (has2 ? I8_NS : 0) + (dmab2 ? n_dma_b : 0) + ((NXB == 3 && xdma) ? n_dma_x : 0);
        switch (mine) {
          case 0: i8_wait_vm<0>(); break;
          case 1: i8_wait_vm<1>(); break;
          case 2: i8_wait_vm<2>(); break;
          case 3: i8_wait_vm<3>(); break;
          case 4: i8_wait_vm<4>(); break;
          case 5: i8_wait_vm<5>(); break;
          case 6: i8_wait_vm<6>(); break;
          case 7: i8_wait_vm<7>(); break;
          default: i8_wait_vm<8>(); break;
        }
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      I8_STAMP(5);
      if (!(TGP_I8_KO & 16)) __builtin_amdgcn_s_barrier();
      I8_STAMP(6);
#if TGP_I8_TRACE
      if ((blockIdx.x == 0 || blockIdx.x == 97) && blk == blockIdx.x && t >= I8_TR_T0 && t < I8_TR_T0 + I8_TR_N && lane == 0) {
        tr_s[7] = ((unsigned long long)(gen1 ? 1 : 0) << 32) | ((unsigned long long)(diag ? 1 : 0) << 16) | (unsigned)ks;
#pragma unroll
        for (int i = 0; i < I8_TR_S; ++i) g_i8_trace[blockIdx.x ? 1 : 0][t - I8_TR_T0][w][i] = tr_s[i];
      }
#endif
      const uint32_t st_old = st0;
      st0 = st1;
      st1 = st2;
      st2 = st_old;
      const uint32_t xb_old = xb1;
      xb1 = xb2;
      xb2 = NXB == 3 ? xb3 : xb_old;
      xb3 = xb_old;
    };
    constexpr uint32_t B_STEP = I8_NS * I8_BN * 32;   // one k-step of the slab
    const int P = nb * (nb + 1) / 2;
    int ib = 0, kb = 0;
#pragma unroll 1
    for (int p = 0; p < P; ++p) {
      int ibn = ib, kbn = kb + 1;   // the next block-step
      if (kbn > ib) {
        kbn = 0;
        ibn = ib + 1;
      }
      const bool hasn = p + 1 < P, diag = kb == ib, diagn = kbn == ibn;
      const uint32_t abase = (uint32_t)(kb * I8_KSTEPS) * row_bytes + (uint32_t)ib * (I8_BM * 32);
      const uint32_t abasen = (uint32_t)(kbn * I8_KSTEPS) * row_bytes + (uint32_t)ibn * (I8_BM * 32);
      const uint32_t bbase = (uint32_t)(kb * I8_KSTEPS) * B_STEP, bbasen = (uint32_t)(kbn * I8_KSTEPS) * B_STEP;
      const int k8 = kb * I8_KSTEPS, t8 = p * I8_KSTEPS;
      // the tile whose training rows a step requests -- t + 3 with three tile buffers, t + 2 with two (LEAD steps ahead): in this
      // block-step while ks + LEAD < 8, else k-step ks + LEAD - 8 of the next one
      constexpr int LEAD = NXB == 3 ? 3 : 2;
#pragma unroll 1
      for (int ks = 0; ks < I8_KSTEPS - 2; ++ks)
        step(ks, diag, k8 + ks, diag, k8 + ks + 1, true, !diag, abase + (uint32_t)(ks + 2) * row_bytes,
             bbase + (uint32_t)(ks + 2) * B_STEP, false, ib, t8 + ks, ks + LEAD < I8_KSTEPS ? diag : (hasn && diagn),
             ks + LEAD < I8_KSTEPS ? k8 + ks + LEAD : kbn * I8_KSTEPS + ks + LEAD - I8_KSTEPS);
      step(I8_KSTEPS - 2, diag, k8 + I8_KSTEPS - 2, diag, k8 + I8_KSTEPS - 1, hasn, hasn && !diagn, abasen, bbasen, false, ib,
           t8 + I8_KSTEPS - 2, hasn && diagn, kbn * I8_KSTEPS + LEAD - 2);
      step(I8_KSTEPS - 1, diag, k8 + I8_KSTEPS - 1, hasn && diagn, kbn * I8_KSTEPS, hasn, hasn && !diagn, abasen + row_bytes,
           bbasen + B_STEP, diag, ib, t8 + I8_KSTEPS - 1, hasn && diagn, kbn * I8_KSTEPS + LEAD - 1);
      ib = ibn;
      kb = kbn;
    }
    // ---- reductions (LDS is free after the last barrier) ---------------------------------------
    // mean: thread (kq = wave, col = lane) holds the partial over its k quads; ssq: lanes l and l ^ 32 share a
    // column, the four wm waves of a column half hold its four row quarters
    double* const mred = red;          // [8][64]
    double* const sred = red + 512;    // [4][64]
    double* const bvs = red + 768;     // [1]
    int64_t* const bis = (int64_t*)(red + 776);
    double* const ered = red + 1024;   // [4][64]
    mred[g_kq * 64 + g_col] = macc;   // (k quad, candidate): the quads are added in order below, whatever thread held them
    {
      double s0 = ssq + __shfl_xor(ssq, 32, 64);
      const double e0 = (double)(esq + __shfl_xor(esq, 32, 64));
      if (lane < 32) {
        sred[wm * 64 + wn * 32 + lane] = s0;
        ered[wm * 64 + wn * 32 + lane] = e0;
      }
    }
    __syncthreads();
    double val = -INFINITY;
    int64_t gidx = INT64_MAX;
    if (tid < 64) {
      const int64_t cj = blk * I8_BN + tid;
      double adv_ratio = -1.0, adv_var = 0.0, adv_evar = 0.0;
      if (cj < a.M) {
        double m = 0.0;
#pragma unroll
        for (int g = 0; g < 8; ++g) m += mred[g * 64 + tid];
        const double mean = m + a.m.mean_const;
        const double s = (sred[tid] + sred[64 + tid]) + (sred[128 + tid] + sred[192 + tid]);
        const double var = fmax(variance - s, VAR_FLOOR);
        if (a.mean_out) a.mean_out[cj] = mean;
        if (a.var_out) a.var_out[cj] = var;
        // a-posteriori bound of THIS candidate's truncation error on the variance (SweepArgs::rep_ub): the dropped
        // digit pairs leave an error of rms 2^-32.8 S_i S' sqrt(i + 1) on c_i, independent over i, hence
        // d var = -2 sum_i c_i d c_i has rms 2 2^-32.8 S' sqrt(sum_i c_i^2 S_i^2 (i + 1)); rep_scale carries K_SIGMA
        double evar = 0.0, ub = -INFINITY;
        bool viol = false;
        if (a.rep_ub) {
          const double es = (ered[tid] + ered[64 + tid]) + (ered[128 + tid] + ered[192 + tid]);
          evar = a.rep_scale * sqrt(es);
          viol = !(evar <= 1e-5 * var + a.rep_floor);
          if (viol) ub = INFINITY;
          // the adversarial stratum of the canary (round 6): this candidate's share of its tolerance -- where the bound sits
          // closest to the tolerance a failure of the error model would show first; the block's worst unflagged one is
          // recorded below, repair_adv_kernel picks the worst of every 1 / 64 of the sweep for the float64 recomputation
          if (!viol) {
            adv_ratio = evar / (1e-5 * var + a.rep_floor);
            adv_var = var;
            adv_evar = evar;
          }
          // the canary: one candidate in 4096 (offset chosen per sweep) leaves its variance and its bound; it is
          // recomputed in float64 whatever its interval says and the two are compared on the device
          if (a.canary_rec && ((cj + a.canary_off) & (I8_CANARY_PERIOD - 1)) == 0) {
            double* rec = a.canary_rec + 2 * ((cj + a.canary_off) / I8_CANARY_PERIOD);
            rec[0] = var;
            rec[1] = evar;
          }
        }
        if (a.acq_kind >= 0) {
          const double v = acq_tail(a.acq_kind, a.acq_param, mean, var, a.m.noise);
          if (a.acq_out) a.acq_out[cj] = v;
          if (!(v != v)) {
            if (!a.rep_ub) {
              val = v;
              gidx = a.index_base + cj;
            } else if (!viol) {
              // every tail is monotone in the variance: the interval's ends are the tail at var -+ e_var
              const double vlo = acq_tail(a.acq_kind, a.acq_param, mean, fmax(var - evar, VAR_FLOOR), a.m.noise);
              const double vhi = acq_tail(a.acq_kind, a.acq_param, mean, var + evar, a.m.noise);
              ub = fmax(v, fmax(vlo, vhi));
              val = fmin(v, fmin(vlo, vhi));  // the block winner carries the LOWER end
              gidx = a.index_base + cj;
            }
          } else if (a.rep_ub && !viol) {
            ub = -INFINITY;
          }
        }
        if (a.rep_ub) a.rep_ub[cj] = ub;
      }
      if (a.blk_val) {
        wave_argmax(val, gidx);
        if (lane == 0) {
          a.blk_val[blk] = val;
          a.blk_idx[blk] = gidx;
        }
      }
      if (a.adv_rec) {  // (ratio, candidate, its int8 variance, its bound) of the block's worst unflagged candidate; ratio < 0: none
        double r = adv_ratio == adv_ratio ? adv_ratio : -1.0;
        int64_t ri = cj;
        wave_argmax(r, ri);
        const int src = (int)(ri - blk * I8_BN);   // the winner's lane (ties: the lowest index)
        const double wv = __shfl(adv_var, src, 64), we = __shfl(adv_evar, src, 64);
        if (lane == 0) {
          double* rec = a.adv_rec + 4 * blk;
          rec[0] = r;
          rec[1] = __longlong_as_double((long long)ri);
          rec[2] = wv;
          rec[3] = we;
        }
      }
    }
    (void)bis;
    // (the slot lives in the reduction scratch = stage 0: everybody reads it before the barrier that precedes the next
    // block's first DMA; no static LDS -- the launcher asks for the full 160 KiB as dynamic)
    volatile unsigned* const next_blk = (volatile unsigned*)bvs;
    if (a.blk_ctr && tid == 0) *next_blk = atomicAdd(a.blk_ctr, 1u);
    __syncthreads();  // scratch / xqs are rewritten by the next block
    blk = a.blk_ctr ? (int64_t)gridDim.x + (int64_t)(unsigned)__builtin_amdgcn_readfirstlane((int)*next_blk) : blk + gridDim.x;
  }
}

template <int KIND, int NS>
hipError_t launch_sweep_i8_dp(hipStream_t s, const SweepArgs& a, int64_t grid) {
  dim3 g((unsigned)grid), b(512);
  const bool tiles = i8_tiles_fit(NS, a.m.dp);   // the generating steps' training rows staged in LDS (tgp_internal.hpp)
  const size_t shmem = (size_t)i8_lds_bytes(NS, a.m.dp, tiles);
  if (shmem > 160 * 1024) return hipErrorInvalidValue;  // NS = 5 with dp = 32
  if (tiles && !a.i8_xsa) return hipErrorInvalidValue;
  return with_dp<MAX_D>(a.m.dp, [&](auto DP) {
    // > 64 KiB of dynamic LDS is opt-in, per function and per device: set on every launch (a few us)
    hipError_t e = hipFuncSetAttribute((const void*)sweep_i8_kernel<KIND, DP(), NS>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((sweep_i8_kernel<KIND, DP(), NS>), g, b, shmem, s, a);
    return hipGetLastError();
  });
}

}  // namespace

#if TGP_I8_TRACE && TGP_SWEEP_KIND == 3
extern "C" int tgp_dev_i8_trace(unsigned long long* out) {  // development aid: the stamps of the last sweep_i8_kernel<3, ., .>
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_i8_trace), sizeof(g_i8_trace));
}
#endif

hipError_t TGP_CAT(launch_sweep_i8_kind, TGP_SWEEP_KIND)(hipStream_t s, const SweepArgs& a, int64_t grid, int planes) {
  return planes == 5 ? launch_sweep_i8_dp<TGP_SWEEP_KIND, 5>(s, a, grid) : launch_sweep_i8_dp<TGP_SWEEP_KIND, 4>(s, a, grid);
}

}  // namespace tgp
