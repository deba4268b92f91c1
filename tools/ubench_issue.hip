// Development aid: single-wave issue cost / latency of the instructions of the factor leaf's pivot chain (gfx950), and the
// float32 instructions of the packed pre-screen's loop at one and at eight waves per SIMD (profiles/r31_prescreen_issue.txt).
//   hipcc -O3 --offload-arch=gfx950 tools/ubench_issue.hip -o tools/ubench_issue
#include <hip/hip_runtime.h>
#include <cstdio>
__device__ unsigned long long g_t[32];
__device__ double g_sink[64];
#define REP16(X) X X X X X X X X X X X X X X X X
template <int MODE>
__global__ void k(double x0) {
  double a[16];
  for (int i = 0; i < 16; ++i) a[i] = x0 + i + threadIdx.x;
  double y = x0 * 0.5, z = x0 + 2.0;
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)");
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll 1
  for (int it = 0; it < 16; ++it) {
    if (MODE == 0) {  // 16 independent plain fmac
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_fmac_f64_e32 %0, %1, %2" : "+v"(a[i]) : "v"(y), "v"(z));
    } else if (MODE == 1) {  // 16 independent dpp fmac
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(a[i]) : "v"(y), "v"(z));
    } else if (MODE == 2) {  // dependent plain fmac chain
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_fmac_f64_e32 %0, %1, %2" : "+v"(a[0]) : "v"(y), "v"(z));
    } else if (MODE == 3) {  // dependent mov_dpp chain (with the 2 wait states)
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("s_nop 1\n\tv_mov_b64_dpp %0, %0 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(a[0]));
    } else if (MODE == 4) {  // dependent rsq chain
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_rsq_f64_e32 %0, %0" : "+v"(a[0]));
    } else if (MODE == 5) {  // dependent mul chain
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(a[0]) : "v"(y));
    } else if (MODE == 6) {  // 16 independent mov_dpp (no nop)
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_mov_b64_dpp %0, %1 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "=v"(a[i]) : "v"(y));
    } else if (MODE == 7) {  // independent readlane pairs
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_readlane_b32 s20, %0, 3\n\tv_readlane_b32 s21, %1, 3" :: "v"(__double2loint(a[i])), "v"(__double2hiint(a[i])) : "s20", "s21");
    } else if (MODE == 8) {  // independent 32-bit fma
#pragma unroll
      for (int i = 0; i < 16; ++i) { float fa = (float)a[i]; asm volatile("v_fmac_f32_e32 %0, %1, %2" : "+v"(fa) : "v"((float)y), "v"((float)z)); a[i] = fa; }
    } else if (MODE == 9) {  // dependent dpp fmac chain through the DPP operand: fmac -> (nop) -> fmac reading it via dpp
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, -%0, %1 row_newbcast:3 row_mask:0xf bank_mask:0xf" : "+v"(a[0]) : "v"(z));
    } else if (MODE == 10) {  // round 6: the other instructions of the int8 sweep's K* generation, 16 independent each
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_rsq_f64_e32 %0, %1" : "=v"(a[i]) : "v"(y));
    } else if (MODE == 11) {
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_rndne_f64_e32 %0, %1" : "=v"(a[i]) : "v"(y));
    } else if (MODE == 12) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { int r; asm volatile("v_cvt_i32_f64_e32 %0, %1" : "=v"(r) : "v"(a[i])); a[i] = __hiloint2double(r, r); }
    } else if (MODE == 13) {
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_ldexp_f64 %0, %1, %2" : "=v"(a[i]) : "v"(y), "v"(3));
    } else if (MODE == 14) {
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_max_f64 %0, %1, %2" : "=v"(a[i]) : "v"(y), "v"(z));
    } else if (MODE == 15) {
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_add_f64 %0, %1, %2" : "=v"(a[i]) : "v"(y), "v"(z));
    } else if (MODE == 16) {
#pragma unroll
      for (int i = 0; i < 16; ++i) asm volatile("v_cvt_f64_i32_e32 %0, %1" : "=v"(a[i]) : "v"(it));
    } else if (MODE == 17) {
#pragma unroll
      for (int i = 0; i < 16; ++i) { int r; asm volatile("v_perm_b32 %0, %1, %2, %3" : "=v"(r) : "v"(it), "v"(i), "v"(0x05010400)); a[i] = __hiloint2double(r, r); }
    } else if (MODE == 18) {  // 64-bit integer shift-add (the digits of the fold)
#pragma unroll
      for (int i = 0; i < 16; ++i) { long long r; asm volatile("v_lshl_add_u64 %0, %1, 8, %2" : "=v"(r) : "v"((long long)it), "v"((long long)i)); a[i] = __longlong_as_double(r); }
    }
  }
  asm volatile("s_nop 0" ::: "memory");
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  double s = 0;
  for (int i = 0; i < 16; ++i) s += a[i];
  g_sink[threadIdx.x] = s;
  if (threadIdx.x == 0) g_t[MODE] = t1 - t0;
}
// The float32 instructions of the packed pre-screen's g loop (prune_prescreen_kernel<KIND, DP, 2>), each line at one wave and
// at eight waves per SIMD (two workgroups of 1024 threads per compute unit on every compute unit; wave 0 of every workgroup
// reports, the mean is printed per instruction and, at eight waves, per instruction and SIMD = ticks / 8).  The streams are
// timed, not checked: where the compiler would put a wait state the asm holds the s_nop the compiled loop has.
typedef float f2 __attribute__((ext_vector_type(2)));
__device__ unsigned long long g_tf[2][32];
__device__ float g_sinkf[1024];
#define PKADD(d, x, s) "v_pk_add_f32 " d ", " x ", " s " op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
#define PKSQ(q, t) "v_pk_fma_f32 " q ", " t ", " t ", " q "\n\t"
// four rows of the distance: 8 VALU, with the scalar instruction the compiled loop has between an add and its square, or without
#define QUAD_S PKADD("%4", "%8", "%9") "s_nop 0\n\t" PKSQ("%0", "%4") PKADD("%5", "%8", "%9") "s_mov_b32 s20, s21\n\t" PKSQ("%1", "%5") \
               PKADD("%6", "%8", "%9") "s_nop 0\n\t" PKSQ("%2", "%6") PKADD("%7", "%8", "%9") "s_mov_b32 s20, s21\n\t" PKSQ("%3", "%7")
#define QUAD_N PKADD("%4", "%8", "%9") PKADD("%5", "%8", "%9") PKADD("%6", "%8", "%9") PKADD("%7", "%8", "%9") \
               PKSQ("%0", "%4") PKSQ("%1", "%5") PKSQ("%2", "%6") PKSQ("%3", "%7")
#define TRANS(OP, FILL) asm volatile(OP " %0, %3\n\t" FILL "v_add_f32 %1, %0, %0" : "=&v"(tr), "=v"(fo[i]), "=&v"(fl) : "v"(y.x), "v"(z.x))
#define FILL1 "v_add_f32 %2, %3, %4\n\t"
constexpr int NF = 17;
template <int MODE>
__global__ __launch_bounds__(1024, 8) void kf(float x0, unsigned long long srow, int slot) {
  f2 a[16];
  for (int i = 0; i < 16; ++i) a[i] = f2{x0 + i + threadIdx.x, x0 - i};
  f2 y = {x0 * 0.5f, x0 * 0.25f}, z = {x0 + 2.0f, x0 + 3.0f}, w = {x0 - 1.0f, x0 - 2.0f};
  float tr, fl, fo[16];
  for (int i = 0; i < 16; ++i) fo[i] = x0;
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)");
  __syncthreads();
  unsigned long long t0 = __builtin_amdgcn_s_memtime();
  asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll 1
  for (int it = 0; it < 16; ++it) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      if (MODE == 0) asm volatile("v_pk_fma_f32 %0, %1, %2, %3" : "=v"(a[i]) : "v"(y), "v"(z), "v"(w));            // three distinct pairs
      else if (MODE == 1) asm volatile("v_pk_fma_f32 %0, %1, %2, %0" : "+v"(a[0]) : "v"(y), "v"(z));               // ... dependent
      else if (MODE == 2) asm volatile("v_pk_fma_f32 %0, %1, %1, %0" : "+v"(a[i]) : "v"(y));                       // the loop's (t, t, q)
      else if (MODE == 3) asm volatile("v_pk_fma_f32 %0, %1, %1, %0" : "+v"(a[0]) : "v"(y));                       // ... dependent
      else if (MODE == 4) asm volatile(PKADD("%0", "%1", "%2") : "=v"(a[i]) : "v"(y), "s"(srow));                  // SGPR-pair row coordinate
      else if (MODE == 5) asm volatile("v_fma_f32 %0, %1, %2, %3" : "=v"(fo[i]) : "v"(y.x), "v"(z.x), "v"(w.x));
      else if (MODE == 6) asm volatile("v_pk_mul_f32 %0, %1, %2" : "=v"(a[i]) : "v"(y), "v"(z));
      else if (MODE == 7) TRANS("v_sqrt_f32", "s_nop 0\n\t");                                                        // used at once
      else if (MODE == 8) TRANS("v_sqrt_f32", FILL1);                                                                // 1, 2, 4 independent between
      else if (MODE == 9) TRANS("v_sqrt_f32", FILL1 FILL1);
      else if (MODE == 10) TRANS("v_sqrt_f32", FILL1 FILL1 FILL1 FILL1);
      else if (MODE == 11) TRANS("v_exp_f32", "s_nop 0\n\t");
      else if (MODE == 12) TRANS("v_exp_f32", FILL1);
      else if (MODE == 13) TRANS("v_exp_f32", FILL1 FILL1);
      else if (MODE == 14) TRANS("v_exp_f32", FILL1 FILL1 FILL1 FILL1);
      else if (MODE == 15 && i < 15)   // 15 x 8 = 120 VALU with 60 scalar instructions interleaved
        asm volatile(QUAD_S : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "=&v"(a[4]), "=&v"(a[5]), "=&v"(a[6]), "=&v"(a[7]) : "v"(y), "s"(srow) : "s20");
      else if (MODE == 16 && i < 15)   // the same 120 VALU, no scalar instruction, no square behind its own add
        asm volatile(QUAD_N : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "=&v"(a[4]), "=&v"(a[5]), "=&v"(a[6]), "=&v"(a[7]) : "v"(y), "s"(srow));
    }
  }
  asm volatile("s_nop 0" ::: "memory");
  unsigned long long t1 = __builtin_amdgcn_s_memtime();
  float s = 0;
  for (int i = 0; i < 16; ++i) s += a[i].x + a[i].y + fo[i];
  g_sinkf[threadIdx.x] = s;
  if (threadIdx.x == 0) atomicAdd(&g_tf[slot][MODE], t1 - t0);
}
template <int MODE>
void run_f32() {
  int dev = 0, cus = 0;
  hipGetDevice(&dev);
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  kf<MODE><<<1, 64>>>(1.5f, 0x3fc000003fc00000ull, 0);
  kf<MODE><<<2 * cus, 1024>>>(1.5f, 0x3fc000003fc00000ull, 1);
  if constexpr (MODE + 1 < NF) run_f32<MODE + 1>();
}
void report_f32() {
  int dev = 0, cus = 0;
  hipGetDevice(&dev);
  hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  hipDeviceSynchronize();
  unsigned long long t[2][32];
  hipMemcpyFromSymbol(t, HIP_SYMBOL(g_tf), sizeof(t));
  const char* names[NF] = {"independent v_pk_fma_f32, three register pairs", "dependent v_pk_fma_f32, three register pairs",
                           "independent v_pk_fma_f32 (t, t, q)", "dependent v_pk_fma_f32 (t, t, q)",
                           "independent v_pk_add_f32, SGPR pair, op_sel_hi neg", "independent v_fma_f32", "independent v_pk_mul_f32",
                           "v_sqrt_f32, s_nop, use (2 VALU)", "v_sqrt_f32, 1 independent, use (3 VALU)", "v_sqrt_f32, 2 independent, use (4 VALU)",
                           "v_sqrt_f32, 4 independent, use (6 VALU)", "v_exp_f32, s_nop, use (2 VALU)", "v_exp_f32, 1 independent, use (3 VALU)",
                           "v_exp_f32, 2 independent, use (4 VALU)", "v_exp_f32, 4 independent, use (6 VALU)",
                           "distance stream, 120 VALU + 60 s_nop / s_mov_b32", "distance stream, 120 VALU, no scalar, no adjacent use"};
  const int valu[NF] = {16, 16, 16, 16, 16, 16, 16, 32, 48, 64, 96, 32, 48, 64, 96, 120, 120};
  for (int m = 0; m < NF; ++m)
    printf("%-52s %6.2f ticks per VALU instruction at 1 wave; %6.2f per VALU instruction and SIMD at 8 waves per SIMD\n", names[m],
           t[0][m] / (16.0 * valu[m]), t[1][m] / (2.0 * cus) / (16.0 * valu[m]) / 8.0);
}
int main() {
  k<0><<<1, 64>>>(1.5); k<1><<<1, 64>>>(1.5); k<2><<<1, 64>>>(1.5); k<3><<<1, 64>>>(1.5); k<4><<<1, 64>>>(1.5);
  k<5><<<1, 64>>>(1.5); k<6><<<1, 64>>>(1.5); k<7><<<1, 64>>>(1.5); k<8><<<1, 64>>>(1.5); k<9><<<1, 64>>>(1.5);
  k<10><<<1, 64>>>(1.5); k<11><<<1, 64>>>(1.5); k<12><<<1, 64>>>(1.5); k<13><<<1, 64>>>(1.5); k<14><<<1, 64>>>(1.5);
  k<15><<<1, 64>>>(1.5); k<16><<<1, 64>>>(1.5); k<17><<<1, 64>>>(1.5); k<18><<<1, 64>>>(1.5);
  hipDeviceSynchronize();
  unsigned long long t[32];
  hipMemcpyFromSymbol(t, HIP_SYMBOL(g_t), sizeof(t));
  const char* names[] = {"independent v_fmac_f64", "independent v_fmac_f64_dpp", "dependent v_fmac_f64", "dependent nop+v_mov_b64_dpp",
                         "dependent v_rsq_f64", "dependent v_mul_f64", "independent v_mov_b64_dpp", "independent readlane pair",
                         "independent v_fmac_f32", "dependent nop+v_fmac_f64_dpp (via dpp src)", "independent v_rsq_f64", "independent v_rndne_f64",
                         "independent v_cvt_i32_f64", "independent v_ldexp_f64", "independent v_max_f64", "independent v_add_f64",
                         "independent v_cvt_f64_i32", "independent v_perm_b32", "independent v_lshl_add_u64"};
  for (int m = 0; m < 19; ++m) printf("%-44s %.1f ticks per instruction (256 instructions, s_memtime)\n", names[m], t[m] / 256.0);
  run_f32<0>();
  report_f32();
  return 0;
}
