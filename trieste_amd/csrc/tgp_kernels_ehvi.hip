// Expected hypervolume improvement on given moments (reference expected_hv_improvement.__call__,
// acquisition/function/multi_objective.py:188-250), in the table form of DESIGN.md 4.6:
//
//   EHVI(x) = sum_cells prod_j max(g_j(ub_j) - g_j(lb_j), 0),   g_j(t) = E[(t - Y_j)^+] = s_j pdf(z) + (t - m_j) cdf(z),
//   z = (t - m_j) / s_j, t = max(bound, -1e10)
//
// (the reference's 2^P corner sum is the product of the per-objective sums, and Psi(lb) - Psi(ub) + nu is exactly
// g(ub) - g(lb): the nu terms cancel).  Every bound of every cell is one of V_j <= F + 2 distinct values per objective, so a
// workgroup that owns C candidates first fills the table G[j][v][c] = g_j(bound_v; candidate c) in LDS -- P V transcendental
// pairs per candidate, however many cells there are -- and then streams the cells past it as index pairs: per cell and
// objective two LDS reads and a subtraction.
//
//   tile width   C = the largest power of two <= 64 with 8 P V C bytes <= 160 KiB (V = the largest bound count): 64 up to
//                P V = 320, 8 at P = 4, V = 512
//   threads      1024 = C lanes x S = 1024 / C slices; slice s takes cells s, s + S, s + 2 S, ... in that order and the S partial
//                sums of a candidate are added in the order s = 0, 1, ..., S - 1 by one thread: the summation order is a function
//                of (P, V, K) alone, there are no atomics, and a candidate's value depends on nothing but its own moments and the
//                partition (not on M, its index or its neighbours in the tile)
//   LDS          the table (candidate index fastest: a wave whose lanes are candidates reads 512 contiguous bytes per
//                ds_read_b64, conflict-free); the partial sums reuse its first 8 KiB after a barrier
//   cells        packed one 32-bit word per (cell, objective): lower index | upper index << 16.  At C = 64 a wave works on one
//                cell at a time and its words are wave-uniform (scalar loads); the next cell's words are fetched before the
//                current cell's products
#include "tgp_dev.hpp"
#include "tgp_internal.hpp"

namespace tgp {

namespace {

constexpr int EHVI_THREADS = 1024;
constexpr int EHVI_LDS = 160 * 1024;

// g(t) with pdf and cdf evaluated AT the rounded z to a few ulp each (their errors from the rounding of z itself cancel in
// g: d g / d z = s cdf(z)): z^2 is taken exactly (z z = zz + ze), and the argument -z / sqrt(2) of erfc carries its rounding
// residual r, applied to first order (d (erfc(x) / 2) / d x = -sqrt(2) pdf(z)).  Without the two corrections the relative error
// of pdf and cdf grows like z^2 ulp, which at 36 sigma is 1e-13.
__device__ __forceinline__ double ehvi_g(double t, double mu, double sd) {
  t = fmax(t, -1e10);
  const double diff = t - mu;
  const double z = diff / sd;
  const double zz = z * z, ze = fma(z, z, -zz);
  double pdf = 0.3989422804014327 * exp(-0.5 * zz);
  pdf = fma(pdf, -0.5 * ze, pdf);
  const double x = -z * 0.7071067811865476;
  const double r = fma(-z, 0.7071067811865476, -x) + z * 4.833646656726457e-17;  // 1 / sqrt(2) = 0.7071067811865476 - 4.83e-17
  const double cdf = fma(-1.4142135623730951 * pdf, r, 0.5 * erfc(x));
  return fma(diff, cdf, sd * pdf);
}

struct EhviDims {
  int nb[EHVI_MAX_P];
};

template <int P>
__device__ __forceinline__ double ehvi_cells(const double* G, const uint32_t* __restrict__ cells, int K, int V, int logC, int c,
                                             int s, int S) {
  double acc = 0.0;
  if (s >= K) return acc;
  uint32_t w[P], wn[P] = {};
#pragma unroll
  for (int j = 0; j < P; ++j) w[j] = cells[(size_t)s * P + j];
  for (int k = s; k < K; k += S) {
    const int kn = k + S;
    if (kn < K) {
#pragma unroll
      for (int j = 0; j < P; ++j) wn[j] = cells[(size_t)kn * P + j];
    }
    double f = 1.0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const int lo = (int)(w[j] & 0xffffu), hi = (int)(w[j] >> 16);
      const double gl = G[(((j * V) + lo) << logC) + c];
      const double gu = G[(((j * V) + hi) << logC) + c];
      f *= fmax(gu - gl, 0.0);
    }
    acc += f;
#pragma unroll
    for (int j = 0; j < P; ++j) w[j] = wn[j];
  }
  return acc;
}

template <int P>
__global__ __launch_bounds__(EHVI_THREADS) void ehvi_tail_kernel(const double* __restrict__ mean,
                                                                 const double* __restrict__ var, int64_t M,
                                                                 const double* __restrict__ bounds, EhviDims dims, int V,
                                                                 const uint32_t* __restrict__ cells, int K, int logC,
                                                                 double* __restrict__ out) {
  extern __shared__ double G[];  // [P][V][C]; afterwards [S][C] partial sums
  const int tid = (int)threadIdx.x;
  const int C = 1 << logC;
  const int64_t cand0 = (int64_t)blockIdx.x << logC;

  // phase 1: the table.  Entries past an objective's bound count, or past the last candidate, are zero (never read by a
  // validated partition / never written out)
  const int total = (P * V) << logC;
  for (int e = tid; e < total; e += EHVI_THREADS) {
    const int c = e & (C - 1), jv = e >> logC;
    const int j = jv / V, v = jv - j * V;
    const int64_t cand = cand0 + c;
    double g = 0.0;
    if (v < dims.nb[j] && cand < M)
      g = ehvi_g(bounds[j * V + v], mean[(int64_t)j * M + cand], sqrt(var[(int64_t)j * M + cand]));
    G[e] = g;
  }
  __syncthreads();

  // phase 2: the cells
  const int c = tid & (C - 1), S = EHVI_THREADS >> logC;
  const int s = tid >> logC;
  double acc;
  if (logC == 6)  // a wave is one slice: the cell words are wave-uniform
    acc = ehvi_cells<P>(G, cells, K, V, logC, c, __builtin_amdgcn_readfirstlane(s), S);
  else
    acc = ehvi_cells<P>(G, cells, K, V, logC, c, s, S);
  __syncthreads();
  G[tid] = acc;  // [s][c]
  __syncthreads();
  if (tid < C && cand0 + tid < M) {
    double sum = 0.0;
    for (int q = 0; q < S; ++q) sum += G[(q << logC) + tid];
    out[cand0 + tid] = sum;
  }
}

template <int P>
void launch_ehvi_p(hipStream_t s, int V, const int* nb, const double* bounds, const uint32_t* cells, int K, const double* mean,
                   const double* var, int64_t M, double* out) {
  (void)hipFuncSetAttribute((const void*)ehvi_tail_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, EHVI_LDS);
  const int C = ehvi_tile_width(P, V);
  int logC = 0;
  while ((1 << logC) < C) ++logC;
  EhviDims dims{};
  for (int j = 0; j < P; ++j) dims.nb[j] = nb[j];
  const int64_t grid = (M + C - 1) / C;
  hipLaunchKernelGGL(ehvi_tail_kernel<P>, dim3((unsigned)grid), dim3(EHVI_THREADS), ehvi_lds_bytes(P, V), s, mean, var, M, bounds,
                     dims, V, cells, K, logC, out);
}

}  // namespace

int ehvi_tile_width(int P, int V) {
  int C = 64;
  while (C > 1 && (size_t)8 * P * V * C > (size_t)EHVI_LDS) C >>= 1;
  return C;
}

size_t ehvi_lds_bytes(int P, int V) {
  const size_t table = (size_t)8 * P * V * ehvi_tile_width(P, V);
  return table > (size_t)8 * EHVI_THREADS ? table : (size_t)8 * EHVI_THREADS;
}

void launch_ehvi_tail(hipStream_t s, int P, int V, const int* nb, const double* bounds, const uint32_t* cells, int K,
                      const double* mean, const double* var, int64_t M, double* out) {
  if (M <= 0) return;
  if (P == 2) launch_ehvi_p<2>(s, V, nb, bounds, cells, K, mean, var, M, out);
  else if (P == 3) launch_ehvi_p<3>(s, V, nb, bounds, cells, K, mean, var, M, out);
  else launch_ehvi_p<4>(s, V, nb, bounds, cells, K, mean, var, M, out);
}

}  // namespace tgp
