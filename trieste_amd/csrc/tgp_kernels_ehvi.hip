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
struct EhviEval {
  double g, cdf, pdf;
};
__device__ __forceinline__ EhviEval ehvi_eval(double t, double mu, double sd) {
  t = fmax(t, -1e10);
  const double diff = t - mu;
  const double z = diff / sd;
  const double zz = z * z, ze = fma(z, z, -zz);
  double pdf = 0.3989422804014327 * exp(-0.5 * zz);
  pdf = fma(pdf, -0.5 * ze, pdf);
  const double x = -z * 0.7071067811865476;
  const double r = fma(-z, 0.7071067811865476, -x) + z * 4.833646656726457e-17;  // 1 / sqrt(2) = 0.7071067811865476 - 4.83e-17
  const double cdf = fma(-1.4142135623730951 * pdf, r, 0.5 * erfc(x));
  return {fma(diff, cdf, sd * pdf), cdf, pdf};
}
__device__ __forceinline__ double ehvi_g(double t, double mu, double sd) { return ehvi_eval(t, mu, sd).g; }

// The same evaluation for the derivatives d g / d m = -cdf(z), d g / d s = pdf(z), where the rounding of z does NOT cancel: z is
// rounded three times (the difference t - mu, the square root, the quotient), each an ulp of z and so z^2 ulp of pdf and of a tail
// cdf.  The three residuals are exact in float64 (two-sum, fma), and pdf and cdf are moved by them to first order
// (cdf' = pdf, pdf' = -z pdf).  g is returned as ehvi_eval computes it.
__device__ __forceinline__ EhviEval ehvi_eval_grad(double t, double mu, double var) {
  const double sd = sqrt(var);
  EhviEval e = ehvi_eval(t, mu, sd);
  t = fmax(t, -1e10);
  const double diff = t - mu, bb = diff - t;
  const double dr = (t - (diff - bb)) + (-mu - bb);          // t - mu = diff + dr
  const double z = diff / sd;
  const double sr = fma(-sd, sd, var) / (2.0 * sd);          // sqrt(var) = sd + sr
  const double dz = (dr + fma(-z, sd, diff) - z * sr) / sd;  // (t - mu) / sqrt(var) = z + dz
  if (e.pdf > 0.0) {   // (where pdf has flushed there is nothing to move: cdf and pdf stay exactly 0 at a clipped bound)
    e.cdf = fma(e.pdf, dz, e.cdf);
    e.pdf = fma(-z * dz, e.pdf, e.pdf);
  }
  return e;
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

// what both launchers derive from the tile width C (a power of two): its logarithm, the grid, the bound counts by value
struct EhviTile {
  int logC = 0;
  EhviDims dims{};
  int64_t grid = 0;
};
static EhviTile ehvi_tile(int P, int C, const int* nb, int64_t M) {
  EhviTile t;
  while ((1 << t.logC) < C) ++t.logC;
  for (int j = 0; j < P; ++j) t.dims.nb[j] = nb[j];
  t.grid = (M + C - 1) / C;
  return t;
}

template <int P>
void launch_ehvi_p(hipStream_t s, int V, const int* nb, const double* bounds, const uint32_t* cells, int K, const double* mean,
                   const double* var, int64_t M, double* out) {
  (void)hipFuncSetAttribute((const void*)ehvi_tail_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, EHVI_LDS);
  const int C = ehvi_tile_width(P, V);
  const EhviTile t = ehvi_tile(P, C, nb, M);
  hipLaunchKernelGGL(ehvi_tail_kernel<P>, dim3((unsigned)t.grid), dim3(EHVI_THREADS), ehvi_lds_bytes(P, V), s, mean, var, M, bounds,
                     t.dims, V, cells, K, t.logC, out);
}

// ---- the value with the adjoints of the moments: what an L-BFGS-B iteration over EHVI asks for -------------------
//   d EHVI / d m_j = -sum_cells (prod_{i != j} D_i) (cdf(z_u) - cdf(z_l)),   d EHVI / d s_j = sum_cells (prod_{i != j} D_i) (pdf(z_u) - pdf(z_l))
// (d g / d m = -cdf(z), d g / d s = pdf(z): the z terms cancel because pdf' = -z pdf), D_j = max(g_j(u_j) - g_j(l_j), 0); an
// objective of a cell whose factor the max clipped contributes no derivative.  d / d v_j = (d / d s_j) / (2 s_j).
// Three tables g, cdf, pdf [P][V][C] (24 P V C bytes, candidate index fastest) from the SAME corrected evaluation as the value
// kernel's; the call serves tens to 2048 points, so the tile is narrow (C <= 8: 2048 points are 256 workgroups) and a
// function of (P, V) alone.  Per thread 1 + 2 P accumulators over its slice of the cells; the S partial sums of each quantity are
// added in slice order by one thread, through the LDS reused after a barrier.  No atomics.
#ifndef TGP_EHVI_GRAD_CMAX
#define TGP_EHVI_GRAD_CMAX 8   // (build-time, for measuring: 4, 8 and 16 were compared; the bindings state 8)
#endif
constexpr int EHVI_GRAD_CMAX = TGP_EHVI_GRAD_CMAX;

template <int P>
__global__ __launch_bounds__(EHVI_THREADS) void ehvi_grad_tail_kernel(const double* __restrict__ mean,
                                                                      const double* __restrict__ var, int64_t M,
                                                                      const double* __restrict__ bounds, EhviDims dims, int V,
                                                                      const uint32_t* __restrict__ cells, int K, int logC,
                                                                      int zero_clipped, double* __restrict__ val,
                                                                      double* __restrict__ gmean, double* __restrict__ gvar) {
  extern __shared__ double G[];  // g, cdf, pdf: [P][V][C] each; afterwards [1 + 2 P][S][C] partial sums
  const int tid = (int)threadIdx.x;
  const int C = 1 << logC;
  const int64_t cand0 = (int64_t)blockIdx.x << logC;
  const int total = (P * V) << logC;
  double* const Tc = G + total;
  double* const Tp = Tc + total;

  // phase 1: the tables (entries past an objective's bound count or past the last candidate are zero)
  for (int e = tid; e < total; e += EHVI_THREADS) {
    const int c = e & (C - 1), jv = e >> logC;
    const int j = jv / V, v = jv - j * V;
    const int64_t cand = cand0 + c;
    EhviEval t{0.0, 0.0, 0.0};
    if (v < dims.nb[j] && cand < M)
      t = ehvi_eval_grad(bounds[j * V + v], mean[(int64_t)j * M + cand], var[(int64_t)j * M + cand]);
    G[e] = t.g;
    Tc[e] = t.cdf;
    Tp[e] = t.pdf;
  }
  __syncthreads();

  // phase 2: the cells of slice s for candidate lane c
  const int c = tid & (C - 1), S = EHVI_THREADS >> logC, s = tid >> logC;
  double acc = 0.0, am[P], as[P];
#pragma unroll
  for (int j = 0; j < P; ++j) am[j] = as[j] = 0.0;
  if (s < K) {
    uint32_t w[P], wn[P] = {};
#pragma unroll
    for (int j = 0; j < P; ++j) w[j] = cells[(size_t)s * P + j];
    for (int k = s; k < K; k += S) {
      const int kn = k + S;
      if (kn < K) {
#pragma unroll
        for (int j = 0; j < P; ++j) wn[j] = cells[(size_t)kn * P + j];
      }
      double del[P], dc[P], dp[P];
#pragma unroll
      for (int j = 0; j < P; ++j) {
        const int il = (((j * V) + (int)(w[j] & 0xffffu)) << logC) + c;
        const int iu = (((j * V) + (int)(w[j] >> 16)) << logC) + c;
        const double d = G[iu] - G[il];
        const bool pos = d > 0.0;   // (the derivative of the function as computed: a clipped factor has none)
        del[j] = pos ? d : 0.0;
        dc[j] = pos ? Tc[iu] - Tc[il] : 0.0;
        dp[j] = pos ? Tp[iu] - Tp[il] : 0.0;
      }
      double f = 1.0;
#pragma unroll
      for (int j = 0; j < P; ++j) f *= del[j];
      acc += f;
      double loo[P];   // the products that leave one objective out, without a division
      if constexpr (P == 2) {
        loo[0] = del[1];
        loo[1] = del[0];
      } else if constexpr (P == 3) {
        loo[0] = del[1] * del[2];
        loo[1] = del[0] * del[2];
        loo[2] = del[0] * del[1];
      } else {
        const double a = del[0] * del[1], b = del[2] * del[3];
        loo[0] = del[1] * b;
        loo[1] = del[0] * b;
        loo[2] = a * del[3];
        loo[3] = a * del[2];
      }
#pragma unroll
      for (int j = 0; j < P; ++j) {
        am[j] = fma(loo[j], dc[j], am[j]);
        as[j] = fma(loo[j], dp[j], as[j]);
      }
#pragma unroll
      for (int j = 0; j < P; ++j) w[j] = wn[j];
    }
  }
  __syncthreads();
  G[tid] = acc;  // [quantity][s][c]
#pragma unroll
  for (int j = 0; j < P; ++j) {
    G[(1 + j) * EHVI_THREADS + tid] = am[j];
    G[(1 + P + j) * EHVI_THREADS + tid] = as[j];
  }
  __syncthreads();
  if (tid < ((1 + 2 * P) << logC)) {
    const int q = tid >> logC, cc = tid & (C - 1);
    const int64_t cand = cand0 + cc;
    if (cand < M) {
      const double* const R = G + q * EHVI_THREADS + cc;
      double sum = 0.0;
      for (int t = 0; t < S; ++t) sum += R[t << logC];
      if (q == 0) {
        val[cand] = sum;
      } else if (q <= P) {
        gmean[(int64_t)(q - 1) * M + cand] = 0.0 - sum;
      } else {
        const double v = var[(int64_t)(q - 1 - P) * M + cand];
        // (zero_clipped: a variance at the posterior's floor was clipped there, and the clip's adjoint is zero)
        gvar[(int64_t)(q - 1 - P) * M + cand] = zero_clipped && !(v > VAR_FLOOR) ? 0.0 : sum / (2.0 * sqrt(v));
      }
    }
  }
}

template <int P>
void launch_ehvi_grad_p(hipStream_t s, int V, const int* nb, const double* bounds, const uint32_t* cells, int K,
                        const double* mean, const double* var, int64_t M, int zero_clipped, double* val, double* gmean,
                        double* gvar) {
  (void)hipFuncSetAttribute((const void*)ehvi_grad_tail_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, EHVI_LDS);
  const int C = ehvi_grad_tile_width(P, V);
  const EhviTile t = ehvi_tile(P, C, nb, M);
  hipLaunchKernelGGL(ehvi_grad_tail_kernel<P>, dim3((unsigned)t.grid), dim3(EHVI_THREADS), ehvi_grad_lds_bytes(P, V), s, mean, var, M,
                     bounds, t.dims, V, cells, K, t.logC, zero_clipped, val, gmean, gvar);
}

// out [n] = ((part_0 + part_1) + part_2) + part_3 over the first P of the arrays part_j = parts + j n: one fixed association
__global__ void ehvi_sum_parts_kernel(const double* __restrict__ parts, int P, int64_t n, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double sum = parts[i];
  for (int j = 1; j < P; ++j) sum += parts[(int64_t)j * n + i];
  out[i] = sum;
}

}  // namespace

int ehvi_grad_tile_width(int P, int V) {
  int C = EHVI_GRAD_CMAX;
  while (C > 1 && (size_t)24 * P * V * C > (size_t)EHVI_LDS) C >>= 1;
  return C;
}

size_t ehvi_grad_lds_bytes(int P, int V) {
  const size_t table = (size_t)24 * P * V * ehvi_grad_tile_width(P, V), sums = (size_t)8 * EHVI_THREADS * (1 + 2 * P);
  return table > sums ? table : sums;
}

void launch_ehvi_grad_tail(hipStream_t s, int P, int V, const int* nb, const double* bounds, const uint32_t* cells, int K,
                           const double* mean, const double* var, int64_t M, int zero_clipped, double* val, double* gmean,
                           double* gvar) {
  if (M <= 0) return;
  with_objectives(P, [&](auto PC) {
    launch_ehvi_grad_p<decltype(PC)::value>(s, V, nb, bounds, cells, K, mean, var, M, zero_clipped, val, gmean, gvar);
  });
}

void launch_ehvi_sum_parts(hipStream_t s, const double* parts, int P, int64_t n, double* out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ehvi_sum_parts_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, parts, P, n, out);
}

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
  with_objectives(P, [&](auto PC) { launch_ehvi_p<decltype(PC)::value>(s, V, nb, bounds, cells, K, mean, var, M, out); });
}

}  // namespace tgp
