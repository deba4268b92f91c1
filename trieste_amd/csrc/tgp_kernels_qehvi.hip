// Batch Monte-Carlo expected hypervolume improvement on given joint moments (reference batch_ehvi.__call__,
// acquisition/function/multi_objective.py:366-410, behind BatchReparametrizationSampler.sample), DESIGN.md 4.6:
//
//   L_j      = chol(cov[j,g] + jitter I)                      j = 0..P-1, each q x q
//   y[s,i,j] = mean[j,g,i] + sum_m L_j[i,m] eps[j,m,s]
//   out[g]   = (1/S) sum_s sum_k sum_{J != {}} (-1)^(|J|+1) prod_j max(ub[k,j] - max(lb[k,j], max_{i in J} y[s,i,j]), 0)
//
// With a[i][j] = ub[k,j] - clamp(y[s,i,j], lb[k,j], ub[k,j]) >= 0 the term of J is prod_j min_{i in J} a[i][j].  A point with
// some a[i][j] == 0 makes every subset that holds it contribute +0.0, so the subsets are walked depth first in lexicographic
// order (J = {i1 < i2 < ...}: {0}, {0,1}, {0,1,2}, ..., {0,1,3}, ..., {q-1}) and a subtree is left as soon as its newest point is
// inactive; the walk carries the running minima of the path, P doubles per level, each level in registers of its own (the
// recursion is unrolled by a template to QEHVI_MAX_Q nested loops: nothing is indexed by the depth, nothing goes to scratch).
//
//   workgroup    one batch g, 256 threads = 4 waves
//   phase 1      thread j < P factorises cov[j,g] + jitter I in LDS, with qei_tail_kernel's arithmetic (pivot sqrt, column
//                quotient, fma(-l_ij, l_kj, .) updates): the factor a single model's reparam_samples computes.  A non-positive
//                pivot reports the group (first report wins) and goes on with pivot 1
//   phase 2      per sample chunk of C = qehvi_sample_chunk(P, q) samples: Y[j][i][s] (sample index fastest) into LDS, one
//                thread per entry, y = fma chain from the mean over m = 0..i
//   phase 3      lane = sample (64 consecutive samples of the chunk per wave pass: conflict-free ds_read_b64), wave w = cell
//                slice w: cells w, w + 4, w + 8, ...; the cell's words and bounds are wave-uniform (scalar loads).  The loop
//                counters of the walk are wave-uniform too; only the activity mask differs between lanes, so a wave visits the
//                union of its lanes' active subtrees
//   sums         per (lane, cell) the terms are added in walk order into c; per lane acc += c over its cells (ascending) of
//                its samples (ascending: chunk, then 64-block); the 4 slices of a lane are added in slice order, then the fixed
//                xor butterfly over the 64 lanes, then one division by S.  The order is a function of (P, q, S, K) alone; no
//                atomics touch a value; nothing read depends on G, on g or on another batch
//   LDS          8 (P q C' + P q q + P q) bytes, C' = min(C, S rounded up to 64): at most 32 KiB + 2.3 KiB, 4 workgroups per CU
#include "tgp_dev.hpp"
#include "tgp_internal.hpp"

namespace tgp {

namespace {

constexpr int QEHVI_THREADS = 256, QEHVI_WAVES = QEHVI_THREADS / 64;
static_assert(QEHVI_WAVES == QEHVI_SLICES, "one wave per cell slice");

// the subsets whose smallest new member is >= first, below a path with running minima m (all > 0), at depth D = |J|
template <int P, int D>
__device__ __forceinline__ void qehvi_walk(const double* Ys, int ldi, int ldj, const double (&lb)[P], const double (&ub)[P],
                                           const double (&m)[P], int first, int q, double& c) {
  for (int i = first; i < q; ++i) {
    double n[P];
    bool live = true;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const double y = Ys[j * ldj + i * ldi];
      n[j] = fmin(m[j], ub[j] - fmin(fmax(y, lb[j]), ub[j]));
      live = live && n[j] > 0.0;
    }
    if (live) {
      double t = n[0];
#pragma unroll
      for (int j = 1; j < P; ++j) t *= n[j];
      c = (D & 1) ? c + t : c - t;
      if constexpr (D < QEHVI_MAX_Q) qehvi_walk<P, D + 1>(Ys, ldi, ldj, lb, ub, n, i + 1, q, c);
    }
  }
}

template <int P>
__global__ __launch_bounds__(QEHVI_THREADS) void qehvi_tail_kernel(const double* __restrict__ mean,
                                                                   const double* __restrict__ cov, int64_t gstride, int q,
                                                                   const double* __restrict__ eps, int S, int chunk,
                                                                   double jitter, const double* __restrict__ bounds, int V,
                                                                   const uint32_t* __restrict__ cells, int K,
                                                                   double* __restrict__ out, int* __restrict__ info) {
  extern __shared__ double qehvi_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t g = blockIdx.x;
  const int qq = q * q;
  double* const Ls = qehvi_lds;        // [P][q][q]
  double* const mu = Ls + P * qq;      // [P][q]
  double* const Y = mu + P * q;        // [P][q][chunk]; afterwards [4][64] partial sums

  // phase 1: moments in, P factorisations
  for (int e = tid; e < P * qq; e += QEHVI_THREADS) {
    const int j = e / qq, r = e - j * qq, i = r / q, k = r - i * q;
    Ls[e] = cov[((int64_t)j * gstride + g) * qq + r] + (i == k ? jitter : 0.0);
  }
  for (int e = tid; e < P * q; e += QEHVI_THREADS) {
    const int j = e / q;
    mu[e] = mean[((int64_t)j * gstride + g) * q + (e - j * q)];
  }
  __syncthreads();
  if (tid < P) {
    double* const A = Ls + tid * qq;
    for (int j = 0; j < q; ++j) {
      double dj = A[j * q + j];
      if (!(dj > 0.0)) {
        atomicCAS(info, 0, (int)(g % 2000000000) + 1);
        dj = 1.0;
      }
      const double sd = sqrt(dj);
      A[j * q + j] = sd;
      for (int i = j + 1; i < q; ++i) A[i * q + j] = A[i * q + j] / sd;
      for (int i = j + 1; i < q; ++i) {
        const double nl = -A[i * q + j];
        for (int k = j + 1; k <= i; ++k) A[i * q + k] = fma(nl, A[k * q + j], A[i * q + k]);
      }
    }
  }
  __syncthreads();

  double acc = 0.0;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cs = min(chunk, S - s0);       // samples of this chunk
    const int ld = (cs + 63) & ~63;          // row length in LDS (<= the allocation's)
    // phase 2: the chunk's samples
    for (int e = tid; e < P * q * ld; e += QEHVI_THREADS) {
      const int ji = e / ld, s = e - ji * ld;
      const int j = ji / q, i = ji - j * q;
      double y = 0.0;
      if (s < cs) {
        y = mu[ji];
        const double* const Lr = Ls + j * qq + i * q;
        const double* const ep = eps + (int64_t)j * q * S + s0 + s;
        for (int m2 = 0; m2 <= i; ++m2) y = fma(Lr[m2], ep[(int64_t)m2 * S], y);
      }
      Y[e] = y;
    }
    __syncthreads();
    // phase 3: the cells of slice `wave` for the samples lane, lane + 64, ...
    for (int b = 0; b < ld; b += 64) {
      const bool valid = b + lane < cs;
      const double* const Ys = Y + b + lane;
      for (int k = wave; k < K; k += QEHVI_WAVES) {
        double lb[P], ub[P], top[P];
#pragma unroll
        for (int j = 0; j < P; ++j) {
          const uint32_t w = cells[(size_t)k * P + j];
          lb[j] = fmax(bounds[j * V + (int)(w & 0xffffu)], -1e10);
          ub[j] = bounds[j * V + (int)(w >> 16)];
          top[j] = INFINITY;
        }
        double c = 0.0;
        if (valid) qehvi_walk<P, 1>(Ys, ld, q * ld, lb, ub, top, 0, q, c);
        acc += c;
      }
    }
    __syncthreads();
  }
  Y[tid] = acc;   // [slice][lane]
  __syncthreads();
  if (tid < 64) {
    double sum = Y[tid];
    for (int w = 1; w < QEHVI_WAVES; ++w) sum += Y[w * 64 + tid];
    sum = wave_sum(sum);
    if (tid == 0) out[g] = sum / (double)S;
  }
}

template <int P>
void launch_qehvi_p(hipStream_t s, int V, const double* bounds, const uint32_t* cells, int K, const double* mean,
                    const double* cov, int64_t G, int64_t gstride, int q, const double* eps, int S, double jitter, double* out,
                    int* info) {
  const int chunk = qehvi_sample_chunk(P, q);
  hipLaunchKernelGGL(qehvi_tail_kernel<P>, dim3((unsigned)G), dim3(QEHVI_THREADS), qehvi_lds_bytes(P, q, S), s, mean, cov, gstride,
                     q, eps, S, chunk, jitter, bounds, V, cells, K, out, info);
}

}  // namespace

int qehvi_sample_chunk(int P, int q) {
  const int fit = (QEHVI_SAMPLE_LDS / (8 * P * q)) & ~63;
  return fit < QEHVI_MAX_CHUNK ? fit : QEHVI_MAX_CHUNK;
}

size_t qehvi_lds_bytes(int P, int q, int S) {
  const int chunk = qehvi_sample_chunk(P, q), padded = (int)(((int64_t)S + 63) & ~(int64_t)63);
  const size_t rows = (size_t)P * q * (padded < chunk ? padded : chunk);
  return 8 * ((size_t)P * q * q + (size_t)P * q + (rows > QEHVI_THREADS ? rows : (size_t)QEHVI_THREADS));
}

void launch_qehvi_tail(hipStream_t s, int P, int V, const double* bounds, const uint32_t* cells, int K, const double* mean,
                       const double* cov, int64_t G, int64_t gstride, int q, const double* eps, int S, double jitter,
                       double* out, int* info) {
  if (G <= 0) return;
  if (P == 2) launch_qehvi_p<2>(s, V, bounds, cells, K, mean, cov, G, gstride, q, eps, S, jitter, out, info);
  else if (P == 3) launch_qehvi_p<3>(s, V, bounds, cells, K, mean, cov, G, gstride, q, eps, S, jitter, out, info);
  else launch_qehvi_p<4>(s, V, bounds, cells, K, mean, cov, G, gstride, q, eps, S, jitter, out, info);
}

}  // namespace tgp
