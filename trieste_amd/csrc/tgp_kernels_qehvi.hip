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
#include "tgp_tail_dev.hpp"

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

// phase 1: the moments of batch g into LDS (Ls [P][q][q] = cov + jitter I, mu [P][q]), then thread j < P factorises matrix j
// in place.  A non-positive pivot reports the group (first report wins) and goes on with pivot 1.  Ends in a barrier.
template <int P>
__device__ __forceinline__ void qehvi_load_and_factor(const double* __restrict__ mean, const double* __restrict__ cov,
                                                      int64_t gstride, int64_t g, int q, double jitter, double* Ls, double* mu,
                                                      int* info, int tid) {
  const int qq = q * q;
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
}

// phase 2: the cs samples from s0 on into Y [P][q][ld] (sample index fastest, the pad zero), one thread per entry: the fma
// chain from the mean over m = 0..i.  The caller synchronises.
template <int P>
__device__ __forceinline__ void qehvi_fill_samples(const double* Ls, const double* mu, const double* __restrict__ eps, int q,
                                                   int S, int s0, int cs, int ld, double* Y, int tid) {
  const int qq = q * q;
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
}

// cell k's bounds (wave-uniform: scalar loads; a lower bound below -1e10 is taken as -1e10) and the walk's starting minima
template <int P>
__device__ __forceinline__ void qehvi_cell_bounds(const double* __restrict__ bounds, int V, const uint32_t* __restrict__ cells,
                                                  int k, double (&lb)[P], double (&ub)[P], double (&top)[P]) {
#pragma unroll
  for (int j = 0; j < P; ++j) {
    const uint32_t w = cells[(size_t)k * P + j];
    lb[j] = fmax(bounds[j * V + (int)(w & 0xffffu)], -1e10);
    ub[j] = bounds[j * V + (int)(w >> 16)];
    top[j] = INFINITY;
  }
}

// the value from every thread's acc through Y [slice][lane] (one barrier): the four slices of a lane in slice order, the fixed
// butterfly over the 64 lanes, one division by S
__device__ __forceinline__ void qehvi_reduce_value(double* Y, double acc, int tid, int S, double* out) {
  Y[tid] = acc;
  __syncthreads();
  if (tid < 64) {
    double sum = Y[tid];
    for (int w = 1; w < QEHVI_WAVES; ++w) sum += Y[w * 64 + tid];
    sum = wave_sum(sum);
    if (tid == 0) *out = sum / (double)S;
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

  qehvi_load_and_factor<P>(mean, cov, gstride, g, q, jitter, Ls, mu, info, tid);

  double acc = 0.0;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cs = min(chunk, S - s0);       // samples of this chunk
    const int ld = (cs + 63) & ~63;          // row length in LDS (<= the allocation's)
    qehvi_fill_samples<P>(Ls, mu, eps, q, S, s0, cs, ld, Y, tid);
    __syncthreads();
    // phase 3: the cells of slice `wave` for the samples lane, lane + 64, ...
    for (int b = 0; b < ld; b += 64) {
      const bool valid = b + lane < cs;
      const double* const Ys = Y + b + lane;
      for (int k = wave; k < K; k += QEHVI_WAVES) {
        double lb[P], ub[P], top[P];
        qehvi_cell_bounds<P>(bounds, V, cells, k, lb, ub, top);
        double c = 0.0;
        if (valid) qehvi_walk<P, 1>(Ys, ld, q * ld, lb, ub, top, 0, q, c);
        acc += c;
      }
    }
    __syncthreads();
  }
  qehvi_reduce_value(Y, acc, tid, S, out + g);
}

// ---------------------------------------------------------------------------------------------
// The same value with its adjoints w.r.t. the joint moments ("the gradient"): gmean [P][gstride][q],
// gcov [P][gstride][q][q] symmetric, objective-major like the inputs -- what tgp_joint_vjp takes per objective.
//
//   term of (cell k, subset J)   sign(J) prod_j n_J[j],  n_J[j] = min_{i in J} a[i][j]
//   d term / d y[s,i*,j]         -sign(J) prod_{j' != j} n_J[j'], where i* is the point of J that attains the minimum in objective
//                                j (strict comparison: the first point in walk order wins a tie) and only where
//                                lb < y[s,i*,j] < ub strictly (a clamped sample contributes nothing)
//   ybar[s,i,j]                  sum over cells and subsets;  gmean[j,i] = (1/S) sum_s ybar;  Lbar_j = (1/S) tril(sum_s ybar eps^T)
//   gcov[j]                      L_j^-T sym(Phi(L_j^T Lbar_j)) L_j^-1 (qei_grad_tail_kernel's form); zero_clipped: a diagonal
//                                entry of cov at VAR_FLOOR gets zero
//
// Phases 1 and 2, the cell bounds and the value's sums are the helpers that qehvi_tail_kernel calls: a lane adds its
// (64-block, cell) sums in the same order whatever the chunk, so the smaller chunk here (qehvi_grad_sample_chunk) leaves the value's bits alone.
//   phase 3      the walk also carries, per level and objective, WHICH level of the path owns the running minimum (0: nobody --
//                the owner's sample sits at or below the cell's lower bound).  Every level has P accumulators in registers (the
//                template recursion's frames: "the adjoint of the point at this level"); a live term adds its P partial
//                products into the owning levels through a compile-time-unrolled select, and a level flushes its accumulators
//                into THIS WAVE's Ybar[j][i][lane] when its loop leaves point i (i is wave-uniform, the column lane-private)
//   phase 4a     per chunk: ybar = ((Ybar_0 + Ybar_1) + Ybar_2) + Ybar_3 (slice order); wave w takes the entries w, w + 4, ... of
//                (gmean[j][i], Lbar_j[i][m <= i]): lane = sample, the fixed butterfly per 64-block, lane 0 adds the blocks
//                (ascending) and chunks (ascending) into the entry's LDS slot
//   phase 4b     wave j: the Cholesky adjoint of objective j, lane c = column c / row c; then coalesced stores
// No atomics touch a value, every order above is a function of (P, q, S, K) alone, nothing read depends on G or g.
//   LDS          8 (5 P q C' + P (2 q q + q + q (q + 3) / 2)) bytes, C' = min(C, S rounded up to 64), C = qehvi_grad_sample_chunk(P, q):
//                the samples and four adjoint copies, the factors, the means, the work matrices, the sums; up to 160 KiB, so
//                one workgroup per CU (a call has at most 2048 / q groups)
template <int P>
struct QehviAdj {
  double g[QEHVI_MAX_Q][P];
};

template <int P, int D>
__device__ __forceinline__ void qehvi_walk_grad(const double* Ys, double* Yb, int ldi, int ldj, const double (&lb)[P],
                                                const double (&ub)[P], const double (&m)[P], const int (&own)[P], int first,
                                                int q, double& c, QehviAdj<P>& A) {
  for (int i = first; i < q; ++i) {
    double n[P];
    int o[P];
    bool live = true;
#pragma unroll
    for (int j = 0; j < P; ++j) {
      const double y = Ys[j * ldj + i * ldi];
      const double a = ub[j] - fmin(fmax(y, lb[j]), ub[j]);
      n[j] = fmin(m[j], a);
      o[j] = a < m[j] ? (y > lb[j] ? D : 0) : own[j];
      live = live && n[j] > 0.0;
    }
    if (live) {
      double t = n[0];
#pragma unroll
      for (int j = 1; j < P; ++j) t *= n[j];
      c = (D & 1) ? c + t : c - t;
#pragma unroll
      for (int j = 0; j < P; ++j) {
        double p = 1.0;   // prod_{j' != j} n[j'], ascending j'
        bool started = false;
#pragma unroll
        for (int j2 = 0; j2 < P; ++j2)
          if (j2 != j) {
            p = started ? p * n[j2] : n[j2];
            started = true;
          }
        const double v = (D & 1) ? -p : p;
#pragma unroll
        for (int l = 1; l <= D; ++l) A.g[l - 1][j] += o[j] == l ? v : 0.0;
      }
      if constexpr (D < QEHVI_MAX_Q) qehvi_walk_grad<P, D + 1>(Ys, Yb, ldi, ldj, lb, ub, n, o, i + 1, q, c, A);
#pragma unroll
      for (int j = 0; j < P; ++j) {
        Yb[j * ldj + i * ldi] += A.g[D - 1][j];
        A.g[D - 1][j] = 0.0;
      }
    }
  }
}

template <int P>
__global__ __launch_bounds__(QEHVI_THREADS) void qehvi_grad_tail_kernel(
    const double* __restrict__ mean, const double* __restrict__ cov, int64_t gstride, int q, const double* __restrict__ eps, int S,
    int chunk, double jitter, const double* __restrict__ bounds, int V, const uint32_t* __restrict__ cells, int K,
    int zero_clipped, double* __restrict__ val, double* __restrict__ gmean, double* __restrict__ gcov, int* __restrict__ info) {
  extern __shared__ double qehvi_lds[];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int64_t g = blockIdx.x;
  const int qq = q * q;
  const int nent = q * (q + 3) / 2;    // per objective: q means and q (q + 1) / 2 entries of Lbar's lower triangle
  const int rowcap = min(chunk, (S + 63) & ~63);
  double* const Ls = qehvi_lds;        // [P][q][q]
  double* const mu = Ls + P * qq;      // [P][q]
  double* const Ms = mu + P * q;       // [P][q][q]: Lbar -> ... -> gcov, in place
  double* const Es = Ms + P * qq;      // [P][nent]: the sums over the samples
  double* const Y = Es + P * nent;     // [P][q][rowcap]; afterwards [4][64] partial sums
  double* const Yb = Y + P * q * rowcap;   // [4][P][q][rowcap]: one adjoint copy per wave

  for (int e = tid; e < P * nent; e += QEHVI_THREADS) Es[e] = 0.0;
  qehvi_load_and_factor<P>(mean, cov, gstride, g, q, jitter, Ls, mu, info, tid);

  double acc = 0.0;
  QehviAdj<P> A;   // every level flushes and clears its own slots before its loop moves on: cleared once, here
#pragma unroll
  for (int l = 0; l < QEHVI_MAX_Q; ++l)
#pragma unroll
    for (int j = 0; j < P; ++j) A.g[l][j] = 0.0;
  for (int s0 = 0; s0 < S; s0 += chunk) {
    const int cs = min(chunk, S - s0);       // samples of this chunk
    const int ld = (cs + 63) & ~63;          // row length in LDS (<= rowcap)
    const int pql = P * q * ld;
    // phase 2: the chunk's samples, the adjoint copies cleared
    qehvi_fill_samples<P>(Ls, mu, eps, q, S, s0, cs, ld, Y, tid);
    for (int e = tid; e < QEHVI_WAVES * pql; e += QEHVI_THREADS) Yb[e] = 0.0;
    __syncthreads();
    // phase 3: the cells of slice `wave` for the samples lane, lane + 64, ...
    double* const Ybw = Yb + wave * pql;
    for (int b = 0; b < ld; b += 64) {
      const bool valid = b + lane < cs;
      const double* const Ys = Y + b + lane;
      for (int k = wave; k < K; k += QEHVI_WAVES) {
        double lb[P], ub[P], top[P];
        int nobody[P];
        qehvi_cell_bounds<P>(bounds, V, cells, k, lb, ub, top);
#pragma unroll
        for (int j = 0; j < P; ++j) nobody[j] = 0;
        double c = 0.0;
        if (valid) qehvi_walk_grad<P, 1>(Ys, Ybw + b + lane, ld, q * ld, lb, ub, top, nobody, 0, q, c, A);
        acc += c;
      }
    }
    __syncthreads();
    // phase 4a: this chunk's part of gmean and Lbar
    for (int e = wave; e < P * nent; e += QEHVI_WAVES) {
      const int j = e / nent, r = e - j * nent;   // r < q: gmean[j][r]; else the r - q th entry (i, m <= i) of the triangle
      int i = r, m2 = -1;
      if (r >= q) {
        int t = r - q;
        i = 0;
        while (t > i) {
          t -= i + 1;
          ++i;
        }
        m2 = t;
      }
      const double* const y0 = Yb + (j * q + i) * ld;
      const double* const ep = eps + ((int64_t)j * q + (m2 < 0 ? 0 : m2)) * S + s0;
      double sum = 0.0;
      for (int b = 0; b < ld; b += 64) {
        const int s = b + lane;
        double v = 0.0;
        if (s < cs) {
          v = ((y0[s] + y0[pql + s]) + y0[2 * pql + s]) + y0[3 * pql + s];
          if (m2 >= 0) v *= ep[s];
        }
        sum += wave_sum(v);
      }
      if (lane == 0) Es[e] += sum;
    }
    __syncthreads();
  }
  // Lbar's lower triangle into Ms, scaled; the means' adjoints out
  const double invS = 1.0 / (double)S;
  for (int e = tid; e < P * nent; e += QEHVI_THREADS) {
    const int j = e / nent, r = e - j * nent;
    const double v = Es[e] * invS;
    if (r < q) {
      gmean[((int64_t)j * gstride + g) * q + r] = v;
    } else {
      int t = r - q, i = 0;
      while (t > i) {
        t -= i + 1;
        ++i;
      }
      Ms[j * qq + i * q + t] = v;
    }
  }
  qehvi_reduce_value(Y, acc, tid, S, val + g);
  // phase 4b: wave j takes objective j (P <= 4 waves); lane c owns column c, later row c (chol_adjoint, as in qei_grad_tail_kernel)
  const bool work = wave < P && lane < q;
  const double* const L = Ls + (wave < P ? wave : 0) * qq;
  double* const M = Ms + (wave < P ? wave : 0) * qq;
  chol_adjoint(L, M, q, q, lane, work, [] { __syncthreads(); });
  __syncthreads();
  for (int e = tid; e < P * qq; e += QEHVI_THREADS) {
    const int j = e / qq, r = e - j * qq, i = r / q, k = r - i * q;
    const int64_t at = ((int64_t)j * gstride + g) * qq + r;
    // (zero_clipped: a variance at the posterior's floor was clipped there, and the clip's adjoint is zero)
    // (the two substitutions leave a matrix that is symmetric to rounding: its symmetric part, in bits)
    gcov[at] = zero_clipped && i == k && !(cov[at] > VAR_FLOOR) ? 0.0 : 0.5 * (Ms[e] + Ms[j * qq + k * q + i]);
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

template <int P>
void launch_qehvi_grad_p(hipStream_t s, int V, const double* bounds, const uint32_t* cells, int K, const double* mean,
                         const double* cov, int64_t G, int64_t gstride, int q, const double* eps, int S, double jitter,
                         int zero_clipped, double* val, double* gmean, double* gcov, int* info) {
  // per launch, as launch_qei_grad_tail_qp: the attribute belongs to the current device, and one process may drive several; a
  // failure shows as the launch's error, which every caller checks
  (void)hipFuncSetAttribute((const void*)qehvi_grad_tail_kernel<P>, hipFuncAttributeMaxDynamicSharedMemorySize, QEHVI_GRAD_LDS);
  hipLaunchKernelGGL(qehvi_grad_tail_kernel<P>, dim3((unsigned)G), dim3(QEHVI_THREADS), qehvi_grad_lds_bytes(P, q, S), s, mean, cov,
                     gstride, q, eps, S, qehvi_grad_sample_chunk(P, q), jitter, bounds, V, cells, K, zero_clipped, val, gmean, gcov,
                     info);
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
  with_objectives(P, [&](auto PC) {
    launch_qehvi_p<decltype(PC)::value>(s, V, bounds, cells, K, mean, cov, G, gstride, q, eps, S, jitter, out, info);
  });
}

// doubles beside the sample slots: the factors, the means, the adjoint work matrices, the sums of gmean and Lbar
static size_t qehvi_grad_fixed_doubles(int P, int q) { return (size_t)P * (2 * q * q + q + q * (q + 3) / 2); }

int qehvi_grad_sample_chunk(int P, int q) {
  const int fit = (int)((QEHVI_GRAD_LDS - 8 * qehvi_grad_fixed_doubles(P, q)) / (8 * (QEHVI_SLICES + 1) * P * q)) & ~63;
  return fit < QEHVI_MAX_CHUNK ? fit : QEHVI_MAX_CHUNK;
}

size_t qehvi_grad_lds_bytes(int P, int q, int S) {
  const int chunk = qehvi_grad_sample_chunk(P, q), padded = (int)(((int64_t)S + 63) & ~(int64_t)63);
  // (the [4][64] partial sums of the value fit the sample slots: 5 P q 64 >= 640 doubles)
  return 8 * (qehvi_grad_fixed_doubles(P, q) + (size_t)(QEHVI_SLICES + 1) * P * q * (padded < chunk ? padded : chunk));
}

void launch_qehvi_grad_tail(hipStream_t s, int P, int V, const double* bounds, const uint32_t* cells, int K, const double* mean,
                            const double* cov, int64_t G, int64_t gstride, int q, const double* eps, int S, double jitter,
                            int zero_clipped, double* val, double* gmean, double* gcov, int* info) {
  if (G <= 0) return;
  with_objectives(P, [&](auto PC) {
    launch_qehvi_grad_p<decltype(PC)::value>(s, V, bounds, cells, K, mean, cov, G, gstride, q, eps, S, jitter, zero_clipped, val, gmean,
                                             gcov, info);
  });
}

}  // namespace tgp
