// PredictiveVariance (reference acquisition/function/active_learning.py:36-110): the determinant of the joint predictive
// covariance of a batch of q points, the D-optimal design criterion.  Per batch
//     A = cov + jitter ON EVERY ENTRY (the reference adds the scalar to the whole matrix),   A = L L^T,
//     logdet = 2 sum_i log L_ii,   det = prod_i (pivot_i),   and with GRAD   gcov = det A^-1 = det W^T W,  W = L^-1,
// gcov symmetric bit for bit, d det = sum gcov o dcov for every symmetric dcov.  det is the running product of the pivots
// (the squares L_ii^2 as the elimination leaves them), which is exp(logdet) to rounding without the |logdet| ulps an
// exponential would add: at q = 1 it is cov + jitter exactly.  A running product can leave the normal range part-way (large and
// small pivots mixed) where the determinant itself is representable: the product's range is watched at every step, and a
// batch whose product left it takes det = exp(logdet) instead.  A batch whose elimination meets a pivot that is not a positive
// finite number gets NaN in every output; nothing is reported through `info`, no other batch is touched.
//
// Two forms:
//   pvar_tail_kernel<QP, GRAD>   q <= 16: ONE WAVE per batch, four batches per 256-thread workgroup, QP = q padded to 1, 2, 4, 8,
//     16 with an identity tail.  The wave's LDS tile [q][q | 1] only stages the batch in and the adjoint out, both coalesced;
//     lane i holds row i in registers, the pivot and the multipliers of a column step reach every lane through v_readlane
//     (wave_bcast), fully unrolled: no barrier, no LDS traffic inside the factorisation.  GRAD: lane c solves column c of
//     W = L^-1 by forward substitution in registers (L's entries by v_readlane), then forms column c of W^T W the same way.
//     A wave beyond the last batch leaves at once (there is no barrier to miss).
//   pvar_tail_block_kernel<GRAD>      16 < q <= 64: ONE WORKGROUP (four waves) per batch, n = q padded to a multiple of 16 with an
//     identity tail (log 1 = 0, a factor 1, a unit block in the inverse; the pad is never written out), the matrix in LDS with
//     row stride n + 4 (an MFMA fragment read then touches every bank pair once).  Right-looking in 16-wide block columns:
//     wave 0 factorises the diagonal block with the one-wave routine above; the rows below it are solved against L_jj^T one row
//     per thread (registers, L_jj by LDS broadcasts); the trailing tiles S_ik -= P_i P_k^T run on v_mfma_f64_16x16x4_f64, dealt
//     over the waves.  GRAD: the four diagonal inverses one per wave (one-wave routine), block column j of W = L^-1 by wave j,
//     W_ij = -W_ii sum_k L_ik W_kj on the matrix pipe, then the lower tiles of W^T W dealt over the waves; the output mirrors
//     the lower triangle.
// Fixed summation orders, no atomics: identical calls give identical bits, and a batch's bits do not depend on its neighbours.
#include "tgp_dev.hpp"
#include "tgp_internal.hpp"
#include "tgp_tail_dev.hpp"

namespace tgp {

struct PvarArgs {
  const double* cov;   // [G][q][q]
  double jitter;
  int q;
  int64_t G;
  double *det, *logdet;   // [G]; logdet may be null
  double *gmean, *gcov;   // GRAD: [G][q] zeros (may be null), [G][q][q]
};

namespace {

// In-wave Cholesky factorisation of a QP x QP matrix, row per lane in registers: lane `li` < QP holds row li in r (lanes that
// share an li hold copies; only lanes 0 .. QP-1 are ever read).  Column step j: the pivot and every multiplier by v_readlane.
// Entries right of the diagonal are updated along with the rest and never read.  prod *= every pivot, in order, and
// `inrange` falls once the product is no normal number; a pivot that is not positive and finite sets `bad` and goes on as 1.
// Returns sum_j log L_jj, j ascending (one log per lane).
template <int QP>
__device__ __forceinline__ double chol_rows_reg(double (&r)[QP], int li, double& prod, bool& inrange, bool& bad) {
#pragma unroll
  for (int j = 0; j < QP; ++j) {
    double dj = wave_bcast(r[j], j);
    if (!(dj > 0.0) || !(dj < __builtin_huge_val())) {
      bad = true;
      dj = 1.0;
    }
    prod *= dj;
    if (!(prod >= 0x1p-1022 && prod < __builtin_huge_val())) inrange = false;
    const double sd = sqrt(dj);
    const double lij = li == j ? sd : r[j] / sd;
    r[j] = lij;
#pragma unroll
    for (int k = j + 1; k < QP; ++k) r[k] = fma(-lij, wave_bcast(lij, k), r[k]);
  }
  double diag = 1.0;
#pragma unroll
  for (int j = 0; j < QP; ++j)
    if (li == j) diag = r[j];
  const double lg = log(diag);
  double lsum = 0.0;
#pragma unroll
  for (int j = 0; j < QP; ++j) lsum += wave_bcast(lg, j);
  return lsum;
}

// Column `li` of W = L^-1 in w (zeros above the diagonal), L row per lane in r as chol_rows_reg leaves it: forward
// substitution, L_ik by v_readlane.  (The loops run over all k < i: the leading zeros of w keep them uniform.)
template <int QP>
__device__ __forceinline__ void inv_cols_reg(const double (&r)[QP], double (&w)[QP], int li) {
#pragma unroll
  for (int i = 0; i < QP; ++i) {
    double t = li == i ? 1.0 : 0.0;
#pragma unroll
    for (int k = 0; k < i; ++k) t = fma(-wave_bcast(r[k], i), w[k], t);
    w[i] = t / wave_bcast(r[i], i);
  }
}

__device__ __forceinline__ double pvar_nan() { return __builtin_nan(""); }
// the determinant: the pivots' product, or exp(logdet) where the product left the normal range on its way
__device__ __forceinline__ double pvar_det(double prod, bool inrange, double lsum) { return inrange ? prod : exp(2.0 * lsum); }

}  // namespace

template <int QP, bool GRAD>
__global__ __launch_bounds__(256) void pvar_tail_kernel(PvarArgs a) {
  extern __shared__ double pvar_lds[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t g = (int64_t)blockIdx.x * 4 + wave;
  if (g >= a.G) return;   // the last workgroup may be partly empty
  const int q = a.q, ld = q | 1;
  double* const T = pvar_lds + wave * q * ld;   // this wave's tile [q][ld]
  const double* const cov = a.cov + g * q * q;
  for (int e = lane; e < q * q; e += 64) T[(e / q) * ld + e % q] = cov[e] + a.jitter;
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
  double r[QP];
#pragma unroll
  for (int k = 0; k < QP; ++k) r[k] = (lane < q && k < q) ? T[lane * ld + k] : (k == lane ? 1.0 : 0.0);
  double prod = 1.0;
  bool inrange = true, bad = false;
  const double lsum = chol_rows_reg<QP>(r, lane, prod, inrange, bad);
  const double det = pvar_det(prod, inrange, lsum);
  if (lane == 0) {
    a.det[g] = bad ? pvar_nan() : det;
    if (a.logdet) a.logdet[g] = bad ? pvar_nan() : 2.0 * lsum;
  }
  if constexpr (GRAD) {
    double w[QP];
    inv_cols_reg<QP>(r, w, lane);
    // column `lane` of W^T W = row `lane`: (a, lane) = sum_{k >= a} W_ka W_k,lane (W_k,lane = 0 for k < lane)
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
#pragma unroll
    for (int i = 0; i < QP; ++i) {
      double s = 0.0;
#pragma unroll
      for (int k = i; k < QP; ++k) s = fma(wave_bcast(w[k], i), w[k], s);
      if (lane < q && i < q) T[lane * ld + i] = s;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    double* const gcov = a.gcov + g * q * q;
    for (int e = lane; e < q * q; e += 64) {
      const int i = e / q, j = e % q;
      gcov[e] = bad ? pvar_nan() : det * T[max(i, j) * ld + min(i, j)];
    }
    if (a.gmean && lane < q) a.gmean[g * q + lane] = 0.0;
  }
}

namespace {

// the fragments of v_mfma_f64_16x16x4_f64 (tgp_dev.hpp) on 16 x 16 tiles of a matrix with row stride ld, k-step k4:
// A[i][k] and B[k][j] read plainly, or transposed (A = X^T: A[i][k] = X[k][i];  B = X^T: B[k][j] = X[j][k])
__device__ __forceinline__ double frag_rowk(const double* X, int ld, int lane, int k4) {   // X[lane & 15][4 k4 + (lane >> 4)]
  return X[(lane & 15) * ld + 4 * k4 + (lane >> 4)];
}
__device__ __forceinline__ double frag_krow(const double* X, int ld, int lane, int k4) {   // X[4 k4 + (lane >> 4)][lane & 15]
  return X[(4 * k4 + (lane >> 4)) * ld + (lane & 15)];
}
__device__ __forceinline__ void tile_store(double* X, int ld, int lane, v4d c) {
#pragma unroll
  for (int r = 0; r < 4; ++r) X[((lane >> 4) + 4 * r) * ld + (lane & 15)] = c[r];
}

}  // namespace

template <bool GRAD>
__global__ __launch_bounds__(256) void pvar_tail_block_kernel(PvarArgs a) {
  extern __shared__ double pvar_lds[];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, li = lane & 15;
  const int64_t g = blockIdx.x;
  const int q = a.q, n = (q + 15) & ~15, nb = n >> 4, ld = n + 4;
  double* const S = pvar_lds;            // [n][ld]: A, then L in its lower triangle, then (GRAD) the lower tiles of W^T W
  double* const W = pvar_lds + n * ld;   // GRAD: [n][ld], L^-1
  double &s_det = S[n], &s_bad = S[n + 1];   // wave 0's results for all, in the padding of row 0 (no tile reaches it)
  const double* const cov = a.cov + g * q * q;
  for (int e = tid; e < n * n; e += 256) {
    const int i = e / n, j = e % n;
    S[i * ld + j] = (i < q && j < q) ? cov[i * q + j] + a.jitter : (i == j ? 1.0 : 0.0);
  }
  double prod = 1.0, lsum = 0.0;   // wave 0's, wave-uniform
  bool inrange = true, bad = false;
  __syncthreads();
  for (int jb = 0; jb < nb; ++jb) {
    double* const D = S + 16 * jb * (ld + 1);   // the diagonal block
    if (wave == 0) {
      double r[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) r[k] = D[li * ld + k];
      lsum += chol_rows_reg<16>(r, li, prod, inrange, bad);
      if (lane < 16) {
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if (k <= li) D[li * ld + k] = r[k];
      }
    }
    __syncthreads();
    // the panel: rows below the block, P L_jj^T = S_ij, one row per thread, sixteen rows per wave
    const int row = 16 * (jb + 1) + 16 * wave + lane;
    if (lane < 16 && row < n) {
      double* const prow = S + row * ld + 16 * jb;
      double p[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) p[k] = prow[k];
#pragma unroll
      for (int j = 0; j < 16; ++j) {
        double t = p[j];
#pragma unroll
        for (int k = 0; k < j; ++k) t = fma(-p[k], D[j * ld + k], t);
        p[j] = t / D[j * ld + j];
      }
#pragma unroll
      for (int k = 0; k < 16; ++k) prow[k] = p[k];
    }
    __syncthreads();
    // the trailing update, lower tiles (ib, kb), jb < kb <= ib: S_ik -= P_i P_k^T
    int t = 0;
    for (int ib = jb + 1; ib < nb; ++ib)
      for (int kb = jb + 1; kb <= ib; ++kb, ++t) {
        if ((t & 3) != wave) continue;
        double* const C = S + 16 * ib * ld + 16 * kb;
        const double *const Pi = S + 16 * ib * ld + 16 * jb, *const Pk = S + 16 * kb * ld + 16 * jb;
        v4d acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = C[((lane >> 4) + 4 * r) * ld + li];
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) acc = mfma_f64(-frag_rowk(Pi, ld, lane, k4), frag_rowk(Pk, ld, lane, k4), acc);
        tile_store(C, ld, lane, acc);
      }
    __syncthreads();
  }
  if (tid == 0) {
    const double det = pvar_det(prod, inrange, lsum);
    s_det = det;
    s_bad = bad ? 1.0 : 0.0;
    a.det[g] = bad ? pvar_nan() : det;
    if (a.logdet) a.logdet[g] = bad ? pvar_nan() : 2.0 * lsum;
  }
  if constexpr (GRAD) {
    // the diagonal blocks of W = L^-1, one per wave (nb <= 4), zeros above the diagonal
    if (wave < nb) {
      const double* const D = S + 16 * wave * (ld + 1);
      double r[16], w[16];
#pragma unroll
      for (int k = 0; k < 16; ++k) r[k] = D[li * ld + k];
      inv_cols_reg<16>(r, w, li);
      if (lane < 16) {
        double* const Wd = W + 16 * wave * (ld + 1);
#pragma unroll
        for (int i = 0; i < 16; ++i) Wd[i * ld + li] = w[i];
      }
    }
    __syncthreads();
    // block column j of W by wave j, rows descending from the diagonal: W_ij = -W_ii (sum_{k = j}^{i-1} L_ik W_kj)
    if (wave < nb - 1) {
      const int j = wave;
      for (int i = j + 1; i < nb; ++i) {
        double* const Wij = W + 16 * i * ld + 16 * j;
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        for (int k = j; k < i; ++k) {
          const double *const Lik = S + 16 * i * ld + 16 * k, *const Wkj = W + 16 * k * ld + 16 * j;
#pragma unroll
          for (int k4 = 0; k4 < 4; ++k4) acc = mfma_f64(frag_rowk(Lik, ld, lane, k4), frag_krow(Wkj, ld, lane, k4), acc);
        }
        tile_store(Wij, ld, lane, acc);   // (through LDS: an accumulator is no B fragment)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const double* const Wii = W + 16 * i * (ld + 1);
        double bv[4];
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) bv[k4] = frag_krow(Wij, ld, lane, k4);
        v4d res = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int k4 = 0; k4 < 4; ++k4) res = mfma_f64(-frag_rowk(Wii, ld, lane, k4), bv[k4], res);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        tile_store(Wij, ld, lane, res);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
      }
    }
    __syncthreads();
    // the lower tiles (ab, bb <= ab) of W^T W over L's remains: sum_{k >= ab} W_ka^T W_kb
    int t = 0;
    for (int ab = 0; ab < nb; ++ab)
      for (int bb = 0; bb <= ab; ++bb, ++t) {
        if ((t & 3) != wave) continue;
        v4d acc = {0.0, 0.0, 0.0, 0.0};
        for (int k = ab; k < nb; ++k) {
          const double *const Wka = W + 16 * k * ld + 16 * ab, *const Wkb = W + 16 * k * ld + 16 * bb;
#pragma unroll
          for (int k4 = 0; k4 < 4; ++k4) acc = mfma_f64(frag_krow(Wka, ld, lane, k4), frag_krow(Wkb, ld, lane, k4), acc);
        }
        tile_store(S + 16 * ab * ld + 16 * bb, ld, lane, acc);
      }
    __syncthreads();
    const double dt = s_det;
    const bool any_bad = s_bad != 0.0;
    double* const gcov = a.gcov + g * q * q;
    for (int e = tid; e < q * q; e += 256) {
      const int i = e / q, j = e % q;
      gcov[e] = any_bad ? pvar_nan() : dt * S[max(i, j) * ld + min(i, j)];
    }
    if (a.gmean && tid < q) a.gmean[g * q + tid] = 0.0;
  }
}

size_t pvar_tail_lds_bytes(int q, bool grad) {
  if (q <= PVAR_WAVE_Q) return (size_t)4 * q * (q | 1) * sizeof(double);
  const int n = (q + 15) & ~15;
  return (size_t)(grad ? 2 : 1) * n * (n + 4) * sizeof(double);
}

template <int QP, bool GRAD>
static void launch_pvar_wave(hipStream_t s, const PvarArgs& a) {
  hipLaunchKernelGGL((pvar_tail_kernel<QP, GRAD>), dim3((unsigned)((a.G + 3) / 4)), dim3(256), pvar_tail_lds_bytes(a.q, GRAD), s, a);
}
template <bool GRAD>
static void launch_pvar_grad(hipStream_t s, const PvarArgs& a) {
  if (a.q > PVAR_WAVE_Q) {
    const size_t lds = pvar_tail_lds_bytes(a.q, GRAD);
    if (lds > 64 * 1024)
      (void)hipFuncSetAttribute((const void*)pvar_tail_block_kernel<GRAD>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL((pvar_tail_block_kernel<GRAD>), dim3((unsigned)a.G), dim3(256), lds, s, a);
  } else if (a.q <= 1) launch_pvar_wave<1, GRAD>(s, a);
  else if (a.q <= 2) launch_pvar_wave<2, GRAD>(s, a);
  else if (a.q <= 4) launch_pvar_wave<4, GRAD>(s, a);
  else if (a.q <= 8) launch_pvar_wave<8, GRAD>(s, a);
  else launch_pvar_wave<16, GRAD>(s, a);
}
void launch_pvar_tail(hipStream_t s, const double* cov, int64_t G, int q, double jitter, double* det, double* logdet,
                      double* gmean, double* gcov) {
  const PvarArgs a{cov, jitter, q, G, det, logdet, gmean, gcov};
  if (gcov) launch_pvar_grad<true>(s, a);
  else launch_pvar_grad<false>(s, a);
}

}  // namespace tgp
