// The pieces that the acquisition tails share (tgp_kernels_misc.hip: qEI; tgp_kernels_bei.hip: batch EI; tgp_kernels_qehvi.hip:
// qEHVI): a value kernel and its gradient twin agree bit for bit because both call the SAME function here, not a copy of it.
// Force-inlined device functions only.
#pragma once
#include "tgp_dev.hpp"

namespace tgp {

// lane l's v in every lane (v_readlane: the result is wave-uniform, a scalar operand of what follows)
__device__ __forceinline__ double wave_bcast(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}

// In-wave Cholesky factorisation of an n x n matrix, row per lane: lane i < n (`live`) owns row i at Lrow (the other lanes
// point at row 0 and never write).  The pivot and the multiplier l_kj reach every lane through wave_bcast, so no lane reads
// another lane's LDS data: no barrier, no fence -- the CALLER fences before the rows are read across lanes.  Entries right of
// the diagonal are updated along with the rest (never read).  A non-positive pivot reports group g in *info (the first
// report wins) and goes on with pivot 1.  on_pivot(j, sd) runs in every lane behind column j, sd = sqrt(pivot).
template <class OnPivot>
__device__ __forceinline__ void wave_chol_rows(double* Lrow, bool live, int lane, int n, int64_t g, int* info, OnPivot on_pivot) {
  for (int j = 0; j < n; ++j) {
    const double x = Lrow[j];
    double dj = wave_bcast(x, j);
    if (!(dj > 0.0)) {
      if (lane == 0) atomicCAS(info, 0, (int)(g % 2000000000) + 1);
      dj = 1.0;
    }
    const double sd = sqrt(dj);
    const double lij = lane == j ? sd : x / sd;
    const bool below = live && lane > j;
    if (live && lane >= j) Lrow[j] = lij;
    const double nl = -lij;
    for (int k = j + 1; k < n; ++k) {
      const double lkj = wave_bcast(lij, k);
      if (below) Lrow[k] = fma(nl, lkj, Lrow[k]);
    }
    on_pivot(j, sd);
  }
}

// The Cholesky adjoint in place: M holds Lbar's lower triangle (whatever lies above it is overwritten) and ends as
// L^-T sym(Phi(L^T Lbar)) L^-1 (Phi: lower triangle, diagonal halved), symmetric to rounding.  L and M are n x n with row stride
// ld; lane c < n (`live`) owns column c, in the last step row c; fixed summation orders.  sync() stands between the four
// steps (three calls) -- the caller's wave fence or barrier -- and the CALLER synchronises once more before M is read
// across lanes.
template <class Sync>
__device__ __forceinline__ void chol_adjoint(const double* L, double* M, int ld, int n, int lane, bool live, Sync sync) {
  // Q = tril(L^T Lbar) in place, column c: Q[a][c] = sum_{k >= a} L[k][a] Lbar[k][c]  (rows ascending: row a is read before
  // it is written and never again), then R's lower triangle = Q / 2 (Phi halves the diagonal, sym the rest)
  if (live)
    for (int a = lane; a < n; ++a) {
      double t = 0.0;
      for (int k = a; k < n; ++k) t = fma(L[k * ld + a], M[k * ld + lane], t);
      M[a * ld + lane] = 0.5 * t;
    }
  sync();
  if (live)
    for (int a = 0; a < lane; ++a) M[a * ld + lane] = M[lane * ld + a];  // R = R^T
  sync();
  if (live)  // Y = L^-T R: back substitution down column c
    for (int a = n - 1; a >= 0; --a) {
      double t = M[a * ld + lane];
      for (int k = a + 1; k < n; ++k) t = fma(-L[k * ld + a], M[k * ld + lane], t);
      M[a * ld + lane] = t / L[a * ld + a];
    }
  sync();
  if (live) {  // Y L^-1: back substitution along row c
    double* const row = M + lane * ld;
    for (int a = n - 1; a >= 0; --a) {
      double t = row[a];
      for (int k = a + 1; k < n; ++k) t = fma(-L[k * ld + a], row[k], t);
      row[a] = t / L[a * ld + a];
    }
  }
}

}  // namespace tgp
