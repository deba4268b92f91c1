// IntegratedVarianceReduction (reference acquisition/function/active_learning.py:304-415, models/gpflow/models.py:355-416): how much
// the predictive variance, averaged with weights over P integration points z, drops when a batch of q points x is observed.
// The conditioned variance is a Schur complement over the q new points,
//     v_old(z) - v_new(z) = c_z^T (Sigma_xx + s^2 I)^-1 c_z = |L^-1 c_z|^2,   L = chol(Sigma_xx + s^2 I),  c_z = cov(x, z),
// so per group of q points
//     reduction = (1/P) sum_z w_z sum_i a_iz^2,   a_.z = L^-1 c_.z                    (no jitter: models.py:390-394)
// and the reference's value -mean(w v_new) = reduction - c0 with c0 = (1/P) sum_z w_z v_old(z) (ivr_c0_kernel).
//
// ivr_tail_kernel<QP, GIVEN>: ONE WAVE per group (a 64-thread workgroup: no s_barrier), QP = q padded to 1, 2, 4, 8, 16.
//   phase 1  lane i < q owns row i of cov + s^2 I in LDS; wave_chol_rows factorises it (pivot and multiplier through
//            v_readlane), a non-positive pivot reports the group through `info`;
//   phase 2  lanes run along z in tiles of 64.  A lane forms its q entries c_iz -- GIVEN: read from cross [G][q][P]; otherwise
//            k(x_i, z) - S[g q + i][z] with S = (W k(X, x))^T (W k(X, Z)) (the reference's A-form) and the distance from
//            x_i / l (LDS, broadcast reads) and Z / l stored transposed [d][ldz] (coalesced along z) -- runs the forward
//            substitution against L in registers (L as LDS broadcasts, fully unrolled over QP, left by wave-uniform branches)
//            and adds w_z sum_i a_i^2 to its own partial sum, tiles ascending;
//   end      one butterfly over the 64 partial sums, then the division by P: a fixed order, identical calls give identical bits.
// A lane with z >= P in the last tile is MASKED (it reads neither cross nor the weights and adds nothing): the padding of S may
// hold anything.  Rows i >= q of the padded QP never enter: every loop over QP is cut at q.  Rows of S beyond the launch's
// last point are never addressed (row = g q + i < G q).  The mean is over P, never the padded width.
#include "tgp_dev.hpp"
#include "tgp_internal.hpp"
#include "tgp_tail_dev.hpp"

namespace tgp {

template <int QP, bool GIVEN>
__global__ __launch_bounds__(64) void ivr_tail_kernel(IvrTailArgs a) {
  extern __shared__ double ivr_lds[];
  const int64_t g = blockIdx.x;
  const int lane = threadIdx.x;
  const int q = a.q, d = a.d;
  const int ldq = q | 1;  // odd row stride
  double* const Ls = ivr_lds;             // [q][ldq]
  double* const xs = ivr_lds + q * ldq;   // [q][d]: x_i / l (not GIVEN)
  const bool live = lane < q;
  double* const Lrow = Ls + (live ? lane : 0) * ldq;
  if (live) {
    const double* const crow = a.cov + (g * q + lane) * q;
    for (int k = 0; k < q; ++k) Lrow[k] = crow[k] + (k == lane ? a.noise : 0.0);
  }
  if constexpr (!GIVEN) {
    for (int e = lane; e < q * d; e += 64) {
      const int c = e % d;
      xs[e] = a.Xq[g * q * d + e] / a.ls[c];
    }
  }
  wave_chol_rows(Lrow, live, lane, q, g, a.info, [](int, double) {});
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // from here on every lane reads every row (and xs)
  double acc = 0.0;
  for (int64_t z0 = 0; z0 < a.P; z0 += 64) {
    const int64_t z = z0 + lane;
    const bool valid = z < a.P;
    double c[QP];
    if constexpr (GIVEN) {
#pragma unroll
      for (int i = 0; i < QP; ++i) c[i] = (i < q && valid) ? a.cross[(g * q + i) * a.P + z] : 0.0;
    } else {
      // (z < ldz always: the padded columns of Zt hold zeros, of S whatever the product left -- masked below)
#pragma unroll
      for (int i = 0; i < QP; ++i) c[i] = 0.0;
      for (int cc = 0; cc < d; ++cc) {
        const double zc = a.Zt[(int64_t)cc * a.ldz + z];
#pragma unroll
        for (int i = 0; i < QP; ++i)
          if (i < q) {
            const double t = xs[i * d + cc] - zc;
            c[i] = fma(t, t, c[i]);
          }
      }
#pragma unroll
      for (int i = 0; i < QP; ++i)
        if (i < q) c[i] = kernel_rt(a.kind, c[i], a.variance) - a.S[(g * q + i) * a.ldz + z];
    }
    // a = L^-1 c in place, s = sum_i a_i^2 in row order
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < QP; ++i)
      if (i < q) {  // (wave-uniform)
        const double* const Li = Ls + i * ldq;
        double t = c[i];
#pragma unroll
        for (int k = 0; k < i; ++k) t = fma(-Li[k], c[k], t);
        t = t / Li[i];
        c[i] = t;
        s = fma(t, t, s);
      }
    if (valid) {
      const double w = a.weights ? a.weights[z] : 1.0;
      acc = fma(w, s, acc);
    }
  }
  acc = wave_sum(acc);
  if (lane == 0) {
    const double red = acc / (double)a.P;
    if (a.reduction) a.reduction[g] = red;
    if (a.out) a.out[g] = red - (a.c0 ? *a.c0 : 0.0);
  }
}

size_t ivr_tail_lds_bytes(int q, int d, bool given) { return (size_t)(q * (q | 1) + (given ? 0 : q * d)) * sizeof(double); }

template <int QP, bool GIVEN>
static void launch_ivr_tail_qp(hipStream_t s, const IvrTailArgs& a, int64_t G) {
  const size_t lds = ivr_tail_lds_bytes(a.q, a.d, GIVEN);
  if (lds > 64 * 1024)
    (void)hipFuncSetAttribute((const void*)ivr_tail_kernel<QP, GIVEN>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  hipLaunchKernelGGL((ivr_tail_kernel<QP, GIVEN>), dim3((unsigned)G), dim3(64), lds, s, a);
}
template <bool GIVEN>
static void launch_ivr_tail_given(hipStream_t s, const IvrTailArgs& a, int64_t G) {
  if (a.q <= 1) launch_ivr_tail_qp<1, GIVEN>(s, a, G);
  else if (a.q <= 2) launch_ivr_tail_qp<2, GIVEN>(s, a, G);
  else if (a.q <= 4) launch_ivr_tail_qp<4, GIVEN>(s, a, G);
  else if (a.q <= 8) launch_ivr_tail_qp<8, GIVEN>(s, a, G);
  else launch_ivr_tail_qp<IVR_MAX_Q, GIVEN>(s, a, G);
}
void launch_ivr_tail(hipStream_t s, const IvrTailArgs& a, int64_t G) {
  if (a.cross) launch_ivr_tail_given<true>(s, a, G);
  else launch_ivr_tail_given<false>(s, a, G);
}

// Zt [d][ldz] = Z [P][d] / l transposed, zero beyond P
__global__ void ivr_scale_z_kernel(const double* __restrict__ Z, const double* __restrict__ ls, int64_t P, int d, int64_t ldz,
                                   double* __restrict__ Zt) {
  const int64_t z = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int c = blockIdx.y;
  if (z >= ldz) return;
  Zt[(int64_t)c * ldz + z] = z < P ? Z[z * d + c] / ls[c] : 0.0;
}
void launch_ivr_scale_z(hipStream_t s, const double* Z, const double* ls, int64_t P, int d, int64_t ldz, double* Zt) {
  hipLaunchKernelGGL(ivr_scale_z_kernel, dim3((unsigned)((ldz + 255) / 256), (unsigned)d), dim3(256), 0, s, Z, ls, P, d, ldz, Zt);
}

// c0 = (1/P) sum_z w_z var_z: one workgroup, thread t sums z = t, t + 256, ... ascending, then a fixed tree
__global__ __launch_bounds__(256) void ivr_c0_kernel(const double* __restrict__ w, const double* __restrict__ var, int64_t P,
                                                     double* __restrict__ c0) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double acc = 0.0;
  for (int64_t z = t; z < P; z += 256) acc = fma(w[z], var[z], acc);
  red[t] = acc;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  if (t == 0) *c0 = red[0] / (double)P;
}
void launch_ivr_c0(hipStream_t s, const double* w, const double* var, int64_t P, double* c0) {
  hipLaunchKernelGGL(ivr_c0_kernel, dim3(1), dim3(256), 0, s, w, var, P, c0);
}

}  // namespace tgp
