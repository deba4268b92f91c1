// Analytic multi-point expected improvement (Chevalier & Ginsbourger) with Genz's sequential-conditioning estimator of
// the multivariate normal CDF on fixed Sobol points, for gfx950:
//   BatchExpectedImprovement / batch_expected_improvement (reference function.py:1189-1805) + MultivariateNormalCDF
//   (function/utils.py:29-199).
#include "tgp_dev.hpp"
#include "tgp_internal.hpp"

namespace tgp {

// Phi^-1(p), float64: Wichura's algorithm AS 241, routine PPND16 (Applied Statistics 37 (1988) 477-484; about 1e-16
// relative).  The callers confine p to [1e-6, 1 - 1e-6] (utils.py:177), so sqrt(-log(min(p, 1 - p))) <= 3.72 and the
// routine's far-tail branch (r > 5) cannot be reached: it is left out.
__device__ __forceinline__ double normal_quantile_mid(double p) {
  const double q = p - 0.5;
  if (fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    double a = 2.5090809287301226727e+3;
    a = fma(a, r, 3.3430575583588128105e+4);
    a = fma(a, r, 6.7265770927008700853e+4);
    a = fma(a, r, 4.5921953931549871457e+4);
    a = fma(a, r, 1.3731693765509461125e+4);
    a = fma(a, r, 1.9715909503065514427e+3);
    a = fma(a, r, 1.3314166789178437745e+2);
    a = fma(a, r, 3.3871328727963666080e+0);
    double b = 5.2264952788528545610e+3;
    b = fma(b, r, 2.8729085735721942674e+4);
    b = fma(b, r, 3.9307895800092710610e+4);
    b = fma(b, r, 2.1213794301586595867e+4);
    b = fma(b, r, 5.3941960214247511077e+3);
    b = fma(b, r, 6.8718700749205790830e+2);
    b = fma(b, r, 4.2313330701600911252e+1);
    b = fma(b, r, 1.0);
    return q * a / b;
  }
  const double r = sqrt(-log(q < 0.0 ? p : 1.0 - p)) - 1.6;
  double c = 7.74545014278341407640e-4;
  c = fma(c, r, 2.27238449892691845833e-2);
  c = fma(c, r, 2.41780725177450611770e-1);
  c = fma(c, r, 1.27045825245236838258e+0);
  c = fma(c, r, 3.64784832476320460504e+0);
  c = fma(c, r, 5.76949722146069140550e+0);
  c = fma(c, r, 4.63033784615654529590e+0);
  c = fma(c, r, 1.42343711074968357734e+0);
  double d = 1.05075007164441684324e-9;
  d = fma(d, r, 5.47593808499534494600e-4);
  d = fma(d, r, 1.51986665636164571966e-2);
  d = fma(d, r, 1.48103976427480074590e-1);
  d = fma(d, r, 6.89767334985100004550e-1);
  d = fma(d, r, 1.67638483018380384940e+0);
  d = fma(d, r, 2.05319162663775882187e+0);
  d = fma(d, r, 1.0);
  const double v = c / d;
  return q < 0.0 ? -v : v;
}

// ---------------------------------------------------------------------------------------------
// ONE WORKGROUP (BEI_WAVES waves) per q-batch; its q + q^2 CDF problems go round-robin over the waves, and inside a
// problem lane = Sobol sample:
//   problem i        (dimension q):      p_i    = CDF(b_i - m_i; 0, Sigma^(i))                        (function.py:1436-1490)
//   problem q+i*q+k  (dimension q - 1):  Phi_ik = CDF(c^(i,k); 0, R^(i,k)), index k removed           (:1492-1649)
//   value = sum_i [(mu_i - T) p_i + sum_k Sigma^(i)_ki N(b_ik; m_ik, Sigma^(i)_kk) Phi_ik]            (:1724-1745)
// on mu = -mean, T = -eta, cov + 1e-6 I (:1772-1803: the constant is the reference's own, not the builder's jitter).
// A problem: the wave builds its n x n matrix (+ the CDF's own 1e-6 I, utils.py:143-144) row per lane in LDS and
// factorises it as qei_tail_kernel does (pivot and multiplier through v_readlane, no barrier); then every lane walks
// the chain of its sample (utils.py:166-197): y_0..y_{n-2} in registers (loops unrolled to QP), C_ij as LDS broadcast
// reads, one Phi and one Phi^-1 per step.  Sums: per lane over its samples in order, xor-butterfly over the wave, the
// q + q^2 terms by one thread in index order -- the same bits from every call.  No clip at zero (the estimate may be
// slightly negative; the reference returns it as it is).
constexpr int BEI_WAVES = 4;

template <int QP>
__global__ __launch_bounds__(64 * BEI_WAVES) void bei_tail_kernel(const double* __restrict__ mean,
                                                                  const double* __restrict__ cov, int64_t G, int q,
                                                                  const double* __restrict__ w1,
                                                                  const double* __restrict__ w2, int S, double eta,
                                                                  double* __restrict__ out, int* __restrict__ info) {
  extern __shared__ double bei_lds[];
  const int64_t g = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ldq = q | 1;  // odd row stride
  const int nprob = q + q * q;
  double* const cv = bei_lds;            // [q][q]: cov + 1e-6 I
  double* const mu = cv + q * q;         // [q]: -mean
  double* const term = mu + q;           // [q + q^2]: the terms of the sum
  // this wave's factor [n][ldq], then x [q], C_ii + 1e-12 [q] and its inverse [q]
  double* const Ls = term + nprob + wave * (q * ldq + 3 * q);
  double* const xs = Ls + q * ldq;
  double* const dg = xs + q;
  double* const ig = dg + q;
  for (int t = threadIdx.x; t < q * q; t += 64 * BEI_WAVES)
    cv[t] = cov[g * q * q + t] + (t / q == t % q ? 1e-6 : 0.0);
  if ((int)threadIdx.x < q) mu[threadIdx.x] = -mean[g * q + threadIdx.x];
  __syncthreads();
  const double T = -eta;
  auto bcast = [](double v, int l) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
    return __hiloint2double(hi, lo);
  };
  // Sigma^(i)_jk (function.py:1413-1424) and d_j = b_ij - m_ij (:1343-1352, :1480)
  auto sig = [&](int i, int j, int k) {
    const double a = (j != i && k != i) ? cv[j * q + k] : 0.0;
    const double b = j != i ? cv[j * q + i] : 0.0;
    const double c = k != i ? cv[i * q + k] : 0.0;
    return ((a - b) - c) + cv[i * q + i];
  };
  auto dif = [&](int i, int j) {
    const double b = j == i ? -T : 0.0;
    const double m = (mu[j] - mu[i]) - (j == i ? mu[i] : 0.0);
    return b - m;
  };
  for (int pr = wave; pr < nprob; pr += BEI_WAVES) {  // (wave-uniform)
    const bool outer = pr < q;
    const int i = outer ? pr : (pr - q) / q;
    const int k = outer ? -1 : (pr - q) % q;
    const int n = outer ? q : q - 1;
    const bool live = lane < n;
    double* const Lrow = Ls + (live ? lane : 0) * ldq;
    if (live) {
      const int u = lane + ((!outer && lane >= k) ? 1 : 0);
      if (outer) {
        for (int c = 0; c < n; ++c) Lrow[c] = sig(i, u, c) + (c == lane ? 1e-6 : 0.0);
        xs[lane] = dif(i, u);
      } else {  // c^(i) and R^(i) for the pivot k (:1520-1525, :1554-1559)
        const double skk = sig(i, k, k), sku = sig(i, k, u);
        for (int c = 0; c < n; ++c) {
          const int v = c + (c >= k ? 1 : 0);
          Lrow[c] = (sig(i, u, v) - sku * sig(i, k, v) / skk) + (c == lane ? 1e-6 : 0.0);
        }
        xs[lane] = dif(i, u) - dif(i, k) * (sku / skk);
      }
    }
    for (int j = 0; j < n; ++j) {  // the factorisation of qei_tail_kernel
      const double x = Lrow[j];
      double dj = bcast(x, j);
      if (!(dj > 0.0)) {
        if (lane == 0) atomicCAS(info, 0, (int)(g % 2000000000) + 1);
        dj = 1.0;
      }
      const double sd = sqrt(dj);
      const double lij = lane == j ? sd : x / sd;
      const bool below = live && lane > j;
      if (live && lane >= j) Lrow[j] = lij;
      const double nl = -lij;
      for (int c = j + 1; c < n; ++c) {
        const double lcj = bcast(lij, c);
        if (below) Lrow[c] = fma(nl, lcj, Lrow[c]);
      }
      if (lane == j) {
        dg[j] = sd + 1e-12;  // utils.py:168, :183
        ig[j] = 1.0 / (sd + 1e-12);
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // from here on every lane reads every row
    // t / dg[j]: the reciprocal is wave-uniform, one residual step gives the quotient's last bit
    auto over = [&](double t, int j) {
      const double z = t * ig[j];
      return fma(fma(-z, dg[j], t), ig[j], z);
    };
    const double e0 = normal_cdf(over(xs[0], 0));
    double res;
    if (n == 1) {
      res = e0;  // (q = 2's inner CDFs: no Sobol point, utils.py:171 alone)
    } else {
      const double* __restrict__ const w = outer ? w1 : w2;  // [S][n]
      double acc = 0.0;
      for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool valid = s < S;
        const double* const ws = w + (int64_t)(valid ? s : 0) * n;
        double y[QP];
        double e = e0, f = e0;
#pragma unroll
        for (int r = 1; r < QP; ++r) {
          if (r < n) {  // (wave-uniform)
            y[r - 1] = normal_quantile_mid(1e-6 + (1.0 - 2e-6) * ws[r - 1] * e);
            const double* const Lr = Ls + r * ldq;
            double sum = 0.0;
#pragma unroll
            for (int c = 0; c < r; ++c) sum = fma(Lr[c], y[c], sum);
            e = normal_cdf(over(xs[r] - sum, r));
            f = e * f;
          }
        }
        if (valid) acc += f;
      }
      res = wave_sum(acc) / (double)S;
    }
    if (lane == 0) {
      if (outer) {
        term[pr] = (mu[i] - T) * res;
      } else {  // Sigma^(i)_ki times the density of N(m_ik, Sigma^(i)_kk) at b_ik (:1725-1730)
        const double sc = sqrt(sig(i, k, k)), z = dif(i, k) / sc;
        term[pr] = sig(i, k, i) * (0.3989422804014327 * exp(-0.5 * z * z) / sc) * res;
      }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");  // the next problem overwrites this wave's rows
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double v = 0.0;
    for (int i = 0; i < q; ++i) {
      double inner = 0.0;
      for (int k = 0; k < q; ++k) inner += term[q + i * q + k];
      v += term[i] + inner;
    }
    out[g] = v;
  }
}

template <int QP>
static void launch_bei_tail_qp(hipStream_t s, const double* mean, const double* cov, int64_t G, int q, const double* w1,
                               const double* w2, int S, double eta, double* out, int* info) {
  const size_t lds = (size_t)(q * q + q + q + q * q + BEI_WAVES * (q * (q | 1) + 3 * q)) * sizeof(double);
  hipLaunchKernelGGL(bei_tail_kernel<QP>, dim3((unsigned)G), dim3(64 * BEI_WAVES), lds, s, mean, cov, G, q, w1, w2, S, eta,
                     out, info);
}
void launch_bei_tail(hipStream_t s, const double* mean, const double* cov, int64_t G, int q, const double* w1,
                     const double* w2, int S, double eta, double* out, int* info) {
  if (q <= 4) launch_bei_tail_qp<4>(s, mean, cov, G, q, w1, w2, S, eta, out, info);
  else if (q <= 8) launch_bei_tail_qp<8>(s, mean, cov, G, q, w1, w2, S, eta, out, info);
  else launch_bei_tail_qp<BEI_MAX_Q>(s, mean, cov, G, q, w1, w2, S, eta, out, info);
}

}  // namespace tgp
