// Analytic multi-point expected improvement (Chevalier & Ginsbourger) with Genz's sequential-conditioning estimator of
// the multivariate normal CDF on fixed Sobol points, for gfx950:
//   BatchExpectedImprovement / batch_expected_improvement (reference function.py:1189-1805) + MultivariateNormalCDF
//   (function/utils.py:29-199).
#include "tgp_dev.hpp"
#include "tgp_internal.hpp"
#include "tgp_tail_dev.hpp"

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
// factorises it with wave_chol_rows, as qei_tail_kernel does (pivot and multiplier through v_readlane, no barrier); then every
// lane walks the chain of its sample (utils.py:166-197): y_0..y_{n-2} in registers (loops unrolled to QP), C_ij as LDS broadcast
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
    wave_chol_rows(Lrow, live, lane, n, g, info, [&](int j, double sd) {
      if (lane == j) {
        dg[j] = sd + 1e-12;  // utils.py:168, :183
        ig[j] = 1.0 / (sd + 1e-12);
      }
    });
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

// ---------------------------------------------------------------------------------------------
// The value AND its adjoints w.r.t. (mean, cov): the forward tail above, problem for problem (the same wave_chol_rows; same
// build, chain, sums), and behind every problem its reverse pass, all inside the wave that owns it:
//   chain     per sample, steps n-1 .. 0: e_r's adjoint = (prefix product)(suffix product) + ybar_r (1 - 2e-6) w_r / phi(y_r)
//             [(Phi^-1)' = 1 / phi(y)], t_r's = ebar_r phi(t_r), through t_r = (x_r - sum_c C_rc y_c) / (C_rr + 1e-12) to xbar_r,
//             Cbar_rc, Cbar_rr and ybar_c.  Prefix products, not f / e_r: an e_r may underflow to zero.
//   sums      xbar [n] and Cbar [n (n + 1) / 2] over the samples.  QP <= 8: per-lane accumulators (the lane's samples in order),
//             one butterfly per entry and problem.  QP = 16: 136 + 16 accumulators (304 registers) next to the chain's 80 doubles of
//             state do not fit the register file, so every entry is reduced over the wave per 64-sample chunk and lane 0 adds the chunks in order.
//   factor    Abar = C^-T sym(Phi(C^T Cbar)) C^-1: chol_adjoint, as in qei_grad_tail_kernel (lane c owns column c / row c).
//   problem   back through R^(i,k) = Sigma_uv - Sigma_ku Sigma_kv / Sigma_kk, c^(i,k) = d_u - d_k Sigma_ku / Sigma_kk and the
//             weight Sigma_ki N(d_k; 0, Sigma_kk) (or mu_i - T) to the adjoints of Sigma^(i) [q][q] and d^(i) [q], and from
//             there (rows by lane, row and column sums) into THIS WAVE's accumulators of cov's and mu's adjoints.
// A wave meets its problems in index order and the four waves' accumulators are added in wave order by one thread per entry:
// no floating-point atomics, the same bits from every call.  Every matrix adjoint is taken of the formula as written (which reads
// cov as a full matrix); the output is its symmetric part -- the adjoint for symmetric perturbations, which is what
// tgp_joint_vjp takes.  zero_clipped: a diagonal entry of cov at the posterior's floor (VAR_FLOOR) gets zero (the clip's adjoint).
template <int QP>
__global__ __launch_bounds__(64 * BEI_WAVES) void bei_grad_tail_kernel(const double* __restrict__ mean,
                                                                       const double* __restrict__ cov, int64_t G, int q,
                                                                       const double* __restrict__ w1,
                                                                       const double* __restrict__ w2, int S, double eta,
                                                                       int zero_clipped, double* __restrict__ val,
                                                                       double* __restrict__ gmean, double* __restrict__ gcov,
                                                                       int* __restrict__ info) {
  extern __shared__ double bei_lds[];
  constexpr bool IN_REGS = QP <= 8;
  constexpr int NACC = IN_REGS ? QP * (QP + 1) / 2 : 1;
  constexpr int NXACC = IN_REGS ? QP : 1;
  const int64_t g = blockIdx.x;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ldq = q | 1;
  const int nprob = q + q * q;
  const int per_wave = 3 * q * ldq + 6 * q + q * q + q;
  double* const cv = bei_lds;            // [q][q]: cov + 1e-6 I
  double* const mu = cv + q * q;         // [q]: -mean
  double* const term = mu + q;           // [q + q^2]
  double* const Ls = term + nprob + wave * per_wave;   // the factor C [n][ldq]
  double* const Ms = Ls + q * ldq;       // [n][ldq]: Cbar (lower) -> Abar (symmetric)
  double* const Sb = Ms + q * ldq;       // [q][ldq]: the adjoint of Sigma^(i) of an inner problem
  double* const xs = Sb + q * ldq;       // [q] the limits
  double* const dg = xs + q;             // [q] C_rr + 1e-12
  double* const ig = dg + q;             // [q] its inverse
  double* const xb = ig + q;             // [q] the limits' adjoint
  double* const db = xb + q;             // [q] the adjoint of d^(i) of an inner problem
  double* const rho = db + q;            // [q] Sigma_ku / Sigma_kk of the kept indices
  double* const cvb = rho + q;           // [q][q]: this wave's sum of cov's adjoint
  double* const mub = cvb + q * q;       // [q]: of mu's
  for (int t = threadIdx.x; t < q * q; t += 64 * BEI_WAVES)
    cv[t] = cov[g * q * q + t] + (t / q == t % q ? 1e-6 : 0.0);
  if ((int)threadIdx.x < q) mu[threadIdx.x] = -mean[g * q + threadIdx.x];
  for (int t = lane; t < q * q + q; t += 64) cvb[t] = 0.0;   // (cvb and mub are contiguous)
  __syncthreads();
  const double T = -eta;
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
  auto wfence = [] { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); };
  for (int pr = wave; pr < nprob; pr += BEI_WAVES) {  // (wave-uniform)
    const bool outer = pr < q;
    const int i = outer ? pr : (pr - q) / q;
    const int k = outer ? -1 : (pr - q) % q;
    const int n = outer ? q : q - 1;
    const bool live = lane < n;
    const int u = lane + ((!outer && lane >= k) ? 1 : 0);   // this lane's index in 0..q-1 (live lanes)
    double* const Lrow = Ls + (live ? lane : 0) * ldq;
    double* const Mrow = Ms + (live ? lane : 0) * ldq;
    if (live) {
      if (outer) {
        for (int c = 0; c < n; ++c) Lrow[c] = sig(i, u, c) + (c == lane ? 1e-6 : 0.0);
        xs[lane] = dif(i, u);
      } else {
        const double skk = sig(i, k, k), sku = sig(i, k, u);
        for (int c = 0; c < n; ++c) {
          const int v = c + (c >= k ? 1 : 0);
          Lrow[c] = (sig(i, u, v) - sku * sig(i, k, v) / skk) + (c == lane ? 1e-6 : 0.0);
        }
        xs[lane] = dif(i, u) - dif(i, k) * (sku / skk);
        rho[lane] = sku / skk;
      }
      for (int c = 0; c < n; ++c) Mrow[c] = 0.0;
      xb[lane] = 0.0;
    }
    wave_chol_rows(Lrow, live, lane, n, g, info, [&](int j, double sd) {
      if (lane == j) {
        dg[j] = sd + 1e-12;
        ig[j] = 1.0 / (sd + 1e-12);
      }
    });
    wfence();
    auto over = [&](double t, int j) {
      const double z = t * ig[j];
      return fma(fma(-z, dg[j], t), ig[j], z);
    };
    const double t0 = over(xs[0], 0);
    const double e0 = normal_cdf(t0);
    double res;
    if (n == 1) {
      res = e0;
      if (lane == 0) {
        const double xr = normal_pdf(t0) * ig[0];
        xb[0] = xr;
        Ms[0] = -xr * t0;
      }
    } else {
      const double* __restrict__ const w = outer ? w1 : w2;  // [S][n]
      double acc = 0.0;
      double Cb[NACC], Xb[NXACC];
#pragma unroll
      for (int a = 0; a < NACC; ++a) Cb[a] = 0.0;
#pragma unroll
      for (int a = 0; a < NXACC; ++a) Xb[a] = 0.0;
      for (int s0 = 0; s0 < S; s0 += 64) {
        const int s = s0 + lane;
        const bool valid = s < S;
        const double* const ws = w + (int64_t)(valid ? s : 0) * n;
        double y[QP], tt[QP], ee[QP], pf[QP], yb[QP];
        double e = e0, f = e0;
        tt[0] = t0;
        ee[0] = e0;
        pf[0] = 1.0;
#pragma unroll
        for (int r = 1; r < QP; ++r) {
          yb[r - 1] = 0.0;
          if (r < n) {  // (wave-uniform)
            y[r - 1] = normal_quantile_mid(1e-6 + (1.0 - 2e-6) * ws[r - 1] * e);
            const double* const Lr = Ls + r * ldq;
            double sum = 0.0;
#pragma unroll
            for (int c = 0; c < r; ++c) sum = fma(Lr[c], y[c], sum);
            pf[r] = f;
            tt[r] = over(xs[r] - sum, r);
            e = normal_cdf(tt[r]);
            ee[r] = e;
            f = e * f;
          }
        }
        if (valid) acc += f;
        const double on = valid ? 1.0 : 0.0;
        double sf = on;   // the product of the e's behind step r (zero on a lane without a sample)
#pragma unroll
        for (int r = QP - 1; r >= 0; --r) {
          if (r < n) {  // (wave-uniform)
            double eb = pf[r] * sf;
            if (r < n - 1) eb = fma(yb[r], (1.0 - 2e-6) * ws[r] / normal_pdf(y[r]), eb);
            const double xr = eb * normal_pdf(tt[r]) * ig[r];   // the adjoint of x_r (and minus that of the row's sum)
            const double* const Lr = Ls + r * ldq;
            if constexpr (IN_REGS) {
              Xb[r] += xr;
              Cb[r * (r + 1) / 2 + r] = fma(-xr, tt[r], Cb[r * (r + 1) / 2 + r]);
#pragma unroll
              for (int c = 0; c < r; ++c) Cb[r * (r + 1) / 2 + c] = fma(-xr, y[c], Cb[r * (r + 1) / 2 + c]);
            } else {
              const double sx = wave_sum(xr), sd_ = wave_sum(-xr * tt[r]);
              if (lane == 0) {
                xb[r] += sx;
                Ms[r * ldq + r] += sd_;
              }
#pragma unroll
              for (int c = 0; c < r; ++c) {
                const double sc = wave_sum(-xr * y[c]);
                if (lane == 0) Ms[r * ldq + c] += sc;
              }
            }
#pragma unroll
            for (int c = 0; c < r; ++c) yb[c] = fma(-xr, Lr[c], yb[c]);
            sf *= ee[r];
          }
        }
      }
      res = wave_sum(acc) / (double)S;
      if constexpr (IN_REGS) {
#pragma unroll
        for (int r = 0; r < QP; ++r) {
          if (r < n) {
            const double sx = wave_sum(Xb[r]);
            if (lane == 0) xb[r] = sx;
#pragma unroll
            for (int c = 0; c <= r; ++c) {
              const double sc = wave_sum(Cb[r * (r + 1) / 2 + c]);
              if (lane == 0) Ms[r * ldq + c] = sc;
            }
          }
        }
      }
    }
    // the weight of this problem in the sum, the term, and the weight's adjoint pieces
    double wgt, pdf = 0.0, skk = 1.0, dk = 0.0, ski = 0.0;
    if (outer) {
      wgt = mu[i] - T;
    } else {
      skk = sig(i, k, k);
      dk = dif(i, k);
      ski = sig(i, k, i);
      const double sc = sqrt(skk), z = dk / sc;
      pdf = 0.3989422804014327 * exp(-0.5 * z * z) / sc;
      wgt = ski * pdf;
    }
    if (lane == 0) term[pr] = outer ? (mu[i] - T) * res : ski * pdf * res;
    wfence();
    const double scale = n == 1 ? wgt : wgt / (double)S;
    if (live) {
      for (int c = 0; c <= lane; ++c) Mrow[c] *= scale;
      xb[lane] *= scale;
    }
    wfence();
    // the factor's adjoint, lane = column: Q = tril(C^T Cbar) / 2 in place, mirrored, C^-T from the left, C^-1 from the right
    chol_adjoint(Ls, Ms, ldq, n, lane, live, wfence);
    wfence();
    // back through the problem's construction to the adjoints of Sigma^(i) (Sp) and d^(i) (dp)
    const double* Sp = Ms;
    const double* dp = xb;
    double mu_i_extra = 0.0;   // what the weight adds to mu_i's adjoint
    if (outer) {
      mu_i_extra = res;
    } else {
      // lane b: h_b = sum_a Abar_ba rho_a; row u(b) of Sp = row b of Abar spread over the kept columns, column k zero
      double hb = 0.0, kk = 0.0, dkb = 0.0;
      if (live) {
        for (int a = 0; a < n; ++a) hb = fma(Mrow[a], rho[a], hb);
        double* const Srow = Sb + u * ldq;
        for (int a = 0; a < n; ++a) Srow[a + (a >= k ? 1 : 0)] = Mrow[a];
        Srow[k] = 0.0;
        const double xbl = xb[lane];
        Sb[k * ldq + u] = -2.0 * hb - xbl * dk / skk;
        kk = (hb + xbl * dk / skk) * rho[lane];
        dkb = -xbl * rho[lane];
        db[u] = xbl;
      }
      kk = wave_sum(kk);
      dkb = wave_sum(dkb);
      const double z2 = dk * dk / skk;
      const double pdfbar = res * ski;   // the weight is Sigma_ki pdf: its adjoint is res
      if (lane == 0) {
        Sb[k * ldq + k] = kk + pdfbar * pdf * (z2 - 1.0) / (2.0 * skk);
        db[k] = dkb - pdfbar * pdf * dk / skk;
      }
      wfence();
      if (lane == 0) Sb[k * ldq + i] += res * pdf;
      wfence();
      Sp = Sb;
      dp = db;
    }
    {  // Sigma^(i)_jk = [j != i][k != i] cv_jk - [j != i] cv_ji - [k != i] cv_ik + cv_ii;  d_j = mu_i - mu_j (+ delta_ij (mu_i - T))
      double rs = 0.0, cs = 0.0, dj = 0.0;
      if (lane < q) {
        for (int c = 0; c < q; ++c) {
          rs += Sp[lane * ldq + c];
          cs += Sp[c * ldq + lane];
        }
        dj = dp[lane];
        if (lane != i) {
          for (int c = 0; c < q; ++c)
            if (c != i) cvb[lane * q + c] += Sp[lane * ldq + c];
          cvb[lane * q + i] -= rs;
          cvb[i * q + lane] -= cs;
          mub[lane] -= dj;
        }
      }
      const double tot = wave_sum(rs), dtot = wave_sum(dj);
      if (lane == i) {
        cvb[i * q + i] += tot;
        mub[i] += dtot + mu_i_extra;
      }
    }
    wfence();  // the next problem overwrites this wave's rows
  }
  __syncthreads();
  const int stride = per_wave;
  const double* const cvb0 = term + nprob + 3 * q * ldq + 6 * q;   // wave 0's accumulators
  for (int t = threadIdx.x; t < q * q; t += 64 * BEI_WAVES) {
    const int r = t / q, c = t % q;
    double a = 0.0;
    for (int wv = 0; wv < BEI_WAVES; ++wv) a += cvb0[wv * stride + r * q + c] + cvb0[wv * stride + c * q + r];
    a *= 0.5;
    if (zero_clipped && r == c && !(cov[g * q * q + t] > VAR_FLOOR)) a = 0.0;
    gcov[g * q * q + t] = a;
  }
  if ((int)threadIdx.x < q) {
    double a = 0.0;
    for (int wv = 0; wv < BEI_WAVES; ++wv) a += cvb0[wv * stride + q * q + threadIdx.x];
    gmean[g * q + threadIdx.x] = -a;
  }
  if (threadIdx.x == 0) {
    double v = 0.0;
    for (int i = 0; i < q; ++i) {
      double inner = 0.0;
      for (int k = 0; k < q; ++k) inner += term[q + i * q + k];
      v += term[i] + inner;
    }
    val[g] = v;
  }
}

size_t bei_grad_tail_lds_bytes(int q) {
  return (size_t)(q * q + q + q + q * q + BEI_WAVES * (3 * q * (q | 1) + 6 * q + q * q + q)) * sizeof(double);
}
template <int QP>
static void launch_bei_grad_tail_qp(hipStream_t s, const double* mean, const double* cov, int64_t G, int q, const double* w1,
                                    const double* w2, int S, double eta, int zero_clipped, double* val, double* gmean,
                                    double* gcov, int* info) {
  hipLaunchKernelGGL(bei_grad_tail_kernel<QP>, dim3((unsigned)G), dim3(64 * BEI_WAVES), bei_grad_tail_lds_bytes(q), s, mean, cov,
                     G, q, w1, w2, S, eta, zero_clipped, val, gmean, gcov, info);
}
void launch_bei_grad_tail(hipStream_t s, const double* mean, const double* cov, int64_t G, int q, const double* w1,
                          const double* w2, int S, double eta, int zero_clipped, double* val, double* gmean, double* gcov,
                          int* info) {
  if (q <= 4) launch_bei_grad_tail_qp<4>(s, mean, cov, G, q, w1, w2, S, eta, zero_clipped, val, gmean, gcov, info);
  else if (q <= 8) launch_bei_grad_tail_qp<8>(s, mean, cov, G, q, w1, w2, S, eta, zero_clipped, val, gmean, gcov, info);
  else launch_bei_grad_tail_qp<BEI_MAX_Q>(s, mean, cov, G, q, w1, w2, S, eta, zero_clipped, val, gmean, gcov, info);
}

}  // namespace tgp
