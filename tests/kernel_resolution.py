"""Bounds of the kernel-function comparisons (TEST INFRASTRUCTURE; tests/test_gpu_kernel_resolution.py compares the
device code with them, tests/test_oracle_tails.py the oracle).

Tolerance: |got - ref| <= eps (A + B s) |ref|, eps = 2^-52, s the argument of the exponential (r^2 / 2, r, sqrt(3) r,
sqrt(5) r).  Counted from the code path in units of eps (one rounding = eps / 2):
* scaled difference t = x/ls - X/ls: 1/2; t^2 carries 1; the d fused multiply-adds of the sum of squares 1/2 each on a
  positive sum: r^2 to (d + 2) / 2.  Only the three coordinates that differ count at d = 40 (the others add exact zeros).
* sqrt halves that and adds its claimed 2 ulp: r to (d + 2) / 4 + 2.  The constant sqrt(3) / sqrt(5) and its product: +1.
* exp at its claimed 2 ulp, its argument error amplified by s.  So
      B = (d + 2) / 2 (rbf: no sqrt, s = r^2 / 2 exactly),  (d + 2) / 4 + 2 (matern12),  (d + 2) / 4 + 3 (matern32 / 52)
  = 2.5, 3.25, 4.25, 4.25 at d = 3: all below the cap (d + 19) / 4 = 5.5.
* polynomial factor: (1 + s) inherits at most s's own relative error (d + 2) / 4 + 3 = 4.25 plus 1/2; for matern52 the
  weighted error (4.25 s + 3 s^2 / 3) / (1 + s + s^2 / 3) <= 3.25 plus two roundings; then the product with the
  exponential and with the variance (1), the exponential's 2:  A <= 4.75 + 1 + 2 = 7.75 (matern32), 7.25 (matern52),
  2.5 (rbf, matern12: the exponential's 2 and the product with the variance).
* the trajectory's short form (traj_shape): SCALE folded into q = SCALE r^2 (+1 before the sqrt), no constant product.
  traj_sqrt is v_rsq_f64 plus ONE coupled Goldschmidt step and no residual step: a seed error e leaves 3/2 e^2, and the
  instruction set guide gives v_rsq_f64 2^29 ulp (e = 2^-23), so 1.5 * 2^-46 = 96 eps, plus three roundings: 97.5 eps
  (tests/test_fast_math_restatement.py restates it).  B = (d + 4) / 2 = 3.5 (rbf: no sqrt),
  (d + 4) / 4 + 97.5 = 99.25 (Matern): this path alone is above (d + 19) / 4 -- on an MI355X its Matern kinds show
  8 eps s at s = 680, which one Goldschmidt step on that seed allows.  A as above.  Its dot-product form adds
  SCALE (d + 2) eps (|a| + |b|)^2 absolute on the exponent in centred coordinates -- zero here (N = 1: b = 0 and
  q = SCALE |a|^2 is the difference form).
* gradients: the same form relative to |dk/dx|_inf of the probe, dk/dx = 2 dk/dr^2 (x - X) / ls^2 (kernel_dr2 is libm's
  exp and sqrt on the same r^2, counted at the same 2 ulp).  The factor 2 t / ls and its product add 3/2 to
  dk/dr^2's own count: rbf -variance / 2 exp(-s): 2.5 + 1.5 = 4; matern12 -variance / 2 exp(-r) / r: 2.5, the
  divisor's own error (d + 2) / 4 + 2 = 3.25 (its s-proportional part is B's) and the division, 6.25 + 1.5 = 7.75; matern32
  -3/2 variance exp(-s): 3 + 1.5 = 4.5; matern52 -5/6 variance (1 + s) exp(-s): (1 + s) exp(-s) changes by
  s^2 / (1 + s) <= s times the relative error of s, which B s covers, leaving the addition's 1/2, the exponential's 2 and
  three products: 4 + 1.5 = 5.5.
* the dense sum adds 17 eps for the summation (17 positive terms, condition 1), each term weighted with its own s.
* the variance chain in the exact one-point design (N = 1, K + noise = 4, W = 1/2 and variance 1: var = 1 - k^2 / 4 >= 3/4,
  d var / dx = -k dk / 2), read through acq_value_grad("nlcb", 2): v = -(k - 2 sd), g_c = -dk_c + dvar_c / sd; with e_k = A + B s the
  count of k and e_d = A_GRAD + B s that of dk (relative to |dk|_inf), `nlcb2_tolerances`:
    C1 = k / 2 and Z = k / 4 are exact scalings; sum C1^2 is one fused product (1/2), the subtraction from 1 one rounding:
        d var = eps [k^2 / 2 e_k + k^2 / 8 + var / 2]
    sd = sqrt(var) at its claimed 2 ulp:  d sd = d var / (2 sd) + 2 eps sd;  2 sd is exact, the subtraction and the sign 1/2:
        d v = eps e_k k + 2 d sd + eps / 2 |v|
    dv/dvar = 2 / (2 sd): the division 1/2 and sd's own relative error;  dvar_c = -2 (k / 4) dk_c: Z's e_k, dk's e_d, one fused
    product (1/2);  g_c = -dk_c + dvar_c / sd: two products and an addition, at most 1 eps of each term:
        d g_c = eps e_d |dk|_inf (1 + k / (2 sd)) + |dvar_c| / sd (eps (e_k + 1) + d sd / sd) + eps (|dk_c| + |dvar_c| / sd)."""
import numpy as np


KINDS = ("rbf", "matern12", "matern32", "matern52")
D_EFF = 3   # coordinates in which probe and training point differ (also in the d = 40 copy)
A_COEF = dict(rbf=2.5, matern12=2.5, matern32=7.75, matern52=7.25)
A_GRAD = dict(rbf=4.0, matern12=7.75, matern32=4.5, matern52=5.5)
B_DIFF = dict(rbf=(D_EFF + 2) / 2, matern12=(D_EFF + 2) / 4 + 2, matern32=(D_EFF + 2) / 4 + 3, matern52=(D_EFF + 2) / 4 + 3)
TRAJ_SQRT = 97.5   # eps: 3/2 (2^-23)^2 + three roundings
B_TRAJ = dict(rbf=(D_EFF + 4) / 2, matern12=(D_EFF + 4) / 4 + TRAJ_SQRT, matern32=(D_EFF + 4) / 4 + TRAJ_SQRT,
              matern52=(D_EFF + 4) / 4 + TRAJ_SQRT)
# caps: A <= 8 and, for every path but the trajectory's Matern short form, B <= (d + 19) / 4
assert max(max(A_COEF.values()), max(A_GRAD.values())) <= 8.0
assert max(max(B_DIFF.values()), B_TRAJ["rbf"]) <= (D_EFF + 19) / 4


def nlcb2_tolerances(kind, B, k, s, dk):
    """(v, g, tol_v, tol_g) of acq_value_grad("nlcb", 2) in the exact one-point design from the goldens' k [M], s [M], dk [M, 3]:
    the closed form in long double and the tolerances counted in the module docstring (float64)."""
    LD = np.longdouble
    eps = 2.0 ** -52
    kl, dkl = np.asarray(k, dtype=LD), np.asarray(dk, dtype=LD)
    var = 1 - kl * kl / 4
    sd = np.sqrt(var)
    v = -(kl - 2 * sd)
    dvar = -(kl / 2)[:, None] * dkl
    g = -dkl + dvar / sd[:, None]
    k, s, dk, varf, sdf = (np.asarray(a, dtype=np.float64) for a in (k, s, dk, var, sd))
    e_k, e_d = A_COEF[kind] + B * s, A_GRAD[kind] + B * s
    d_var = eps * (k * k / 2 * e_k + k * k / 8 + varf / 2)
    d_sd = d_var / (2 * sdf) + 2 * eps * sdf
    tol_v = eps * e_k * k + 2 * d_sd + eps / 2 * np.abs(np.asarray(v, dtype=np.float64))
    advar = np.abs(np.asarray(dvar, dtype=np.float64)) / sdf[:, None]
    dk_inf = np.abs(dk).max(axis=1)
    tol_g = ((eps * e_d * dk_inf * (1 + k / (2 * sdf)))[:, None] + advar * (eps * (e_k + 1) + d_sd / sdf)[:, None]
             + eps * (np.abs(dk) + advar))
    return v, g, tol_v, tol_g
