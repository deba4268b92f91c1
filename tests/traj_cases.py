"""The RFF phase of the trajectory kernel at its own resolution (TEST INFRASTRUCTURE, numpy only; tests/test_traj_cases.py
checks it on the CPU, tests/test_gpu_trajectories.py compares the device with it).

An RFF-weight trajectory (tgp_traj_create_rff, no canonical part) with mean_const = 0 evaluates
    f_b(x) = sum_f s theta_fb cos(sum_c (x_c / ls_c) W_fc + b_f),   s = sqrt(2 variance / F),
in csrc/tgp_kernels_traj.hip traj_eval_kernel as sum_f ws_fb traj_cos_halfturns(y_f) with the phase in HALF TURNS,
y_f = arg_f / pi + 1/2, cos(arg) = sin(pi y).  The reference is exact: tests/golden/traj_phase_goldens.json holds every
cos(arg_f) of a case in mpmath (as a double and its remainder) on the exact doubles x, ls, W, b, and s the same way; the
weights theta are DATA (read back from the device) and the sum over f is taken in rational arithmetic (`rff_errors`).

The bound (`rff_bound`), term by term from the code, with u = 2^-53 one rounding:
* xq_c = x_c / ls_c in the kernel: one rounding, u |x_c / ls_c|.
* Wh_fc = W_fc * INV_PI on the host (tgp_api.hip): INV_PI is the double next to 1 / pi (u) and the product rounds (u): 2 u.
  So every product x_c W_fc / (ls_c pi) the kernel forms carries 3 u of itself.
* bh_f = b_f * INV_PI + 1/2: 2 u |b_f| / pi as above, and the sum rounds, u (|b_f| / pi + 1/2).
* arg = fma(xq_c, Wh_fc, arg), c = 0 .. d - 1 (the padded columns add exact zeros): d roundings of partial sums, each at
  most u A_f with A_f = sum_c |x_c W_fc / (ls_c pi)| + |b_f| / pi + 1/2.
  Together |dy_f| <= (3 + d) u A_f to first order; (d + 4) u A_f leaves one u A_f for the second-order terms.
* sin(pi y) has slope at most pi: pi |dy_f| on the cosine.  n = rint(y) and f = y - n are exact (|f| <= 1/2 is a multiple
  of the last place of y).
* the polynomial f P(f^2) of traj_cos_halfturns: POLY_ABS_ERR = 2 * 2^-52 absolute, asserted on the CPU restatement against
  mpmath in tests/test_traj_cases.py (its worst case there is recorded in that test) -- not measured on the device.
  So the phase value errs by e_f = pi (d + 4) u A_f + POLY_ABS_ERR.
* ws_fb = s theta_fb on the device (theta_tail_kernel) with s = sqrt(2 variance / F) on the host: the division rounds (u), the
  square root halves that and rounds (u), the product rounds (u): 3 u |s theta_fb| at most.
* acc_b = fma(ph_f, ws_fb, acc_b), F roundings of partial sums each at most u sum_f |ws_fb| (|ph| <= 1).  mean_const = 0 adds
  an exact zero.
      |df_b(x)| <= sum_f |s theta_fb| (e_f(x) + (F + 3) u)        (times 1 + 2^-20: the bound's own float64 evaluation)
Nothing in it is fitted to what the device returns."""
from __future__ import annotations

import json
import math
import os
from fractions import Fraction

import numpy as np

U = 2.0 ** -53
INV_PI = 0.31830988618379067154            # the constant of tgp_api.hip
COEFFS = (7.697847275590284e-07, -2.1903499125519212e-05, 0.00046629981702308817, -0.007370430506093225,
          0.08214588657312355, -0.599264529318946, 2.5501640398773007, -5.167712780049969, 3.141592653589793)
POLY_ABS_ERR = 2.0 * 2.0 ** -52
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj_phase_goldens.json")

REGIMES = ("small", "typical", "far")
DIMS = (1, 8)
FEATURES = (1, 24)
M_POINTS = 4
VARIANCE = 1.7
KIND = "matern52"


def load_goldens():
    with open(GOLDEN) as f:
        return json.load(f)


def case_inputs(regime: str, d: int, F: int):
    """The float64 inputs of one case: (x [M, d], ls [d], W [F, d], b [F], lo).  ``small``: |arg| < 1; ``typical``: the
    spectral draws of the sampler on the unit box with the default lengthscales; ``far``: the box [1024, 1025]^d with
    lengthscale 0.05, |arg| ~ 1e5."""
    from trieste_amd.sampler import sample_rff_basis

    rng = np.random.default_rng([REGIMES.index(regime), d, F, 20260101])
    W, b = sample_rff_basis(KIND, F, d, rng)
    lo = 0.0
    ls = np.full(d, 0.2 * math.sqrt(d))
    if regime == "small":
        W = 0.4 * ls * np.tanh(W) / d        # |sum_c (x_c / ls_c) W_fc| < 0.4
        b = rng.uniform(0.0, 0.5, size=F)
    elif regime == "far":
        lo, ls = 1024.0, np.full(d, 0.05)
    x = lo + rng.uniform(size=(M_POINTS, d))
    return x, ls, np.ascontiguousarray(W), b, lo


# ---- the kernel's arithmetic restated: every fused multiply-add with one rounding --------------------------------------------------
def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))   # int / int division rounds correctly


def halfturn_cos(y, coeffs=COEFFS, parity=True):
    """traj_cos_halfturns: sin(pi y) = (-1)^n sin(pi f), n = rint(y), f = y - n, f P(f^2).  ``parity=False`` drops the sign."""
    n = float(round(y))                    # round half to even, as rint
    f = y - n
    if parity and int(n) & 1:              # the kernel moves bit 0 of (int) n onto the sign of f
        f = -f
    z = f * f
    p = coeffs[0]
    for c in coeffs[1:]:
        p = fma(p, z, c)
    return f * p


def rff_restated(x, ls, W, b, theta, variance, coeffs=COEFFS, parity=True, half=0.5):
    """The device's value [M, B] of an RFF-weight trajectory with mean_const = 0 (host preparation of tgp_traj_create_rff, then
    traj_eval_kernel).  ``coeffs``, ``parity``, ``half`` plant a defect."""
    x, W, theta = np.asarray(x, float), np.asarray(W, float), np.asarray(theta, float)
    F, d = W.shape
    ws = math.sqrt(2.0 * variance / F) * theta
    Wh = W * INV_PI
    bh = np.asarray(b, float) * INV_PI + half
    out = np.zeros((x.shape[0], theta.shape[1]))
    for j in range(x.shape[0]):
        xq = x[j] / ls
        for f in range(F):
            arg = float(bh[f])
            for c in range(d):
                arg = fma(float(xq[c]), float(Wh[f, c]), arg)
            ph = halfturn_cos(arg, coeffs, parity)
            for bb in range(theta.shape[1]):
                out[j, bb] = fma(ph, float(ws[f, bb]), float(out[j, bb]))
    return out


def rff_bound(x, ls, W, b, theta, variance):
    """|device - exact| <= this, [M, B]: the module docstring, term by term."""
    x, W, theta = np.asarray(x, float), np.asarray(W, float), np.asarray(theta, float)
    F, d = W.shape
    A = (np.abs(x / ls) @ np.abs(W).T + np.abs(b)) / math.pi + 0.5          # [M, F]
    e = math.pi * (d + 4) * U * A + POLY_ABS_ERR
    S = np.abs(math.sqrt(2.0 * variance / F) * theta)                       # [F, B]
    return (1.0 + 2.0 ** -20) * ((e + (F + 3) * U) @ S)


def _frac(hilo):
    return Fraction(hilo[0]) + Fraction(hilo[1])


def rff_errors(got, cos_hilo, scale_hilo, theta):
    """|got - sum_f s theta_fb cos_f| [M, B] with the sum in rational arithmetic: cos_hilo [M][F][2] and scale_hilo [2] are
    the golden's pairs, theta [F, B] the exact doubles."""
    got, theta = np.asarray(got, float), np.asarray(theta, float)
    s = _frac(scale_hilo)
    th = [[Fraction(float(v)) for v in row] for row in theta]
    err = np.empty(got.shape)
    for j in range(got.shape[0]):
        cs = [_frac(c) for c in cos_hilo[j]]
        for bb in range(got.shape[1]):
            want = s * sum(cs[f] * th[f][bb] for f in range(len(cs)))
            err[j, bb] = float(abs(Fraction(float(got[j, bb])) - want))
    return err
