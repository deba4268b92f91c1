"""Reference, models, regime bins and tolerances of the entropy-search tail tests (TEST INFRASTRUCTURE; used by
tests/test_entropy_regimes_conditions.py on the CPU and tests/test_gpu_entropy_regimes.py on the GPU).

MES and GIBBON are means over the min-value samples s of per-sample functions of gamma = (s - mean) / sd:
    f_MES(gamma)       = -gamma h / 2 - log Phi(-gamma),            h = phi(gamma) / Phi(-gamma)
    f_GIB(gamma, rho2) = -1/2 log(1 + rho2 h (gamma - h)),          rho2 = var / (var + noise)
A single sample plays the role tests/acq_regimes.py gives ``param``: gamma is that module's z, its five models, candidate
sets and parameter lists (``p.params``) are the sample lists here.  One model is added (``CONFIGS``): relative noise 1e-10 on
unit variance, whose near-data candidates (sd about 1e-5) put the same samples at gamma up to 4e6.

The reference is NOT the oracle: ``sample_terms`` is a float64 restatement of the mathematical functions that forms no
difference of two terms of size gamma^2, compared with 50-digit values in tests/test_entropy_regimes_conditions.py:
* gamma < 0: h = phi / (1 - Phi(gamma)) from erfc, log Phi(-gamma) = log1p(-Phi(gamma));
* 0 <= gamma <= 5: h = sqrt(2 / pi) / erfcx(gamma / sqrt 2), log Phi(-gamma) = log(erfcx / 2) - gamma^2 / 2;
* gamma > 5: Laplace's continued fraction h = gamma + delta, delta = 1 / (gamma + t_2), t_k = k / (gamma + t_{k+1}), 60
  levels by backward division; gamma delta = 1 - t_2 delta, so f_MES = -gamma delta / 2 + log(2 pi) / 2 + log h,
  w = 1 - h delta = delta (t_2 - delta) and delta^2 - w = delta^2 t_2 (t_3 - t_2);
* GIBBON through log1p(-rho2 h delta) where h delta < 1/2, else log((1 - rho2) + rho2 w) with 1 - rho2 = noise / (var + noise).

The tolerance of a value is 1e-5 |ref| plus the first-order sensitivity of the tail to 8 ulp of the moments it is evaluated at
(no absolute floor), that of a gradient row the one of ``acq_regimes.gradient_check``."""
import math

import numpy as np
from scipy.special import erfc, erfcx

from tests import acq_regimes as R
from tests.util import EPS

CONFIGS = [R._cfg("m52_d8_N200_noise1e-10", 8, "matern52", 200, 1e-10, 1.0, 0.2)]
ALL_CONFIGS = R.CONFIGS + CONFIGS
IDS = [c["name"] for c in ALL_CONFIGS]
NEW = CONFIGS[0]["name"]

G_BINS = ((-37.0, -20.0), (-20.0, -8.0), (-8.0, 8.0), (8.0, 20.0), (20.0, 37.0), (37.0, 1e3), (1e3, 1e5), (1e5, 1e8))
G_BIN_NAMES = ("[-37,-20)", "[-20,-8)", "[-8,8]", "(8,20]", "(20,37]", "(37,1e3]", "(1e3,1e5]", "(1e5,1e8]")
ACQS = ("mes", "gibbon")
GRAD_G = (-33.0, -25.0, -14.0, -7.0, 0.0, 5.0, 12.0, 25.0, 100.0, 1e4)
CLAMP_LB = 1e-8
_HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
_SQRT_2_PI = math.sqrt(2.0 / math.pi)
_U_CF, _LEVELS = 5.0, 60


def problem(name):
    return R.problem(next(c for c in ALL_CONFIGS if c["name"] == name))


def g_bin(g):
    """Index into G_BINS, -1 outside [-37, 1e8]; [-8, 8] is closed, the bins below are open above, those above open below."""
    g = np.asarray(g)
    out = np.full(g.shape, -1)
    for i, (lo, hi) in enumerate(G_BINS):
        if i < 2:
            out[(g >= lo) & (g < hi)] = i
        elif i == 2:
            out[(g >= lo) & (g <= hi)] = i
        else:
            out[(g > lo) & (g <= hi)] = i
    return out


def populated(p):
    """The (bin, sigma class) cells that must hold >= MIN_CELL asserted pairs.  The five models of tests/acq_regimes.py fill
    the six bins up to gamma = 1e3 in the near-data, interior and prior classes -- but for the prior class in (37, 1e3], which
    is empty in four of them (a sample 37 prior standard deviations above the prior mean is in no list) -- and the clipped
    class where the noise lies below the clip; the low-noise model fills every bin with near-data candidates."""
    cells = {(b, k) for b in range(6) for k in (1, 2, 3)} - {(5, 3)}
    if p.name == "m52_d8_N200_lownoise_tiny":
        cells |= {(b, 0) for b in range(6)}
    if p.name == NEW:
        cells |= {(6, 1), (7, 1)}
    return cells


# ---- the float64 reference --------------------------------------------------------------------------------------------
def _continued_fraction(u):
    """(delta, t_2, t_3 - t_2) of h = u + delta for u > 5, by backward division from t_61 = 0."""
    t = np.zeros_like(u)
    for k in range(_LEVELS, 3, -1):
        t = k / (u + t)
    t3 = 3.0 / (u + t)          # t = t_4
    t2 = 2.0 / (u + t3)
    return 1.0 / (u + t2), t2, t3 - t2


def sample_terms(gamma, rho2=None, one_minus_rho2=None):
    """dict of the per-sample functions at gamma (any shape; rho2 broadcasts): mes, dmes = d/dgamma, and with rho2 given
    gib, dgib = d/dgamma, dgib_drho2.  ``one_minus_rho2`` defaults to 1 - rho2 (exact in float64 for rho2 >= 1/2)."""
    u = np.asarray(gamma, dtype=np.float64)
    lo, cf = u < 0.0, u > _U_CF
    mid = ~lo & ~cf
    with np.errstate(all="ignore"):
        ul = np.where(lo, u, -1.0)
        hl = np.exp(-0.5 * ul * ul) / math.sqrt(2.0 * math.pi) / (0.5 * erfc(ul / math.sqrt(2.0)))
        ll = np.log1p(-0.5 * erfc(-ul / math.sqrt(2.0)))
        um = np.where(mid, u, 1.0)
        ex = erfcx(um / math.sqrt(2.0))
        hm = _SQRT_2_PI / ex
        lm = np.log(0.5 * ex) - 0.5 * um * um
        uc = np.where(cf, u, 10.0)
        delta_c, t2, t32 = _continued_fraction(uc)
    h = np.where(lo, hl, np.where(mid, hm, uc + delta_c))
    delta = np.where(cf, delta_c, h - u)
    hd = h * delta
    w = np.where(cf, delta_c * (t2 - delta_c), 1.0 - hd)
    hd = np.where(cf, 1.0 - w, hd)
    one_ud = np.where(cf, t2 * delta_c, 1.0 - u * delta)
    dhd = h * np.where(cf, delta_c * delta_c * t2 * t32, delta * delta - w)        # (h delta)'
    out = dict(mes=np.where(cf, -0.5 * uc * delta_c + _HALF_LOG_2PI + np.log(uc + delta_c),
                            -0.5 * u * h - np.where(lo, ll, lm)),
               dmes=0.5 * h * one_ud)
    if rho2 is not None:
        rho2 = np.asarray(rho2, dtype=np.float64)
        n1 = 1.0 - rho2 if one_minus_rho2 is None else np.asarray(one_minus_rho2, dtype=np.float64)
        inner = n1 + rho2 * w
        with np.errstate(all="ignore"):
            out["gib"] = np.where(hd < 0.5, -0.5 * np.log1p(-rho2 * np.minimum(hd, 0.5)), -0.5 * np.log(inner))
        out["dgib"] = 0.5 * rho2 * dhd / inner
        out["dgib_drho2"] = 0.5 * hd / inner
    return out


def gammas(samples, mean, var):
    """[M, S]"""
    sd = np.maximum(np.sqrt(var), CLAMP_LB)
    return (np.asarray(samples, dtype=np.float64).reshape(1, -1) - mean[:, None]) / sd[:, None]


def tails(p, acq, samples, mean, var):
    """The acquisition [M]: the mean over the samples of the per-sample reference."""
    g = gammas(samples, mean, var)
    if acq == "mes":
        return sample_terms(g)["mes"].mean(axis=1)
    den = var + p.noise
    return sample_terms(g, (var / den)[:, None], (p.noise / den)[:, None])["gib"].mean(axis=1)


def tail_coefficients(p, acq, samples, mean, var):
    """(d tail / d mean, d tail / d var) [M]: dgamma/dmean = -1 / sd, dgamma/dvar = -gamma / (2 var) (0 where sd is clamped),
    drho2/dvar = noise / (var + noise)^2."""
    g = gammas(samples, mean, var)
    sd = np.maximum(np.sqrt(var), CLAMP_LB)
    free = np.sqrt(var) > CLAMP_LB
    if acq == "mes":
        fu = sample_terms(g)["dmes"]
        return -fu.mean(axis=1) / sd, np.where(free, -(fu * g).mean(axis=1) / (2.0 * var), 0.0)
    den = var + p.noise
    t = sample_terms(g, (var / den)[:, None], (p.noise / den)[:, None])
    fu = t["dgib"]
    return (-fu.mean(axis=1) / sd,
            np.where(free, -(fu * g).mean(axis=1) / (2.0 * var), 0.0) + t["dgib_drho2"].mean(axis=1) * p.noise / den ** 2)


def sensitivity(p, acq, samples, mean, var):
    """First-order change of the tail under errors of 8 ulp in the moments."""
    a, b = tail_coefficients(p, acq, samples, mean, var)
    return np.abs(a) * 8.0 * EPS * np.abs(mean) + np.abs(b) * 8.0 * EPS * var


def value_check(p, acq, samples, got, mean, var, ref=None):
    """Compare one sweep's values with the reference at the moments given (``ref``: another function of the same moments, for
    the restated defects).  -> (err, tol, asserted mask, problems)."""
    got = np.asarray(got, dtype=np.float64)
    ref = tails(p, acq, samples, mean, var) if ref is None else ref
    what = f"{acq} S={np.size(samples)} s[0]={float(np.ravel(samples)[0])!r}"
    problems = []
    if not np.all(np.isfinite(got)):
        problems.append(f"{what}: non-finite values")
    asserted = np.abs(ref) >= R.TINY
    if np.any(np.abs(got[~asserted]) > R.TINY * (1.0 + R.RTOL)):
        problems.append(f"{what}: |value| above 1e-290 where the reference is below it")
    if np.any(got[asserted] < 0.0):
        problems.append(f"{what}: negative values")
    sens = sensitivity(p, acq, samples, mean, var)
    if np.any(sens[asserted] > 1e-6 * np.abs(ref[asserted])):
        problems.append(f"{what}: the sensitivity to the moments exceeds 1e-6 |ref|")
    tol = R.RTOL * np.abs(ref) + sens
    err = np.abs(got - ref)
    bad = asserted & ~(err <= tol)
    if np.any(bad):
        g = gammas(samples, mean, var)
        i = int(np.argmax(np.where(bad, err / tol, 0.0)))
        names = sorted({G_BIN_NAMES[b] for b in g_bin(g[bad]).ravel() if b >= 0})
        problems.append(f"{what}: {int(bad.sum())} candidates outside the tolerance, gamma in {', '.join(names)}; worst at {i}: "
                        f"gamma={g[i].min():.6g}..{g[i].max():.6g} sd={math.sqrt(var[i]):.3e} got={got[i]!r} ref={ref[i]!r}")
    return err, tol, asserted, problems


def cell_counts(p, acq, samples, mean, var):
    """[gamma-bin, sigma class] -> number of asserted (candidate, sample) pairs, one sample at a time."""
    cls = R.sigma_class(p, var)
    counts = np.zeros((len(G_BINS), len(R.SIGMA_CLASSES)), dtype=np.int64)
    for s in samples:
        ref = tails(p, acq, [s], mean, var)
        gb = g_bin(gammas([s], mean, var)[:, 0])
        ok = (np.abs(ref) >= R.TINY) & (gb >= 0)
        np.add.at(counts, (gb[ok], cls[ok]), 1)
    return counts


def assert_cells(p, acq, counts):
    for b, k in sorted(populated(p)):
        assert counts[b, k] >= R.MIN_CELL, (p.name, acq, G_BIN_NAMES[b], R.SIGMA_CLASSES[k], counts.tolist())


# ---- gradients ----------------------------------------------------------------------------------------------------------
def grad_samples(p, mean, var, j):
    """Samples of the gradient runs: ``GRAD_G`` at the far field's moments and at candidate j's."""
    return ([p.c + g * math.sqrt(p.variance) for g in GRAD_G]
            + [float(mean[j] + g * math.sqrt(var[j])) for g in GRAD_G])


def coefficient_partials(p, acq, samples, mean, var):
    """(|da/dmean|, |da/dvar|, |db/dmean|, |db/dvar|) of ``tail_coefficients`` by central differences over 1e-4 sd and
    1e-4 var (a shift of gamma by 1e-4 and 5e-5 |gamma|): the coefficients are smooth in gamma on that scale, and the term
    they feed is asserted to stay below a tenth of the tolerance, so two digits of these derivatives are enough."""
    dm, dv = 1e-4 * np.sqrt(var), 1e-4 * var
    am_p, bm_p = tail_coefficients(p, acq, samples, mean + dm, var)
    am_m, bm_m = tail_coefficients(p, acq, samples, mean - dm, var)
    av_p, bv_p = tail_coefficients(p, acq, samples, mean, var + dv)
    av_m, bv_m = tail_coefficients(p, acq, samples, mean, var - dv)
    return (np.abs(am_p - am_m) / (2.0 * dm), np.abs(av_p - av_m) / (2.0 * dv),
            np.abs(bm_p - bm_m) / (2.0 * dm), np.abs(bv_p - bv_m) / (2.0 * dv))


def gradient_check(p, acq, samples, grad, mean, var, dmean_dx, dvar_dx):
    """``acq_regimes.gradient_check`` (same row rule, same tolerance) with the chain rule's coefficients from the reference."""
    err, tol, rows, ref, problems = R.gradient_check(
        p, acq, float(np.ravel(samples)[0]), grad, mean, var, dmean_dx, dvar_dx,
        coefficients=tail_coefficients(p, acq, samples, mean, var),
        partials=coefficient_partials(p, acq, samples, mean, var))
    return err, tol, rows, ref, problems
