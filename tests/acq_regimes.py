"""Models, parameter lists, regime bins and tolerances of the acquisition-tail tests (TEST INFRASTRUCTURE; used by
tests/test_acq_regimes_conditions.py on the CPU; the comparison of the engine's tails on the GPU builds on it).

A candidate's regime is z = (param - mean) / sd and its sigma class.  ``param`` is free, so one model and one candidate set
reach every regime through a list of parameters:
* eta + t sd(Y) for 33 values of t from -40 to 40;
* c + z sqrt(variance) for the 18 values ``Z_GRID`` (three per z-bin): exact for far-field candidates (mean c, variance
  sigma^2);
* mean_j + z sd_j on the same grid for four representative candidates of each other sigma class (their neighbours in mean
  fall into the bins next to them).

The tolerance of a value is 1e-5 |ref| plus the first-order sensitivity of the tail to 8 ulp of the moments it is evaluated
at (``sensitivity``): no absolute floor.  A gradient row is compared in the same way (``gradient_check``): against the chain
rule at the same moments, at 1e-5 of the row's largest component plus the sensitivity of the chain rule's coefficients to
8 ulp of the moments."""
import functools
import math

import numpy as np

from oracle import gp_oracle as O
from tests.util import EPS, cancellation_floor

RTOL = 1e-5
TINY = 1e-290                 # below it a reference value is not compared relatively
M = 2100
Z_BINS = ((-37.0, -30.0), (-30.0, -20.0), (-20.0, -10.0), (-10.0, -3.0), (-3.0, 3.0), (3.0, 37.0))
Z_BIN_NAMES = ("[-37,-30)", "[-30,-20)", "[-20,-10)", "[-10,-3)", "[-3,3]", "(3,37]")
Z_GRID = (-35.5, -33.0, -31.0, -28.0, -25.0, -21.0, -18.0, -14.0, -11.0, -8.0, -5.0, -3.5, -2.0, 0.0, 2.0, 4.0, 12.0, 30.0)
SIGMA_CLASSES = ("clipped", "near-data", "interior", "prior")
BETAS = (-3.0, 0.0, 1.96, 10.0)   # -LCB: mean - beta sd stays at 27 sqrt(variance) or more (c = 37.5 sqrt(variance)): no cancellation
MIN_CELL = 20


def _cfg(name, d, kind, N, rel_noise, variance, ls_scale):
    return dict(name=name, d=d, kind=kind, N=N, rel_noise=rel_noise, variance=variance, ls_scale=ls_scale)


CONFIGS = [
    _cfg("m52_d8_N300", 8, "matern52", 300, 1e-2, 1.0, 0.2),                # the DMA sweep
    _cfg("m52_d8_N200_lownoise_tiny", 8, "matern52", 200, 1e-5, 3.7e-9, 0.2),  # noise below the 1e-12 clip: the clipped class
    _cfg("rbf_d2_N100_tiny", 2, "rbf", 100, 1e-2, 3.7e-9, 0.06),
    _cfg("m32_d24_N257_huge", 24, "matern32", 257, 1e-2, 4.1e7, 0.3),       # dp = 32: the register-staged sweep
    _cfg("m12_d40_N130", 40, "matern12", 130, 1e-2, 1.0, 0.4),              # the wide form
]
IDS = [c["name"] for c in CONFIGS]


class P:
    """One configuration's problem."""


def problem(cfg):
    """The problem of a configuration: a name from ``CONFIGS``, or a configuration of another module's list (``_cfg``)."""
    if isinstance(cfg, str):
        cfg = next(c for c in CONFIGS if c["name"] == cfg)
    return _problem(tuple(cfg.items()))


@functools.lru_cache(maxsize=None)
def _problem(items):
    cfg = dict(items)
    name, d, N = cfg["name"], cfg["d"], cfg["N"]
    rng = np.random.default_rng(4321)
    X = rng.uniform(size=(N, d))
    f = O.ackley(X)
    p = P()
    p.cfg, p.name, p.d, p.N, p.kind = cfg, name, d, N, cfg["kind"]
    p.variance, p.noise = cfg["variance"], cfg["rel_noise"] * cfg["variance"]
    p.c = 37.5 * math.sqrt(p.variance)
    p.X = X
    p.Y = math.sqrt(p.variance) * (f - f.mean()) / f.std() + p.c
    p.ls = cfg["ls_scale"] * np.sqrt(d) * rng.permutation(np.geomspace(0.5, 2.0, d))
    Xq = rng.uniform(size=(M, d))
    Xq[:40] = X[:40]                                       # exactly at training inputs
    Xq[40:60] = X[40:60] + 1e-6                            # next to them
    Xq[60:120] = X[(60 + np.arange(60)) % N] + 0.02 * rng.uniform(-1.0, 1.0, size=(60, d))   # a fraction of a lengthscale away
    Xq[130] = Xq[131]                                       # a duplicate (ties -> first index)
    Xq[-40:] = 200.0 + rng.uniform(size=(40, d))           # far field: every kernel value underflows
    p.Xq = np.ascontiguousarray(Xq)
    with O.difference_form():
        p.st = O.gpr_update(p.kind, p.variance, p.ls, p.noise, p.c, X, p.Y)
        p.om, p.ov = O.predict(p.st, p.Xq)
        p.eta = O.eta_min_mean(p.st)
    p.floor = cancellation_floor(N, p.variance, p.noise)
    p.params = parameters(p, p.om, p.ov)
    return p


def sigma_class(p, var):
    """0 clipped at 1e-12, 1 near-data (sd < 0.3 sqrt(variance)), 2 interior, 3 prior (sd >= 0.999 sqrt(variance))."""
    rel = np.sqrt(var / p.variance)
    return np.where(var <= O.VAR_FLOOR, 0, np.where(rel < 0.3, 1, np.where(rel < 0.999, 2, 3)))


def z_bin(z):
    """Index into Z_BINS, -1 outside [-37, 37]; [-3, 3] is closed, (3, 37] open below."""
    z = np.asarray(z)
    out = np.full(z.shape, -1)
    for i, (lo, hi) in enumerate(Z_BINS):
        if i < 4:
            out[(z >= lo) & (z < hi)] = i
        elif i == 4:
            out[(z >= lo) & (z <= hi)] = i
        else:
            out[(z > lo) & (z <= hi)] = i
    return out


def parameters(p, mean, var):
    """The parameter list of the EI / PI / AEI runs (see the module docstring), sorted, on the moments given."""
    sd = np.sqrt(var)
    out = [p.eta + t * float(np.std(p.Y)) for t in np.linspace(-40.0, 40.0, 33)]
    out += [p.c + z * math.sqrt(p.variance) for z in Z_GRID]
    cls = sigma_class(p, var)
    for k in (0, 1, 2):
        idx = np.flatnonzero(cls == k)
        if idx.size == 0:
            continue
        order = idx[np.argsort(mean[idx])]
        for j in order[np.linspace(0, order.size - 1, 4).astype(int)]:
            out += [float(mean[j] + z * sd[j]) for z in Z_GRID]
    return np.array(sorted(set(out)))


def tails(p, acq, param, mean, var):
    if acq == "ei":
        return O.expected_improvement(mean, var, param)
    if acq == "pi":
        return O.probability_of_improvement(mean, var, param)
    if acq == "aei":
        return O.augmented_expected_improvement(mean, var, param, p.noise)
    return O.negative_lower_confidence_bound(mean, var, param)


def tail_partials(p, acq, param, mean, var):
    """(|d tail / d mean|, |d tail / d var|) of the oracle's tails."""
    sd = np.sqrt(var)
    if acq == "nlcb":
        return np.ones_like(mean), np.abs(param) / (2.0 * sd)
    z = (param - mean) / sd
    cdf, pdf = O.normal_cdf(z), O.normal_pdf(z)
    if acq == "pi":
        return pdf / sd, pdf * np.abs(z) / (2.0 * var)
    dmu, dvar = cdf, pdf / (2.0 * sd)
    if acq == "ei":
        return dmu, dvar
    ei = (param - mean) * cdf + sd * pdf
    sn, st = math.sqrt(p.noise), np.sqrt(p.noise + var)
    aug, daug = 1.0 - sn / st, 0.5 * sn / (st * (p.noise + var))
    return dmu * aug, dvar * aug + np.abs(ei) * daug


def sensitivity(p, acq, param, mean, var, dmean=None, dvar=None):
    """First-order change of the tail under errors of 8 ulp in the moments (or the errors given)."""
    pm, pv = tail_partials(p, acq, param, mean, var)
    dmean = 8.0 * EPS * np.abs(mean) if dmean is None else dmean
    dvar = 8.0 * EPS * var if dvar is None else dvar
    return pm * dmean + pv * dvar


def value_check(p, acq, param, got, mean, var):
    """Compare one sweep's values with the oracle's tail at the moments given.  -> (err, tol, asserted mask, z, problems)."""
    got = np.asarray(got, dtype=np.float64)
    ref = tails(p, acq, param, mean, var)
    problems = []
    if not np.all(np.isfinite(got)):
        problems.append(f"{acq} param={param!r}: non-finite values")
    asserted = np.abs(ref) >= TINY
    z = (param - mean) / np.sqrt(var) if acq != "nlcb" else np.zeros_like(mean)
    small = ~asserted
    if np.any(np.abs(got[small]) > TINY * (1.0 + RTOL)):
        problems.append(f"{acq} param={param!r}: |value| above 1e-290 where the reference underflows")
    sens = sensitivity(p, acq, param, mean, var)
    if np.any(sens[asserted] > 1e-6 * np.abs(ref[asserted])):
        problems.append(f"{acq} param={param!r}: the sensitivity to the moments exceeds 1e-6 |ref|")
    tol = RTOL * np.abs(ref) + sens
    err = np.abs(got - ref)
    if acq != "nlcb" and np.any(got[asserted] < 0.0):
        problems.append(f"{acq} param={param!r}: negative values")
    bad = asserted & ~(err <= tol)
    if np.any(bad):
        i = int(np.argmax(np.where(bad, err / tol, 0.0)))
        problems.append(f"{acq} param={param!r}: {int(bad.sum())} candidates outside the tolerance; worst at {i}: z={z[i]:.3f} "
                        f"sd={math.sqrt(var[i]):.3e} got={got[i]!r} ref={ref[i]!r}")
    return err, tol, asserted, z, problems


def cell_counts(p, acq, params, mean, var):
    """[z-bin, sigma class] -> number of asserted (candidate, parameter) pairs."""
    cls = sigma_class(p, var)
    counts = np.zeros((len(Z_BINS), len(SIGMA_CLASSES)), dtype=np.int64)
    for param in params:
        ref = tails(p, acq, param, mean, var)
        zb = z_bin((param - mean) / np.sqrt(var))
        ok = (np.abs(ref) >= TINY) & (zb >= 0)
        np.add.at(counts, (zb[ok], cls[ok]), 1)
    return counts


def deep_tail(p, mean, var):
    """(parameter, candidate indices) of the arg-max tests: at param = c - 24 sqrt(variance) the far-field candidates sit at
    z = -24 (forty equal values: the tie goes to the first) and the candidates with -35 <= z <= -22 have EI, PI and AEI below
    1e-100 but normal; the others (small sd: z far below -37) would underflow and are left out of this candidate set."""
    param = p.c - 24.0 * math.sqrt(p.variance)
    z = (param - mean) / np.sqrt(var)
    return param, np.flatnonzero((z >= -35.0) & (z <= -22.0))


GRAD_Z = (-33.0, -25.0, -14.0, -5.0, 0.0, 12.0)   # gradient runs: param = c + z sqrt(variance) and mean_j + z sd_j of one near-data j


def grad_subset(p):
    """300 candidates of the gradient runs: at / next to / near training inputs, interior, far field."""
    return np.concatenate([np.arange(0, 140), np.arange(1000, 1120), np.arange(M - 40, M)])


def grad_coefficients(p, acq, param, mean, var):
    """(a, b) with grad = a dmean + b dvar -- the chain rule of the oracle's ``acq_value_and_grad``."""
    sd = np.sqrt(var)
    if acq == "nlcb":
        return -np.ones_like(mean), param / (2.0 * sd)
    z = (param - mean) / sd
    cdf, pdf = O.normal_cdf(z), O.normal_pdf(z)
    if acq == "pi":
        return -pdf / sd, -pdf * z / (2.0 * var)
    if acq == "ei":
        return -cdf, pdf / (2.0 * sd)
    ei = (param - mean) * cdf + sd * pdf
    sn, st = math.sqrt(p.noise), np.sqrt(p.noise + var)
    aug, daug = 1.0 - sn / st, 0.5 * sn / (st * (p.noise + var))
    return -cdf * aug, pdf / (2.0 * sd) * aug + ei * daug


def moment_gradients(p, Xs):
    """(d mean / dx, d var / dx) [P, d] of the oracle, recovered from two -LCB gradients (beta = 0 and 2):
    grad(-LCB) = -dmean + beta / (2 sd) dvar."""
    _, g0 = O.acq_value_and_grad(p.st, "nlcb", 0.0, Xs)
    _, g2 = O.acq_value_and_grad(p.st, "nlcb", 2.0, Xs)
    with O.difference_form():
        _, var = O.predict(p.st, Xs)
    return -g0, (g2 - g0) * np.sqrt(var)[:, None]


def grad_params(p, mean, var, j):
    """Parameters of the gradient runs: ``GRAD_Z`` at the far field's moments and at candidate j's."""
    return ([p.c + z * math.sqrt(p.variance) for z in GRAD_Z]
            + [float(mean[j] + z * math.sqrt(var[j])) for z in GRAD_Z])


def grad_rows(p, var):
    """Candidates whose gradient is compared: sd >= 0.05 sqrt(variance)."""
    return np.sqrt(var) >= 0.05 * math.sqrt(p.variance)


def coefficient_partials(p, acq, param, mean, var):
    """(|da/dmean|, |da/dvar|, |db/dmean|, |db/dvar|) of ``grad_coefficients`` (upper bounds where terms are summed).
    With z = (param - mean) / sd: dz/dmean = -1 / sd, dz/dvar = -z / (2 var), Phi' = phi, phi' = -z phi."""
    sd = np.sqrt(var)
    if acq == "nlcb":
        zero = np.zeros_like(mean)
        return zero, zero, zero, np.abs(param) / (4.0 * sd * var)
    z = (param - mean) / sd
    cdf, pdf = O.normal_cdf(z), O.normal_pdf(z)
    az = np.abs(z)
    if acq == "pi":      # a = -phi / sd, b = -phi z / (2 var)
        return (pdf * az / var, pdf * np.abs(z * z - 1.0) / (2.0 * sd * var),
                pdf * np.abs(z * z - 1.0) / (2.0 * sd * var), pdf * az * np.abs(z * z - 3.0) / (4.0 * var * var))
    # EI: a = -Phi, b = phi / (2 sd)
    am, av = pdf / sd, pdf * az / (2.0 * var)
    bm, bv = pdf * az / (2.0 * var), pdf * np.abs(z * z - 1.0) / (4.0 * sd * var)
    if acq == "ei":
        return am, av, bm, bv
    # AEI: a = a_ei aug, b = b_ei aug + ei daug; aug = 1 - sqrt(noise / (noise + var))
    ei = np.abs((param - mean) * cdf + sd * pdf)
    sn, st = math.sqrt(p.noise), np.sqrt(p.noise + var)
    aug, daug = 1.0 - sn / st, 0.5 * sn / (st * (p.noise + var))
    d2aug = 0.75 * sn / (st * (p.noise + var) ** 2)
    return (am * aug, av * aug + cdf * daug,
            bm * aug + cdf * daug, bv * aug + 2.0 * pdf / (2.0 * sd) * daug + ei * d2aug)


def gradient_check(p, acq, param, grad, mean, var, dmean_dx, dvar_dx, coefficients=None, partials=None):
    """Compare gradients [P, d] with the chain rule at the moments given: ref = a dmean/dx + b dvar/dx with (a, b) from
    ``grad_coefficients`` at (mean, var) (or ``coefficients``, with their ``partials`` in the order of
    ``coefficient_partials``: another module's tails) and the oracle's moment gradients.  Per row, the tolerance is 1e-5 |ref|_inf
    plus the first-order change of (a, b) under 8 ulp of the moments; that term must stay below 1e-6 |ref|_inf.  Rows with
    sd < 0.05 sqrt(variance) are not compared; rows whose reference gradient is below 1e-290 must be finite and below 1e-290
    themselves.  -> (err, tol, asserted rows, ref, problems)."""
    grad = np.asarray(grad, dtype=np.float64)
    a, b = grad_coefficients(p, acq, param, mean, var) if coefficients is None else coefficients
    ref = a[:, None] * dmean_dx + b[:, None] * dvar_dx
    am, av, bm, bv = coefficient_partials(p, acq, param, mean, var) if partials is None else partials
    dm, dv = 8.0 * EPS * np.abs(mean), 8.0 * EPS * var
    sens = (am * dm + av * dv)[:, None] * np.abs(dmean_dx) + (bm * dm + bv * dv)[:, None] * np.abs(dvar_dx)
    scale = np.abs(ref).max(axis=1)
    wide = grad_rows(p, var)
    rows = wide & (scale >= TINY)
    problems = []
    if not np.all(np.isfinite(grad)):
        problems.append(f"{acq} param={param!r}: non-finite gradient")
        return np.abs(grad - ref), sens, rows, ref, problems
    small = wide & ~rows
    if np.any(np.abs(grad[small]) > TINY * (1.0 + RTOL)):
        problems.append(f"{acq} param={param!r}: gradient above 1e-290 where the reference underflows")
    if np.any(sens[rows].max(axis=1, initial=0.0) > 1e-6 * scale[rows]):
        problems.append(f"{acq} param={param!r}: the gradient's sensitivity to the moments exceeds 1e-6 |grad ref|_inf")
    tol = RTOL * scale[:, None] + sens
    err = np.abs(grad - ref)
    bad = rows[:, None] & ~(err <= tol)
    if np.any(bad):
        r = np.where(bad, err / np.where(tol > 0.0, tol, 1e-320), 0.0)
        i = int(np.argmax(r.max(axis=1)))
        problems.append(f"{acq} param={param!r}: {int(bad.any(axis=1).sum())} gradient rows outside the tolerance, worst "
                        f"x{r.max():.3g} at {i} (z={(param - mean[i]) / math.sqrt(var[i]):.2f} sd={math.sqrt(var[i]):.3e}): "
                        f"got {grad[i][:3]} ref {ref[i][:3]}")
    return err, tol, rows, ref, problems
