"""numpy / scipy restatements of the expected hypervolume improvement (TEST INFRASTRUCTURE).

``reference_form`` is the formula as the reference writes it (expected_hv_improvement.__call__,
acquisition/function/multi_objective.py:188-250): the problem negated to a maximisation, Psi and nu with ``1 - cdf``, the
clip of the negated lower bounds at 1e10, and the sum over the 2^P corner combinations gathered from the stacked
(Psi difference, nu) factors.  ``product_form`` is the same with the corner sum written as a product of sums;
``g_difference_form`` is the algebra the device kernel evaluates, sum_cells prod_j max(g_j(ub) - g_j(lb), 0) with
g_j(t) = E[(t - Y_j)^+]; ``scale`` is the size of what cancels in either, the yardstick of every comparison.

All take mean, var [M, P] and cell bounds lb, ub [K, P] and return [M]."""
from itertools import product

import numpy as np
from scipy.stats import norm


def _factors(mean, var, lb, ub):
    """(max(Psi(lb) - Psi(ub), 0), nu), each [M, K, P], in the reference's negated coordinates."""
    mean, var = np.asarray(mean, np.float64), np.asarray(var, np.float64)
    lb, ub = np.asarray(lb, np.float64), np.asarray(ub, np.float64)
    neg_mean, std = -mean[:, None, :], np.sqrt(var)[:, None, :]   # [M, 1, P]
    neg_lb, neg_ub = -ub[None], np.minimum(-lb[None], 1e10)       # [1, K, P]

    def Psi(a, b, m, s):
        return s * norm.pdf((b - m) / s) + (m - a) * (1 - norm.cdf((b - m) / s))

    def nu(lo, up, m, s):
        return (up - lo) * (1 - norm.cdf((up - m) / s))

    psi_ub = Psi(neg_lb, neg_ub, neg_mean, std)
    psi_lb = Psi(neg_lb, neg_lb, neg_mean, std)
    return np.maximum(psi_lb - psi_ub, 0.0), nu(neg_lb, neg_ub, neg_mean, std)


def reference_form(mean, var, lb, ub):
    psi, nu_ = _factors(mean, var, lb, ub)
    stacked = np.stack([psi, nu_], axis=-2)                        # [M, K, 2, P]
    P = stacked.shape[-1]
    cross = np.array(list(product(*[[0, 1]] * P)))                 # [2^P, P]
    combos = stacked[:, :, cross, np.arange(P)]                    # [M, K, 2^P, P]
    return np.sum(np.sum(np.prod(combos, axis=-1), axis=-1), axis=-1)


def product_form(mean, var, lb, ub):
    psi, nu_ = _factors(mean, var, lb, ub)
    return np.sum(np.prod(psi + nu_, axis=-1), axis=-1)


def _g(t, mean, std):
    z = (t - mean) / std
    return std * norm.pdf(z) + (t - mean) * norm.cdf(z)


def g_difference_form(mean, var, lb, ub):
    mean, std = np.asarray(mean, np.float64)[:, None, :], np.sqrt(np.asarray(var, np.float64))[:, None, :]
    lo = np.maximum(np.asarray(lb, np.float64), -1e10)[None]
    up = np.maximum(np.asarray(ub, np.float64), -1e10)[None]
    return np.sum(np.prod(np.maximum(_g(up, mean, std) - _g(lo, mean, std), 0.0), axis=-1), axis=-1)


def _s_terms(mean, var, lb, ub):
    """s_j(ub) + s_j(lb) [M, K, P], s_j(t) = sigma pdf(z) + |t - mu| cdf(z)."""
    mean, std = np.asarray(mean, np.float64)[:, None, :], np.sqrt(np.asarray(var, np.float64))[:, None, :]

    def s(t):
        t = np.maximum(np.asarray(t, np.float64), -1e10)[None]
        z = (t - mean) / std
        return std * norm.pdf(z) + np.abs(t - mean) * norm.cdf(z)

    return s(ub) + s(lb)


def scale(mean, var, lb, ub):
    """sum_cells prod_j (s_j(ub) + s_j(lb)), s_j(t) = sigma pdf(z) + |t - mu| cdf(z): the terms of g with their signs removed,
    inside each g and between the two."""
    return np.sum(np.prod(_s_terms(mean, var, lb, ub), axis=-1), axis=-1)


def hypervolume_improvement_2d(front, reference, y):
    """The hypervolume a point y adds to a two-objective front, for y [S, 2], by the staircase sum -- no cells involved:
    area([y, ref]) minus the area of the union of the boxes [max(y, f_i), ref] over the front sorted by its first
    objective."""
    front = np.asarray(front, np.float64)
    front = front[np.argsort(front[:, 0])]
    ref = np.asarray(reference, np.float64)
    y = np.minimum(np.asarray(y, np.float64), ref)                  # beyond the reference point nothing is added
    p = np.minimum(np.maximum(front[None], y[:, None, :]), ref)     # [S, F, 2]: x ascending, y descending along F
    prev = np.concatenate([np.full((y.shape[0], 1), ref[1]), p[:, :-1, 1]], axis=1)
    union = np.sum((ref[0] - p[:, :, 0]) * (prev - p[:, :, 1]), axis=1)
    return np.prod(ref - y, axis=-1) - union


def within_sigmas_of_front(mean, var, front, k=4.0):
    """[M] bool: no front point dominates the candidate's mean by more than k posterior standard deviations in every
    objective -- the regime where the reference's ``1 - cdf`` still carries the value."""
    shifted = np.asarray(mean)[:, None, :] - k * np.sqrt(np.asarray(var))[:, None, :]
    return ~np.any(np.all(np.asarray(front)[None] <= shifted, axis=-1), axis=-1)


def reference_rounding_floor(mean, ub):
    """sum_cells prod_j |mu_j - ub_j|.  The reference forms every factor from ``1 - cdf`` times (mu_j - ub_j) in its negated
    coordinates, and that difference is rounded to an ulp of ONE however small it is: the reference's float64 error is a few
    eps of this sum whatever the value is.  It depends on the geometry alone -- not on the variances, the values or ``scale``."""
    mean_ = np.asarray(mean, np.float64)[:, None, :]
    return np.sum(np.prod(np.abs(mean_ - np.asarray(ub, np.float64)[None]), axis=-1), axis=-1)


def random_moments(rng, front, reference, M, lb, ub):
    """(mean, var, kept fraction): M candidates on which the reference's formula is a yardstick at a few eps of ``scale``.  Drawn:
    a uniform point of [min front - 0.2, reference] that no front point dominates, moved up by at most one posterior
    standard deviation per objective, var log-uniform in [1e-6, 1].  Kept: those whose reference_rounding_floor -- the
    reference's own absolute rounding, the one stated cause -- is at most twice their scale; a narrow marginal just inside
    the top of a large cell has a small scale and a floor the size of the cell, and there a comparison relative to ``scale``
    would measure the reference form, not the candidate (of the dropped draws under 1 % actually exceed the tolerance, the
    worst by 6e-12 of the scale; the goldens hold the kernel there).  The fraction kept is returned so that a test can show
    it.  None is in the tail: no front point dominates a mean by more than four standard deviations."""
    front, reference = np.asarray(front, np.float64), np.asarray(reference, np.float64)
    low = front.min(axis=0) - 0.2
    means, variances = np.empty((0, front.shape[1])), np.empty((0, front.shape[1]))
    drawn = kept = 0
    for _ in range(200):
        cand = rng.uniform(low, reference, size=(4 * M, front.shape[1]))
        cand = cand[~np.any(np.all(front[None] <= cand[:, None, :], axis=-1), axis=-1)]
        var = 10.0 ** rng.uniform(-6.0, 0.0, size=cand.shape)
        mean = cand + rng.uniform(0.0, 1.0, size=cand.shape) * np.sqrt(var)
        keep = reference_rounding_floor(mean, ub) <= 2.0 * scale(mean, var, lb, ub)
        drawn, kept = drawn + len(keep), kept + int(keep.sum())
        means, variances = np.concatenate([means, mean[keep]])[:M], np.concatenate([variances, var[keep]])[:M]
        if len(means) == M:
            break
    assert len(means) == M and np.all(within_sigmas_of_front(means, variances, front))
    return means, variances, kept / drawn
