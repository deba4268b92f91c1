"""numpy restatements of the batch Monte-Carlo expected hypervolume improvement (TEST INFRASTRUCTURE).

``reference_form`` is the loop as the reference writes it (batch_ehvi.acquisition, acquisition/function/
multi_objective.py:366-410): for j = 1..B the C(B, j) subsets of the batch gathered from the samples, their overlap vertex
(the maximum over the subset), the maximum with every cell's lower bound, the lengths max(ub - vertex, 0), their product over
the objectives, summed over subsets and cells, with the sign (-1)^(j+1), averaged over the samples.  ``abs_terms`` is the
same sum with every sign positive: the scale of what cancels.  ``exact_union`` is the hypervolume improvement of the q points
of ONE sample in exact rational arithmetic, by coordinate compression: no cells, no inclusion-exclusion.
``value_from_moments`` is the value from given joint moments: numpy's Cholesky factor, the samples, ``reference_form``."""
from fractions import Fraction
from itertools import combinations, product

import numpy as np


def _signed_terms(samples, lb, ub, signed):
    samples = np.asarray(samples, np.float64)                       # [..., S, B, P]
    lb_points, ub_points = np.asarray(lb, np.float64), np.asarray(ub, np.float64)
    batch_size = samples.shape[-2]
    indices = list(range(batch_size))
    q_subset_indices = [list(combinations(indices, i)) for i in range(1, batch_size + 1)]
    hv_contrib = np.zeros(samples.shape[:-2])

    def hv_contrib_on_samples(obj_samples):                         # [..., S, Cq_j, j, P]
        overlap_vertices = np.max(obj_samples, axis=-2)             # [..., S, Cq_j, P]
        overlap_vertices = np.maximum(np.expand_dims(overlap_vertices, -3),
                                      lb_points[None, None, :, None, :])   # [..., S, K, Cq_j, P]
        lengths_j = np.maximum(ub_points[None, None, :, None, :] - overlap_vertices, 0.0)
        areas_j = np.sum(np.prod(lengths_j, axis=-1), axis=-1)      # [..., S, K]
        return np.sum(areas_j, axis=-1)                             # [..., S]

    for j in range(1, batch_size + 1):
        q_choose_j = np.array(q_subset_indices[j - 1])              # [Cq_j, j]
        j_sub_samples = np.take(samples, q_choose_j, axis=-2)       # [..., S, Cq_j, j, P]
        sign = float((-1) ** (j + 1)) if signed else 1.0
        hv_contrib = hv_contrib + sign * hv_contrib_on_samples(j_sub_samples)
    return np.mean(hv_contrib, axis=-1)


def reference_form(samples, lb, ub):
    """samples [..., S, B, P], cell bounds lb, ub [K, P] -> [...]."""
    samples = np.asarray(samples, np.float64)
    if samples.ndim == 3:
        return _signed_terms(samples[None], lb, ub, True)[0]
    return _signed_terms(samples, lb, ub, True)


def abs_terms(samples, lb, ub):
    """The sum of ``reference_form`` with every term's sign positive."""
    samples = np.asarray(samples, np.float64)
    if samples.ndim == 3:
        return _signed_terms(samples[None], lb, ub, False)[0]
    return _signed_terms(samples, lb, ub, False)


def exact_union(sample_points, front, ref):
    """The hypervolume (up to ``ref``) that the points ``sample_points`` [q, P] dominate and no point of ``front`` [F, P]
    does, as a Fraction: every coordinate of points, front and reference point taken exactly, the space cut into the grid
    boxes between consecutive coordinates per objective, a box counted when some sample point and no front point lies at or
    below its lower corner."""
    pts = [[Fraction(float(v)) for v in p] for p in np.asarray(sample_points, np.float64)]
    frt = [[Fraction(float(v)) for v in p] for p in np.asarray(front, np.float64).reshape(-1, len(pts[0]))]
    rf = [Fraction(float(v)) for v in np.asarray(ref, np.float64)]
    P = len(rf)
    axes = []
    for j in range(P):
        values = sorted({v for v in [p[j] for p in pts] + [f[j] for f in frt] if v < rf[j]} | {rf[j]})
        axes.append(values)
    total = Fraction(0)
    for corner in product(*[range(len(a) - 1) for a in axes]):
        low = [axes[j][corner[j]] for j in range(P)]
        if any(all(f[j] <= low[j] for j in range(P)) for f in frt):
            continue
        if any(all(p[j] <= low[j] for j in range(P)) for p in pts):
            vol = Fraction(1)
            for j in range(P):
                vol *= axes[j][corner[j] + 1] - axes[j][corner[j]]
            total += vol
    return total


def samples_from_moments(mean, cov, eps, jitter):
    """mean [P, G, q], cov [P, G, q, q] objective-major, eps [P, q, S] -> samples [G, S, q, P]."""
    mean, cov, eps = np.asarray(mean, np.float64), np.asarray(cov, np.float64), np.asarray(eps, np.float64)
    q = mean.shape[-1]
    L = np.linalg.cholesky(cov + jitter * np.eye(q))               # [P, G, q, q]
    y = mean[..., None] + np.einsum("pgim,pms->pgis", L, eps)      # [P, G, q, S]
    return np.ascontiguousarray(np.transpose(y, (1, 3, 2, 0)))


def value_from_moments(mean, cov, eps, jitter, lb, ub):
    """The value the device computes from the same inputs -> [G]."""
    return reference_form(samples_from_moments(mean, cov, eps, jitter), lb, ub)


def abs_terms_from_moments(mean, cov, eps, jitter, lb, ub):
    return abs_terms(samples_from_moments(mean, cov, eps, jitter), lb, ub)
