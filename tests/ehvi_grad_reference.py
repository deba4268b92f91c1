"""numpy / scipy restatement of the gradient of the expected hypervolume improvement with respect to the moments (TEST
INFRASTRUCTURE), in the form the device kernel evaluates (tests/ehvi_reference.py ``g_difference_form``):

    EHVI = sum_cells prod_j D_j,   D_j = max(g_j(u_j) - g_j(l_j), 0),   g_j(t) = s_j pdf(z) + (t - m_j) cdf(z),  z = (t - m_j) / s_j

Since pdf' = -z pdf the z terms cancel: d g / d m = -cdf(z), d g / d s = pdf(z), hence

    d EHVI / d m_j = -sum_cells (prod_{i != j} D_i) (cdf(z_u) - cdf(z_l))
    d EHVI / d v_j = (1 / (2 s_j)) sum_cells (prod_{i != j} D_i) (pdf(z_u) - pdf(z_l))

An objective of a cell whose factor the max clipped to zero contributes no derivative (the derivative of the function as
computed).  The scales are the same sums with the signs of their terms removed: the yardsticks of every comparison.

All take mean, var [M, P] and cell bounds lb, ub [K, P] and return two [M, P] arrays."""
import numpy as np
from scipy.stats import norm

from tests.ehvi_reference import _s_terms


def _z(mean, var, bound):
    mean, std = np.asarray(mean, np.float64)[:, None, :], np.sqrt(np.asarray(var, np.float64))[:, None, :]
    t = np.maximum(np.asarray(bound, np.float64), -1e10)[None]
    return t, (t - mean) / std, mean, std


def _leave_one_out(f):
    """[M, K, P] -> [M, K, P]: the product over the last axis of all entries but the j-th, without a division."""
    P = f.shape[-1]
    return np.stack([np.prod(np.delete(f, j, axis=-1), axis=-1) for j in range(P)], axis=-1)


def g_difference_grad(mean, var, lb, ub):
    """(d EHVI / d mean, d EHVI / d var), each [M, P]."""
    tu, zu, m, s = _z(mean, var, ub)
    tl, zl, _, _ = _z(mean, var, lb)
    cu, cl, pu, pl = norm.cdf(zu), norm.cdf(zl), norm.pdf(zu), norm.pdf(zl)
    d = (s * pu + (tu - m) * cu) - (s * pl + (tl - m) * cl)          # [M, K, P]
    active = d > 0.0
    loo = _leave_one_out(np.where(active, d, 0.0))
    gmean = -np.sum(loo * np.where(active, cu - cl, 0.0), axis=1)
    gstd = np.sum(loo * np.where(active, pu - pl, 0.0), axis=1)
    return gmean, gstd / (2.0 * s[:, 0, :])


def grad_scales(mean, var, lb, ub):
    """(scale_m, scale_v), each [M, P]: scale_m[j] = sum_cells prod_{i != j} S_i (cdf(z_u) + cdf(z_l)), scale_v[j] =
    sum_cells prod_{i != j} S_i (pdf(z_u) + pdf(z_l)) / (2 s_j), S_i = s_i(u) + s_i(l) as in ``ehvi_reference._s_terms``."""
    _, zu, _, s = _z(mean, var, ub)
    _, zl, _, _ = _z(mean, var, lb)
    loo = _leave_one_out(_s_terms(mean, var, lb, ub))
    scale_m = np.sum(loo * (norm.cdf(zu) + norm.cdf(zl)), axis=1)
    scale_v = np.sum(loo * (norm.pdf(zu) + norm.pdf(zl)), axis=1) / (2.0 * s[:, 0, :])
    return scale_m, scale_v
