"""numpy / scipy restatement of the reference's analytic multi-point expected improvement, on given moments and Sobol
points: ``batch_expected_improvement`` (trieste/acquisition/function/function.py:1315-1805) and ``MultivariateNormalCDF``
(trieste/acquisition/function/utils.py:109-199).  Test infrastructure: the yardstick of the GPU tests, never imported by
the package.  Every function names the reference lines it follows; arrays carry the reference's shapes (B q-batches of Q
points), so the restatement holds [B * Q * Q, S, Q] values: callers chunk B.
"""
from __future__ import annotations

import numpy as np
from scipy.special import ndtr, ndtri

CALL_JITTER = 1e-6  # function.py:1776-1783 (hard-coded; the builder's jitter argument is never applied)
CDF_JITTER = 1e-6   # utils.py:114 (the default of MultivariateNormalCDF.__call__, which the caller never overrides)


def mvn_cdf(x, cov, w, jitter: float = CDF_JITTER):
    """utils.py:142-197 with mean 0: x [P, n], cov [P, n, n], w [S, >= n - 1] Sobol points -> [P]."""
    x = np.asarray(x, dtype=np.float64)
    P, n = x.shape
    C = np.linalg.cholesky(cov + jitter * np.eye(n)[None])                   # :143-144
    S = w.shape[0]
    e = np.broadcast_to(ndtr(x[:, None, 0] / (C[:, None, 0, 0] + 1e-12)), (P, S))   # :167-173
    f = e
    y = np.zeros((P, S, max(n - 1, 0)))
    for i in range(1, n):                                                    # :175-195
        y[:, :, i - 1] = ndtri(1e-6 + (1 - 2e-6) * w[None, :, i - 1] * e)    # :177
        tot = np.sum(C[:, None, i, :i] * y[:, :, :i], axis=-1)               # :190
        e = ndtr((x[:, None, i] - tot) / (C[:, None, i, i] + 1e-12))
        f = e * f                                                            # :194
    return np.mean(f, axis=-1)                                               # :197


def compute_bm(mean, threshold):
    """function.py:1343-1352: b [B, Q, Q] = -diag(T), m_ij = mean_j - mean_i - delta_ij mean_i."""
    B, Q = mean.shape
    eye = np.eye(Q)[None]
    b = -threshold[:, None, None] * eye
    m = mean[:, None, :] - mean[:, :, None]
    m = m - mean[:, :, None] * eye
    return b, m


def compute_sigma(cov):
    """function.py:1411-1432: Sigma[b, i, j, k] = cov_jk [j != i][k != i] - cov_ji [j != i] - cov_ik [k != i] + cov_ii."""
    B, Q, _ = cov.shape
    out = np.empty((B, Q, Q, Q))
    for i in range(Q):
        dj = np.ones((Q, 1))
        dj[i] = 0.0
        dk = dj.T
        out[:, i] = cov * dj * dk - cov[:, :, i:i + 1] * dj - cov[:, i:i + 1, :] * dk + cov[:, i:i + 1, i:i + 1]
    return out


def compute_c_R(diff, Sigma):
    """function.py:1520-1534 and 1554-1587 on diff [P, Q] = b - m and Sigma [P, Q, Q] (P = B * Q):
    c [P, Q, Q - 1], R [P, Q, Q - 1, Q - 1], the pivot's own index removed."""
    P, Q = diff.shape
    diag = np.diagonal(Sigma, axis1=-2, axis2=-1)                            # [P, Q]
    ratio = Sigma / diag[:, :, None]
    c_full = diff[:, None, :] - diff[:, :, None] * ratio                     # [P, k, j]
    R_full = Sigma[:, None, :, :] - Sigma[:, :, :, None] * Sigma[:, :, None, :] / diag[:, :, None, None]   # [P, k, u, v]
    c = np.empty((P, Q, Q - 1))
    R = np.empty((P, Q, Q - 1, Q - 1))
    for k in range(Q):
        keep = [j for j in range(Q) if j != k]
        c[:, k] = c_full[:, k][:, keep]
        R[:, k] = R_full[:, k][:, keep][:, :, keep]
    return c, R


def batch_ei_parts(mean, cov, eta, w1, w2):
    """function.py:1651-1745 behind the preamble of ``__call__`` (:1772-1803): mean [B, Q] and cov [B, Q, Q] as the model
    returns them, eta a scalar, w1 [S, Q], w2 [S, Q - 1] ->
    (value [B], p [B, Q], Phi [B, Q, Q], terms [B, Q + Q * Q] = the summands of the value)."""
    mean = np.asarray(mean, dtype=np.float64)
    cov = np.asarray(cov, dtype=np.float64)
    B, Q = mean.shape
    if Q < 2:
        raise ValueError("the reference refuses Q = 1 (MultivariateNormalCDF(dim=0), utils.py:51)")
    cov = cov + CALL_JITTER * np.eye(Q)[None]                                # :1776-1783
    mean = -mean                                                             # :1798
    T = np.full(B, -float(eta))                                              # :1785, :1800
    b, m = compute_bm(mean, T)
    Sigma = compute_sigma(cov)                                               # [B, Q, Q, Q]
    diff = (b - m).reshape(B * Q, Q)                                         # :1480, :1521
    Sig_r = Sigma.reshape(B * Q, Q, Q)
    p = mvn_cdf(diff, Sig_r, w1).reshape(B, Q)                               # :1482-1488
    c, R = compute_c_R(diff, Sig_r)
    if Q == 2:   # dimension one: utils.py:167-173 alone, no Sobol point
        Phi = mvn_cdf(c.reshape(B * Q * Q, 1), R.reshape(B * Q * Q, 1, 1), np.zeros((1, 0)))
    else:
        Phi = mvn_cdf(c.reshape(B * Q * Q, Q - 1), R.reshape(B * Q * Q, Q - 1, Q - 1), w2)
    Phi = Phi.reshape(B, Q, Q)                                               # :1647
    S_diag = np.diagonal(Sigma, axis1=-2, axis2=-1)                          # [B, i, k] = Sigma^(i)_kk        (:1725)
    scale = S_diag ** 0.5
    z = (b - m) / scale
    pdf = np.exp(-0.5 * z * z) / (scale * np.sqrt(2.0 * np.pi))              # :1726-1727
    idx = np.arange(Q)
    Sigma_diag = Sigma[:, idx, :, idx].transpose(1, 0, 2)                    # [B, i, k] = Sigma^(i)_ki        (:1729-1730)
    outer = (mean - T[:, None]) * p                                          # :1734
    inner = Sigma_diag * pdf * Phi                                           # :1737-1740
    value = np.sum(outer + np.sum(inner, axis=2), axis=1)                    # :1743
    terms = np.concatenate([outer, inner.reshape(B, Q * Q)], axis=1)
    return value, p, Phi, terms


def batch_ei(mean, cov, eta, w1, w2, chunk: int = 0):
    """The value alone, [B]; ``chunk`` q-batches at a time (0: a chunk that keeps the [chunk * Q * Q, S, Q] arrays near 64 MB)."""
    mean = np.asarray(mean, dtype=np.float64)
    B, Q = mean.shape
    if chunk <= 0:
        chunk = max(1, int(8e6 // (Q * Q * max(w1.shape[0], 1) * Q)))
    out = np.empty(B)
    for g0 in range(0, B, chunk):
        out[g0:g0 + chunk] = batch_ei_parts(mean[g0:g0 + chunk], cov[g0:g0 + chunk], eta, w1, w2)[0]
    return out


def batch_ei_scale(mean, cov, eta, w1, w2, chunk: int = 0):
    """(value [B], sum of |summands| [B]): the scale a float64 evaluation of the (cancelling) sum is accurate to."""
    mean = np.asarray(mean, dtype=np.float64)
    B, Q = mean.shape
    if chunk <= 0:
        chunk = max(1, int(8e6 // (Q * Q * max(w1.shape[0], 1) * Q)))
    val, scale = np.empty(B), np.empty(B)
    for g0 in range(0, B, chunk):
        v, _, _, t = batch_ei_parts(mean[g0:g0 + chunk], cov[g0:g0 + chunk], eta, w1, w2)
        val[g0:g0 + chunk], scale[g0:g0 + chunk] = v, np.sum(np.abs(t), axis=1)
    return val, scale


def sobol_points(S: int, q: int, skip: int = 0):
    """The two point sets of one skip (function.py:1756-1770; ``tf.math.sobol_sample`` starts after the all-zero point):
    w1 [S, q], w2 [S, q - 1]."""
    import warnings

    from scipy.stats import qmc

    out = []
    for dim in (q, q - 1):
        if dim == 0:
            out.append(np.zeros((S, 0)))
            continue
        gen = qmc.Sobol(d=dim, scramble=False)
        gen.fast_forward(int(skip) + 1)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            out.append(np.ascontiguousarray(gen.random(S)))
    return out[0], out[1]


def brute_force_qei(mean, cov, eta, num_samples: int, seed: int = 0):
    """Plain Monte-Carlo E[max(eta - min_j f_j, 0)], f ~ N(mean, cov + 1e-6 I): the quantity the closed form estimates."""
    mean = np.asarray(mean, dtype=np.float64)
    B, Q = mean.shape
    rng = np.random.default_rng(seed)
    L = np.linalg.cholesky(np.asarray(cov) + CALL_JITTER * np.eye(Q)[None])
    out = np.empty(B)
    for g in range(B):
        f = mean[g][:, None] + L[g] @ rng.standard_normal((Q, num_samples))
        out[g] = np.mean(np.maximum(eta - f.min(axis=0), 0.0))
    return out
