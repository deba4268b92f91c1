"""numpy restatement of the batch Monte-Carlo expected improvement and of its adjoints w.r.t. the joint moments (TEST
INFRASTRUCTURE: the yardstick of tests/test_gpu_qei_tail.py, never imported by the package), written from the formula:

    L = chol(cov + jitter I);  f_s = mean + L eps[:, s];  value = mean_s max(eta - min_i f_s,i, 0)
    gmean_i = -count_i / S,    count_i = the improving draws (eta - min > 0, strictly) whose smallest sample is point i
                               (``np.argmin``: the first point on a tie)
    Lbar = tril(sum_s df_s eps_s^T),  df_s = -1/S at the arg-min of an improving draw
    gcov = L^-T sym(Phi(L^T Lbar)) L^-1   (Phi: lower triangle, diagonal halved); gcov_ii = 0 where cov_ii <= 1e-12

The "scales" are the same sums and chains with every term replaced by its absolute value: what the roundings of an
implementation are relative to.  The "lips" bound the first-order change of a result per unit of change of its input
between two float64 factorisations, away from a kink: the value moves by at most (improving draws / S) x the movement of the
samples; gmean is a count and does not move; gcov depends on the factor alone (Lbar is fixed by the counts and eps):

    d gcov = -L^-T dL^T gcov - gcov dL L^-1 + L^-T sym(Phi(dL^T Lbar)) L^-1
    |d gcov| <= delta (|L^-T| E^T G + G E |L^-1| + |L^-T| sym(Phi(E^T |Lbar|)) |L^-1|)

for |dL| <= delta E entrywise (E: the lower triangle of ones, G = gcov_scale >= |gcov|).
``kink_distance`` is, per group, the smallest distance of any draw to a change of branch: |eta - min_i f_s,i|, and for an
improving draw of q > 1 points the gap between its two smallest samples."""
import numpy as np
from scipy.linalg import solve_triangular

VAR_FLOOR = 1e-12


def factor(cov, jitter):
    cov = np.asarray(cov, np.float64)
    return np.linalg.cholesky(cov + jitter * np.eye(cov.shape[-1]))


def samples_from_factor(mean, L, eps):
    """mean [G, q], L [G, q, q], eps [q, S] -> [G, S, q]."""
    return np.asarray(mean, np.float64)[:, None, :] + np.einsum("gjk,ks->gsj", L, np.asarray(eps, np.float64))


def _adjoint(Li, A, Lbar):
    """Li^T sym(Phi(A^T Lbar)) Li: the absolute-value chain, with Li = |L^-1| and A = |L| (or E) as plain products."""
    Q = np.tril(A.T @ Lbar)
    Q[np.diag_indices_from(Q)] *= 0.5
    return Li.T @ (0.5 * (Q + Q.T)) @ Li


def cholesky_adjoint(L, Lbar):
    """gcov = L^-T sym(Phi(L^T Lbar)) L^-1 for one q x q factor, by triangular solves."""
    Q = np.tril(L.T @ Lbar)
    Q[np.diag_indices_from(Q)] *= 0.5
    R = 0.5 * (Q + Q.T)
    Y = solve_triangular(L, R, lower=True, trans="T")                      # L^-T R
    return solve_triangular(L, Y.T, lower=True, trans="T").T               # (L^-T Y^T)^T = Y L^-1


def moment_adjoints(mean, cov, eps, eta, jitter, clip=True):
    """mean [G, q], cov [G, q, q], eps [q, S] -> dict of value [G], samples [G, S, q], counts [G, q] (integers), improving [G]
    (the number of improving draws), gmean [G, q], gcov [G, q, q] (symmetric; with ``clip`` a diagonal entry is zero where
    cov_ii <= 1e-12), the scales value_scale / samples_scale / gcov_scale, the lips value_lip [G] (per unit of the samples) and
    gcov_lip [G, q, q] (per unit of the factor's entries), and kink_distance [G]."""
    mean, cov, eps = (np.asarray(a, np.float64) for a in (mean, cov, eps))
    G, q = mean.shape
    S = eps.shape[1]
    L = factor(cov, jitter)
    f = samples_from_factor(mean, L, eps)
    f_scale = np.abs(mean)[:, None, :] + np.einsum("gjk,ks->gsj", np.abs(L), np.abs(eps))
    jmin = np.argmin(f, axis=2)                                            # [G, S]: the first index on ties
    mn = np.take_along_axis(f, jmin[..., None], axis=2)[..., 0]
    imp = eta - mn
    improving = imp > 0.0
    out = dict(samples=f, samples_scale=f_scale, value=np.sum(np.where(improving, imp, 0.0), axis=1) / S,
               improving=improving.sum(axis=1), value_lip=improving.sum(axis=1) / S,
               value_scale=np.sum(np.where(improving, abs(eta) + np.take_along_axis(f_scale, jmin[..., None], axis=2)[..., 0], 0.0),
                                  axis=1) / S,
               counts=np.zeros((G, q), np.int64), gcov=np.empty((G, q, q)), gcov_scale=np.empty((G, q, q)),
               gcov_lip=np.empty((G, q, q)))
    E = np.tril(np.ones((q, q)))
    for g in range(G):
        hit = np.zeros((q, S))
        hit[jmin[g, improving[g]], np.flatnonzero(improving[g])] = 1.0     # hit[i, s]: draw s improves at point i
        out["counts"][g] = hit.sum(axis=1).astype(np.int64)
        Lbar = np.tril(-(hit @ eps.T) / S)                                 # [q, q]: sum_s df[s, i] eps[k, s]
        Labs = np.tril((hit @ np.abs(eps).T) / S)
        gc = cholesky_adjoint(L[g], Lbar)
        Li = np.abs(solve_triangular(L[g], np.eye(q), lower=True))
        scale = _adjoint(Li, np.abs(L[g]), Labs)
        lip = Li.T @ E.T @ scale + scale @ E @ Li + _adjoint(Li, E, Labs)
        if clip:
            clipped = np.flatnonzero(np.diagonal(cov[g]) <= VAR_FLOOR)
            gc[clipped, clipped] = 0.0
        out["gcov"][g], out["gcov_scale"][g], out["gcov_lip"][g] = gc, scale, lip
    out["gmean"] = -out["counts"] / S
    gap = np.full((G, S), np.inf)
    if q > 1:
        two = np.partition(f, 1, axis=2)[..., :2]
        gap = np.where(improving, two[..., 1] - two[..., 0], np.inf)
    out["kink_distance"] = np.minimum(np.abs(imp), gap).min(axis=1)
    return out
