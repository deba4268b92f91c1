"""numpy restatement of the gradient of the batch Monte-Carlo expected hypervolume improvement w.r.t. the joint moments (TEST
INFRASTRUCTURE), written from the formula and not from the kernel's walk.

``sample_adjoints`` loops over the subsets of the batch as ``qehvi_reference._signed_terms`` does and differentiates the
maximum over the subset, the maximum with the cell's lower bound and the maximum with zero explicitly: the derivative of a
subset's term w.r.t. the sample of the point that attains the overlap vertex in objective j (``np.argmax``: the first point on
a tie) is -sign prod_{j' != j} length_j', and zero unless lb < vertex < ub strictly.  A lower bound below -1e10 is taken as
-1e10, as the device takes it.  ``moment_adjoints`` carries those to the adjoints of (mean, cov) through the samples
y = mean + L eps and the Cholesky adjoint  gcov = L^-T sym(Phi(L^T Lbar)) L^-1  (Phi: lower triangle, diagonal halved) with
``scipy.linalg.solve_triangular``.  The "scales" are the same sums with every term's sign removed, for gcov propagated as
|L^-T| sym(Phi(|L^T| |Lbar|)) |L^-1|: what the roundings of an implementation are relative to.
``kink_distance`` is, per group, the smallest distance of any sample coordinate to a cell bound of its objective or to another
point's sample in the same objective and draw: within it the value is a polynomial of the samples."""
from itertools import combinations

import numpy as np
from scipy.linalg import solve_triangular

from tests import qehvi_reference as R

LOWEST = -1e10


def sample_adjoints(samples, lb, ub, signed=True, lipschitz=False):
    """samples [G, S, q, P], cell bounds lb, ub [K, P] -> d value / d samples [G, S, q, P] (the 1 / S included); with
    ``signed=False`` the sum of the absolute values of the same terms; with ``lipschitz=True`` (and ``signed=False``) the sum
    over the same terms of sum_{j' != j} prod_{j'' != j, j'} length_j'': by how much the terms can move per unit of change
    (in the maximum norm) of the samples, away from a kink."""
    y = np.asarray(samples, np.float64)
    lo = np.maximum(np.asarray(lb, np.float64), LOWEST)[None, None]         # [1, 1, K, P]
    hi = np.asarray(ub, np.float64)[None, None]
    G, S, q, P = y.shape
    out = np.zeros_like(y)
    for size in range(1, q + 1):
        sign = float((-1) ** (size + 1)) if signed else 1.0
        for J in combinations(range(q), size):
            sub = y[:, :, list(J), :]                                       # [G, S, |J|, P]
            vertex, owner = np.max(sub, axis=2), np.argmax(sub, axis=2)     # [G, S, P]: the first point wins a tie
            v = vertex[:, :, None, :]                                       # [G, S, 1, P]
            lengths = np.maximum(hi - np.maximum(v, lo), 0.0)               # [G, S, K, P]
            inside = (v > lo) & (v < hi)
            for j in range(P):
                if lipschitz:
                    others = sum(np.prod(np.delete(lengths, [j, j2], axis=-1), axis=-1) for j2 in range(P) if j2 != j)
                else:
                    others = np.prod(np.delete(lengths, j, axis=-1), axis=-1)   # [G, S, K]
                d = -sign * np.sum(np.where(inside[..., j], others, 0.0), axis=-1)       # [G, S]
                if not signed:
                    d = np.abs(d)
                for pos, i in enumerate(J):
                    out[:, :, i, j] += np.where(owner[:, :, j] == pos, d, 0.0)
    return out / S


def _cholesky_adjoint(L, Lbar):
    """gcov = L^-T sym(Phi(L^T Lbar)) L^-1 for one q x q factor."""
    Q = np.tril(L.T @ Lbar)
    Q[np.diag_indices_from(Q)] *= 0.5
    R_ = 0.5 * (Q + Q.T)
    Y = solve_triangular(L, R_, lower=True, trans="T")                      # L^-T R
    return solve_triangular(L, Y.T, lower=True, trans="T").T                 # (L^-T Y^T)^T = Y L^-1


def _cholesky_adjoint_scale(L, Lbar_scale):
    q = L.shape[0]
    Li = np.abs(solve_triangular(L, np.eye(q), lower=True))
    Q = np.tril(np.abs(L).T @ Lbar_scale)
    Q[np.diag_indices_from(Q)] *= 0.5
    return Li.T @ (0.5 * (Q + Q.T)) @ Li


def moment_adjoints(mean, cov, eps, jitter, lb, ub):
    """mean [P, G, q], cov [P, G, q, q] objective-major, eps [P, q, S] -> dict of value [G], gmean [P, G, q], gcov [P, G, q, q]
    (symmetric), their scales gmean_scale / gcov_scale, the bounds gmean_lip / gcov_lip of their change per unit of change of
    the samples (``sample_adjoints(lipschitz=True)`` carried through the same absolute-value chain), and the samples
    [G, S, q, P]."""
    mean, cov, eps = (np.asarray(a, np.float64) for a in (mean, cov, eps))
    P, G, q = mean.shape
    samples = R.samples_from_moments(mean, cov, eps, jitter)
    L = np.linalg.cholesky(cov + jitter * np.eye(q))
    ybar, yabs = sample_adjoints(samples, lb, ub, True), sample_adjoints(samples, lb, ub, False)
    ylip = sample_adjoints(samples, lb, ub, False, lipschitz=True)
    out = dict(value=R.reference_form(samples, np.maximum(lb, LOWEST), ub), samples=samples,
               gmean=np.empty((P, G, q)), gcov=np.empty((P, G, q, q)), gmean_scale=np.empty((P, G, q)),
               gcov_scale=np.empty((P, G, q, q)), gmean_lip=np.empty((P, G, q)), gcov_lip=np.empty((P, G, q, q)))
    for j in range(P):
        for g in range(G):
            yb, ya = ybar[g, :, :, j], yabs[g, :, :, j]                     # [S, q]
            out["gmean"][j, g], out["gmean_scale"][j, g] = yb.sum(axis=0), ya.sum(axis=0)
            Lbar = np.tril(yb.T @ eps[j].T)                                 # [q, q]: sum_s ybar[s, i] eps[m, s]
            Lbar_scale = np.tril(ya.T @ np.abs(eps[j]).T)
            out["gcov"][j, g] = _cholesky_adjoint(L[j, g], Lbar)
            out["gcov_scale"][j, g] = _cholesky_adjoint_scale(L[j, g], Lbar_scale)
            out["gmean_lip"][j, g] = ylip[g, :, :, j].sum(axis=0)
            out["gcov_lip"][j, g] = _cholesky_adjoint_scale(L[j, g], np.tril(ylip[g, :, :, j].T @ np.abs(eps[j]).T))
    return out


def kink_distance(samples, lb, ub):
    """samples [G, S, q, P] -> [G]: the smallest distance of a sample coordinate to a (finite) cell bound of its objective or
    to another point's sample in the same objective and draw (inf when there is neither)."""
    y = np.asarray(samples, np.float64)
    G, S, q, P = y.shape
    best = np.full(G, np.inf)
    lo = np.maximum(np.asarray(lb, np.float64), LOWEST)
    for j in range(P):
        bounds = np.unique(np.concatenate([lo[:, j], np.asarray(ub, np.float64)[:, j]]))
        bounds = bounds[np.isfinite(bounds)]
        if len(bounds):
            best = np.minimum(best, np.abs(y[..., j][..., None] - bounds).reshape(G, -1).min(axis=1))
        for a, b in combinations(range(q), 2):
            best = np.minimum(best, np.abs(y[:, :, a, j] - y[:, :, b, j]).min(axis=1))
    return best
