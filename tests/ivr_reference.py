"""TEST INFRASTRUCTURE: the integrated variance reduction (reference acquisition/function/active_learning.py:304-415) twice.

1. ``oracle_route``: the reference's route on the numpy oracle -- ``conditional_predict_f(Z, additional_data = x)`` per batch,
   the weights, ``-mean``.
2. ``tail_restatement`` / ``factored_route``: the factored form the engine computes,
       reduction = (1/P) sum_z w_z |L^-1 c_z|^2,  L = chol(Sigma_xx + s^2 I),  out = reduction - c0,  c0 = (1/P) sum_z w_z var_old(z),
   with the tail in the kernel's order (trieste_amd/csrc/tgp_kernels_ivr.hip): the right-looking row factorisation of
   wave_chol_rows, the forward substitution row by row with the terms k ascending, sum_i a_i^2 in row order, lane l of 64 adds
   the tiles z = l, l + 64, ... ascending, one xor butterfly (32, 16, ..., 1), the division by P.  numpy has no fused
   multiply-add: a product and its addition round separately here, which the counted bound allows for (it counts both).
   The keyword ``defect`` plants one of five mistakes, so that the tests can show that their tolerance rejects each.

The two tolerances of the GPU tests are derived here, not tuned:

``tail_bound``: the tail on GIVEN moments.  Unit roundoff u = 2^-53, gamma_n = n u / (1 - n u).  With M = |L^-1|, ah_z = M |c_z| >= |a_z|
   and yh_z = M^T ah_z >= |A^-1 c_z| (A = cov + s^2 I), to first order in u, per integration point
       factorisation   L L^T = A + dA, |dA| <= gamma_{q+2} |L| |L^T|  (Higham, Accuracy and Stability, Thm 10.3; one more
                       rounding for the noise added to the diagonal)   ->   |d s_z| <= gamma_{q+2} yh_z^T |L| |L^T| yh_z
       substitution    (L + dL) a = c, |dL| <= gamma_q |L|  (Thm 8.5)    ->   |d a_z| <= gamma_q M |L| ah_z,  |d s_z| <= 2 ah_z^T |d a_z|
       sum_i a_i^2     q products, q additions                          ->   |d s_z| <= gamma_{q+1} |ah_z|^2
   and over z: a lane's T = ceil(P / 64) weighted additions (product and sum), six butterfly additions, one division:
       |d reduction| <= (1/P) sum_z w_z (the three above) + gamma_{2 T + 7} (1/P) sum_z w_z |ah_z|^2.
   A sum of non-negative terms: no condition number beyond the one of the q x q system, which M carries; no free constant.

``reduction_atol``: behind the posterior every entry of cov and cross is within f = tests.util.cancellation_floor of the oracle's.
   First order through the same two steps: dA = f (all entries) gives |d s_z| <= f (sum_i yh_zi)^2, d c = f gives
   |d s_z| <= 2 f sum_i yh_zi; reduction_atol = (1/P) sum_z w_z (f |yh_z|_1^2 + 2 f |yh_z|_1).
"""
from __future__ import annotations

import numpy as np

from oracle import gp_oracle as O

U = 2.0 ** -53
LANES = 64
DEFECTS = ("no_noise", "unclipped_c0", "weights_after_sum", "padded_mean", "last_tile_dropped")


def gamma(n):
    return n * U / (1.0 - n * U)


# ---- weights (active_learning.py:398-405) ---------------------------------------------------------------------------------------
def normal_pdf(x, mean, sd):
    z = (x - mean) / sd
    return np.exp(-0.5 * z * z) / (sd * np.sqrt(2.0 * np.pi))


def normal_cdf(x, mean, sd):
    from scipy.special import erfc

    return 0.5 * erfc(-(x - mean) / (sd * np.sqrt(2.0)))


def weights_of(mean_old, var_old, threshold):
    """None -> None (all ones); one threshold -> the posterior pdf there; two -> the probability of the interval."""
    if threshold is None:
        return None
    t = np.atleast_1d(np.asarray(threshold, dtype=np.float64))
    sd = np.sqrt(var_old)
    if t.size == 1:
        return normal_pdf(t[0], mean_old, sd)
    return np.maximum(normal_cdf(t[1], mean_old, sd) - normal_cdf(t[0], mean_old, sd), 0.0)


def _w(weights, P):
    return np.ones(P) if weights is None else np.asarray(weights, dtype=np.float64).reshape(P)


# ---- 1. the reference's route ------------------------------------------------------------------------------------------------------
def oracle_route(state, Z, Xq, weights=None):
    """Xq [G, q, d] -> out [G] = -mean_z(w_z conditional variance at z given the batch)."""
    Z = np.asarray(Z, dtype=np.float64)
    w = _w(weights, Z.shape[0])
    out = np.empty(len(Xq))
    for g, x in enumerate(np.asarray(Xq, dtype=np.float64)):
        _, var = O.conditional_predict_f(state, Z, x, np.ones(x.shape[0]))
        out[g] = -np.mean(var * w)
    return out


def oracle_moments(state, Z, Xq):
    """-> cov [G, q, q] (predict_joint), cross [G, q, P] (covariance_between_points), var_old [P] (predict, clipped)."""
    Xq = np.asarray(Xq, dtype=np.float64)
    _, cov = O.predict_joint(state, Xq)
    cross = np.stack([O.covariance_between_points(state, x, np.asarray(Z, dtype=np.float64)) for x in Xq])
    _, var_old = O.predict(state, Z)
    return cov, cross, var_old


def route_on_moments(cov, cross, var_old, weights, noise):
    """conditional_predict_f's arithmetic (LAPACK factorisation and solve, var_old - sum a^2, -mean) on moments computed once
    -> (out [G], reduction [G]): what ``oracle_route`` returns, without recomputing the posterior per weight vector."""
    G, q, P = cross.shape
    w = _w(weights, P)
    out, red = np.empty(G), np.empty(G)
    for g in range(G):
        L = np.linalg.cholesky(cov[g] + noise * np.eye(q))
        A = np.linalg.solve(L, cross[g])
        s = np.sum(A * A, axis=0)
        out[g], red[g] = -np.mean((var_old - s) * w), np.mean(w * s)
    return out, red


def oracle_reduction(state, Z, Xq, weights=None):
    """The reduction by the oracle's own (LAPACK) factorisation and solve: mean_z w_z |L^-1 c_z|^2 per batch."""
    cov, cross, _ = oracle_moments(state, Z, Xq)
    w = _w(weights, cross.shape[-1])
    red = np.empty(len(cov))
    for g in range(len(cov)):
        L = np.linalg.cholesky(cov[g] + state.noise * np.eye(cov.shape[-1]))
        A = np.linalg.solve(L, cross[g])
        red[g] = np.mean(w * np.sum(A * A, axis=0))
    return red


# ---- 2. the factored form, tail in the kernel's order --------------------------------------------------------------------------------
def chol_rows(A):
    """wave_chol_rows on a stack A [G, q, q]: column j's pivot, the multipliers, then the update of the trailing rows."""
    L = np.array(A, dtype=np.float64)
    q = L.shape[-1]
    bad = np.zeros(L.shape[0], dtype=bool)
    for j in range(q):
        dj = L[:, j, j].copy()
        broke = ~(dj > 0.0)
        bad |= broke
        dj[broke] = 1.0
        sd = np.sqrt(dj)
        L[:, j + 1:, j] = L[:, j + 1:, j] / sd[:, None]
        L[:, j, j] = sd
        for k in range(j + 1, q):
            L[:, k:, k] = L[:, k:, k] - L[:, k:, j] * L[:, k, j][:, None]   # rows >= k of column k (the lower triangle is all that is read)
    return np.tril(L), bad


def tail_restatement(cov, cross, weights=None, noise=0.0, defect=None):
    """cov [G, q, q], cross [G, q, P] -> reduction [G] in the kernel's order."""
    cov, cross = np.asarray(cov, dtype=np.float64), np.asarray(cross, dtype=np.float64)
    G, q, P = cross.shape
    w = _w(weights, P)
    A = cov.copy()
    if defect != "no_noise":
        A[:, np.arange(q), np.arange(q)] = A[:, np.arange(q), np.arange(q)] + noise
    L, _ = chol_rows(A)
    a = np.empty_like(cross)
    s = np.zeros((G, P))
    for i in range(q):
        t = cross[:, i, :].copy()
        for k in range(i):
            t = t - L[:, i, k][:, None] * a[:, k, :]
        a[:, i, :] = t / L[:, i, i][:, None]
        s = s + a[:, i, :] * a[:, i, :]
    T = (P + LANES - 1) // LANES
    if defect == "last_tile_dropped":
        T -= 1
    acc = np.zeros((G, LANES))
    for tile in range(T):
        n = min(LANES, P - tile * LANES)
        sl = slice(tile * LANES, tile * LANES + n)
        acc[:, :n] = acc[:, :n] + (s[:, sl] if defect == "weights_after_sum" else w[sl] * s[:, sl])
    lanes = np.arange(LANES)
    for off in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[:, lanes ^ off]
    red = acc[:, 0]
    if defect == "weights_after_sum":
        red = red * np.mean(w)
    return red / (T * LANES if defect == "padded_mean" else P)


def c0_of(var_old, weights=None, defect=None, var_unclipped=None):
    P = len(var_old)
    v = var_unclipped if defect == "unclipped_c0" else var_old
    return float(np.sum(_w(weights, P) * v) / P)


def factored_route(state, Z, Xq, weights=None, defect=None):
    """-> (out [G], reduction [G], c0) from the oracle's moments through the kernel-order tail."""
    cov, cross, var_old = oracle_moments(state, Z, Xq)
    unclipped = O.predict(state, Z, clip=False)[1] if defect == "unclipped_c0" else None
    red = tail_restatement(cov, cross, weights, state.noise, defect)
    c0 = c0_of(var_old, weights, defect, unclipped)
    return red - c0, red, c0


# ---- tolerances ---------------------------------------------------------------------------------------------------------------------
def _magnitudes(cov, cross, noise):
    """M = |L^-1|, ah = M |c| [G, q, P], yh = M^T ah [G, q, P], absL [G, q, q] of A = cov + noise I (LAPACK factor)."""
    cov = np.asarray(cov, dtype=np.float64)
    q = cov.shape[-1]
    L = np.linalg.cholesky(cov + noise * np.eye(q))
    M = np.abs(np.linalg.inv(L))
    ah = M @ np.abs(cross)
    yh = np.swapaxes(M, -1, -2) @ ah
    return M, ah, yh, np.abs(L)


def tail_bound(cov, cross, weights=None, noise=0.0):
    """[G]: the counted first-order bound on the kernel's reduction against the exact one on the same (float64) moments."""
    cross = np.asarray(cross, dtype=np.float64)
    G, q, P = cross.shape
    w = _w(weights, P)
    M, ah, yh, aL = _magnitudes(cov, cross, noise)
    LtY = np.swapaxes(aL, -1, -2) @ yh                          # |L^T| yh
    fact = gamma(q + 2) * np.sum(LtY * LtY, axis=1)             # yh^T |L| |L^T| yh
    da = gamma(q) * (M @ (aL @ ah))
    subst = 2.0 * np.sum(ah * da, axis=1)
    sq = np.sum(ah * ah, axis=1)
    T = (P + LANES - 1) // LANES
    per_z = fact + subst + gamma(q + 1) * sq + gamma(2 * T + 7) * sq
    return np.sum(w * per_z, axis=1) / P


def reduction_atol(cov, cross, weights, noise, f):
    """[G]: how far an error of f in every entry of cov and of cross moves the reduction, to first order."""
    cross = np.asarray(cross, dtype=np.float64)
    P = cross.shape[-1]
    w = _w(weights, P)
    _, _, yh, _ = _magnitudes(cov, cross, noise)
    y1 = np.sum(yh, axis=1)                                     # |yh_z|_1  [G, P]
    return np.sum(w * (f * y1 * y1 + 2.0 * f * y1), axis=1) / P
