"""The 50-digit reference of the predictive-variance tail (tgp_kernels_pvar.hip) and the two derived bounds.

With u = 2^-53 and the reference's own L and A^-1 of A = L L^T:
  logdet:  |d logdet| <= 2 [(q + 2) u sum_ij |A^-1|_ij (|L||L|^T)_ij + 4 q u (1 + max_i |log L_ii|)] -- Cholesky's backward error
           |dA| <= (q + 2) u |L||L|^T through d logdet = tr(A^-1 dA), valid for any summation order (the matrix pipe's included),
           then the logs and their sum; both doubled.  det: the same relatively, plus 2 u.
  gcov:    |gcov - det A^-1|_ij <= det [8 (q + 1) u (|A^-1| |L||L|^T |A^-1|)_ij + |A^-1|_ij (the det bound)] -- the
           factorisation, two triangular steps and the product, about 4 (q + 1) u, doubled.
Scaling A by 4^k scales every quantity of the reference by an exact power of two (L by 2^k, A^-1 by 4^-k, det by 4^(k q)) and
logdet by q k log 4, so batches that differ by such a factor share one factorisation here."""
import functools

import mpmath as mp
import numpy as np

U = 2.0 ** -53


def matern52(X, lengthscale=1.0):
    r = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1)) / lengthscale
    return (1.0 + np.sqrt(5.0) * r + 5.0 / 3.0 * r * r) * np.exp(-np.sqrt(5.0) * r)


def covariances(q, n, seed, close=False):
    """n matrices k(X, X) + 1e-3 I, X random in [0, 1]^4; ``close``: the second point 1e-6 from the first."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, q, 4))
    if close:
        X[:, 1] = X[:, 0] + 1e-6 / 2.0
    return np.stack([matern52(x) + 1e-3 * np.eye(q) for x in X])


@functools.lru_cache(maxsize=None)
def _factor(key, q):
    A = np.frombuffer(key).reshape(q, q)
    with mp.workdps(50):
        M = mp.matrix(A.tolist())
        return mp.cholesky(M), mp.inverse(M)


def reference(A, k=0):
    """A [q, q] float64 (jitter included), the batch being 4^k A -> logdet, det, gcov = det A^-1 and the bounds on the three."""
    q, k = A.shape[0], int(k)
    L, Ai = _factor(np.ascontiguousarray(A).tobytes(), q)
    with mp.workdps(50):
        ld = 2 * sum(mp.log(L[i, i]) for i in range(q)) + q * k * mp.log(4)
        det = mp.exp(ld)
        absL = np.abs(np.array(L.tolist(), dtype=np.float64)) * 2.0 ** k
        absAi = np.abs(np.array(Ai.tolist(), dtype=np.float64)) * 4.0 ** -k
        gcov = np.array([[float(det * Ai[i, j] / mp.mpf(4) ** k) for j in range(q)] for i in range(q)])
        maxlog = max(abs(float(mp.log(L[i, i]) + k * mp.log(2))) for i in range(q))
    LLt = absL @ absL.T
    b_ld = 2.0 * ((q + 2) * U * float((absAi * LLt).sum()) + 4 * q * U * (1.0 + maxlog))
    b_det = b_ld + 2.0 * U                                                       # relative
    b_g = float(det) * (8 * (q + 1) * U * (absAi @ LLt @ absAi) + absAi * b_det)   # elementwise
    return float(ld), float(det), gcov, b_ld, b_det, b_g


@functools.lru_cache(maxsize=None)
def _unscaled_parts(key, q):
    """What every exponent pattern of ``reference_scaled`` shares: log L_ii (mpmath), |L||L|^T, |A^-1|, det(A) = man 2^ex with
    man in [1/2, 1) kept apart from its exponent, and man A^-1 rounded once."""
    L, Ai = _factor(key, q)
    with mp.workdps(50):
        logs = [mp.log(L[i, i]) for i in range(q)]
        absL = np.abs(np.array(L.tolist(), dtype=np.float64))
        absAi = np.abs(np.array(Ai.tolist(), dtype=np.float64))
        man, ex = mp.frexp(mp.exp(2 * sum(logs)))
        G0 = np.array([[float(man * Ai[i, j]) for j in range(q)] for i in range(q)])
    return logs, absL @ absL.T, absAi, man, int(ex), G0


def reference_scaled(A, s, by_exp=False):
    """A [q, q] float64 (jitter included), s [q] integers, the batch being D A D with D = diag(2^s_i) -> logdet (float), det
    (an mpmath number: it may lie outside float64's range), gcov = det (D A D)^-1 and the three bounds of ``reference``
    restated with the exponent vector.  ``by_exp``: the bounds of a batch whose det is exp(logdet) and not the pivots'
    product: relatively the logdet bound, the rounding of 2 lsum (2 u |logdet|) and the exponential's own error, ASSUMED
    to be within 4 u on the device.  While nothing leaves the normal range the scaling is exact in the kernel -- L_ij
    scales by 2^s_i, W = L^-1 by 2^-s_j, W^T W by 2^(-s_i-s_j) -- and in the reference: logdet = logdet(A) + 2 log 2 sum s,
    det = det(A) 4^(sum s), gcov_ij = det A^-1_ij 2^(-s_i-s_j), so every exponent pattern shares A's one factorisation.  The
    bounds scale elementwise the same way: sum_ij |A^-1|_ij (|L||L|^T)_ij does not change at all, max |log L_ii| becomes
    max |log L_ii + s_i log 2|, and the gcov bound carries 2^(-s_i-s_j) and the scaled det.  gcov and its bound are float64
    and overflow to inf or underflow towards 0 where the scaled values do: the caller checks them only where they are normal."""
    q = A.shape[0]
    s = np.asarray(s, dtype=np.int64)
    logs, LLt, absAi, man, ex, G0 = _unscaled_parts(np.ascontiguousarray(A).tobytes(), q)
    with mp.workdps(50):
        ld = 2 * sum(logs) + 2 * int(s.sum()) * mp.log(2)
        det = mp.exp(ld)
        maxlog = max(abs(float(logs[i] + int(s[i]) * mp.log(2))) for i in range(q))
    b_ld = 2.0 * ((q + 2) * U * float((absAi * LLt).sum()) + 4 * q * U * (1.0 + maxlog))
    b_det = b_ld + (2.0 * U * abs(float(ld)) + 4.0 * U if by_exp else 2.0 * U)
    shift = int(ex) + 2 * int(s.sum()) - s[:, None] - s[None, :]       # exponent of det 2^(-s_i-s_j) over its mantissa
    with np.errstate(over="ignore", under="ignore"):
        gcov = np.ldexp(G0, shift)
        b_g = np.ldexp(float(man) * (8 * (q + 1) * U * (absAi @ LLt @ absAi) + absAi * b_det), shift)
    return float(ld), det, gcov, b_ld, b_det, b_g
