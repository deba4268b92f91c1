"""The exact joint sampler (tgp_sample_joint, GPEngine.sample_joint) at its own resolution (TEST INFRASTRUCTURE, no GPU code;
tests/test_sample_resolution.py checks it on the CPU, tests/test_gpu_sample_resolution.py applies it to the device).

The call factorises A = cov(Xq, Xq) + jitter I on the device, A padded with the identity to Pp = n rounded up to 64, and
returns out[s, j] = mean_j + sum_t L_jt eps_ts.  Comparing SAMPLES with a float64 oracle compares factors, and a factor moves
by (error of A) / sqrt(jitter): such a comparison needs a tolerance of 1e-8 and more.  The RESIDUAL  L L^T - A  is not
amplified, and the entry lets a test read L: on a model with Y = 0 and mean constant 0 (alpha = 0, the posterior mean exactly 0,
the covariance untouched) eps = I_n returns out[s, j] = L_js -- a sum of one factor entry and exact zeros.

Reference arithmetic and units are tests/factor_resolution.py's: numpy.longdouble (eps 2^-63), EPS = 2^-52, INFL = 1 + 2^-30
on every weight that is evaluated in float64.  gamma_k = k EPS / (1 - k EPS): Higham's gamma_k with the unit roundoff replaced
by EPS, i.e. twice his constant (`residual_tolerance` says what the factor of two is for).

A_ref = k(Xq, Xq) - c^T c + jitter I in long double, c = L_K^-1 k(X, Xq) with L_K the long-double factor of K_exact.  All query
sets are PREFIXES of one set per model (`query_points`), so one reference per model serves every n.

The three terms of the residual bound are derived at `residual_tolerance` (a: the factorisation, c: the long-double weights)
and `covariance_tolerance` (b: the device's A is not A_ref); the draws' at `draw_tolerance`."""
import functools
import types

import numpy as np

from tests import factor_resolution as F
from tests.factor_resolution import EPS, EPS_LD, INFL, LD

N_TRAIN = 250
SIZES = (1, 2, 63, 64, 65, 128, 129, 192, 257, 320, 577)          # padded 64, 128, 192, 320, 640: both sides of each 64 and of 256
DRAW_PAIRS = ((1, 65), (2, 130), (63, 64), (64, 1), (65, 63), (128, 130), (129, 65), (192, 63), (257, 64), (320, 64), (577, 1))
JITTER = 1e-6
LOW_JITTER = 1e-10
WIDE = "wide"                                                       # d = 40: N = 120, n = 70, matern52
MODELS = tuple(f"{k}@{s:g}" for k, s in F.HYPERS) + (WIDE,)
# The bound was accepted on this evidence (tests/test_sample_resolution.py asserts it): numpy's float64 Cholesky of the
# float64-rounded A_ref stays below REFERENCE_MARGIN of it on every query set, with term (b) reduced to the rounding of A_ref.
REFERENCE_MARGIN = 0.25


def pad64(n):
    return -(-int(n) // 64) * 64


def gamma(k):
    return float(k * EPS / (1 - k * EPS))


@functools.lru_cache(maxsize=None)
def model(name):
    """kind, noise, d, variance, mean constant, X, Y, lengthscales of one case: factor_resolution's N = 250 design under one of
    its four HYPERS, or the wide one."""
    from oracle import gp_oracle as O

    m = types.SimpleNamespace(name=name, variance=F.VARIANCE, mean=F.MEAN)
    if name == WIDE:
        m.kind, m.noise, m.d, m.n_max = "matern52", 1e-2, 40, 70
        X, Y = O.synthetic_problem(O.ackley, m.d, 120)
        m.X, m.Y, m.ls = np.ascontiguousarray(X), np.asarray(Y, dtype=np.float64).reshape(-1), np.asarray(O.default_lengthscales(m.d))
    else:
        kind, noise = name.split("@")
        m.kind, m.noise, m.d, m.n_max = kind, float(noise), F.D, max(SIZES)
        m.X, m.Y, m.ls = F.problem(N_TRAIN)
    m.N = m.X.shape[0]
    return m


@functools.lru_cache(maxsize=None)
def query_points(name):
    """n_max points whose every prefix is a query set: position j is an exact copy of a training input when j % 8 == 1 (the
    covariance there is of the order of the noise or below and the jitter carries the pivot), a point at distance 1e-3 from a
    training input when j % 8 == 5, a uniform point otherwise.  n = 1 is generic, n = 2 generic + copy, n >= 6 has all three."""
    m = model(name)
    rng = np.random.default_rng(577 + m.d)
    Xq = rng.uniform(size=(m.n_max, m.d))
    for j in range(m.n_max):
        if j % 8 == 1:
            Xq[j] = m.X[j // 8]
        elif j % 8 == 5:
            u = rng.standard_normal(m.d)
            Xq[j] = m.X[100 + j // 8] + 1e-3 * u / np.linalg.norm(u)
    Xq.setflags(write=False)
    return Xq


def posterior(name):
    m = model(name)
    if name != WIDE:
        return F.posterior(m.kind, m.noise, m.N)
    return _wide_posterior()


@functools.lru_cache(maxsize=1)
def _wide_posterior():
    m = model(WIDE)
    return F.Posterior(m.kind, m.variance, m.ls, m.noise, m.mean, m.X, m.Y)


class Reference:
    """The long-double posterior of a model at a query set: pred (factor_resolution.Posterior.predict), k(Xq, Xq) with its
    assembly bound, cov = k - c^T c."""

    def __init__(self, name, Xq=None):
        self.m = m = model(name)
        self.Xq = query_points(name) if Xq is None else np.ascontiguousarray(Xq, dtype=np.float64)
        self.post = posterior(name)
        self.pred = self.post.predict(self.Xq)
        self.kqq, self.eqq = F.K_exact(m.kind, m.variance, m.ls, 0.0, self.Xq, self.Xq, parts=True)
        cc = self.pred[3]
        self.cov = self.kqq - cc.T @ cc

    def A(self, n, jitter):
        return self.cov[:n, :n] + LD(jitter) * np.eye(n, dtype=LD)

    def mean(self, n):
        return self.pred[0][:n]


@functools.lru_cache(maxsize=None)
def reference(name):
    return Reference(name)


# ---- (b): the device's A is not A_ref ------------------------------------------------------------------------------------------
def covariance_tolerance(ref, ms, jitter):
    """|A_dev - A_ref| entry by entry ([n_max, n_max], float64), in the manner of factor_resolution.posterior_tolerances: first-order
    sensitivities with the residuals of `update`'s arrays L, W (GPEngine.get_factor; each bounded on its own by
    tests/test_gpu_factor_resolution.py) MEASURED in long double (``ms``, a factor_resolution.Measured) and the reference's
    beta = K^-1 k*, c = L_K^-1 k*.  The device forms (tgp_sample_joint)
        C = fl(W K*),   S = fl(C^T C),   A_ij = fl(fl(k_ij - S_ij) + jitter [i == j]),
    K* by the assembly of `update` (bound e_K*, factor_resolution.K_exact parts) and k_ij in the difference form (x_i - x_j) / ls,
    whose one extra rounding of t moves r^2 by at most eps r^2 <= eps sum_c |t_c| (|a_c| + |b_c|): inside the same bound e_qq.
      W^T W is not K^-1:  K -> L L^T moves k_i^T K^-1 k_j by beta_i^T R_K beta_j (R_K symmetric: the smaller of the two
        orders bounds it), W^T W - (L L^T)^-1 = L^-T (E_l + E_l^T) L^-1 by c_i^T E_l c_j + c_j^T E_l c_i, E_l = W L - I;
      the product W K* (c_v eps |W||k*| per column, c_v = N / 2 + 2) and the Gram product (c_v eps |c_i|^T |c_j|);
      K* assembled with error e_K* (|beta_i|^T e_j + |beta_j|^T e_i), k_ij with e_qq;
      the two roundings of the tail: eps (|k_ij| + |c_i|^T |c_j| + jitter).
    Second-order terms are dropped (factor_resolution.Bounds asserts they are below 2^-12 of the first).  The reference's own
    error -- the long-double factor's N 2^-63 |L||L|^T through beta -- is part of the budget at 64 times its bound."""
    mean, var, beta, cc, ks, ek = ref.pred
    f = lambda v: np.asarray(np.abs(v), dtype=np.float64)
    ab, ac = f(beta), f(cc)
    e, c_v, N = float(EPS), ref.post.N / 2 + 2.0, ref.post.N
    t_rk = ab.T @ f(ms.RK(beta))
    t_el = ac.T @ f(ms.El(cc))
    t_wk = ac.T @ (f(ms.W) @ f(ks))
    t_ek = ab.T @ f(ek)
    gram = ac.T @ ac
    aL = f(ref.post.L)
    own = 64 * float(EPS_LD) * N * (ab.T @ (aL @ (aL.T @ ab)))
    tol = (np.minimum(t_rk, t_rk.T) + (t_el + t_el.T) + c_v * e * (t_wk + t_wk.T) + c_v * e * gram + (t_ek + t_ek.T) + f(ref.eqq)
           + e * (f(ref.kqq) + gram + jitter) + own)
    return tol * INFL


def assert_finer_than_the_floor(name, tol):
    """Term (b) is never looser than what the project grants tgp_cov_between (tests/test_gpu_parity.py
    test_covariance_between_points_matches_oracle): cancellation_floor on the diagonal, ten times it off the diagonal."""
    from tests.util import cancellation_floor

    m = model(name)
    floor = cancellation_floor(m.N, m.variance, m.noise)
    off = tol - np.diag(np.diag(tol))
    assert np.diag(tol).max() <= floor and off.max() <= 10 * floor, (name, np.diag(tol).max(), off.max(), floor)
    return float(np.diag(tol).max() / floor), float(off.max() / (10 * floor))


def rounding_tolerance(A):
    """Term (b) for a factor of the float64-ROUNDED A_ref: one rounding, eps / 2 |A|."""
    return np.asarray(np.abs(A), dtype=np.float64) * float(EPS) / 2 * INFL


# ---- (a) + (b) + (c): the residual of the factor ----------------------------------------------------------------------------------
def residual_tolerance(L, tol_A):
    """|L L^T - A_ref| <= gamma_(Pp+1) (|L||L|^T)_ij + tol_A_ij, the weights inflated by INFL.
    (a) A Cholesky factorisation in any order of summation satisfies L L^T = A + dA, |dA| <= gamma_(n+1) |L||L|^T (Higham,
        Accuracy and Stability of Numerical Algorithms, 2nd ed., Theorem 10.3): an entry of A - L L^T passes through at most n + 1
        roundings.  The device factorises the PADDED matrix, so the count is Pp + 1 (the identity rows add none: products with
        exact zeros; a blocked update's store of a partial trailing block is one of the Pp + 1).  Higham's unit is eps / 2; gamma here
        is k EPS, TWICE his: the second half is for what the device does besides substitution -- its pivot is p rsqrt(p) with a
        reciprocal square root of a few eps, and the recursion's panel L21 = A21 W11^T multiplies by an explicit inverse
        (tests/factor_resolution.py counts both for `update`, data-dependently, from W; this entry does not return W).
    (b) tol_A: `covariance_tolerance` for the device, `rounding_tolerance` for a factor of the rounded A_ref.
    (c) |L||L|^T is evaluated in float64 from non-negative terms (relative error below n eps): INFL = 1 + 2^-30."""
    aL = np.abs(np.asarray(L, dtype=np.float64))
    n = aL.shape[0]
    return np.tril((gamma(pad64(n) + 1) * (aL @ aL.T) + np.asarray(tol_A, dtype=np.float64)[:n, :n]) * INFL)


def factor_checks(what, L, A_ref, tol_A, bad=None):
    """The structure of a factor read from the entry -- exactly lower triangular, positive diagonal -- and its residual; returns
    the worst residual / bound."""
    L = np.asarray(L, dtype=np.float64)
    n = L.shape[0]
    msgs = []
    if L.shape != (n, n) or A_ref.shape != (n, n):
        msgs.append(f"{what}: factor {L.shape} against A {A_ref.shape}")
    elif not np.array_equal(np.triu(L, 1), np.zeros_like(L)):
        msgs.append(f"{what}: the factor is not exactly lower triangular")
    elif not np.all(np.diag(L) > 0):
        msgs.append(f"{what}: a diagonal entry of the factor is not positive")
    if msgs:
        if bad is None:
            raise AssertionError(msgs[0])
        bad += msgs
        return float("inf")
    G = np.abs(L) @ np.abs(L).T
    R = F.tri_LLt(L.astype(LD)) - np.tril(A_ref)
    return F.check(f"{what} |L L^T - A|", R, residual_tolerance(L, tol_A), np.tril(G), n, bad)


# ---- the draws --------------------------------------------------------------------------------------------------------------------
def draw_tolerance(L, eps, mean):
    """out[s, j] = fl(mean_j + fl(sum_t L_jt eps_ts)) against the same expression in long double WITH THE FACTOR JUST READ: the
    product's Pp terms (zero padding adds none) gamma_Pp sum_t |L_jt||eps_ts| in any order, the final sum's one rounding
    eps / 2 (|mean_j| + |sum|) <= EPS |mean_j| + EPS sum_t |L_jt||eps_ts|, and one more EPS of the weight for the float64
    evaluation of this tolerance itself:  (gamma_Pp + 2 EPS) sum_t |L_jt||eps_ts| + EPS |mean_j|,  times INFL.  [S, n]."""
    L, eps = np.abs(np.asarray(L, dtype=np.float64)), np.abs(np.asarray(eps, dtype=np.float64))
    w = (L @ eps).T
    return ((gamma(pad64(L.shape[0])) + 2 * float(EPS)) * w + float(EPS) * np.abs(np.asarray(mean, dtype=np.float64))[None, :]) * INFL


def draw_checks(what, out, L, eps, mean, bad=None):
    """Shape [S, n] and every entry of the draws; returns the worst error / tolerance."""
    n, S = np.shape(eps)
    out = np.asarray(out)
    if out.shape != (S, n):
        msg = f"{what}: draws of shape {out.shape}, expected {(S, n)}"
        if bad is None:
            raise AssertionError(msg)
        bad.append(msg)
        return float("inf")
    want = (np.asarray(mean, dtype=np.float64).astype(LD)[:, None]
            + np.asarray(L, dtype=np.float64).astype(LD) @ np.asarray(eps, dtype=np.float64).astype(LD)).T
    w = (np.abs(np.asarray(L, dtype=np.float64)) @ np.abs(np.asarray(eps, dtype=np.float64))).T
    return F.check(f"{what} |draws - (mean + L eps)|", out.astype(LD) - want, draw_tolerance(L, eps, mean), w, n, bad)


def draws(n, S, seed=0):
    return np.random.default_rng(20261127 + 1000 * n + S + seed).standard_normal((n, S))


# ---- a float64 restatement of the pipeline, with the device's padding -----------------------------------------------------------
def restate(ref, W, alpha, n, jitter, eps=None, jitter_everywhere=False):
    """tgp_sample_joint in numpy float64 from `update`'s W and alpha: C = W K*, A = k - C^T C + jitter I with the identity in the
    padding, its Cholesky factor at the padded size, zero-padded draws.  Returns (Lp [Pp, Pp], mean [n], out [S, n] or None).
    ``jitter_everywhere``: the planted fault of a jitter added to every entry."""
    m = ref.m
    ks = np.asarray(ref.pred[4][:, :n], dtype=np.float64)
    C = np.asarray(W, dtype=np.float64) @ ks
    A = np.asarray(ref.kqq[:n, :n], dtype=np.float64) - C.T @ C + jitter * (np.ones((n, n)) if jitter_everywhere else np.eye(n))
    Pp = pad64(n)
    Ap = np.eye(Pp)
    Ap[:n, :n] = A
    Lp = np.linalg.cholesky(Ap)
    mean = m.mean + ks.T @ np.asarray(alpha, dtype=np.float64)
    if eps is None:
        return Lp, mean, None
    S = eps.shape[1]
    Ep = np.zeros((Pp, pad64(S)))
    Ep[:n, :S] = eps
    R = Lp @ Ep
    return Lp, mean, np.ascontiguousarray((mean[:, None] + R[:n, :S]).T)


@functools.lru_cache(maxsize=None)
def reference_arrays(name):
    """The float64 reference's (L, W, alpha) of a model's `update`."""
    if name != WIDE:
        m = model(name)
        return F.reference_factor(m.kind, m.noise, m.N)
    import scipy.linalg as sl

    from oracle import gp_oracle as O

    m = model(name)
    with O.difference_form():
        st = O.gpr_update(m.kind, m.variance, m.ls, m.noise, m.mean, m.X, m.Y)
    return (np.tril(st.L), np.tril(sl.solve_triangular(st.L, np.eye(m.N), lower=True)), sl.cho_solve((st.L, True), m.Y - m.mean))


def measured(name, L, W, alpha):
    post = posterior(name)
    return F.Measured(L, W, alpha, post.K, post.err)


# ---- breakdown sets: jitter 0 ---------------------------------------------------------------------------------------------------------
def separated_points(n, d, seed):
    """n uniform points of the unit cube, no two closer than 0.15 (greedy rejection; fixed seed)."""
    rng = np.random.default_rng(seed)
    pts = []
    while len(pts) < n:
        x = rng.uniform(size=d)
        if all(np.linalg.norm(x - p) >= 0.15 for p in pts):
            pts.append(x)
    return np.array(pts)


BREAKDOWN_PAIRS = ((40, 3, 20), (100, 10, 90), (130, 5, 129))       # (n, a, b): b in the first 64-block, in the second, b = n - 1


@functools.lru_cache(maxsize=None)
def duplicate_pair_set(n, a, b):
    Xq = separated_points(n, F.D, 9000 + n)
    Xq[b] = Xq[a]
    Xq.setflags(write=False)
    return Xq


@functools.lru_cache(maxsize=None)
def open_breakdown_set(which):
    """The three sets whose outcome rounding decides: (model name, Xq).  Two triplicated-point sets (n = 70: the copies inside the
    first block and across the boundary) on matern52@0.01, one of 66 copies of training inputs at noise 1e-5."""
    if which == 2:
        return "matern52@1e-05", np.ascontiguousarray(model("matern52@1e-05").X[:66])
    Xq = separated_points(70, F.D, 9500 + which)
    for j in ((30, 50) if which == 0 else (63, 64)):
        Xq[j] = Xq[7]
    return "matern52@0.01", Xq


def pd_index(message):
    """The point index a NotPositiveDefiniteError names."""
    import re

    found = re.search(r"at point (-?\d+)", message)
    assert found, f"the message names no point: {message!r}"
    return int(found.group(1))
