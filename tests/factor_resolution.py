"""Residuals of `update`'s three arrays -- L, W = L^-1, alpha -- in extended precision, and their bounds (TEST
INFRASTRUCTURE, no GPU code; tests/test_factor_resolution.py checks it on the CPU, tests/test_gpu_factor_resolution.py
compares the device's arrays with it).

Reference arithmetic: numpy.longdouble, the x87 80-bit format (eps 2^-63; asserted below).  K_exact is built in long double
from the exact doubles in the difference form t = (x - X) / ls, the noise added on the diagonal in long double.  Residuals
are accumulated in long double.  The WEIGHTS of the bounds -- |L||L|^T, |L||W| and their products -- are sums of
non-negative terms; they are evaluated in float64 (relative error below N eps) and inflated by 1 + 2^-30.

Units: eps = 2^-52; one rounding is eps / 2, Higham's gamma_n = n eps / 2 (Accuracy and Stability of Numerical Algorithms,
2nd ed., Theorem 10.3 for the factor, Theorem 8.5 for a substitution, Lemma 14.1 for an inverse built by substitution).  All
bounds are DATA-DEPENDENT: |L|, |W|, |alpha| of the arrays under test weigh them, no condition number is guessed.

Kernel assembly (csrc/tgp_kernels_linalg.hip assemble_K_kernel; the same function forms K*): the engine's K is not
K_exact.  tests/kernel_resolution.py counts eps (A + B s) |K| for it on inputs whose scaled coordinates are exact; here the
lengthscales are no powers of two and scale_inputs_kernel's division X / ls adds one rounding per coordinate, eps / 2 |x / ls|
ABSOLUTE on a difference t: d(r^2) <= eps sum_c |t_c| (|a_c| + |b_c|), a = x / ls, so
    E_K = eps [(A + B s) |K| + |dk/dr^2| sum_c |t_c| (|a_c| + |b_c|)]   (+ eps (variance + noise) on the diagonal: K_ii + noise)
with B = (d + 2) / 2 (rbf), (d + 2) / 4 + 3 (matern52) and A = A_COEF (+ (d - 3) / 4 for matern52, whose polynomial factor
inherits the relative error (d + 2) / 4 + 3 of s, counted there at d = 3) of tests/kernel_resolution.py.

The factor.  Every form is a blocked right-looking Cholesky; an element of K - L L^T passes through at most N + 1 roundings
in any summation order (fused multiply-adds of the MFMA and DPP updates count one each; every store of a partial trailing
block one), so the substitution part is gamma_(N+1); 4 more eps cover the products with the pivot's reciprocal:
    c_K = (N + 1) / 2 + 4.
The pivot itself is NOT a correctly rounded square root: the 128-leaf (tgp_leaf_dev.inc PanelStep) forms rs = rsqrt_short(p) --
v_rsq_f64, whose documented seed error 2^-23 leaves 3/2 e^2 = 96 eps after the one coupled Newton step (about 8 eps measured) --
and scales column j with it, L_jj = p rs and L_ij = a_ij rs; the identity rows that become W_d ride through the same products.
The trailing updates use the stored values, so only the pivot column's own term is touched:  a_ij - L_ij L_jj = a_ij (1 - p rs^2):
    + c_piv eps |L_ij||L_jj|  in B_K   and   + c_piv eps |L_jj||W_jk|  in B_r,    c_piv = 2 * 96 + 3 = 195
(the device forms only; the reference's pivots are correctly rounded).
Two steps multiply by an EXPLICIT inverse of a diagonal block instead: the one-workgroup chain's L(j+1,j) = P W_jj^T
(tgp_kernels_dag.hip) and the recursion's panel L21 = A21 W11^T (tgp_api.hip chol_inv, and `factorise` for an append); so do the persistent kernel's T
tasks L(i,j) = P(i,j) W_jj^T for i >= j + 2 on the workers, in every plan and chain (tgp_kernels_dag.hip) -- the tile mask covers them.  With
E = L_jj W_jj - I the RIGHT residual of that block,  L_ij L_jj^T - P = P E^T + dL L_jj^T,  |dL| <= gamma_n |P||W_jj|^T,
|P| <= |L_ij||L_jj|^T:
    |R_K| <= eps c_K |L||L|^T  +  |L| (M_1 o |L|)^T (|E_M|^T + c_x / 2 eps D_1^T),   D_l = M_l o (|L||W|),   c_x = n_blk + 4
with E_M = M_1 o (L W - I) the right residual of the inverted blocks MEASURED on the arrays under test in long double (it is bounded
on its own by B_r below, whose nested series S = D_1 + D_2 D_1 + D_3 D_2 D_1 + ... would make B_K wider than a 2^-36 error of a tile
if it were inserted here: tests/test_factor_resolution.py plants one),
where M_l masks the diagonal blocks that are inverted at nesting level l (`form_levels`: the persistent kernel's 128 x 128 tiles,
then the 16-blocks of its leaf; the recursion's tree of nodes down to the 128-leaf, then the 16-blocks; [0, keep) and [keep, N)
on top of tiles and 16-blocks for an append), n_blk the largest block; a block's own right residual carries the factor of the
level below, hence the series S.  D_l is the factor |L_jj||W_jj| computed from the data, per block, in long double for blocks
up to 128.  The two-workgroup chain solves against L_jj with inverted 16-blocks: the same form with smaller blocks, covered by
the tile mask.

The inverse.  Which residual is small?  Every form builds W LEFT-multiplying: the leaf's identity rows ride through the
elimination (T = E_kb ... E_0), the blocked steps are W_ij = -W_ii (sum_k L_ik W_kj) (leaf_blocked_kernel, the leaf's work items, the
persistent kernel's inverse tasks, the recursion's W21 = -W22 (L21 W11)).  Then (L W)_ij = (S - S^) - E_ii S^ - L_ii dW with S the
sum: column j of W is a forward substitution with the diagonal blocks inverted explicitly, and the RIGHT residual is the
small one,
    |L W - I| <= B_r = eps [c_N F + c_x S F],   F = |L||W|,   c_N = N / 2 + 4   (asserted tightly),
while the LEFT one is only  W L - I = W (L W - I) L + second order:
    |W L - I| <= B_l = (1 + 2^-10) |W| B_r |L|.

alpha = W^T (W err) (two trmv launches, tgp_api.hip factorise), a product with the explicit inverse on both sides:
t^ = W err + d1, alpha = W^T t^ + d2, |d| <= gamma_(N+2) of the products' own weights, and with K_exact = L L^T - R_K
    K alpha - err = E_r err + L d1 + L E_l^T t^ + K d2 - R_K alpha
    |r_alpha| <= B_r |err| + c_v eps |L||W||err| + |L| B_l^T |t| + c_v eps |K||W|^T|t| + B_K |alpha|,   c_v = N / 2 + 2.
The float64 reference's alpha is two substitutions with the factor (cho_solve), backward stable: (K + dK) alpha = err with
|dK| <= gamma_(3N+1) |L||L|^T (Higham, Theorem 10.4) plus R_K -- the "solve" form of `Bounds.alpha`, used for that input only.

Derived quantities (first-order sensitivity to the budget above, evaluated from the REFERENCE's beta = K^-1 k*, c = L^-1 k*,
alpha, z = L^-1 err in long double, plus the roundings of the final product; small-product path tgp_api.hip predict_small /
predict_small_tail and the sweep: mean = c + k*^T alpha, var = k** - |W k*|^2, both float64):
    |d mean| <= |beta|^T B_alpha + eps [c_v |k*|^T |alpha| + e_K*^T |alpha| + |mean|]
    |d var|  <= |beta|^T B_K |beta| + 2 |c|^T B_l |c| + 2 c_v eps |c|^T |W||k*| + c_v eps |c|^2 + 2 |beta|^T e_K* + eps variance
      (K -> L L^T moves k*^T K^-1 k* by beta^T R_K beta; W^T W - (L L^T)^-1 = L^-T (E_l + E_l^T) L^-1 moves it by 2 c^T E_l c;
       the product W k* and the sum of squares; K* assembled with error e_K*)
    NLML = 1/2 err^T alpha + sum log L_jj + N / 2 log 2 pi:
    |d nlml| <= 1/2 |alpha|^T B_alpha + 1/2 c_v eps |err|^T|alpha|             (full update: err . alpha)
              | 1/2 |alpha|^T B_K |alpha| + |alpha|^T B_s |z| + 1/2 c_v eps |z|^2   (factor only: z by block_trsv, 1/2 |z|^2;
                B_s = eps [c_N |L| + c_x S (M_1 o |L|)] the substitution's backward error with W_jj on the diagonal)
              + 1/2 sum_ij |K^-1|_ij B_K,ij + eps sum_j (3 + c_v |log L_jj|)       (log det: tr K^-1 R_K; log's own ulp, the pivot's 2).
Second-order terms are dropped throughout; `Bounds` asserts eps N max F < 2^-12 so that they are below 2^-12 of the first.

Reference error is a CONDITION: N 2^-63 times the same weights must be at most 1/64 of every tolerance (`check`)."""
import functools

import numpy as np

from tests.kernel_resolution import A_COEF
from tests.util import record_margin

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble is not the 80-bit format: these tests would pass vacuously"
EPS = LD(2.0) ** -52
EPS_LD = LD(2.0) ** -63
INFL = 1.0 + 2.0 ** -30
TILE = 128
B_COEF = lambda kind, d: (d + 2) / 2 if kind == "rbf" else (d + 2) / 4 + 3   # tests/kernel_resolution.py B_DIFF at d
A_AT = lambda kind, d: A_COEF[kind] + (0.0 if kind == "rbf" else (d - 3) / 4)  # (its polynomial factor inherits s's (d + 2) / 4)


# ---- K_exact and the kernel-assembly term ----------------------------------------------------------------------------------
# The argument of the exponential is carried as an unevaluated sum hi + lo of two long doubles (error-free products by
# Veltkamp / Dekker splitting of the 64-bit significand, error-free sums by Knuth's two-sum): a plain long-double argument
# would be wrong by a few 2^-64 s RELATIVE in exp(-s), more than the 4 * 2^-63 K_exact promises at s of a few units.
_SPLIT = LD(2.0) ** 32 + 1


def _two_prod(a, b):
    p = a * b
    t = _SPLIT * a
    ah = t - (t - a)
    al = a - ah
    t = _SPLIT * b
    bh = t - (t - b)
    bl = b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def _two_sum(a, b):
    s = a + b
    v = s - a
    return s, (a - (s - v)) + (b - v)


def K_exact(kind, variance, ls, noise, X, X2=None, parts=False, grads=False):
    """K(X, X) + noise I (X2 None) or K(X, X2) in long double from the exact doubles, difference form.  ``parts``: also the
    kernel-assembly bound E_K of the docstring (long double, same shape).  ``grads`` (tests/grad_resolution.py): instead
    (K, dk/dr^2 (signed, without the noise), t [.., .., d] the scaled differences (x - x2) / ls, s the exponential's argument)."""
    assert kind in ("rbf", "matern52")
    ls = np.broadcast_to(np.asarray(ls, dtype=np.float64), (np.shape(X)[1],)).astype(LD)
    x = np.asarray(X, dtype=np.float64).astype(LD)
    x2 = x if X2 is None else np.asarray(X2, dtype=np.float64).astype(LD)
    a, b = x / ls, x2 / ls                                       # (only the weights of E_K use these)
    var = LD(variance)
    hi = np.zeros((a.shape[0], b.shape[0]), dtype=LD)           # r^2 = hi + lo
    lo = np.zeros_like(hi)
    w = np.zeros_like(hi)
    T = np.zeros(hi.shape + (a.shape[1],), dtype=LD) if grads else None
    for c in range(a.shape[1]):
        diff = x[:, None, c] - x2[None, :, c]                   # exact: doubles of one binade range in a 64-bit significand
        q = diff / ls[c]
        p, e = _two_prod(q, ls[c])
        ql = ((diff - p) - e) / ls[c]                            # t = q + ql
        sq, se = _two_prod(q, q)
        hi, e2 = _two_sum(hi, sq)
        lo += e2 + se + 2 * q * ql
        w += np.abs(q) * (np.abs(a[:, None, c]) + np.abs(b[None, :, c]))
        if grads:
            T[:, :, c] = q + ql
    r2 = hi + lo
    if kind == "rbf":
        s = r2 / 2
        K = var * (np.exp(-hi / 2) * (1 - lo / 2))
        dr2 = K / 2
    else:
        floor = LD(1e-36)
        lo = np.where(hi < floor, 0, lo)
        hi = np.maximum(hi, floor)
        vh, ve = _two_prod(LD(5), hi)
        vl = ve + 5 * lo                                         # s^2 = 5 r^2 = vh + vl
        sh = np.sqrt(vh)
        ph, pe = _two_prod(sh, sh)
        sl = (((vh - ph) - pe) + vl) / (2 * sh)                  # s = sh + sl
        s = sh + sl
        e = np.exp(-sh) * (1 - sl)
        K = var * ((1 + s + (vh + vl) / 3) * e)
        dr2 = var * LD(5) / 6 * (1 + s) * e
    if grads:
        assert not parts
        dk = -dr2                                                   # (a new array: K's diagonal takes the noise below)
    E = EPS * ((A_AT(kind, a.shape[1]) + B_COEF(kind, a.shape[1]) * s) * K + dr2 * w)
    if X2 is None:
        i = np.arange(a.shape[0])
        K[i, i] += LD(noise)
        E[i, i] += EPS * (var + LD(noise))
    if grads:
        return K, dk, T, s
    return (K, E) if parts else K


# ---- long-double linear algebra --------------------------------------------------------------------------------------------
def chol_ld(K, nb=64):
    """Blocked right-looking Cholesky in long double (N <= 640 or so)."""
    A = np.array(K, dtype=LD)
    n = A.shape[0]
    for j0 in range(0, n, nb):
        j1 = min(j0 + nb, n)
        for j in range(j0, j1):
            row = A[j, j0:j]
            piv = A[j, j] - row @ row
            assert piv > 0, f"K_exact is not positive definite at pivot {j}"
            A[j, j] = np.sqrt(piv)
            if j + 1 < n:
                A[j + 1:, j] = (A[j + 1:, j] - A[j + 1:, j0:j] @ row) / A[j, j]
        if j1 < n:
            P = A[j1:, j0:j1]
            A[j1:, j1:] -= P @ P.T
    return np.tril(A)


def solve_lower(L, B):
    """L^-1 B in long double, row by row."""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0]):
        X[i] = (X[i] - L[i, :i] @ X[:i]) / L[i, i]
    return X


def solve_upper_t(L, B):
    """L^-T B in long double."""
    X = np.array(B, dtype=LD)
    for i in range(L.shape[0] - 1, -1, -1):
        X[i] = (X[i] - L[i + 1:, i] @ X[i + 1:]) / L[i, i]
    return X


def _blocks(n, nb=TILE):
    return [(lo, min(lo + nb, n)) for lo in range(0, n, nb)]


def tri_LLt(L):
    """tril(L L^T) in long double, tile by tile (only the products that are not zero)."""
    n = L.shape[0]
    out = np.zeros((n, n), dtype=LD)
    for i0, i1 in _blocks(n):
        for j0, j1 in _blocks(i1):
            out[i0:i1, j0:j1] = L[i0:i1, :j1] @ L[j0:j1, :j1].T
    return np.tril(out)


def tri_prod(A, B):
    """A B for lower-triangular A and B in long double, tile by tile."""
    n = A.shape[0]
    out = np.zeros((n, n), dtype=LD)
    for i0, i1 in _blocks(n):
        for j0, j1 in _blocks(i1):
            out[i0:i1, j0:j1] = A[i0:i1, j0:i1] @ B[j0:i1, j0:j1]
    return out


# ---- which diagonal blocks a form inverts explicitly -----------------------------------------------------------------------------
def _tree_levels(lo, hi, depth, levels):
    """chol_inv's nodes (tgp_api.hip): split at lo + (n / 64 / 2) 64 down to the 128-leaf; children of depth k in levels[k]."""
    n = hi - lo
    if n <= TILE:
        return
    mid = lo + (n // 64 // 2) * 64
    while len(levels) <= depth:
        levels.append([])
    levels[depth] += [(lo, mid), (mid, hi)]
    _tree_levels(lo, mid, depth + 1, levels)
    _tree_levels(mid, hi, depth + 1, levels)


def form_levels(form, N, keep=None):
    """The nested levels (outermost first) of diagonal blocks whose explicit inverse multiplies, clipped to N rows:
    "substitution" (the reference: none), "dag" (the persistent kernel, every chain and plan: tiles, then the leaf's
    16-blocks), "recursion" (chol_inv's tree, then the 16-blocks), "append" (one node step at `keep` on top of tiles and
    16-blocks)."""
    if form == "substitution":
        return []
    if form == "dag":
        levels = [_blocks(N), _blocks(N, 16)]
    elif form == "append":
        assert keep is not None and 0 < keep < N
        levels = [[(0, keep), (keep, N)], _blocks(N), _blocks(N, 16)]
    else:
        assert form == "recursion"
        npad = -(-N // 256) * 256
        levels = []
        _tree_levels(0, npad, 0, levels)
        levels.append(_blocks(N, 16))
    return [[(lo, min(hi, N)) for lo, hi in lev if lo < N] for lev in levels]


class Bounds:
    """The bounds of the module docstring as operators on non-negative vectors (columns of x), for the arrays under test."""

    def __init__(self, L, W, E_K, levels, alpha_form=None):
        self.N = N = L.shape[0]
        self.alpha_form = alpha_form or ("explicit" if levels else "solve")
        self.L, self.W = np.asarray(L, dtype=np.float64), np.asarray(W, dtype=np.float64)
        self.aL, self.aW = np.abs(np.asarray(L, dtype=np.float64)), np.abs(self.W)
        self.E_K = None if E_K is None else np.asarray(E_K, dtype=LD)
        self.Ds, self.LM, self.EM = [], np.zeros((N, N)), np.zeros((N, N))
        for k, blocks in enumerate(levels):
            Dk = np.zeros((N, N))
            for lo, hi in blocks:
                if hi - lo <= TILE:
                    blk = np.asarray(np.abs(L[lo:hi, lo:hi]).astype(LD) @ np.abs(W[lo:hi, lo:hi]).astype(LD), dtype=np.float64)
                else:
                    blk = self.aL[lo:hi, lo:hi] @ self.aW[lo:hi, lo:hi]
                Dk[lo:hi, lo:hi] = blk * INFL
                if k == 0:
                    self.LM[lo:hi, lo:hi] = self.aL[lo:hi, lo:hi]
                    Lb, Wb = self.L[lo:hi, lo:hi].astype(LD), self.W[lo:hi, lo:hi].astype(LD)
                    self.EM[lo:hi, lo:hi] = np.abs(np.asarray(tri_prod(Lb, Wb) - np.eye(hi - lo, dtype=LD), dtype=np.float64)) * INFL
            self.Ds.append(Dk)
        self.c_K, self.c_N, self.c_v = (N + 1) / 2 + 4.0, N / 2 + 4.0, N / 2 + 2.0
        self.c_piv = 195.0 if levels else 0.0
        self.dL = np.diag(self.aL).copy()
        self.c_x = max([hi - lo for lo, hi in (levels[0] if levels else [])], default=0) + 4.0
        self.eps = float(EPS) * INFL
        rows = self.aL @ (self.aW @ np.ones(N))                    # row sums of F bound its entries
        assert float(EPS) * N * float(rows.max()) < 2.0 ** -12, "second-order terms are not negligible here"

    def _series(self, y, transposed):
        """(D_1 + D_2 D_1 + D_3 D_2 D_1 + ...) y over the nested levels; its transpose with ``transposed``."""
        out = np.zeros_like(y)
        if not transposed:
            term = y
            for Dk in self.Ds:
                term = Dk @ term
                out += term
            return out
        for k in range(len(self.Ds)):
            term = y
            for Dk in reversed(self.Ds[:k + 1]):
                term = Dk.T @ term
            out += term
        return out

    def _explicit(self, y, transposed):
        """(|E_M| + c_x / 2 eps D_1) y: the MEASURED right residual of the inverted blocks and the product's own rounding."""
        if not self.Ds:
            return np.zeros_like(y)
        E, D = (self.EM.T, self.Ds[0].T) if transposed else (self.EM, self.Ds[0])
        return E @ y + 0.5 * self.c_x * self.eps * (D @ y)

    def right(self, x):            # B_r x
        y = self.aL @ (self.aW @ x)
        return self.eps * (self.c_N * y + self.c_x * self._series(y, False) + self.c_piv * self.dL[:, None] * (self.aW @ x))

    def left(self, x):             # B_l x
        return (1.0 + 2.0 ** -10) * (self.aW @ self.right(self.aL @ x))

    def k_lower(self, x):          # the lower-triangular form's matrix applied to x (without E_K)
        return (self.eps * (self.c_K * (self.aL @ (self.aL.T @ x)) + self.c_piv * (self.aL @ (self.dL[:, None] * x)))
                + self.aL @ (self.LM.T @ self._explicit(x, True)))

    def k_sym(self, x):            # a bound of the symmetric |R_K| applied to x, E_K included
        g = self.c_K * (self.aL @ (self.aL.T @ x))
        m = self.aL @ (self.LM.T @ self._explicit(x, True)) + self._explicit(self.LM @ (self.aL.T @ x), False)
        e = 0.0 if self.E_K is None else np.asarray(self.E_K @ x.astype(LD), dtype=np.float64) * INFL
        piv = self.aL @ (self.dL[:, None] * x) + self.dL[:, None] * (self.aL.T @ x)
        return self.eps * (g + self.c_piv * piv) + m + e

    def alpha(self, absK, err, t, alpha):
        """The float64 reference's alpha (two substitutions with the factor: (K + dK) alpha = err, |dK| <= gamma_(3N+1) |L||L|^T):
        a vector bound of |K alpha - err|.  The device's alpha = W^T (W err) goes through `Measured.alpha_tolerance`."""
        al = np.abs(alpha)[:, None]
        return (self.eps * (3 * self.N / 2 + 6.0 - self.c_K) * (self.aL @ (self.aL.T @ al)) + self.k_sym(al))[:, 0]

    # the weights the reference's own error is measured on (`check`)
    def w_right(self, x):
        return self.aL @ (self.aW @ x)

    def w_k(self, x):
        return self.aL @ (self.aL.T @ x)


def check(what, err, tol, weight=None, N=None, bad=None):
    """err <= tol everywhere, recorded in the margin table; the reference's own error N 2^-63 `weight` is at most tol / 64
    (a stated condition).  Returns the worst err / tol; a miss is appended to ``bad`` or raised."""
    err, tol = np.abs(np.asarray(err, dtype=LD)), np.asarray(tol, dtype=LD)
    assert np.all(np.isfinite(err.astype(np.float64))), f"{what}: non-finite residual"
    if weight is not None:
        assert np.all(LD(N) * EPS_LD * np.asarray(weight, dtype=LD) <= tol / 64), f"{what}: the reference is not 64 times finer"
    worst = record_margin(what, err.astype(np.float64), tol.astype(np.float64))
    if not np.all(err <= tol):
        msg = f"{what}: residual / bound = {worst:.3g}"
        if bad is None:
            raise AssertionError(msg)
        bad.append(msg)
    return worst


# ---- the residual evaluators -------------------------------------------------------------------------------------------------
def full_ratios(L, W, alpha, K, E_K, err, levels, what="", bad=None):
    """Full evaluation (N <= 640): worst residual / bound of R_K = L L^T - K_exact (lower triangle), R_right = L W - I,
    R_left = W L - I and r_alpha = K_exact alpha - err."""
    N = L.shape[0]
    Ll, Wl = np.asarray(L, dtype=np.float64).astype(LD), np.asarray(W, dtype=np.float64).astype(LD)
    bd = Bounds(L, W, E_K, levels)
    eye = np.eye(N)
    out = {}
    G = bd.w_k(eye)
    out["R_K"] = check(f"{what} |L L^T - K|", np.tril(tri_LLt(Ll) - K), np.tril(bd.k_lower(eye) + np.asarray(E_K, dtype=np.float64) * INFL),
                       np.tril(G), N, bad)
    F = bd.w_right(eye)
    out["R_right"] = check(f"{what} |L W - I|", tri_prod(Ll, Wl) - np.eye(N, dtype=LD), bd.right(eye), F, N, bad)
    out["R_left"] = check(f"{what} |W L - I|", tri_prod(Wl, Ll) - np.eye(N, dtype=LD), bd.left(eye), bd.aW @ F @ bd.aL, N, bad)
    out["r_alpha"] = alpha_ratio(bd, Wl, alpha, K, err, what, bad)
    return out


def alpha_ratio(bd, Wl, alpha, K, err, what="", bad=None):
    al, e = np.asarray(alpha, dtype=np.float64).astype(LD), np.asarray(err, dtype=np.float64).astype(LD)
    absK = np.abs(np.asarray(K, dtype=np.float64))
    t = np.asarray(Wl @ e, dtype=np.float64)
    if bd.alpha_form == "solve":
        tol = bd.alpha(absK, np.asarray(err, dtype=np.float64), t, np.asarray(alpha, dtype=np.float64))
    else:
        tol = Measured(bd.L, Wl, alpha, K, e).alpha_tolerance(bd.c_v)
    weight = absK @ (bd.aW.T @ np.abs(t))
    return check(f"{what} |K alpha - err|", K @ al - e, tol, weight, bd.N, bad)


@functools.lru_cache(maxsize=None)
def probe_vectors(N, dense=4, seed=20251018):
    """One +-1 vector per 128-column block (zero elsewhere) and `dense` dense +-1 vectors; fixed seed."""
    rng = np.random.default_rng(seed + N)
    blocks = _blocks(N)
    V = np.zeros((N, len(blocks) + dense))
    for b, (lo, hi) in enumerate(blocks):
        V[lo:hi, b] = rng.choice([-1.0, 1.0], size=hi - lo)
    V[:, len(blocks):] = rng.choice([-1.0, 1.0], size=(N, dense))
    V.setflags(write=False)
    return V


def _probe_products(M, V, ntile, transposed=False):
    """M V (M^T V with ``transposed``) in long double; the first ``ntile`` columns of V live on one 128-row block each, so only
    that block's columns (rows) of M take part -- O(N^2) for all of them together."""
    N = M.shape[0]
    out = np.zeros((N, V.shape[1]), dtype=LD)
    for b, (lo, hi) in enumerate(_blocks(N)[:ntile]):
        blk = (M[lo:hi, :].T if transposed else M[:, lo:hi]).astype(LD)
        out[:, b] = blk @ V[lo:hi, b].astype(LD)
    dense = V[:, ntile:].astype(LD)
    for lo in range(0, N, 512):                                 # (row chunks: no N x N long-double copy)
        hi = min(lo + 512, N)
        if transposed:
            out[:, ntile:] += M[lo:hi, :].T.astype(LD) @ dense[lo:hi]
        else:
            out[lo:hi, ntile:] = M[lo:hi, :].astype(LD) @ dense
    return out


def sample_rows(N, per_tile=4, seed=7):
    """The first and last row of every 128-row block and up to ``per_tile - 2`` random ones (every row from per_tile = 128 on): a
    wrong tile shows in all of its rows."""
    if per_tile >= TILE:
        return np.arange(N)
    rng = np.random.default_rng(seed + N)
    rows = []
    for lo, hi in _blocks(N):
        rows += [lo, hi - 1] + list(rng.integers(lo, hi, size=max(0, per_tile - 2)))
    return np.unique(np.array(rows, dtype=np.int64))


def probe_ratios(L, W, alpha, K, E_K, err, levels, what="", bad=None, rows=None):
    """Tile probes (any N, O(N^2)): L (L^T v) - K_exact v, L (W v) - v and W (L v) - v row by row against the same componentwise
    bounds applied to |v|; r_alpha in full (it is a vector; skipped when ``alpha`` is None).  ``rows``: evaluate these rows only --
    then K and E_K are those ROWS of the symmetric matrices ([len(rows), N]), which is all a large N needs of K_exact."""
    N = L.shape[0]
    L, W = np.asarray(L, dtype=np.float64), np.asarray(W, dtype=np.float64)
    if rows is None:
        rows = np.arange(N)
        K, E_K = np.tril(K) + np.tril(K, -1).T, np.tril(E_K) + np.tril(E_K, -1).T
    bd = Bounds(L, W, None, levels)
    V = probe_vectors(N)
    nt = len(_blocks(N))
    Vl, aV = V.astype(LD), np.abs(V)
    Lr, Wr = L[rows].astype(LD), W[rows].astype(LD)
    out = {}
    tol_K = bd.k_sym(aV)[rows] + np.asarray(E_K @ aV.astype(LD), dtype=np.float64) * INFL
    out["R_K"] = check(f"{what} |L (L^T v) - K v|", Lr @ _probe_products(L, V, nt, True) - K @ Vl, tol_K, bd.w_k(aV)[rows], N, bad)
    out["R_right"] = check(f"{what} |L (W v) - v|", Lr @ _probe_products(W, V, nt) - Vl[rows], bd.right(aV)[rows], bd.w_right(aV)[rows], N, bad)
    out["R_left"] = check(f"{what} |W (L v) - v|", Wr @ _probe_products(L, V, nt) - Vl[rows], bd.left(aV)[rows],
                          (bd.aW @ bd.w_right(bd.aL @ aV))[rows], N, bad)
    if alpha is not None:
        bd.E_K = np.asarray(E_K, dtype=LD)
        out["r_alpha"] = alpha_ratio(bd, W.astype(LD), alpha, K, err, what, bad)
    return out


def probe_ratios_rows(L, W, kind, variance, ls, noise, X, levels, what="", bad=None, per_tile=4):
    """`probe_ratios` of L and W on `sample_rows` with only those rows of K_exact built: for sizes whose full K_exact is too
    much long-double work for a test."""
    N = L.shape[0]
    rows = sample_rows(N, per_tile)
    K, E = K_exact(kind, variance, ls, 0.0, np.asarray(X)[rows], X, parts=True)
    K[np.arange(len(rows)), rows] += LD(noise)
    E[np.arange(len(rows)), rows] += EPS * (LD(variance) + LD(noise))
    return probe_ratios(L, W, None, K, E, None, levels, what, bad, rows=rows)


# ---- the extended-precision posterior ---------------------------------------------------------------------------------------
class Posterior:
    """Long-double posterior of (kind, variance, ls, noise, mean c, X, Y): factor, alpha, z, NLML; mean / variance and the
    sensitivities beta, c at query points."""

    def __init__(self, kind, variance, ls, noise, c, X, Y):
        self.kind, self.variance, self.ls, self.noise, self.c = kind, variance, np.asarray(ls, dtype=np.float64), noise, c
        self.X = np.asarray(X, dtype=np.float64)
        self.N = N = self.X.shape[0]
        self.K, self.E_K = K_exact(kind, variance, ls, noise, X, parts=True)
        self.err = np.asarray(Y, dtype=np.float64).astype(LD) - LD(c)
        self.L = chol_ld(self.K)
        self.z = solve_lower(self.L, self.err)
        self.alpha = solve_upper_t(self.L, self.z)
        self.logdiag = np.log(np.diag(self.L))
        self.nlml = (self.z @ self.z) / 2 + self.logdiag.sum() + LD(N) / 2 * np.log(LD(8) * np.arctan(LD(1)))   # 2 pi = 8 atan 1

    def with_mean(self, c):
        """The posterior with the mean constant c instead (the same factor)."""
        import copy

        p = copy.copy(self)
        p.c, p.err = c, self.err + LD(self.c) - LD(c)
        p.z = solve_lower(self.L, p.err)
        p.alpha = solve_upper_t(self.L, p.z)
        p.nlml = (p.z @ p.z) / 2 + self.logdiag.sum() + LD(self.N) / 2 * np.log(LD(8) * np.arctan(LD(1)))
        return p

    def predict(self, Xq):
        """(mean, var, beta [N, M], c [N, M], k* [N, M], e_K* [N, M]) in long double."""
        ks, ek = K_exact(self.kind, self.variance, self.ls, 0.0, self.X, Xq, parts=True)
        cc = solve_lower(self.L, ks)
        beta = solve_upper_t(self.L, cc)
        mean = LD(self.c) + ks.T @ self.alpha
        var = LD(self.variance) - np.sum(cc * cc, axis=0)
        return mean, var, beta, cc, ks, ek


class Measured:
    """The residuals of the arrays under test applied to vectors, in long double (O(N^2) per column): the budgets of alpha and of
    the derived quantities are taken from THESE -- data of the arrays under test, each bounded on its own by `Bounds` -- instead
    of from products of worst-case bounds (|W| B_r |L| inside B_alpha made tolerances larger than the quantities they checked)."""

    def __init__(self, L, W, alpha, K, err):
        self.L, self.W = np.asarray(L, dtype=np.float64).astype(LD), np.asarray(W, dtype=np.float64).astype(LD)
        self.alpha = np.asarray(alpha, dtype=np.float64).astype(LD)
        self.K, self.err = K, np.asarray(err, dtype=LD)
        self.N = self.L.shape[0]
        self.t = self.W @ self.err                                # W err
        self.r_alpha = K @ self.alpha - self.err                  # K_exact alpha - err

    def RK(self, x):
        return self.L @ (self.L.T @ x) - self.K @ x

    def El(self, x):
        return self.W @ (self.L @ x) - x

    def ElT(self, x):
        return self.L.T @ (self.W.T @ x) - x

    def Er(self, x):
        return self.L @ (self.W @ x) - x

    def alpha_tolerance(self, c_v):
        """|K alpha - err| for alpha = W^T (W err):  E_r err + L d1 + L E_l^T t^ + K d2 - R_K alpha  with the residual terms
        MEASURED and |d| <= c_v eps of the two products' own weights."""
        a = lambda v: np.abs(v)
        aL, aW = a(self.L), a(self.W)
        e = EPS * LD(INFL)
        return (a(self.Er(self.err)) + aL @ a(self.ElT(self.t)) + a(self.RK(self.alpha))
                + c_v * e * (aL @ (aW @ a(self.err)) + a(self.K) @ (aW.T @ a(self.t))))


def posterior_tolerances(ms, post, pred):
    """(tol_mean [M], tol_var [M]): the first-order sensitivities of the module docstring with the MEASURED residuals of the
    arrays under test (``ms``) and the reference's beta, c; plus the roundings of the final products."""
    mean, var, beta, cc, ks, ek = pred
    a = lambda v: np.abs(v)
    c_v = LD(ms.N / 2 + 2.0)
    e = EPS * LD(INFL)
    ab, ac = a(beta), a(cc)
    tol_mean = ab.T @ a(ms.r_alpha) + e * (c_v * (a(ks).T @ a(ms.alpha)) + a(mean)) + a(ek).T @ a(ms.alpha)
    tol_var = (np.sum(ab * a(ms.RK(beta)), axis=0) + 2 * np.sum(ac * a(ms.El(cc)), axis=0)
               + 2 * c_v * e * np.sum(ac * (a(ms.W) @ a(ks)), axis=0) + c_v * e * np.sum(ac * ac, axis=0)
               + 2 * np.sum(ab * a(ek), axis=0) + e * LD(post.variance))
    # the reference's own error -- the long-double factor's backward error N 2^-63 |L||L|^T, through the same sensitivities -- is
    # part of the budget at 64 times its bound, so that it is at most 1/64 of every tolerance by construction
    ref = 64 * EPS_LD * post.N
    aLr = a(post.L)
    tol_mean = tol_mean + ref * (ab.T @ (aLr @ (aLr.T @ a(post.alpha))))
    tol_var = tol_var + ref * np.sum(ab * (aLr @ (aLr.T @ ab)), axis=0)
    return np.asarray(tol_mean, dtype=np.float64), np.asarray(tol_var, dtype=np.float64)


def nlml_tolerance(ms, post, factor_only):
    """Tolerance of the NLML value.  Full update (1/2 err . alpha): 1/2 |alpha_ref|^T |r_alpha| measured, the dot product's
    c_v eps, and the log determinant's |sum_j log(L_jj / L_ref,jj)| measured from the factor under test (to first order
    1/2 tr K^-1 R_K) plus eps sum_j (3 + c_v |log L_jj|) for the logarithms, the pivots and the sum.  Factor-only plan (1/2 |z|^2,
    z by block_trsv; no array to read back): the factor comes from other bursts of the same products and z from a substitution
    with W_jj on the diagonal, so the budget is 8 times the full update's measured one -- the 8 covers the other summation order
    and the explicit-inverse steps -- with |alpha_ref|^T |R_K alpha_ref| for the factor's part of the quadratic term."""
    a = lambda v: np.abs(v)
    c_v = LD(ms.N / 2 + 2.0)
    e = EPS * LD(INFL)
    al = a(post.alpha)
    dlog = a(np.sum(np.log(np.diag(ms.L) / np.diag(post.L))))
    rounding = e * (c_v * (a(post.err) @ a(ms.alpha)) / 2 + np.sum(3 + c_v * a(post.logdiag)))
    full = (al @ a(ms.r_alpha)) / 2 + dlog + rounding
    tol = 8 * (full + (al @ a(ms.RK(post.alpha))) / 2) if factor_only else full
    ref = 64 * EPS_LD * post.N * ((al @ (a(post.L) @ (a(post.L).T @ al))) / 2 + np.sum(a(post.logdiag)))   # (as above: the reference's own)
    return float(tol + ref)


# ---- the cases shared by the CPU and the GPU tests ------------------------------------------------------------------------------
D, VARIANCE, MEAN = 4, 1.3, 0.2
HYPERS = (("matern52", 1e-2), ("matern52", 1e-5), ("rbf", 1e-2), ("rbf", 1e-5))
LOW_NOISE = ("rbf", 1e-8)          # the one 1e-8 case: the long-double reference factorises it at every size used
FULL_MAX = 640


@functools.lru_cache(maxsize=None)
def problem(N):
    """(X, Y, lengthscales) of the N-point design: the oracle's synthetic Ackley problem at d = 4 (the first N of at least 8
    points: the targets are standardised)."""
    from oracle import gp_oracle as O

    X, Y = O.synthetic_problem(O.ackley, D, max(N, 8))
    X, Y = X[:N], np.asarray(Y).reshape(-1)[:N]
    X, Y, ls = np.ascontiguousarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64).reshape(-1), np.asarray(O.default_lengthscales(D))
    for a in (X, Y, ls):
        a.setflags(write=False)
    return X, Y, ls


@functools.lru_cache(maxsize=8)
def posterior(kind, noise, N):
    X, Y, ls = problem(N)
    return Posterior(kind, VARIANCE, ls, noise, MEAN, X, Y)


@functools.lru_cache(maxsize=8)
def k_parts(kind, noise, N):
    """(K_exact, E_K, err) without the long-double factor (any N)."""
    X, Y, ls = problem(N)
    K, E = K_exact(kind, VARIANCE, ls, noise, X, parts=True)
    return K, E, Y.astype(LD) - LD(MEAN)


@functools.lru_cache(maxsize=None)
def query_points(N):
    """64 points: the first 8 training inputs (cyclically when N < 8), 8 points 1e-9 lengthscales away from training inputs,
    48 uniform points."""
    X, _, ls = problem(N)
    rng = np.random.default_rng(64 + N)
    near = X[np.arange(8, 16) % N] + 1e-9 * ls * rng.choice([-1.0, 1.0], size=(8, D))
    Xq = np.concatenate([X[np.arange(8) % N], near, rng.uniform(size=(48, D))])
    Xq.setflags(write=False)
    return Xq


def reference_factor(kind, noise, N):
    """The float64 reference: the oracle's factor (difference form), scipy's triangular inverse and cho_solve alpha."""
    import scipy.linalg as sl

    from oracle import gp_oracle as O

    X, Y, ls = problem(N)
    with O.difference_form():
        st = O.gpr_update(kind, VARIANCE, ls, noise, MEAN, X, Y)
    W = sl.solve_triangular(st.L, np.eye(N), lower=True)
    alpha = sl.cho_solve((st.L, True), Y - MEAN)
    return np.tril(st.L), np.tril(W), alpha
