"""The three gradient paths -- tgp_acq_value_grad, tgp_joint_forward / tgp_joint_vjp, tgp_nlml's gradient -- judged DOWNSTREAM
of `update` (TEST INFRASTRUCTURE, no GPU code; tests/test_grad_resolution.py checks it on the CPU,
tests/test_gpu_grad_resolution.py compares the device's results with it).

tests/factor_resolution.py judges L, W and alpha.  Here the reference takes THE ENGINE'S OWN W and alpha (get_factor) as
inputs and evaluates the same function of (W, alpha, X, theta, queries) in long double; kernel values, dk/dr^2 and the scaled
differences come from the exact doubles (`K_exact(..., grads=True)`).  The budget therefore holds only roundings that the
gradient paths themselves commit.  Every tolerance is
    |got - ref| <= eps sum_terms (c + A + B s) |term|   (+ the scaled-difference term below)
with eps = 2^-52 (one rounding = eps / 2), the terms the non-negative weights of the sum under test, (A, B) the kernel-function
counts of tests/kernel_resolution.py (A_COEF / A_AT for a value, A_GRAD for dk/dx and dK/dls, B_COEF), and c counted below.

Kernel entries (csrc/tgp_kernels_grad.hip).  K* and the tail form t = fl(x / ls) - Xs: the division x / ls rounds,
|dt_c| <= eps tau_c, tau_c = (|a_c| + |b_c|) / 2 (a = x / ls, b = X / ls; the subtraction's own rounding is in B), so
    d(r^2) <= eps [(d + 2) / 2 r^2 + w],   w = 2 sum_c |t_c| tau_c           (= E_K's second term, tests/factor_resolution.py)
    E_k  = eps [(A + B s) |k| + |dk/dr^2| w]                                                           (a kernel value)
    E_dk = eps [(A_GRAD + B s) |dk_c| + |d2| w 2 |t_c| / ls_c + 2 |dk/dr^2| tau_c / ls_c]   (dk/dx_c = 2 dk/dr^2 t_c / ls_c)
    E_dl = eps [(A_GRAD + B s) |dK/dls_c| + |d2| w 2 t_c^2 / ls_c + 4 |dk/dr^2| |t_c| tau_c / ls_c]  (dK/dls_c = -2 dk/dr^2 t_c^2 / ls_c)
d2 = d^2 k / d(r^2)^2: |dk/dr^2| / 2 (rbf), |dk/dr^2| 5 / (2 (1 + s)) (matern52).  The cross terms between query points
(joint_pick_kernel, joint_vjp_coord, cov_tail) form t = fl(fl(x_i - x_j) / ls): no absolute term, one more relative rounding
on t, i.e. tau_c = |t_c| / 2 -- "direct" form below; w is then r^2 and the same formulas hold.

Products (gemm_tall, launch_gemm: f64 MFMA, any order).  An entry of W K*, W^T C, C1^T C1 or W^T W is a sum of n non-zero
products, each fused (the padding and the zeros of a triangle add exactly): at most n roundings in ANY order,
    c_p(n) = n / 2 + 2     (2: the k-split's extra adds, never more than two roundings deep at these sizes)
times the product of the absolute values, with n = i + 1 for row i of W K* (`c_rows`), N - k for row k of W^T C (`c_cols`),
N - max(i, j) for (W^T W)_ij and N for the Gram product: c_p <= N / 2 + 2 = c_N.  No order is assumed, so the tall product's
tiling is not restated.

The tail sums (grad_partial_kernel / grad_partial_wide_kernel / predict_small_partial_kernel, then the finish kernels): a lane
adds n_lane = ceil(Npad / 256) fused terms (Npad / 16 rows per slice, 16 row phases), the fold over the four phases of a wave
2 adds, the four waves through LDS 2, the 16 slice partials in order 16, the mean constant 1:
    c_s = (n_lane + 21) / 2       (11 at Npad = 256, 11.5 at 512).

acq_value_grad("nlcb", beta): mean = c + sum_k k*_k alpha_k, var = variance - sum_i C1_i^2, C1 = W k*, Z = W^T C1:
    tol_mean  = eps c_s (sum |k*||alpha| + |c|) + sum E_k |alpha|
    dC1       = eps c_rows |W||k*| + |W| E_k
    tol_var   = eps [(c_s + 1) sum C1^2 + variance] + 2 sum |C1| dC1
    dZ        = eps (c_cols |W|^T |C1| + |W|^T c_rows |W||k*|) + |W|^T |W| E_k
    tol_dmean = sum_k |alpha_k| (eps c_s |dk_k| + E_dk)
    tol_dvar  = 2 sum_k [dZ_k |dk_k| + |Z_k| (eps c_s |dk_k| + E_dk)]
and to first order through v = -(mean - beta sd), sd = sqrt(var) (2 eps), g = -dmean + beta / (2 sd) dvar:
    tol_v = tol_mean + beta (tol_var / (2 sd) + 2 eps sd) + eps (beta sd + |v|)
    tol_g = tol_dmean + beta / (2 sd) [tol_dvar + |dvar| (tol_var / (2 var) + 3 eps)] + 3/2 eps (|dmean| + beta |dvar| / (2 sd))
At beta = 0 the tail is exact (v = -mean, g = -dmean).  The beta = 2 comparison is made where var_ref >= 2^20 tol_var, so that
the division by sd stays benign (`ok`); the engine's clip at 1e-12 is far below that.

joint_forward / joint_vjp, groups [G, q, d]: cov_ij = k(x_i, x_j) - C1_i . C1_j (the Gram product; the diagonal is
variance - |C1_i|^2), Gs = gc + gc^T, D_k = sum_j Gs_ij C1_kj (joint_mix_kernel: q fused terms and Gs's own rounding),
Z' = W^T D, grad_ic = gm_i sum_k alpha_k dk_k - sum_k Z'_k dk_k + sum_{j != i} Gs_ij dk(x_i, x_j)/dx_ic:
    tol_cov = eps [(A + (B + 1) s) |k_ij| + (c_p + 1) sum_k |C1_ki||C1_kj| + |k_ij| + |cov_ij|] + sum_k (|C1_ki| dC1_kj + dC1_ki |C1_kj|)
    dD  = eps (q / 2 + 1) sum_j |Gs_ij||C1_kj| + sum_j |Gs_ij| dC1_kj,      dZ' = eps c_cols |W|^T |D| + |W|^T dD
    tol_vjp = |gm_i| tol_dmean + sum_k [dZ'_k |dk_k| + |Z'_k| (eps c_s |dk_k| + E_dk)] + sum_{j != i} |Gs_ij| E_dk(direct, A_GRAD + 1, B + 1)
              + eps (q / 2 + 3) [|gm_i||sum alpha dk| + |sum Z' dk| + sum_{j != i} |Gs_ij||dk_ij|]
(the last line: joint_vjp_coord's q fused cross terms, Gs_ij formed again, gm sa - sz).  The largest per-term coefficient is
dZ''s on |W|^T |W||K*||Gs|: 2 c_p + q / 2 + 1 = N + q / 2 + 5.

tgp_nlml's gradient: G = W^T W - alpha alpha^T, grad_theta = 1/2 sum_ij G_ij dK_ij/dtheta over the lower 64 x 64 pair tiles
(sym = 2 off the diagonal), d nlml / d mean = -sum alpha:
    tol_theta = eps / 2 sum_ij [(c_N (|W|^T |W|)_ij + c_a |alpha_i||alpha_j|) |dK_ij| + (c_red + A + B s_ij) |G_ij dK_ij|] + 1/2 sum_ij |G_ij| E'
    c_N   = c_p(N - max(i, j)) <= N / 2 + 2                     the W^T W product
    c_a   = 1 / 2                                               alpha_i alpha_j, one product
    c_red = 20:  G's subtraction 1/2, f1 = G dk/dr^2 1/2, t_c^2 1/2, the 16-row loop of a lane 16 fused adds = 8, wave_sum
                 6 adds = 3, the four-wave add 2 adds = 1, the scale -2 / ls (a division and a product) 1, nlml_final*_kernel:
                 a thread's own loop adds at most ceil((Npad / 64)^2 / 256) = 1 partial to 0 (exact) up to Npad = 1024, wave_sum 3,
                 the waves in order (4 at N <= 1024) 2:  19.5
    E' the kernel entry's absolute part: the last two terms of E_dl (lengthscales), |dk/dr^2| w / variance (variance), 0 (noise)
    tol_mean = 8 eps sum |alpha|      (a thread's ceil(N / 256) <= 4 adds, wave_sum 6, 4 waves: 14 roundings = 7)
The wide kernels (d > 32) commit the same roundings: r^2 over all dp coordinates in every chunk, the terms of a chunk's own
coordinates, the same reductions.

Cap: no counted per-term coefficient exceeds N + q + 96 eps in addition to (A + B s) (`CAP`, asserted where they are formed).
Reference error is a CONDITION, as in tests/factor_resolution.py: N 2^-63 times the same weights is at most 1/64 of every
tolerance (`check`).  Second-order terms are dropped; the inflation 1 + 2^-30 of the float64 weights covers their rounding.

`restate_*`: plain float64 numpy restatements of the three paths in the kernels' summation order -- 16 slices, 16 row phases
folded four and four, the 16 slice partials in order; 64 x 64 lower pair tiles, 16 rows per wave, sym -- which must meet every
tolerance with room (tests/test_grad_resolution.py) and in which the defects a parity tolerance cannot see are planted."""
import functools

import numpy as np

from tests import factor_resolution as F
from tests.factor_resolution import A_AT, B_COEF, EPS, INFL, K_exact, LD
from tests.kernel_resolution import A_GRAD

GT_KS, TILE, WIDE_CHUNK, MAX_D, VAR_FLOOR = 16, 64, 32, 32, 1e-12
C_A, C_RED, C_MEAN = 0.5, 20.0, 8.0
VAR_MARGIN = 2.0 ** 20
_e = float(EPS) * INFL
f64 = lambda a: np.asarray(a, dtype=np.float64)


def c_p(N):
    return N / 2 + 2.0


def c_rows(N):
    """c_p of the rows of W k* (row i of the lower-triangular W holds i + 1 entries: the zeros beyond add exactly) as a column."""
    return ((np.arange(N) + 1) / 2 + 2.0)[:, None]


def c_cols(N):
    """c_p of the rows of W^T C (column k of W holds N - k entries) as a column."""
    return ((N - np.arange(N)) / 2 + 2.0)[:, None]


def c_s(N):
    npad = -(-N // 256) * 256
    return (-(-npad // 256) + 21) / 2


def CAP(N, q=0):
    return N + q + 96.0


# ---- kernel entries in long double with their own error bounds --------------------------------------------------------------------
class Entries:
    """k, dk/dr^2, t, s of K(X, X2) in long double and the bounds E_k, E_dk, E_dl of the module docstring (float64, inflated).
    ``direct``: the form t = (x - x2) / ls of the cross terms between query points (A + 1, B + 1, no absolute term)."""

    def __init__(self, kind, variance, ls, X, X2, direct=False):
        self.kind, self.variance = kind, variance
        self.ls = np.broadcast_to(f64(ls), (np.shape(X)[1],))
        d = len(self.ls)
        self.k, self.dr2, self.t, self.s = K_exact(kind, variance, ls, 0.0, X, X2, grads=True)
        lsl = self.ls.astype(LD)
        self.dk = -2 * self.dr2[:, :, None] * self.t / lsl                    # dk / dx_c of the SECOND argument (t = (x - x2) / ls)
        self.dl = -2 * self.dr2[:, :, None] * self.t * self.t / lsl           # dK / dls_c
        at, adr, s = np.abs(f64(self.t)), np.abs(f64(self.dr2)), f64(self.s)
        if direct:
            tau, extra = at / 2, 1.0
        else:
            a, b = np.abs(f64(X) / self.ls), np.abs(f64(X2) / self.ls)
            tau, extra = (a[:, None, :] + b[None, :, :]) / 2, 0.0
        w = 2 * np.sum(at * tau, axis=2)
        d2 = adr / 2 if kind == "rbf" else adr * 2.5 / (1 + s)
        B = B_COEF(kind, d) + extra
        self.rel_k = A_AT(kind, d) + B * s                                   # (eps units, relative part)
        self.rel_d = A_GRAD[kind] + extra + B * s
        self.E_k = _e * (self.rel_k * np.abs(f64(self.k)) + adr * w)
        self.abs_dk = _e * ((d2 * w)[:, :, None] * 2 * at / self.ls + 2 * adr[:, :, None] * tau / self.ls)
        self.abs_dl = _e * ((d2 * w)[:, :, None] * 2 * at * at / self.ls + 4 * adr[:, :, None] * at * tau / self.ls)
        self.E_dk = _e * self.rel_d[:, :, None] * np.abs(f64(self.dk)) + self.abs_dk
        self.E_dkdr2_w = _e * adr * w                                        # |dk/dr^2| w: the variance term's absolute part


# ---- the three long-double references -----------------------------------------------------------------------------------------------
def nlml_gradient(kind, variance, ls, noise, X, W, alpha):
    """-> (grad [d + 3] long double in tgp_nlml's order: lengthscales, variance, noise, mean; tol [d + 3]; weight [d + 3] the
    weights the reference's own error is measured on)."""
    N, d = np.shape(X)
    Wl, al = np.asarray(W, dtype=LD), np.asarray(alpha, dtype=LD)
    en = Entries(kind, variance, ls, X, X)
    G = Wl.T @ Wl - np.outer(al, al)
    aG = np.abs(f64(G))
    aW, aa = np.abs(f64(W)), np.abs(f64(alpha))
    WW, AA = (aW.T @ aW) * INFL, np.outer(aa, aa)
    assert max(c_p(N), C_RED, C_MEAN) <= CAP(N)
    depth = N - np.maximum(np.arange(N)[:, None], np.arange(N)[None, :])     # non-zero products of (W^T W)_ij
    prod = (depth / 2 + 2.0) * WW + C_A * AA
    grad, tol, wgt = np.zeros(d + 3, dtype=LD), np.zeros(d + 3), np.zeros(d + 3)

    def one(slot, dK, rel, absolute):
        adK = np.abs(f64(dK))
        grad[slot] = np.sum(G * dK) / 2
        tol[slot] = (_e * np.sum(prod * adK + (C_RED + rel) * aG * adK) + np.sum(aG * absolute)) / 2
        wgt[slot] = np.sum((depth / N * WW + AA) * adK) / 2

    for c in range(d):
        one(c, en.dl[:, :, c], en.rel_d, en.abs_dl[:, :, c])
    one(d, en.k / LD(variance), en.rel_k, en.E_dkdr2_w / variance)
    one(d + 1, np.eye(N, dtype=LD), 0.0, 0.0)
    grad[d + 2], tol[d + 2], wgt[d + 2] = -np.sum(al), _e * C_MEAN * np.sum(aa), np.sum(aa)
    if np.asarray(alpha).dtype == np.float64:                                # (doubles: the exact sum as hi + lo, no reference error)
        import math

        hi = math.fsum(f64(alpha).tolist())
        grad[d + 2], wgt[d + 2] = -(LD(hi) + LD(math.fsum(f64(alpha).tolist() + [-hi]))), 0.0
    return grad, tol, wgt


def _tail(N, en, W, alpha, c, cols=None):
    """The arrays every tail shares at the points ``cols`` of ``en``: long-double k*, C1 = W k*, mean; float64 bounds."""
    Wl, al = np.asarray(W, dtype=LD), np.asarray(alpha, dtype=LD)
    aW, aa = np.abs(f64(W)), np.abs(f64(alpha))
    ks = en.k
    C1 = Wl @ ks
    ak = np.abs(f64(ks))
    Wk = (aW @ ak) * INFL
    dC1 = _e * c_rows(N) * Wk + aW @ en.E_k
    mean = LD(c) + ks.T @ al
    w_mean = ak.T @ aa + abs(c)
    tol_mean = _e * c_s(N) * w_mean + en.E_k.T @ aa
    # the reference's own products have the same depths: its weights carry depth / N (`check` multiplies by N 2^-63)
    return dict(Wl=Wl, al=al, aW=aW, aa=aa, ks=ks, C1=C1, aC1=np.abs(f64(C1)), Wk=Wk, dC1=dC1, mean=mean, w_mean=w_mean,
                tol_mean=tol_mean, Wk_ref=Wk * (np.arange(N) + 1)[:, None] / N, cols_ref=(N - np.arange(N))[:, None] / N)


def value_gradient(kind, variance, ls, c, X, W, alpha, Xq, beta):
    """acq_value_grad("nlcb", beta) at Xq [P, d] -> dict of long-double references (mean, var, dmean [P, d], dvar, v, g), their
    tolerances tol_*, the reference-error weights w_*, and ``ok`` [P]: where the beta > 0 comparison is made."""
    N, d = np.shape(X)
    en = Entries(kind, variance, ls, X, Xq)
    t = _tail(N, en, W, alpha, c)
    aa, aW, C1, aC1 = t["aa"], t["aW"], t["C1"], t["aC1"]
    cs, cp = c_s(N), c_p(N)
    assert max(2 * cp, cs) <= CAP(N)
    var = LD(variance) - np.sum(C1 * C1, axis=0)
    w_var = np.sum(aC1 * (aC1 + 2 * t["Wk_ref"]), axis=0)
    tol_var = _e * ((cs + 1) * np.sum(aC1 * aC1, axis=0) + variance) + 2 * np.sum(aC1 * t["dC1"], axis=0)
    Z = t["Wl"].T @ C1
    aZ = np.abs(f64(Z))
    WWk = (aW.T @ t["Wk"]) * INFL
    dZ = _e * (c_cols(N) * (aW.T @ aC1) + aW.T @ (c_rows(N) * t["Wk"])) + aW.T @ (aW @ en.E_k)
    adk = np.abs(f64(en.dk))
    E_term = _e * cs * adk + en.E_dk                                           # [N, P, d]
    dmean = np.einsum("k,kpc->pc", t["al"], en.dk)
    dvar = -2 * np.einsum("kp,kpc->pc", Z, en.dk)
    tol_dmean = np.einsum("k,kpc->pc", aa, E_term)
    tol_dvar = 2 * (np.einsum("kp,kpc->pc", dZ, adk) + np.einsum("kp,kpc->pc", aZ, E_term))
    w_dmean = np.einsum("k,kpc->pc", aa, adk)
    w_dvar = 2 * np.einsum("kp,kpc->pc", aW.T @ t["Wk_ref"] + t["cols_ref"] * (aW.T @ aC1) + aZ, adk)
    ok = f64(var) >= VAR_MARGIN * tol_var
    out = dict(mean=t["mean"], var=var, dmean=dmean, dvar=dvar, tol_mean=t["tol_mean"], tol_var=tol_var, tol_dmean=tol_dmean,
               tol_dvar=tol_dvar, w_mean=t["w_mean"], w_var=w_var, w_dmean=w_dmean, w_dvar=w_dvar, ok=ok)
    if beta == 0.0:
        out.update(v=-t["mean"], g=-dmean, tol_v=t["tol_mean"], tol_g=tol_dmean, w_v=t["w_mean"], w_g=w_dmean,
                   ok=np.ones(len(ok), dtype=bool))
        return out
    vs = np.where(ok, var, 1)                                                # (the points left out: placeholders, never compared)
    sd = np.sqrt(vs)
    sdf, b = f64(sd), float(beta)
    v = -(t["mean"] - LD(beta) * sd)
    g = -dmean + (LD(beta) / (2 * sd))[:, None] * dvar
    tol_v = t["tol_mean"] + b * (tol_var / (2 * sdf) + 2 * _e * sdf) + _e * (b * sdf + np.abs(f64(v)))
    h = (b / (2 * sdf))[:, None]
    advar = np.abs(f64(dvar))
    tol_g = (tol_dmean + h * (tol_dvar + advar * (tol_var / (2 * f64(vs)) + 3 * _e)[:, None])
             + 1.5 * _e * (np.abs(f64(dmean)) + h * advar))
    out.update(v=v, g=g, tol_v=tol_v, tol_g=tol_g, w_v=t["w_mean"] + b * w_var / (2 * sdf), w_g=w_dmean + h * w_dvar)
    return out


def joint(kind, variance, ls, c, X, W, alpha, Xg, gmean, gcov):
    """joint_forward and joint_vjp of the groups Xg [G, q, d] with the adjoints gmean [G, q], gcov [G, q, q] (any, not
    symmetric) -> dict mean [G, q], cov [G, q, q], vjp [G, q, d] in long double with tol_* and w_*.  The formula is the one
    written above joint_mix_kernel (csrc/tgp_kernels_grad.hip)."""
    Xg = f64(Xg)
    Gn, q, d = Xg.shape
    N = np.shape(X)[0]
    en = Entries(kind, variance, ls, X, Xg.reshape(-1, d))
    t = _tail(N, en, W, alpha, c)
    aW, aa, cs, cp = t["aW"], t["aa"], c_s(N), c_p(N)
    assert 2 * cp + q / 2 + 1 <= CAP(N, q)
    adk = np.abs(f64(en.dk))
    E_term = _e * cs * adk + en.E_dk
    sa = np.einsum("k,kpc->pc", t["al"], en.dk)
    tol_sa = np.einsum("k,kpc->pc", aa, E_term)
    w_sa = np.einsum("k,kpc->pc", aa, adk)
    cov, tol_cov, w_cov = (np.zeros((Gn, q, q), dtype=LD), np.zeros((Gn, q, q)), np.zeros((Gn, q, q)))
    vjp, tol_vjp, w_vjp = (np.zeros((Gn, q, d), dtype=LD), np.zeros((Gn, q, d)), np.zeros((Gn, q, d)))
    off = ~np.eye(q, dtype=bool)
    for g in range(Gn):
        sl = slice(g * q, (g + 1) * q)
        eq = Entries(kind, variance, ls, Xg[g], Xg[g], direct=True)
        kq = np.where(off, eq.k, LD(variance))
        C1, aC1, dC1 = t["C1"][:, sl], t["aC1"][:, sl], t["dC1"][:, sl]
        cov[g] = kq - C1.T @ C1
        CC = (aC1.T @ aC1) * INFL
        akq = np.abs(f64(kq))
        cross = aC1.T @ dC1
        tol_cov[g] = _e * (off * eq.rel_k * akq + (cp + 1) * CC + akq + np.abs(f64(cov[g]))) + cross + cross.T
        wc = aC1.T @ t["Wk_ref"][:, sl]                                         # (the reference's C1 is wrong by N 2^-63 |W||k*|)
        w_cov[g] = wc + wc.T + CC + 4 * akq / N                              # (K_exact: 4 * 2^-63 relative)
        gm = np.asarray(gmean[g], dtype=LD)
        Gs = np.asarray(gcov[g], dtype=LD)
        Gs = Gs + Gs.T
        aGs = np.abs(f64(Gs))
        D = C1 @ Gs.T                                                       # D[k, i] = sum_j Gs_ij C1_kj
        Zp = t["Wl"].T @ D
        aD, aZp = np.abs(f64(D)), np.abs(f64(Zp))
        dD = _e * (q / 2 + 1) * (aC1 @ aGs.T) + dC1 @ aGs.T
        dZp = _e * c_cols(N) * (aW.T @ aD) + aW.T @ dD
        dkg, adkg, Eg = en.dk[:, sl], adk[:, sl], E_term[:, sl]
        sz = np.einsum("kp,kpc->pc", Zp, dkg)
        tol_sz = np.einsum("kp,kpc->pc", dZp, adkg) + np.einsum("kp,kpc->pc", aZp, Eg)
        Go = np.where(off, Gs, 0)
        aGo = np.abs(f64(Go))
        cr = -np.einsum("ij,ijc->ic", Go, eq.dk)                             # d k(x_i, x_j) / d x_i = -d / d x_j
        tol_cr = np.einsum("ij,ijc->ic", aGo, eq.E_dk)
        w_cr = np.einsum("ij,ijc->ic", aGo, np.abs(f64(eq.dk)))
        agm = np.abs(f64(gm))[:, None]
        vjp[g] = gm[:, None] * sa[sl] - sz + cr
        tol_vjp[g] = (agm * tol_sa[sl] + tol_sz + tol_cr
                      + _e * (q / 2 + 3) * (agm * np.abs(f64(sa[sl])) + np.abs(f64(sz)) + w_cr))
        WWkG = aW.T @ (t["Wk_ref"][:, sl] @ aGs.T) + t["cols_ref"] * (aW.T @ aD)   # (|W|^T |W||K*||Gs_i|)_k at the reference's depths
        w_vjp[g] = agm * w_sa[sl] + np.einsum("kp,kpc->pc", WWkG + aZp, adkg) + w_cr
    return dict(mean=t["mean"].reshape(Gn, q), tol_mean=t["tol_mean"].reshape(Gn, q), w_mean=t["w_mean"].reshape(Gn, q),
                cov=cov, tol_cov=tol_cov, w_cov=w_cov, vjp=vjp, tol_vjp=tol_vjp, w_vjp=w_vjp)


# ---- plain float64 restatements in the kernels' summation order, and the planted defects ---------------------------------------
def _k64(kind, variance, r2, r2_dr2=None):
    """(k, dk/dr^2) in float64 as csrc/tgp_dev.hpp writes them; ``r2_dr2``: another r^2 for dk/dr^2 (a planted defect)."""
    q = r2 if r2_dr2 is None else r2_dr2
    if kind == "rbf":
        return variance * np.exp(-0.5 * r2), -0.5 * variance * np.exp(-0.5 * q)
    s = 2.23606797749979 * np.sqrt(np.maximum(r2, 1e-36))
    sq = 2.23606797749979 * np.sqrt(np.maximum(q, 1e-36))
    return variance * (1.0 + s + s * s / 3.0) * np.exp(-s), -(5.0 / 6.0) * variance * (1.0 + sq) * np.exp(-sq)


def _r2(t):
    r2 = np.zeros(t.shape[:-1])
    for c in range(t.shape[-1]):
        r2 = r2 + t[..., c] * t[..., c]
    return r2


def slice_sum(T, N, drop_slice=None):
    """sum over the rows (axis 0) of T [N, ...] as grad_partial_kernel and grad_finish_kernel add them: GT_KS slices of
    Npad / 16 rows, 16 row phases per slice (row = slice start + 16 n + phase), the phases of a wave folded (0 + 1) + (2 + 3), the
    four waves (0 + 1) + (2 + 3), the 16 slice partials in order.  ``drop_slice``: that partial is lost (a planted defect)."""
    npad = -(-N // 256) * 256
    chunk = npad // GT_KS
    pad = np.zeros((npad,) + T.shape[1:])
    pad[:N] = T
    A = pad.reshape((GT_KS, chunk // 16, 4, 4) + T.shape[1:])              # slice, n, wave, phase
    lane = A[:, 0]
    for n in range(1, chunk // 16):
        lane = lane + A[:, n]
    wave = (lane[:, :, 0] + lane[:, :, 1]) + (lane[:, :, 2] + lane[:, :, 3])
    part = (wave[:, 0] + wave[:, 1]) + (wave[:, 2] + wave[:, 3])
    total = np.zeros(T.shape[1:])
    for ks in range(GT_KS):
        if ks != drop_slice:
            total = total + part[ks]
    return total


def _entries64(kind, variance, ls, X, Xq, f32_row=None):
    """float64 k* [N, P], dk/dx [N, P, d] in the tail's form t = Xq / ls - X / ls."""
    t = (f64(Xq) / ls)[None, :, :] - (f64(X) / ls)[:, None, :]
    r2 = _r2(t)
    q = None
    if f32_row is not None:                                                   # dk/dr^2 of one training row from a float32 r^2
        q = r2.copy()
        q[f32_row] = r2[f32_row].astype(np.float32).astype(np.float64)
    k, dr2 = _k64(kind, variance, r2, q)
    return k, (2.0 * dr2)[:, :, None] * t / ls


def restate_value_gradient(kind, variance, ls, c, X, W, alpha, Xq, beta, defect=None):
    """-> (v [P], g [P, d], mean, var_raw, dmean, dvar) in float64.  Defects: "drop_slice" (slice 8), "skip_last_row",
    "f32_r2" (training row N // 2)."""
    N = np.shape(X)[0]
    ls, W, alpha = np.broadcast_to(f64(ls), (np.shape(X)[1],)), f64(W), f64(alpha)
    k, dk = _entries64(kind, variance, ls, X, Xq, N // 2 if defect == "f32_r2" else None)
    C1 = W @ k
    Z = W.T @ C1
    live = np.ones(N)
    if defect == "skip_last_row":
        live[N - 1] = 0.0
    drop = 8 if defect == "drop_slice" else None
    ssum = lambda T: slice_sum(T * live.reshape((N,) + (1,) * (T.ndim - 1)), N, drop)
    mean = ssum(k * alpha[:, None]) + c
    var = variance - ssum(C1 * C1)
    dmean = ssum(alpha[:, None, None] * dk)
    dvar = -2.0 * ssum(Z[:, :, None] * dk)
    sd = np.sqrt(np.maximum(var, VAR_FLOOR))
    v = -(mean - beta * sd)
    g = -dmean + (beta / (2.0 * sd))[:, None] * dvar
    return v, g, mean, var, dmean, dvar


def restate_joint(kind, variance, ls, c, X, W, alpha, Xg, gmean, gcov, defect=None):
    """-> (mean [G, q], cov [G, q, q], vjp [G, q, d]) in float64.  Defects: "gs_one_triangle" (Gs = 2 gc in group 0),
    "skip_cross_last" (the cross term j = q - 1 skipped), "f32_r2"."""
    Xg = f64(Xg)
    Gn, q, d = Xg.shape
    N = np.shape(X)[0]
    ls, W, alpha = np.broadcast_to(f64(ls), (d,)), f64(W), f64(alpha)
    k, dk = _entries64(kind, variance, ls, X, Xg.reshape(-1, d), N // 2 if defect == "f32_r2" else None)
    C1 = W @ k
    mean = (slice_sum(k * alpha[:, None], N) + c).reshape(Gn, q)
    sa = slice_sum(alpha[:, None, None] * dk, N)
    cov, vjp = np.zeros((Gn, q, q)), np.zeros((Gn, q, d))
    for g in range(Gn):
        sl = slice(g * q, (g + 1) * q)
        t = (Xg[g][:, None, :] - Xg[g][None, :, :]) / ls
        kq, dr2 = _k64(kind, variance, _r2(t))
        S = np.tril(C1[:, sl].T @ C1[:, sl])
        S = S + np.tril(S, -1).T                                              # (the lower triangle is read for both)
        cov[g] = kq - S
        cov[g][np.arange(q), np.arange(q)] = np.maximum(variance - np.diag(S), VAR_FLOOR)
        gc = f64(gcov[g])
        Gs = 2.0 * gc if (defect == "gs_one_triangle" and g == 0) else gc + gc.T
        D = np.zeros((N, q))
        for j in range(q):
            D = D + Gs[:, j][None, :] * C1[:, sl][:, j][:, None]
        Zp = W.T @ D
        grad = f64(gmean[g])[:, None] * sa[sl] - slice_sum(Zp[:, :, None] * dk[:, sl], N)
        for j in range(q - 1 if defect == "skip_cross_last" else q):
            cross = Gs[:, j][:, None] * ((2.0 * dr2[:, j])[:, None] * t[:, j, :] / ls)
            cross[j] = 0.0
            grad = grad + cross
        vjp[g] = grad
    return mean, cov, vjp


def _tree(a, axis):
    """wave_sum: a butterfly over the 64 lanes."""
    a = np.moveaxis(a, axis, 0)
    while a.shape[0] > 1:
        h = a.shape[0] // 2
        a = a[:h] + a[h:]
    return a[0]


def restate_nlml_gradient(kind, variance, ls, noise, X, W, alpha, defect=None):
    """-> grad [d + 3] in float64 as nlml_grad_kernel / nlml_grad_wide_kernel and nlml_final*_kernel add it.  Defects:
    "tile_once" (the pair tile (1, 0) weighted 1), "skip_last_row", "wide_chunk" (the last chunk's lengthscale terms from
    chunk 0's coordinates)."""
    N, d = np.shape(X)
    ls, W, alpha = np.broadcast_to(f64(ls), (d,)), f64(W), f64(alpha)
    npad = -(-N // 256) * 256
    nb = npad // TILE
    Xs = np.zeros((npad, d))
    Xs[:N] = f64(X) / ls
    al = np.zeros(npad)
    al[:N] = alpha
    Kinv = np.zeros((npad, npad))
    Kinv[:N, :N] = W.T @ W
    live = np.zeros((npad, npad), dtype=bool)
    live[:N - 1 if defect == "skip_last_row" else N, :N] = True
    G = np.where(live, Kinv - al[:, None] * al[None, :], 0.0)
    t = Xs[:, None, :] - Xs[None, :, :]
    ds2 = t * t
    r2 = np.zeros((npad, npad))
    for c in range(d):
        r2 = r2 + ds2[:, :, c]
    k, dr2 = _k64(kind, variance, r2)
    if defect == "wide_chunk":
        assert d > MAX_D
        c0 = (d - 1) // WIDE_CHUNK * WIDE_CHUNK
        ds2 = ds2.copy()
        ds2[:, :, c0:] = ds2[:, :, :d - c0]
    terms = np.concatenate([(G * dr2)[:, :, None] * ds2, (G * k)[:, :, None], (G * np.eye(npad))[:, :, None]], axis=2)
    A = terms.reshape(nb, 4, 16, nb, TILE, d + 2)                             # tile row, wave, row of the wave, tile column, lane
    acc = A[:, :, 0]
    for r in range(1, 16):
        acc = acc + A[:, :, r]
    wave = _tree(acc, 3)                                                      # [tile row, wave, tile column, term]
    tile = (wave[:, 0] + wave[:, 1]) + (wave[:, 2] + wave[:, 3])
    by, bx = np.meshgrid(np.arange(nb), np.arange(nb), indexing="ij")
    sym = np.where(bx > by, 0.0, np.where(bx == by, 1.0, 2.0))
    if defect == "tile_once":
        sym[1, 0] = 1.0
    part = sym[:, :, None] * tile
    part[:, :, :d] *= -2.0 / ls
    part[:, :, d] /= variance
    flat = np.zeros((64 * -(-nb * nb // 64), d + 2))
    flat[:nb * nb] = part.reshape(nb * nb, d + 2)
    waves = _tree(flat.reshape(-1, 64, d + 2), 1)
    total = np.zeros(d + 2)
    for w in waves:
        total = total + w
    return np.concatenate([0.5 * total, [-np.sum(alpha)]])


# ---- the cases shared by the CPU and the GPU tests -------------------------------------------------------------------------------
SIZES = (17, 130, 256, 257, 386)
P_SIZES = (1, 17, 64)
GROUPS = ((1, 5), (2, 8), (5, 14), (17, 3), (64, 1))                          # (q, G)
CASES = [(kind, noise, N, 4) for kind, noise in F.HYPERS for N in SIZES] + [("matern52", 1e-2, 130, 13), ("rbf", 1e-5, 130, 40)]


@functools.lru_cache(maxsize=None)
def design(N, d):
    """(X, Y, lengthscales, query points [72, d]).  d = 4: `problem` and `query_points` of tests/factor_resolution.py, eight more
    uniform points behind them (5 x 14 points straddle joint_mix_kernel's 64-column block).  d = 13, 40: built the same way with
    ARD lengthscales 0.2 sqrt(d) (0.85 .. 1.15), for which the median off-diagonal K lies in [0.05, 0.5]
    (tests/test_grad_resolution.py asserts it)."""
    rng = np.random.default_rng(6400 + 8 * N + d)
    if d == F.D:
        X, Y, ls = F.problem(N)
        Xq = np.concatenate([F.query_points(N), rng.uniform(size=(8, d))])
    else:
        from oracle import gp_oracle as O

        X, Y = O.synthetic_problem(O.ackley, d, max(N, 8))
        X, Y = np.ascontiguousarray(X[:N], dtype=np.float64), f64(Y).reshape(-1)[:N].copy()
        ls = 0.2 * np.sqrt(d) * (0.85 + 0.3 * ((0.6180339887498949 * np.arange(1, d + 1)) % 1.0))
        near = X[np.arange(8, 16) % N] + 1e-9 * ls * rng.choice([-1.0, 1.0], size=(8, d))
        Xq = np.concatenate([X[np.arange(8) % N], near, rng.uniform(size=(56, d))])
    for a in (X, Y, ls, Xq):
        a.setflags(write=False)
    return X, Y, ls, Xq


@functools.lru_cache(maxsize=None)
def adjoints(q, G, upper=False):
    """Random normal gmean [G, q] and NON-symmetric gcov [G, q, q]; ``upper``: gcov strictly upper triangular."""
    rng = np.random.default_rng(1000 * q + G)
    gm, gc = rng.standard_normal((G, q)), rng.standard_normal((G, q, q))
    if upper:
        gc = np.triu(gc, 1)
    gm.setflags(write=False)
    gc.setflags(write=False)
    return gm, gc


def reference_factor(kind, noise, N, d):
    """The float64 (L, W, alpha) of a case: the oracle's factor (difference form), scipy's inverse and cho_solve."""
    if d == F.D:
        return F.reference_factor(kind, noise, N)
    import scipy.linalg as sl

    from oracle import gp_oracle as O

    X, Y, ls, _ = design(N, d)
    with O.difference_form():
        st = O.gpr_update(kind, F.VARIANCE, ls, noise, F.MEAN, X, Y)
    W = sl.solve_triangular(st.L, np.eye(N), lower=True)
    return np.tril(st.L), np.tril(W), sl.cho_solve((st.L, True), Y - F.MEAN)


def compare(what, got, ref, tol, weight, N, bad, mask=None):
    """`check` of tests/factor_resolution.py (the margin recorded, the reference 64 times finer) on the entries ``mask``."""
    got, ref, tol, weight = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD), f64(tol), f64(weight)
    assert got.shape == ref.shape == tol.shape, (what, got.shape, ref.shape, tol.shape)
    if mask is not None:
        m = np.broadcast_to(mask.reshape(mask.shape + (1,) * (got.ndim - mask.ndim)), got.shape)
        got, ref, tol, weight = got[m], ref[m], tol[m], weight[m]
    return F.check(what, got - ref, tol, weight, N, bad)
