"""The numpy side of the float32 pre-screen of the pruned EI arg-max (TEST INFRASTRUCTURE; tests/test_prescreen_cases.py on
the CPU, tests/test_gpu_prune_prescreen.py on the GPU; on general models tests/test_prune_general_cases.py and
tests/test_gpu_prune_general.py).  DESIGN.md 4.1 has the derivation.

Phase 0 forms every candidate's posterior mean in float32 kernel arithmetic,

    a = float32(rs (Xq / ls - Xs_0)),  b_k = float32(rs (Xs_k - Xs_0)),  rs = sqrt(SCALE)     (centred in float64, then rounded)
    q_k = sum_c (a_c - b_kc)^2  in float32,   f_k = shape(q_k)  with float32 sqrt and exp2,
    mean32 = variance sum_k alpha_k f_k + c   in float64,

and holds |mean32 - mean| <= E with u = 2^-24, S = |a|_2 + max_k |b_k|_2:

    E = |alpha|_1 variance (1.0625 u [G1 S + G2 (2 dp + 10) + 10] + 2^-53 [2 G1 (rs |Xs_0| + S) + 256 + Npad] + 2^-60)
        + 2^-50 (|mean32| + |eta|).

``restate`` is that arithmetic in the kernel's order (numpy's float32 sqrt is correctly rounded and its exp2 is libm's: both
inside the 2 ulp the bound grants the hardware instructions; a float32 fma is restated as the float64 sum rounded once more,
which differs from the fused one by a double rounding the bound's 2 dp roundings cover)."""
import functools
import math

import numpy as np
from scipy.linalg import cho_solve

from oracle import gp_oracle as O
from tests import prune_cases as PC
from tests import prune_screen_cases as S

U = 2.0 ** -24
L2E = 1.4426950408889634
KINDS = ("rbf", "matern12", "matern32", "matern52")
SCALE = {"rbf": 0.5 * L2E, "matern12": L2E * L2E, "matern32": 3.0 * L2E * L2E, "matern52": 5.0 * L2E * L2E}
G1 = {"rbf": 0.72, "matern12": 0.70, "matern32": 0.26, "matern52": 0.20}    # >= sup 2 sqrt(q) |f'(q)|
G2 = {"rbf": 0.37, "matern12": 0.19, "matern32": 0.28, "matern52": 0.31}    # >= sup q |f'(q)|
FLOOR = {k: 1e-36 * SCALE[k] for k in KINDS}
TAIL_INFLATE, MIN_BOUND = 1.0 + 4e-5, 1e-290
F32 = np.float32


def dpad(d):
    return next(p for p in (2, 4, 6, 8, 16) if d <= p)


def shape32(kind, q):
    """The shape on float32 q, float32 arithmetic throughout."""
    q = q.astype(F32)
    if kind == "rbf":
        return np.exp2(-q)
    il, il2 = F32(1.0 / L2E), F32(1.0 / (3.0 * L2E * L2E))
    qc = np.maximum(q, F32(FLOOR[kind]))
    v = np.sqrt(qc)
    e = np.exp2(-v)
    if kind == "matern12":
        return e
    p = (il.astype(np.float64) * v + 1.0).astype(F32)                     # fmaf(IL, v, 1)
    if kind == "matern32":
        return p * e
    return (il2.astype(np.float64) * qc + p).astype(F32) * e              # fmaf(IL2, qc, p)


def shape_true(kind, q):
    """The shape in extended precision on q = SCALE r^2."""
    q = np.asarray(q, dtype=np.longdouble)
    if kind == "rbf":
        return np.exp2(-q)
    s = np.sqrt(np.maximum(q, np.longdouble(FLOOR[kind]))) / np.longdouble(L2E)
    poly = {"matern12": 1.0, "matern32": 1.0 + s, "matern52": 1.0 + s + s * s / 3.0}[kind]
    return poly * np.exp(-s)


def restate(kind, variance, ls, X, alpha, mean_const, Xq, centre_after_rounding=False):
    """-> (mean32 [M], an [M]): the device's float32 mean and the candidates' scaled centred norms.
    ``centre_after_rounding`` plants the defect the design rules out: the operands rounded first, centred in float32."""
    rs = math.sqrt(SCALE[kind])
    Xs, xr = X / ls, Xq / ls
    a64, b64 = rs * (xr - Xs[0]), rs * (Xs - Xs[0])
    if centre_after_rounding:
        a = (rs * xr).astype(F32) - (rs * Xs[0]).astype(F32)
        b = (rs * Xs).astype(F32) - (rs * Xs[0]).astype(F32)
    else:
        a, b = a64.astype(F32), b64.astype(F32)
    q = np.zeros((Xq.shape[0], X.shape[0]), dtype=F32)
    for c in range(X.shape[1]):
        t = (a[:, c, None] - b[None, :, c]).astype(np.float64)             # float32 subtraction, held in float64
        q = (t * t + q).astype(F32)
    f = shape32(kind, q).astype(np.float64)
    return variance * (f @ alpha) + mean_const, np.sqrt((a64 * a64).sum(1))


def true_mean(kind, variance, ls, X, alpha, mean_const, Xq):
    """The mean in extended precision from the raw inputs (long double: 64-bit significand)."""
    ld = np.longdouble
    xr, Xs = Xq.astype(ld) / ls.astype(ld), X.astype(ld) / ls.astype(ld)
    r2 = np.zeros((Xq.shape[0], X.shape[0]), dtype=ld)
    for c in range(X.shape[1]):
        t = xr[:, c, None] - Xs[None, :, c]
        r2 += t * t
    return ld(variance) * (shape_true(kind, ld(SCALE[kind]) * r2) @ alpha.astype(ld)) + ld(mean_const)


def model_extent(kind, ls, X):
    """-> (xmax, x0): the largest rs |Xs_k - Xs_0|_2 over the rows and rs |Xs_0|_2."""
    rs = math.sqrt(SCALE[kind])
    Xs = X / ls
    return rs * math.sqrt(((Xs - Xs[0]) ** 2).sum(1).max()), rs * math.sqrt((Xs[0] ** 2).sum())


def bound(kind, d, npad, l1, variance, an, xmax, x0, m32, eta, drop=None):
    """E per candidate.  ``drop`` plants a defect: one term of c left out ("conversion", "chain" or "direct")."""
    s = an + xmax
    terms = {"conversion": G1[kind] * s, "chain": G2[kind] * (2 * dpad(d) + 10), "direct": 10.0}
    c32 = 1.0625 * U * sum(v for k, v in terms.items() if k != drop)
    c64 = 2.0 ** -53 * (2.0 * G1[kind] * (x0 + s) + 256.0 + npad)
    return l1 * variance * (c32 + c64 + 2.0 ** -60) + 2.0 ** -50 * (np.abs(m32) + abs(eta))


def lower_seed(eta, m32, E, round_up=False):
    """eta - mean32 - E rounded DOWN (``round_up``: the planted defect, the same two roundings pushed up instead)."""
    s = (eta - m32) - E
    return np.nextafter(s, np.inf) if round_up else np.where(s > 0.0, s * (1.0 - 2.0 ** -50), 0.0)


def block_quantities(eta, variance, m32, E):
    """-> (ub32 [blocks], prebest): the pre-screen's bound per 128-candidate block and its lower seed over all of them."""
    m = m32.shape[0]
    nblk = -(-m // PC.CAND_BLOCK)
    with np.errstate(over="ignore"):
        ok = (E * E <= variance) & np.isfinite(m32)      # E above the prior standard deviation says nothing
    with np.errstate(all="ignore"):
        t = PC.ei_tail(eta - (m32 - E), np.full_like(m32, max(variance, O.VAR_FLOOR)))
    ub = np.where(ok & ~np.isnan(t), np.maximum(t * TAIL_INFLATE, MIN_BOUND), np.inf)
    seed = np.where(ok, lower_seed(eta, m32, E), 0.0)
    pad = nblk * PC.CAND_BLOCK - m
    ub = np.concatenate([ub, np.full(pad, -np.inf)]).reshape(nblk, PC.CAND_BLOCK).max(1)
    seed = np.concatenate([seed, np.zeros(pad)]).reshape(nblk, PC.CAND_BLOCK).max(1)
    seed = np.where(np.isinf(ub), 0.0, seed)
    return ub, float(seed.max())


def dismissed(ub32, prebest):
    return (prebest > PC.MIN_BEST) & (ub32 * PC.MARGIN < prebest)


@functools.lru_cache(maxsize=None)
def model_alpha(name):
    st, _ = PC.oracle_state(name)
    alpha = cho_solve((st.L, True), st.err)
    alpha.setflags(write=False)
    return alpha


def restated_blocks(name, label, Xq):
    """-> (ub32 [blocks], prebest, m32, E) of a prune_cases model over candidates Xq at a threshold of prune_screen_cases."""
    st, _ = PC.oracle_state(name)
    p = PC.problem(name)
    alpha = model_alpha(name)
    eta = S.threshold(name, label)
    m32 = np.empty(Xq.shape[0])
    an = np.empty(Xq.shape[0])
    for lo in range(0, Xq.shape[0], 4096):
        m32[lo: lo + 4096], an[lo: lo + 4096] = restate(p.kind, p.variance, p.ls, p.X, alpha, p.mean_const, Xq[lo: lo + 4096])
    xmax, x0 = model_extent(p.kind, p.ls, p.X)
    npad = -(-p.N // PC.ROW_BLOCK) * PC.ROW_BLOCK
    E = bound(p.kind, p.d, npad, np.abs(alpha).sum(), p.variance, an, xmax, x0, m32, eta)
    ub32, prebest = block_quantities(eta, p.variance, m32, E)
    return ub32, prebest, m32, E


# The recorded case of the GPU test's count condition: on the whole plain set the restatement dismisses `dismissed` blocks,
# at least half of the oracle's S.RECORDED[name]["screened"][label] (tests/test_prescreen_cases.py recomputes it)
SHARE_CASE = ("m52_N512_d8", "eta")
SHARE_DISMISSED = 1024
# The same on a general model, one whose variance (1e-4) lies below every E: under a cap E <= variance, a length compared
# with its square, phase 0 dismissed nothing here (tests/test_prune_general_cases.py recomputes the count)
SHARE_CASE_GENERAL = ("g_m32_d3_N513_small", "eta+3")
SHARE_DISMISSED_GENERAL = 1023
