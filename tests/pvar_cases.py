"""Inputs, scaled references, bounds and restated chunk rules for tests/test_gpu_pvar_edges.py (TEST INFRASTRUCTURE; imports
without a GPU; tests/test_pvar_cases.py proves this file's own conditions on the CPU).

A. RANGE.  A base matrix A0 = covariances(q, 3, seed) + jitter and integer exponents s: the batch is D A0 D, D = diag(2^s_i),
   called with jitter 0.  The scaling is exact in the kernel and in the reference while nothing leaves the normal range
   (tests/pvar_reference.py ``reference_scaled``), so one 50-digit factorisation per base matrix serves every pattern.  What the
   patterns steer is the RUNNING PRODUCT of the pivots, the kernel's det: where it leaves the normal range part-way the kernel
   returns exp(logdet) instead (``chol_rows_reg``'s ``inrange``, ``pvar_det``).  ``range_cases`` names for every pattern the path
   it must take and the class of its determinant; ``running_product`` is the float64 product of the reference's pivots, from
   which tests/test_pvar_cases.py proves both with a margin of 2^8 each way.
B. PIVOTS.  Every position a bad pivot can take relative to the 16-blocks, and every kind of bad pivot.
C. CHUNKS.  The two chunk rules of trieste_amd/csrc/tgp_api.hip restated (they mirror that file and must move with it), rows of
   G = chunk + 3 groups tiled from a bank of 257, and the model, candidates and tolerance of the ``pvar_values`` row."""
from __future__ import annotations

import functools
import math
from dataclasses import dataclass

import numpy as np

from oracle import gp_oracle as O
from tests import pvar_reference as R

U = R.U
JITTER = 1e-6
TINY, HUGE = 2.0 ** -1022, np.finfo(np.float64).max

# ---- A. range ---------------------------------------------------------------------------------------------------------------
RANGE_QS = (16, 33, 64)            # the wave form; the block form with a pad; the block form with four full 16-blocks
RANGE_C = {16: 70, 33: 40, 64: 40}
OVER_SUM = {16: (600,), 33: (600,), 64: (600, 800)}   # det(A0) of the q = 64 bases is about 2^-320: 4^600 of it is 2^880, no overflow


@functools.lru_cache(maxsize=None)
def range_bases(q: int) -> np.ndarray:
    """[3, q, q] ([1, 64, 64]: a 50-digit factorisation at q = 64 takes as long as the rest of the test): the base matrices,
    jitter folded in.  Read-only."""
    A = R.covariances(q, 3, seed=300 + q)[:1 if q == 64 else 3] + JITTER
    A.setflags(write=False)
    return A


def log2_pivots(A0) -> np.ndarray:
    """log2 of the reference's pivots L_ii^2 of A0."""
    logs = R._unscaled_parts(np.ascontiguousarray(A0).tobytes(), A0.shape[0])[0]
    return np.array([float(2 * v) for v in logs]) / math.log(2.0)


def scaled_pivots(A0, s) -> np.ndarray:
    """The reference's pivots of D A0 D, 4^s_i L_ii^2, to float64 (the power of two applied exactly)."""
    lp = log2_pivots(A0)
    return np.ldexp(np.exp2(lp - np.floor(lp)), (np.floor(lp) + 2 * np.asarray(s)).astype(int))


def running_product(A0, s) -> np.ndarray:
    """The float64 running product of the reference's pivots of D A0 D, multiplied in the kernel's order."""
    out, p = np.empty(len(s)), 1.0
    with np.errstate(over="ignore", under="ignore"):
        for i, v in enumerate(scaled_pivots(A0, s)):
            p = p * v
            out[i] = p
    return out


def _spread(total: int, n: int) -> np.ndarray:
    """n integers as equal as they can be that sum to total."""
    base, rest = divmod(int(total), n)
    out = np.full(n, base, dtype=np.int64)
    out[:rest] += 1
    return out


def small_then_large(q: int, c: int, net: int = 0) -> np.ndarray:
    """-c on the first half, +c on the second (the middle row of an odd q stays 0): the product falls below 2^-1022 part-way
    and the exponents sum to 0.  A net shift goes where it keeps the product leaving the range in the first half: a negative
    one onto the first half, a positive one onto the second."""
    h = q // 2
    s = np.zeros(q, dtype=np.int64)
    s[:h], s[q - h:] = -c, c
    if net < 0:
        s[:h] += _spread(net, h)
    elif net > 0:
        s[q - h:] += _spread(net, h)
    return s


def interleaved(q: int, c: int) -> np.ndarray:
    s = np.zeros(q, dtype=np.int64)
    s[:2 * (q // 2)] = np.tile([-c, c], q // 2)
    return s


def dip(A0) -> np.ndarray:
    """The first half scaled down until the product after its last pivot is about 2^-1064 -- SUBNORMAL, ten bits left,
    neither zero nor normal -- and the second half scaled up by as much: the product comes back into the normal range, short
    of the bits it lost, within the next 16-block.  Zero and infinity stay what they are under further factors, so this is the only pattern
    at which a range flag that forgets between two 16-blocks returns a wrong determinant."""
    q = A0.shape[0]
    h = q // 2
    total = int(round((-1064.0 - log2_pivots(A0)[:h].sum()) / 2.0))
    s = np.zeros(q, dtype=np.int64)
    s[:h], s[q - h:] = _spread(total, h), _spread(-total, h)
    return s


@dataclass(frozen=True)
class RangeCase:
    name: str
    base: int            # which of the three base matrices
    s: tuple             # the exponents
    by_exp: bool         # the kernel must take exp(logdet): the running product leaves the normal range part-way
    det_class: str       # "normal", "subnormal", "zero" or "inf": where the reference's determinant lies


@functools.lru_cache(maxsize=None)
def range_cases(q: int):
    """Every pattern on every base matrix: 3 x 10 (at q = 64: 11) batches of one mixed call."""
    c, out = RANGE_C[q], []
    for b, A0 in enumerate(range_bases(q)):
        l2det = log2_pivots(A0).sum()
        pats = [("unscaled", np.zeros(q, dtype=np.int64), False, "normal"),
                ("small-then-large", small_then_large(q, c), True, "normal"),
                ("large-then-small", -small_then_large(q, c), True, "normal"),
                ("interleaved", interleaved(q, c), False, "normal"),
                ("dip", dip(A0), True, "normal"),
                ("net+250", small_then_large(q, c, 250), True, "normal"),
                ("net-250", small_then_large(q, c, -250), True, "normal"),
                ("sum-600", small_then_large(q, c, -600), True, "zero"),
                ("subnormal", small_then_large(q, c, int(round((-1045.0 - l2det) / 2.0))), True, "subnormal")]
        for over in OVER_SUM[q]:
            pats.append((f"sum+{over}", small_then_large(q, c, over), True, "inf" if l2det + 2 * over > 1024 else "normal"))
        out += [RangeCase(n, b, tuple(int(v) for v in s), e, k) for n, s, e, k in pats]
    return tuple(out)


def range_batch(q: int) -> np.ndarray:
    """[len(range_cases(q)), q, q]: D A0 D of every case (exact: powers of two)."""
    A = range_bases(q)
    return np.stack([np.ldexp(A[c.base], np.add.outer(c.s, c.s)) for c in range_cases(q)])


# ---- B. pivots --------------------------------------------------------------------------------------------------------------
PIVOT_QS = (7, 16, 33, 64)         # QP = 8 with the pad inside the wave; the full wave form; the block form, padded and full
PIVOT_KINDS = ("negative", "nan", "inf", "nan-below")


def pivot_positions(q: int):
    p = {0, q - 1}
    if q == 7:
        p.add(3)
    if q > 16:
        p |= {15, 16, 17, 31, 32}
    if q == 64:
        p |= {47, 48, 63}
    return sorted(p)


@functools.lru_cache(maxsize=None)
def pivot_bases(q: int) -> np.ndarray:
    """[5, q, q], to be called with JITTER.  Read-only."""
    A = R.covariances(q, 5, seed=400 + q)
    A.setflags(write=False)
    return A


def spoiled(A, kind: str, p: int) -> np.ndarray:
    """A copy of A [q, q] whose elimination meets a bad pivot at step p exactly (the steps before it never read row p)."""
    A, q = A.copy(), A.shape[0]
    if kind == "negative":
        A[p, p] = -A[p, p]
    elif kind == "nan":
        A[p, p] = np.nan
    elif kind == "inf":
        A[p, p] = np.inf
    elif kind == "nan-below":          # lower triangle only; it reaches the last pivot through the column's multiplier
        assert p < q - 1
        A[q - 1, p] = np.nan
    else:
        raise KeyError(kind)
    return A


def zero_pivot_batch(q: int) -> np.ndarray:
    """4 C, C a unit-diagonal Matern-5/2 correlation matrix whose point 1 is point 0 again; for a call with jitter 0.  The
    first pivot is 4, its root 2, the multiplier of row 1 is 4 / 2 = 2 and the second pivot fma(-2, 2, 4) = 0 exactly."""
    X = np.random.default_rng(500 + q).uniform(size=(q, 4))
    X[1] = X[0]
    return 4.0 * R.matern52(X)


def pivots_float64(A) -> np.ndarray:
    """The pivots of the kernel's elimination restated in float64 (right-looking, column by column; numpy has no fused
    multiply-add, which changes nothing where the products are exact, as in the first two steps of ``zero_pivot_batch``).
    Stops at the first pivot that is not positive and finite: the pivots from there on are NaN."""
    r, q = np.array(A, dtype=np.float64), len(A)
    piv = np.full(q, np.nan)
    for j in range(q):
        piv[j] = r[j, j]
        if not (piv[j] > 0.0 and piv[j] < np.inf):
            break
        col = r[j:, j] / math.sqrt(piv[j])
        col[0] = math.sqrt(piv[j])
        r[j:, j] = col
        r[j + 1:, j + 1:] -= np.outer(col[1:], col[1:])
    return piv


def upper_spoiled(cov) -> np.ndarray:
    """cov [5, q, q] with NaN in the whole strict upper triangle of batch 1 and the strict upper triangle of batch 3 times
    1.5; the lower triangles and the diagonals untouched."""
    out, q = cov.copy(), cov.shape[1]
    up = np.triu(np.ones((q, q), dtype=bool), 1)
    out[1][up] = np.nan
    out[3][up] *= 1.5
    return out


# ---- C. chunks --------------------------------------------------------------------------------------------------------------
BANK = 257


def chunk_pvar(q: int) -> int:             # tgp_pvar_moments, tgp_pvar_values (joint_group_chunk)
    return max(1, 2 ** 30 // (8 * q * q))


def chunk_pvar_grad(q: int) -> int:        # tgp_pvar_moments_grad
    return max(1, 2 ** 28 // (8 * q * q))


@dataclass(frozen=True)
class ChunkRow:
    entry: str           # "moments", "moments_grad" or "values"
    q: int
    with_logdet: bool
    chunk: int           # the restated rule at this q

    @property
    def G(self) -> int:
        return self.chunk + 3

    @property
    def bad(self) -> int:
        """The group of the second chunk that gets a covariance that is not positive definite."""
        return self.chunk + 1


CHUNK_ROWS = {
    "moments-q64-logdet": ChunkRow("moments", 64, True, chunk_pvar(64)),          # block form
    "moments-q16": ChunkRow("moments", 16, False, chunk_pvar(16)),                # wave form; G mod 4 = 3: a partly empty workgroup
    "moments_grad-q16": ChunkRow("moments_grad", 16, False, chunk_pvar_grad(16)),  # wave form, 268 MB each way
    "moments_grad-q64": ChunkRow("moments_grad", 64, False, chunk_pvar_grad(64)),  # block form
    "values-q64": ChunkRow("values", 64, True, chunk_pvar(64)),
}
TABLE_CHUNKS = {"moments-q64-logdet": 32768, "moments-q16": 524288, "moments_grad-q16": 131072, "moments_grad-q64": 8192,
                "values-q64": 32768}


@functools.lru_cache(maxsize=None)
def cov_bank(q: int) -> np.ndarray:
    """[257, q, q]: distinct well-conditioned covariances, drawn as tests/chunk_cases.py draws its rows'.  Read-only."""
    A = np.random.default_rng([4545, q]).standard_normal((BANK, q, q))
    cov = A @ np.swapaxes(A, 1, 2) / q + 0.1 * np.eye(q)
    cov.setflags(write=False)
    return cov


def tiled(bank: np.ndarray, G: int) -> np.ndarray:
    """bank [257, ...] -> [G, ...], out[g] = bank[g % 257]."""
    return np.take(bank, np.arange(G) % BANK, axis=0)


# the pvar_values row: d = 2, N = 40; at the oracle's default lengthscale 64 points in the unit square are nearly dependent
# (lambda_min 3e-6 at 0.2), at 0.02 the smallest eigenvalue over the bank is 2.3e-3
VALUES_D, VALUES_N, VALUES_VARIANCE, VALUES_NOISE, VALUES_LENGTHSCALE = 2, 40, 1.0, 1e-2, 0.02


@functools.lru_cache(maxsize=None)
def values_model():
    """(X, Y, lengthscales, mean constant, oracle state) of the model behind the pvar_values row."""
    X, Y = O.synthetic_problem(O.ackley, VALUES_D, VALUES_N)
    ls = np.full(VALUES_D, VALUES_LENGTHSCALE)
    c = float(np.mean(Y))
    return X, Y, ls, c, O.gpr_update("matern52", VALUES_VARIANCE, ls, VALUES_NOISE, c, X, Y)


@functools.lru_cache(maxsize=None)
def values_bank() -> np.ndarray:
    """[257, 64, 2] candidates, i.i.d. uniform.  Read-only."""
    x = np.random.default_rng(5151).uniform(size=(BANK, CHUNK_ROWS["values-q64"].q, VALUES_D))
    x.setflags(write=False)
    return x


def tail_bounds_float64(A):
    """(b_ld, b_det) of tests/pvar_reference.py from numpy's own factor and inverse of A.  These matrices are well conditioned
    (``values_tolerances`` is used behind lambda_min >= 1e-3), so the float64 |L| and |A^-1| are right to ten digits and the
    bounds with them; 257 factorisations at fifty digits would take minutes."""
    q = A.shape[0]
    absL, absAi = np.abs(np.linalg.cholesky(A)), np.abs(np.linalg.inv(A))
    maxlog = float(np.abs(np.log(np.diag(absL))).max())
    b_ld = 2.0 * ((q + 2) * U * float((absAi * (absL @ absL.T)).sum()) + 4 * q * U * (1.0 + maxlog))
    return b_ld, b_ld + 2.0 * U


@functools.lru_cache(maxsize=None)
def values_reference():
    """Per bank group, from the oracle's joint covariance: (logdet [257] of cov + JITTER on every entry by numpy, lambda_min
    [257] of cov + JITTER I, tol_logdet [257], tol_det [257] relative).  The tolerance is for TWO DEVICE RESULTS of the same
    group whose posteriors took different product paths: their covariances differ by at most
    |dcov|_max <= 2 (N + 2) u variance (two summation orders of k** - sum_n v_n^2, the argument of
    test_one_point_is_the_predictive_variance_plus_jitter), which moves logdet by at most
    |tr(A^-1 dcov)| <= |dcov|_max sum_ij |A^-1|_ij <= q |dcov|_max |A^-1|_inf; to that the tail's own bound once per side."""
    st = values_model()[4]
    cov = O.predict_joint(st, values_bank())[1]
    q = cov.shape[1]
    dcov = 2.0 * (VALUES_N + 2) * U * VALUES_VARIANCE
    ld, lam, t_ld, t_det = (np.empty(BANK) for _ in range(4))
    for g, c in enumerate(cov):
        A = c + JITTER
        ld[g] = np.linalg.slogdet(A)[1]
        lam[g] = np.linalg.eigvalsh(c + JITTER * np.eye(q)).min()
        b_ld, b_det = tail_bounds_float64(A)
        moved = q * dcov * float(np.abs(np.linalg.inv(A)).sum(axis=1).max())
        t_ld[g], t_det[g] = moved + 2.0 * b_ld, moved + 2.0 * b_det
    for a in (ld, lam, t_ld, t_det):
        a.setflags(write=False)
    return ld, lam, t_ld, t_det


def neighbour_pairs(chunk: int):
    """The bank indices of every pair (g, g +- 1) and (g, g +- chunk) of a tiled call: a staging error reads one of these."""
    b = np.arange(BANK)
    return [(int(i), int((i + s) % BANK)) for i in b for s in (-1, 1, -chunk, chunk)]
