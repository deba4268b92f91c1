"""Models, candidate sets and the numpy side of the pruned EI arg-max (TEST INFRASTRUCTURE; tests/test_prune_bound.py on
the CPU, tests/test_gpu_prune.py on the GPU).

The fused EI arg-max gives a 128-candidate block up at a 256-row boundary of W once, for every candidate of the block,

    best > MIN_BEST   and   ub * MARGIN < best                                     (strict),

where ``best`` is the largest finished block maximum of the launch and ``ub`` is the engine's EI tail at the candidate's
mean and at ``max(variance - partial column norm, VAR_FLOOR)``: the column norm only grows, so that variance bounds the
final one from above, and EI grows with the variance.  MARGIN = 1 + 2^-14 is three times the factor 1 + 2e-5 by which two
evaluations of a tail held to RTOL = 1e-5 of a monotone function (tests/acq_regimes.py) can be out of order; below
MIN_BEST nothing is given up because values under TINY = 1e-290 are not held relatively."""
import contextlib
import functools
import math

import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import erfc

from oracle import gp_oracle as O

MARGIN = 1.0 + 2.0 ** -14
MIN_BEST = 1e-280
ROW_BLOCK, CAND_BLOCK = 256, 128
FIRST_ROUND = 256                 # candidate blocks in flight at once (one per compute unit): they see no `best`
M = 131072 + 77                   # 1024 full blocks = 4 x 256 and a ragged one
PLANT_DISTANCE = 0.02             # lengthscales between the planted candidate and the training minimum


def ei_tail(diff, var):
    """The engine's EI tail restated in numpy float64: diff Phi(z) + sd phi(z), Phi(z) = erfc(-z / sqrt 2) / 2."""
    sd = np.sqrt(var)
    z = diff / sd
    return diff * (0.5 * erfc(-z * 0.7071067811865476)) + sd * (0.3989422804014327 * np.exp(-0.5 * z * z))


def gives_up(ub, best):
    """The rule for one block: ub [candidates], best a scalar."""
    return bool(best > MIN_BEST and np.all(ub * MARGIN < best))


def _cfg(name, kind, N, d, noise):
    return dict(name=name, kind=kind, N=N, d=d, noise=noise)


# N = 256: one row block, no checkpoint; N = 700 pads to 768 (three row blocks); all four kernel kinds at N = 512, d = 8
CONFIGS = [
    _cfg("m52_N256_d8", "matern52", 256, 8, 1e-2),
    _cfg("m52_N512_d8", "matern52", 512, 8, 1e-2),
    _cfg("rbf_N512_d8", "rbf", 512, 8, 1e-2),
    _cfg("m12_N512_d8", "matern12", 512, 8, 1e-2),
    _cfg("m32_N512_d8", "matern32", 512, 8, 1e-2),
    _cfg("m52_N512_d2", "matern52", 512, 2, 1e-2),
    _cfg("m52_N700_d8", "matern52", 700, 8, 1e-2),
    _cfg("m52_N700_d16_lownoise", "matern52", 700, 16, 1e-5),
    _cfg("m52_N768_d8", "matern52", 768, 8, 1e-2),
    _cfg("m52_N768_d8_lownoise", "matern52", 768, 8, 1e-5),
    _cfg("m32_N768_d16", "matern32", 768, 16, 1e-2),
]
IDS = [c["name"] for c in CONFIGS]
SHARE_IDS = [c["name"] for c in CONFIGS if c["N"] >= 512]   # where a block has a checkpoint to be given up at


def _gcfg(name, kind, N, d, variance, lo, width, rel_noise, offset=37.5):
    return dict(name=name, kind=kind, N=N, d=d, variance=variance, rel_noise=rel_noise, offset=offset,
                lo=np.array(np.broadcast_to(np.asarray(lo, dtype=np.float64), (d,))),
                width=np.array(np.broadcast_to(np.asarray(width, dtype=np.float64), (d,))))


def _unequal(d, seed):
    return np.round(np.random.default_rng(seed).uniform(0.5, 4.0, size=d), 2)


# General models (tests/test_prune_general_cases.py on the CPU, tests/test_gpu_prune_general.py on the GPU).  On CONFIGS
# sigma^2, sigma and 1 are one number, a dropped mean changes nothing and ls[0] is every lengthscale: the very quantities the
# bounds are made of.  Each model here departs in all four ways at once, as tests/test_gpu_general.py builds its models: ARD
# lengthscales width * 0.2 sqrt(d) * permutation(geomspace(0.35, 3.5, d)) with the shortest not at index 0, a kernel
# variance far from 1 with the noise relative to it, observations sqrt(variance) * standardised ackley + offset with the
# constant mean their average, and a box lo + width * [0, 1]^d far from the origin.  More than one row block each; the
# padded dimensions 4 and 6 among them.
GENERAL = [
    _gcfg("g_m52_d8_N512_at1024", "matern52", 512, 8, 250.0, 1024.0, 1.0, 1e-2),
    _gcfg("g_rbf_d6_N700_at100", "rbf", 700, 6, 0.37, 100.0, [0.5, 4.0, 1.0, 2.0, 3.0, 0.7], 1e-2),
    _gcfg("g_m32_d3_N513_small", "matern32", 513, 3, 1e-4, [300.0, 0.5, -20.0], [10.0, 1.5, 3.0], 1e-3, offset=-1000.0),
    _gcfg("g_m12_d5_N600_neg", "matern12", 600, 5, 250.0, -40.0 + 7.0 * np.arange(5), _unequal(5, 2), 1e-2),
    _gcfg("g_m52_d16_N700_lownoise", "matern52", 700, 16, 0.37, 100.0, _unequal(16, 3), 1e-5),
    # beyond the issue's five: a variance so large that a bound formed without it is passed by a wide margin
    _gcfg("g_m32_d4_N520_var1e4", "matern32", 520, 4, 1e4, [-300.0, 50.0, 2048.0, -7.0], _unequal(4, 5), 1e-2),
]
GENERAL_IDS = [c["name"] for c in GENERAL]
# The exact twin of m52_N512_d8: X, candidates and lengthscales times 4, Y times 2^-10, variance and noise times 4^-10,
# mean 0.  Every operation of the engine commutes exactly with these scalings (tests/test_gpu_general.py,
# test_output_scaling_by_a_power_of_two_is_exact): same winner index, value times 2^-10, same decisions.
TWIN, TWIN_OF, TWIN_X, TWIN_Y = "g_twin_m52_N512_d8", "m52_N512_d8", 4.0, 2.0 ** -10


def is_general(name):
    return name in GENERAL_IDS or name == TWIN


def form(name):
    """The oracle's distance form for a model: the difference form on a general one (the dot-product form is no reference
    far from the origin, tests/test_oracle_difference_form.py), the default on CONFIGS."""
    return O.difference_form() if is_general(name) else contextlib.nullcontext()


class P:
    """One configuration's problem."""


def _general_problem(cfg):
    p = P()
    p.name, p.kind, p.N, p.d = cfg["name"], cfg["kind"], cfg["N"], cfg["d"]
    p.lo, p.width = cfg["lo"], cfg["width"]
    rng = np.random.default_rng(5678)
    U = rng.uniform(size=(p.N, p.d))
    p.X = p.lo + p.width * U
    f = O.ackley(U)
    p.variance, p.noise, p.rel_noise = cfg["variance"], cfg["rel_noise"] * cfg["variance"], cfg["rel_noise"]
    p.Y = np.sqrt(p.variance) * (f - f.mean()) / f.std() + cfg["offset"]
    p.mean_const = float(np.mean(p.Y))
    rel = rng.permutation(np.geomspace(0.35, 3.5, p.d))
    if int(np.argmin(rel)) == 0:
        rel = np.roll(rel, 1)
    p.ls = p.width * 0.2 * np.sqrt(p.d) * rel
    assert int(np.argmin(p.ls / p.width)) != 0
    i = int(np.argmin(p.Y))
    step = (0.5 - U[i]) * p.width / p.ls
    p.plant = p.X[i] + PLANT_DISTANCE * p.ls * step / np.linalg.norm(step)
    return p


def _twin_problem():
    q = problem(TWIN_OF)
    p = P()
    p.name, p.kind, p.N, p.d = TWIN, q.kind, q.N, q.d
    p.lo, p.width = np.zeros(q.d), np.full(q.d, TWIN_X)
    p.X, p.Y, p.ls, p.plant = q.X * TWIN_X, q.Y * TWIN_Y, q.ls * TWIN_X, q.plant * TWIN_X
    p.variance, p.noise, p.rel_noise, p.mean_const = TWIN_Y * TWIN_Y, q.noise * TWIN_Y * TWIN_Y, q.noise, 0.0
    return p


@functools.lru_cache(maxsize=None)
def problem(name):
    if name == TWIN:
        return _twin_problem()
    if name in GENERAL_IDS:
        return _general_problem(next(c for c in GENERAL if c["name"] == name))
    cfg = next(c for c in CONFIGS if c["name"] == name)
    p = P()
    p.name, p.kind, p.N, p.d, p.noise = name, cfg["kind"], cfg["N"], cfg["d"], cfg["noise"]
    p.X, p.Y = O.synthetic_problem(O.ackley, p.d, p.N)
    p.ls = O.default_lengthscales(p.d)
    p.variance, p.mean_const = 1.0, 0.0
    p.lo, p.width, p.rel_noise = np.zeros(p.d), np.ones(p.d), p.noise
    # the planted candidate: PLANT_DISTANCE lengthscales from the training minimum, towards the centre of the box
    i = int(np.argmin(p.Y))
    step = 0.5 - p.X[i]
    p.plant = p.X[i] + PLANT_DISTANCE * p.ls * step / np.linalg.norm(step)
    return p


@functools.lru_cache(maxsize=None)
def oracle_state(name):
    p = problem(name)
    with form(name):
        st = O.gpr_update(p.kind, p.variance, p.ls, p.noise, p.mean_const, p.X, p.Y)
        return st, O.eta_min_mean(st)


@functools.lru_cache(maxsize=None)
def candidates(name):
    """The plain candidate set: uniform on the model's box, lo + width * U with U the same draw for every model.
    Read-only; the cases copy it."""
    p = problem(name)
    Xq = np.random.default_rng(977).uniform(size=(M, p.d))
    if is_general(name):
        Xq = p.lo + p.width * Xq
    Xq.setflags(write=False)
    return Xq


def planted(name, index):
    Xq = candidates(name).copy()
    Xq[index] = problem(name).plant
    return Xq


def partial_bounds(st, eta, Xq):
    """-> (mean [M], ub [nrb][M]): ub[i] the EI tail at the variance bound after row blocks 0 .. i (ub[-1]: the value)."""
    K = O.kernel_matrix(st.kind, st.variance, st.lengthscales, st.X, Xq)
    A = solve_triangular(st.L, K, lower=True)
    mean = solve_triangular(st.L.T, A, lower=False).T @ st.err + st.mean_const
    nrb = -(-st.N // ROW_BLOCK)
    sq = np.zeros((nrb * ROW_BLOCK, Xq.shape[0]))
    sq[: st.N] = A * A
    cum = np.cumsum(sq.reshape(nrb, ROW_BLOCK, -1).sum(1), 0)
    var = np.maximum(st.variance - cum, O.VAR_FLOOR)
    return mean, ei_tail((eta - mean)[None, :], var)


def sweep_with_rule(mean, ub, lag):
    """The block-stop rule run over ub [nrb][M] block by block; block b knows the maxima of the blocks up to b - lag that
    were swept to the end.  -> (winner value, winner index, given_up [blocks] bool)."""
    nrb, m = ub.shape
    nblk = -(-m // CAND_BLOCK)
    done_max = np.full(nblk, -np.inf)
    given = np.zeros(nblk, dtype=bool)
    for b in range(nblk):
        cols = slice(b * CAND_BLOCK, min(m, (b + 1) * CAND_BLOCK))
        known = done_max[: max(0, b - lag + 1)]
        best = max(0.0, known.max()) if known.size else 0.0
        given[b] = any(gives_up(ub[i, cols], best) for i in range(nrb - 1))   # the last row block has no checkpoint
        if not given[b]:
            v = ub[-1, cols]
            v = v[~np.isnan(v)]
            done_max[b] = v.max() if v.size else -np.inf
    vals = np.where(np.repeat(given, CAND_BLOCK)[:m], -np.inf, ub[-1])
    i = int(O.argmax_first(vals))
    return float(vals[i]), i, given
