"""Inputs, probe groups and float64 references for the chunked batch calls (TEST INFRASTRUCTURE; imports without a GPU).

Five entry points of the C-ABI walk their groups in chunks so that the [G, q, q] covariances stay within a bounded scratch
(``for_group_chunks`` in trieste_amd/csrc/tgp_api.hip).  The functions ``chunk_*`` below RESTATE the chunk rules of that
file; they mirror it and must move with it (tests/test_gpu_chunked_calls.py checks the restatement against the chunk count
the library reports, for the four entries that report one).

Every entry is taken at its largest q (the chunk shrinks as q grows) with G = chunk + t groups:
  t = 1               "small": the ragged chunk has t q <= 2048 points and takes the small-product posterior
  t = 2048 // q + 1   "joint": the ragged chunk stays on the joint kernel
  t = 0               "exact": one chunk, one launch (the two cheapest entries only)

The model behind the three entries that compute a posterior: d = 4, N = 64 (``synthetic_problem`` of the oracle on Ackley),
Matern-5/2, unit variance, noise 1e-2, lengthscale LENGTHSCALE in every dimension, candidates i.i.d. uniform: every group
is statistically like every other.  ``reparam_sample_atol`` of tests/util.py grows like 1 / sqrt(lambda_min) of a group's
covariance + jitter I, so the groups have to be well conditioned: lambda_min >= 1e-3 of the kernel variance on the probe
groups (tests/test_chunk_cases.py asserts it).  At the oracle's default lengthscale for d = 4, 0.4, the probe sets meet
that by 4 % (smallest 1.04e-3) and 6 of 3000 random 64-point groups fall below it (smallest 1.5e-4) -- but the whole-output
comparison of the GPU test applies the probes' largest tolerance to EVERY group.  LENGTHSCALE = 0.2: smallest 1.0e-2 over
the probe sets, 1.8e-3 over the same 3000 random groups.

The two entries on given moments: the mean is distinct per group, the covariance is bank[g % 257], a bank of 257 matrices
drawn as tests/test_gpu_batch_ei.py draws its random moments (257 is prime: the pattern does not repeat with the chunk).

The four newer chunked entries on given moments (tgp_qei_moments, tgp_qei_moments_grad, tgp_qehvi_moments,
tgp_qehvi_moments_grad) have rows of their own, MOMENTS_ROWS, for tests/test_gpu_moments_chunks.py: G = chunk + 3 groups, mean
AND covariance of group g are those of group g % 257 of a bank of 257 distinct groups, and the expected output is the output of
one small call on the bank, tiled the same way (``moments_row_inputs``, ``tiled``)."""
from __future__ import annotations

import functools
from dataclasses import dataclass, field
from typing import Dict

import numpy as np

from oracle import gp_oracle as O
from tests import batch_ei_grad_reference as GR
from tests import batch_ei_reference as R
from tests.test_batch_ei_grad_reference import GRAD_RESTATEMENT_WORST
from tests.test_batch_ei_reference import RESTATEMENT_WORST
from tests.test_gpu_batch_ei import _perturbed, _random_moments
from tests.util import cancellation_floor, reparam_sample_atol

KERNEL_TOL = 100.0 * RESTATEMENT_WORST        # tests/test_gpu_batch_ei.py
GRAD_TOL = 100.0 * GRAD_RESTATEMENT_WORST     # tests/test_gpu_batch_ei_grad.py
JOINT_SMALL_P = 2048                          # points up to which a (chunk of a) call takes the small-product posterior


# ---- the chunk rules of trieste_amd/csrc/tgp_api.hip, restated: they mirror that file and must move with it --------------
def chunk_qei(q: int, S: int = 0) -> int:                 # tgp_qei, tgp_batch_ei, tgp_batch_ei_moments
    return max(1, 2 ** 30 // (q * q * 8))


def chunk_moments_grad(q: int, S: int = 0) -> int:        # tgp_batch_ei_moments_grad
    return max(1, 2 ** 28 // (q * q * 8))


def chunk_reparam(q: int, S: int) -> int:                 # tgp_reparam_samples
    return max(1, 2 ** 28 // (q * max(q, S) * 8))


def chunk_qei_moments(q: int, S: int = 0, samples: bool = False) -> int:   # tgp_qei_moments; tgp_qei_moments_grad (no samples)
    return chunk_reparam(q, S) if samples else chunk_qei(q)


def chunk_qehvi(P: int, q: int) -> int:                   # tgp_qehvi_moments (qehvi_group_chunk), tgp_qehvi_values
    return max(1, 2 ** 28 // (8 * P * q * (q + 1)))


def chunk_qehvi_grad(P: int, q: int) -> int:              # tgp_qehvi_moments_grad
    return max(1, chunk_qehvi(P, q) // 2)


@dataclass(frozen=True)
class MomentsRow:
    """A row of tests/test_gpu_moments_chunks.py: a chunked entry on given moments at G = chunk + 3 groups."""
    entry: str
    q: int
    S: int
    P: int          # objectives of the stacked arrays (1: the qEI entries)
    samples: bool
    chunk: int      # the restated rule at this shape

    @property
    def G(self) -> int:
        return self.chunk + 3


MOMENTS_ROWS = {r_id: MomentsRow(*r) for r_id, r in {
    "qei_moments": ("qei_moments", 64, 4, 1, False, chunk_qei_moments(64, 4)),
    "qei_moments-samples": ("qei_moments", 64, 3, 1, True, chunk_qei_moments(64, 3, samples=True)),
    "qei_moments_grad": ("qei_moments_grad", 64, 4, 1, False, chunk_qei_moments(64, 4)),
    "qehvi_moments": ("qehvi_moments", 8, 1, 2, False, chunk_qehvi(2, 8)),
    "qehvi_moments_grad": ("qehvi_moments_grad", 8, 1, 2, False, chunk_qehvi_grad(2, 8)),
}.items()}
TABLE_MOMENTS_CHUNKS = {"qei_moments": 32768, "qei_moments-samples": 8192, "qei_moments_grad": 32768, "qehvi_moments": 233016,
                        "qehvi_moments_grad": 116508}


@dataclass(frozen=True)
class Entry:
    name: str
    q: int
    S: int
    rule: object          # (q, S) -> chunk
    posterior: bool       # computes the joint posterior of candidates (else: takes moments)
    exact: bool           # also run with G = chunk exactly
    reports_chunks: bool  # last_kernel_ms()[1] is the chunk count

    @property
    def chunk(self) -> int:
        return self.rule(self.q, self.S)


ENTRIES = {e.name: e for e in (
    Entry("reparam_samples", 64, 3, chunk_reparam, True, True, False),     # S < q: the output stays at a few MB
    Entry("qei", 64, 4, chunk_qei, True, False, True),
    Entry("batch_ei_moments_grad", 16, 2, chunk_moments_grad, False, True, True),
    Entry("batch_ei", 16, 2, chunk_qei, True, False, True),
    Entry("batch_ei_moments", 16, 2, chunk_qei, False, False, True),
)}
TABLE_CHUNKS = {"reparam_samples": 8192, "qei": 32768, "batch_ei_moments_grad": 131072, "batch_ei": 524288,
                "batch_ei_moments": 524288}


@dataclass(frozen=True)
class Case:
    entry: Entry
    kind: str   # "small", "joint" or "exact"

    @property
    def t(self) -> int:
        return {"exact": 0, "small": 1, "joint": JOINT_SMALL_P // self.entry.q + 1}[self.kind]

    @property
    def G(self) -> int:
        return self.entry.chunk + self.t

    @property
    def chunks(self) -> int:
        return -(-self.G // self.entry.chunk)

    @property
    def id(self) -> str:
        return f"{self.entry.name}-{self.kind}"


CASES = [Case(e, k) for e in ENTRIES.values() for k in ("small", "joint", "exact") if k != "exact" or e.exact]
CASE = {c.id: c for c in CASES}


def g_max(entry: Entry) -> int:
    return max(c.G for c in CASES if c.entry is entry)


def probe_groups(case: Case) -> np.ndarray:
    """{0, 1, chunk-2, chunk-1, chunk, chunk+1, G-1} clipped to what exists, plus 200 seeded random indices of which 20 lie
    in the ragged chunk when it has that many groups.  Sorted, unique."""
    chunk, G = case.entry.chunk, case.G
    rng = np.random.default_rng([7, chunk, G])
    rand = rng.choice(G, size=200, replace=False)
    if G - chunk >= 20:
        rand[:20] = chunk + rng.choice(G - chunk, size=20, replace=False)
    fixed = np.array([0, 1, chunk - 2, chunk - 1, chunk, chunk + 1, G - 1])
    fixed = fixed[(fixed >= 0) & (fixed < G)]
    return np.unique(np.concatenate([fixed, rand])).astype(np.int64)


# ---- inputs ---------------------------------------------------------------------------------------------------------------
D, N, KIND, VARIANCE, NOISE, JITTER = 4, 64, "matern52", 1.0, 1e-2, 1e-6
LENGTHSCALE = 0.2
FLOOR = cancellation_floor(N, VARIANCE, NOISE)


@functools.lru_cache(maxsize=None)
def model():
    """(X, Y, lengthscales, mean constant, oracle state) of the model behind the posterior entries."""
    X, Y = O.synthetic_problem(O.ackley, D, N)
    ls = np.full(D, LENGTHSCALE)
    c = float(np.mean(Y))
    return X, Y, ls, c, O.gpr_update(KIND, VARIANCE, ls, NOISE, c, X, Y)


def _seed(entry: Entry) -> int:
    return 100 + list(ENTRIES).index(entry.name)


@functools.lru_cache(maxsize=None)
def candidates(name: str) -> np.ndarray:
    """[g_max, q, D] i.i.d. uniform candidates of a posterior entry; a case takes the first G groups.  Read-only."""
    e = ENTRIES[name]
    x = np.random.default_rng(_seed(e)).uniform(size=(g_max(e), e.q, D))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def draws(name: str) -> np.ndarray:
    """eps [q, S] of tgp_qei / tgp_reparam_samples."""
    e = ENTRIES[name]
    return np.random.default_rng(_seed(e) + 50).standard_normal((e.q, e.S))


@functools.lru_cache(maxsize=None)
def sobol(q: int, S: int):
    return R.sobol_points(S, q, skip=5 + q)


BANK = 257


@functools.lru_cache(maxsize=None)
def moment_bank(q: int) -> np.ndarray:
    """[257, q, q] covariances as tests/test_gpu_batch_ei.py draws them."""
    bank = _random_moments(q, BANK, np.random.default_rng(4242))[1]
    bank.setflags(write=False)
    return bank


@functools.lru_cache(maxsize=None)
def moment_means(q: int, G: int) -> np.ndarray:
    """[G, q]: a distinct mean per group.  Read-only; the two moments entries take the first G' <= G rows."""
    mean = np.random.default_rng(4343).standard_normal((G, q))
    mean.setflags(write=False)
    return mean


def moment_covs(q: int, groups) -> np.ndarray:
    return moment_bank(q)[np.asarray(groups) % BANK]


MOMENTS_G = max(g_max(e) for e in ENTRIES.values() if not e.posterior)


def moments_eta(q: int) -> float:
    """The median of the row minima, as in tests/test_gpu_batch_ei.py."""
    return float(np.median(moment_means(q, MOMENTS_G).min(axis=1)))


# ---- the rows of the four newer entries on given moments ----------------------------------------------------------------------
TWO_CELLS = (np.array([[-10.0, -10.0], [0.5, -10.0]]), np.array([[0.5, 1.5], [1.5, 0.5]]))   # left of the front {(0.5, 0.5)}


@functools.lru_cache(maxsize=None)
def moments_row_inputs(row_id: str):
    """(mean bank [257, q] or [P, 257, q], cov bank [257, q, q] or [P, 257, q, q], eps [q, S] or [P, q, S], eta) of a row: 257
    distinct well-conditioned groups.  Read-only."""
    r = MOMENTS_ROWS[row_id]
    rng = np.random.default_rng([4444, r.q, r.S, r.P])
    lead = (BANK,) if r.P == 1 else (r.P, BANK)
    A = rng.standard_normal(lead + (r.q, r.q))
    cov = A @ np.swapaxes(A, -1, -2) / r.q + 0.1 * np.eye(r.q)
    mean = rng.standard_normal(lead + (r.q,)) if r.P == 1 else rng.uniform(0.0, 1.0, lead + (r.q,))
    eps = rng.standard_normal((r.q, r.S) if r.P == 1 else (r.P, r.q, r.S))
    for a in (mean, cov, eps):
        a.setflags(write=False)
    return mean, cov, eps, float(np.median(mean.min(axis=-1)))


def tiled(bank: np.ndarray, G: int, stacked: bool) -> np.ndarray:
    """bank [257, ...] -> [G, ...] with out[g] = bank[g % 257]; stacked: bank [P, 257, ...] -> out[j, g] = bank[j, g % 257]."""
    return np.take(bank, np.arange(G) % BANK, axis=1 if stacked else 0)


# ---- references -----------------------------------------------------------------------------------------------------------
def reparam_restatement(mean, cov, eps, jitter=JITTER):
    """mean [n, q], cov [n, q, q], eps [q, S] -> samples [n, S, q] = mean + (chol(cov + jitter I) eps)^T, in float64."""
    q = mean.shape[1]
    L = np.linalg.cholesky(cov + jitter * np.eye(q))
    return mean[:, None, :] + np.swapaxes(L @ eps, 1, 2)


def qei_restatement(mean, cov, eps, eta, jitter=JITTER):
    s = reparam_restatement(mean, cov, eps, jitter)
    return np.mean(np.maximum(eta - s.min(axis=2), 0.0), axis=1)


def _sample_atols(cov, eps):
    return np.array([reparam_sample_atol(c[None], FLOOR, eps, JITTER) for c in cov])


def evaluate(case: Case, groups, eta=None, with_tol=True):
    """The reference on `groups`: (want, tol, keep, eta, moments).  want / tol: output name -> array whose first axis is the
    group; tol None without `with_tol`; keep [n]: False where a tolerance says nothing (tgp_batch_ei alone, by the rule of
    its parity test); eta: the incumbent, chosen from the moments of `groups` unless given; moments: the oracle's (mean,
    cov) of a posterior entry."""
    e = case.entry
    groups = np.asarray(groups, dtype=np.int64)
    keep = np.ones(groups.size, dtype=bool)
    tol = None
    if e.posterior:
        mean, cov = O.predict_joint(model()[4], candidates(e.name)[groups])
    else:
        mean, cov = moment_means(e.q, MOMENTS_G)[groups], moment_covs(e.q, groups)
    if e.name == "reparam_samples":
        eps = draws(e.name)
        want = {"samples": reparam_restatement(mean, cov, eps)}
        if with_tol:
            tol = {"samples": 1e-5 * np.abs(want["samples"]) + _sample_atols(cov, eps)[:, None, None]}
    elif e.name == "qei":
        eps = draws(e.name)
        eta = float(np.median(mean)) if eta is None else eta          # (tests/test_gpu_wide.py's choice)
        want = {"qei": qei_restatement(mean, cov, eps, eta)}
        if with_tol:   # a qEI value moves by no more than the largest change of a sample
            tol = {"qei": 1e-5 * np.abs(want["qei"]) + _sample_atols(cov, eps)}
    elif e.name == "batch_ei":
        w1, w2 = sobol(e.q, e.S)
        eta = float(np.median(mean.min(axis=1))) if eta is None else eta
        want = {"value": R.batch_ei(mean, cov, eta, w1, w2)}
        if with_tol:   # test_batch_ei_behind_the_posterior_matches_the_restatement_on_the_oracles_moments
            moved = np.zeros(groups.size)
            for seed in range(5):
                m2, c2 = _perturbed(mean, cov, FLOOR, np.random.default_rng(100 + seed))
                moved = np.maximum(moved, np.abs(R.batch_ei(m2, c2, eta, w1, w2) - want["value"]))
            atol = 2.0 * moved
            keep = atol <= 1e-2 * want["value"].max()
            tol = {"value": 1e-5 * np.abs(want["value"]) + atol}
    elif e.name == "batch_ei_moments":
        w1, w2 = sobol(e.q, e.S)
        eta = moments_eta(e.q) if eta is None else eta
        val, scale = R.batch_ei_scale(mean, cov, eta, w1, w2)
        want = {"value": val}
        tol = {"value": KERNEL_TOL * scale}
    elif e.name == "batch_ei_moments_grad":
        w1, w2 = sobol(e.q, e.S)
        eta = moments_eta(e.q) if eta is None else eta
        val, gm, gc, scale = GR.batch_ei_value_grad(mean, cov, eta, w1, w2)
        want = {"value": val, "gmean": gm, "gcov": gc}
        tol = {"value": KERNEL_TOL * scale,
               "gmean": GRAD_TOL * np.abs(gm).max(axis=1, keepdims=True) * np.ones_like(gm),
               "gcov": GRAD_TOL * np.abs(gc).max(axis=(1, 2), keepdims=True) * np.ones_like(gc)}
    else:
        raise KeyError(e.name)
    return want, tol, keep, eta, (mean, cov)


@dataclass
class Reference:
    case: Case
    groups: np.ndarray
    want: Dict[str, np.ndarray]
    tol: Dict[str, np.ndarray]
    keep: np.ndarray
    eta: float
    moments: tuple
    T: Dict[str, float] = field(default_factory=dict)   # the largest tolerance of an output over the kept probes


@functools.lru_cache(maxsize=None)
def reference(case_id: str) -> Reference:
    """The reference of a case on its probe groups, computed once and shared; nobody writes to it."""
    case = CASE[case_id]
    groups = probe_groups(case)
    want, tol, keep, eta, moments = evaluate(case, groups)
    for a in list(want.values()) + list(tol.values()):
        a.setflags(write=False)
    return Reference(case, groups, want, tol, keep, eta, moments, {k: float(np.max(v[keep])) for k, v in tol.items()})


def separation(case_id: str) -> Dict[str, float]:
    """Per output, over the probe pairs (g, g'), g' = g +- 1 or g +- chunk inside the call: (the fraction whose references
    differ -- largest entry of the difference -- by more than 100 x the probe's own comparison tolerance, the fraction whose
    references differ by more than 2 T, the bound of the GPU test's whole-output comparison of a posterior entry)."""
    ref = reference(case_id)
    case, e = ref.case, ref.case.entry
    pairs = [(i, g + s) for i, g in enumerate(ref.groups) if ref.keep[i] for s in (-1, 1, -e.chunk, e.chunk)
             if 0 <= g + s < case.G]
    others = np.unique([p[1] for p in pairs])
    want = evaluate(case, others, eta=ref.eta, with_tol=False)[0]
    where = {int(g): j for j, g in enumerate(others)}
    out = {}
    for k in ref.want:
        far = far2t = 0
        for i, g2 in pairs:
            diff = float(np.max(np.abs(ref.want[k][i] - want[k][where[int(g2)]])))
            far += diff > 100.0 * float(np.max(ref.tol[k][i]))
            far2t += diff > 2.0 * ref.T[k]
        out[k] = (far / len(pairs), far2t / len(pairs))
    return out
