"""CPU: the yardsticks of the Monte-Carlo qEI tails (tests/test_gpu_qei_tail.py).  The numpy restatement
(tests/qei_reference.py) against the 50-digit goldens of tests/make_qei_tail_goldens.py -- value, samples, exact counts, the
closed-form adjoint of the covariance and, for q <= 4, central differences of the 50-digit value -- which measures the two
constants the GPU tolerances are built on; the seeded inputs the GPU file runs the kernels on (the sweep over every q in
every regime, the sample-count edges, the degenerate batches); and the conditions those comparisons rely on, from the
restatement alone: every group further from a kink than two float64 factorisations can move a sample, improving AND
non-improving draws where the regime is meant to have both.  No group is left out anywhere: the cap is zero.

Tolerance of a GPU comparison (u = 2^-53):  100 x the constant below x the scale of the entry  (+ lip x sample_atol  for the
near-duplicate and jitter-dominated inputs, where the two float64 factorisations differ by conditioning: ``sample_atol`` is
``tests.test_gpu_qehvi._sample_atol``, the bound for two factorisations by this same ``wave_chol_rows``; the lips are those of
tests/qei_reference.py.  gcov's lip is per unit of the FACTOR's entries; ``sample_atol`` = floor + dL q max|eps| bounds the
factor's movement dL wherever q max|eps| >= 1, which ``conditioned_tolerances`` asserts)."""
import functools
import os

import numpy as np
import pytest

from tests import make_qei_tail_goldens as MK
from tests import qei_reference as QR
from tests.test_gpu_qehvi import _sample_atol

U = 2.0 ** -53
JITTER = MK.JITTER

# The restatement's own worst error against the goldens as a fraction of the entry's scale, measured by
# test_restatement_matches_the_mpmath_goldens on this fixture (value and samples; gcov).  The GPU tests give the kernels 100 x
# these figures: both sides are float64 evaluations of one formula, the kernel's fma chains against numpy's / LAPACK's order.
# Measured: 9.99e-16 (a sample of "q=33 near-duplicate pair"; the values are at most 1.7e-16, the samples elsewhere at most
# 3.4e-16) and 3.81e-14 (gcov of "q=64 s=1e6 t=-2"; the q = 64 cases at s = 1 and 1e6 give 1.2e-14 ... 3.8e-14, the near-duplicate
# pairs up to 1.2e-14, everything else at most 2.4e-15: LAPACK's two triangular solves over 64 rows).
QEI_RESTATEMENT_WORST = 9.99e-16
QEI_GRAD_RESTATEMENT_WORST = 3.81e-14

SWEEP_G, SWEEP_S = 8, 65
# seed of the sweep's inputs at q: 9000 + q unless named here (the first seed counted up in steps of 100 that meets the conditions)
SWEEP_SEEDS = {3: 9103, 4: 9804, 5: 9705, 7: 10407, 8: 9108, 9: 9109, 10: 9210, 11: 9111, 13: 9413, 14: 9414, 15: 9415, 16: 9216,
               17: 9217, 18: 9118, 20: 9220, 22: 9222, 23: 9923, 24: 9524, 25: 9125, 28: 9128, 30: 9130, 31: 9131, 32: 9732,
               33: 9233, 39: 9239, 40: 9140, 42: 9142, 43: 9143, 44: 9144, 47: 9147, 49: 9249, 50: 9250, 51: 9151, 52: 9152,
               54: 9154, 56: 9156, 57: 9157, 59: 9359, 61: 9361}
EDGE_Q, EDGE_S = (7, 8, 9, 63, 64), (1, 63, 64, 65, 128, 129)
DEGENERATE_Q = (2, 5, 33)


@functools.lru_cache(maxsize=None)
def load_tail_goldens():
    return MK.load()


def errors(got, want, scale):
    """|got - want| as fractions of ``scale``; a zero scale demands an exactly equal result (inf otherwise)."""
    got, want, scale = (np.asarray(a, np.float64) for a in (got, want, scale))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, np.abs(got - want) / scale, np.where(got == want, 0.0, np.inf))


def restate(c):
    """``moment_adjoints`` of a golden case as a call of one group."""
    return QR.moment_adjoints(c["mean"][None], c["cov"][None], c["eps"], c["eta"], c["jitter"])


def conditioned(c):
    """Is the golden case one of those whose comparison carries the conditioning term?"""
    return c["s"] == 1e-4 or c["base"].endswith("pair") or c["base"].endswith("zero")


def conditioned_tolerances(r, mean, cov, eps, jitter):
    """The conditioning terms  lip x sample_atol  of (value [G], samples: a scalar, gcov [G, q, q]) for a restatement ``r``."""
    q = cov.shape[-1]
    atol = _sample_atol(mean, cov, eps, jitter)
    assert q * np.abs(eps).max() >= 1.0 or not np.any(r["gcov_scale"])       # sample_atol bounds the factor's movement
    return atol * r["value_lip"], atol, atol * r["gcov_lip"]


def sweep_seed(q):
    return SWEEP_SEEDS.get(q, 9000 + q)


def random_moments(rng, G, q, s):
    """G q-batches of the kind of ``tests.test_batch_ei_regimes.regime_moments`` (three shared factors, own variances
    0.02 ... 0.5, means standard normal + 5) at the output scale s."""
    A = rng.standard_normal((G, q, 3))
    cov = 0.3 * (A @ A.transpose(0, 2, 1)) / 3.0
    cov[:, np.arange(q), np.arange(q)] += rng.uniform(0.02, 0.5, size=(G, q))
    return (rng.standard_normal((G, q)) + 5.0) * s, cov * (s * s)


def same_threshold(mean, cov, t):
    """One eta per call, as the entries take it: the threshold rule of the goldens applied to the first batch; the means of
    every other batch are moved so that the rule gives it the same eta (every batch sits in the regime, not only the median
    one) -> (mean, eta)."""
    per_batch = np.array([MK.threshold(m, c, t) for m, c in zip(mean, cov)])
    return mean + (per_batch[0] - per_batch)[:, None], float(per_batch[0])


@functools.lru_cache(maxsize=None)
def sweep_inputs(q, s, t):
    """(mean [G, q], cov [G, q, q], eps [q, S], eta) of the sweep at q in the regime (s, t): G = 8, S = 65, the eta of
    ``same_threshold``.  Shared with tests/test_gpu_qei_tail.py; nobody changes the arrays."""
    rng = np.random.default_rng(sweep_seed(q))
    eps = rng.standard_normal((q, SWEEP_S))
    mean, cov = random_moments(rng, SWEEP_G, q, s)
    mean, eta = same_threshold(mean, cov, t)
    for a in (mean, cov, eps):
        a.setflags(write=False)
    return mean, cov, eps, eta


def edge_inputs(q, S):
    """(mean, cov, eps, eta, jitter) of the sample-count edges: G = 8 unit-scale batches, eta at t = 0."""
    rng = np.random.default_rng(100 * q + S)
    eps = rng.standard_normal((q, S))
    mean, cov = random_moments(rng, 8, q, 1.0)
    mean, eta = same_threshold(mean, cov, 0.0)
    return mean, cov, eps, eta, JITTER


def largest_fitting_draws(q):
    """The largest S that ``GPEngine.qei_value_grad_fits`` accepts at q (the rule of the library's ``qei_grad_tail_lds_bytes``:
    8 (2 q (q|1) + 128) + 4 (S rounded up to even) bytes within 160 KiB), by bisection on the rule itself."""
    from trieste_amd.engine import GPEngine

    lo, hi = 1, 1 << 20
    assert GPEngine.qei_value_grad_fits(q, lo) and not GPEngine.qei_value_grad_fits(q, hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if GPEngine.qei_value_grad_fits(q, mid) else (lo, mid)
    return lo


def duplicate_inputs(q):
    """G = 4 unit-scale batches whose point 1 IS point 0 (rows and columns of cov equal, means equal): the second pivot is
    the jitter, and which of the two is the smaller is decided by sqrt(jitter) eps_1 alone."""
    rng = np.random.default_rng(300 + q)
    eps = rng.standard_normal((q, 33))
    mean, cov = random_moments(rng, 4, q, 1.0)
    cov[:, 1, :], cov[:, :, 1] = cov[:, 0, :], cov[:, :, 0]
    cov[:, 1, 1] = cov[:, 0, 0]
    mean[:, 1] = mean[:, 0]
    mean, eta = same_threshold(mean, cov, 0.0)
    return mean, cov, eps, eta, JITTER


def zero_cov_inputs(q):
    """cov = 0 exactly: L = sqrt(jitter) I, every diagonal entry clipped.  The means lie within a few sqrt(jitter) of each
    other so that every point is the arg-min of some draw."""
    rng = np.random.default_rng(400 + q)
    eps = rng.standard_normal((q, 33))
    mean = 5.0 + 1e-3 * rng.standard_normal((4, q))
    return mean, np.zeros((4, q, q)), eps, float(mean.min() + 1e-3), JITTER


def mixed_clip_inputs(q):
    """``duplicate_inputs``' kind without the duplicate, tiny variances at two points: cov_00 = 1e-12 exactly (clipped) and
    cov_11 the next float above (not clipped), both uncorrelated with the rest."""
    rng = np.random.default_rng(500 + q)
    eps = rng.standard_normal((q, 65))
    mean, cov = random_moments(rng, 4, q, 1.0)
    cov[:, :2, :], cov[:, :, :2] = 0.0, 0.0
    cov[:, 0, 0], cov[:, 1, 1] = QR.VAR_FLOOR, np.nextafter(QR.VAR_FLOOR, 1.0)
    mean[:, :2] = mean.min(axis=1, keepdims=True) - 1.0 + 1e-4 * rng.standard_normal((4, 2))   # the two are often the arg-min
    mean, eta = same_threshold(mean, cov, 0.0)
    return mean, cov, eps, eta, JITTER


def kinks_are_out_of_reach(mean, cov, eps, eta, jitter):
    """-> (every group's kink distance exceeds sample_atol, the restatement)"""
    r = QR.moment_adjoints(mean, cov, eps, eta, jitter)
    return bool(np.all(r["kink_distance"] > _sample_atol(mean, cov, eps, jitter))), r


def regime_holds(r, S, t):
    """The draws of every group are of the kinds the regime is meant to hold."""
    n = r["improving"]
    return bool(np.all((n >= 1) & (n <= S - 1))) if t < 0 else bool(np.all(4 * n >= S))


# ---- the restatement against the goldens ----------------------------------------------------------------------------------
def test_the_file_holds_the_grid_of_cases():
    cases = load_tail_goldens()
    grid = {(c["q"], c["S"], c["s"], c["t"]) for c in cases if c["base"] == f"q{c['q']}"}
    assert grid == {(q, S, s, t) for q, S in MK.SIZES for s in MK.SCALES for t in MK.SHIFTS}
    assert {(q, S) for q, S in MK.SIZES} == {(1, 16), (2, 16), (3, 16), (9, 8), (17, 4), (33, 4), (64, 4), (9, 65)}
    assert sorted(c["q"] for c in cases if c["base"].endswith("pair")) == [2, 3, 9, 17, 33, 64]
    assert sum(c["base"].endswith("zero") and not np.any(c["cov"]) for c in cases) == 1
    assert len(cases) == 8 * 9 + 6 + 1 and all(c["jitter"] == 1e-6 for c in cases)
    assert os.path.getsize(MK.OUT) < 256 * 1024      # (packed: tests/make_qei_tail_goldens.compact)
    for c in cases:
        assert c["eta"] == MK.threshold(c["mean"], c["cov"], c["t"])
        assert c["samples"].shape == (c["S"], c["q"]) and c["gcov"].shape == (c["q"], c["q"])
        assert (len(c["diffs"]) == c["q"] * (c["q"] + 1) // 2) == (c["q"] <= 4)


def test_restatement_matches_the_mpmath_goldens():
    worst_v, worst_g = (0.0, ""), (0.0, "")
    for n, c in enumerate(load_tail_goldens()):
        r = restate(c)
        np.testing.assert_array_equal(r["counts"][0], c["counts"], err_msg=c["note"])
        ev = errors(r["value"][0], c["value"], r["value_scale"][0]).max()
        es = errors(r["samples"][0], c["samples"], r["samples_scale"][0]).max()
        eg = errors(r["gcov"][0], c["gcov"], r["gcov_scale"][0]).max()
        assert np.all(np.abs(c["gcov_unclipped"]) <= r["gcov_scale"][0] * (1 + 1e-9)), c["note"]
        print(f"case {n:2d} {c['note']:44s} value {ev:.2e} samples {es:.2e} gcov {eg:.2e} of the scales")
        worst_v, worst_g = max(worst_v, (max(ev, es), c["note"])), max(worst_g, (eg, c["note"]))
    print(f"restatement vs mpmath: value and samples worst {worst_v[0]:.3e} ({worst_v[1]}); gcov worst {worst_g[0]:.3e} ({worst_g[1]})")
    assert worst_v[0] <= 2.0 * QEI_RESTATEMENT_WORST and worst_g[0] <= 2.0 * QEI_GRAD_RESTATEMENT_WORST
    # the constants are the measured figures, not a cap far above them
    assert worst_v[0] >= 0.5 * QEI_RESTATEMENT_WORST and worst_g[0] >= 0.5 * QEI_GRAD_RESTATEMENT_WORST


def test_closed_form_agrees_with_central_differences_of_the_value():
    """q <= 4: the goldens' own closed-form adjoint (unclipped) and the restatement's, contracted with every symmetric unit
    direction of cov, against the 50-digit central differences: the closed form is not its own witness."""
    seen = 0
    for c in load_tail_goldens():
        if c["q"] > 4:
            continue
        r = QR.moment_adjoints(c["mean"][None], c["cov"][None], c["eps"], c["eta"], c["jitter"], clip=False)
        for (i, j), want in c["diffs"].items():
            fold = 1.0 if i == j else 2.0
            scale = fold * r["gcov_scale"][0, i, j]
            assert errors(fold * c["gcov_unclipped"][i, j], want, scale) <= 1e-15, (c["note"], i, j)
            assert errors(r["gcov"][0, i, j] + (r["gcov"][0, j, i] if i != j else 0.0), want, scale) <= 2.0 * QEI_GRAD_RESTATEMENT_WORST, \
                (c["note"], i, j)
            seen += 1
    assert seen == 9 * (1 + 3 + 6) + 3 + 6 + 6


# ---- the conditions ---------------------------------------------------------------------------------------------------------
def test_golden_cases_meet_the_conditions():
    for c in load_tail_goldens():
        ok, r = kinks_are_out_of_reach(c["mean"][None], c["cov"][None], c["eps"], c["eta"], c["jitter"])
        assert ok, (c["note"], r["kink_distance"])
        assert regime_holds(r, c["S"], c["t"]) or c["base"].endswith("zero"), (c["note"], r["improving"])
        assert 1 <= r["improving"][0], c["note"]
        conditioned_tolerances(r, c["mean"][None], c["cov"][None], c["eps"], c["jitter"])
    zero = [c for c in load_tail_goldens() if c["base"].endswith("zero")][0]
    assert np.all(np.diagonal(zero["gcov_unclipped"]) != 0.0) and not np.any(np.diagonal(zero["gcov"]))


@pytest.mark.parametrize("q", range(1, 65))
def test_sweep_inputs_meet_the_conditions(q):
    for s in MK.SCALES:
        for t in MK.SHIFTS:
            mean, cov, eps, eta = sweep_inputs(q, s, t)
            ok, r = kinks_are_out_of_reach(mean, cov, eps, eta, JITTER)
            assert ok, (q, s, t, r["kink_distance"])
            assert regime_holds(r, SWEEP_S, t), (q, s, t, r["improving"])
            conditioned_tolerances(r, mean, cov, eps, JITTER)


def test_edge_and_degenerate_inputs_meet_the_conditions():
    for q in EDGE_Q:
        for S in EDGE_S:
            ok, r = kinks_are_out_of_reach(*edge_inputs(q, S))
            assert ok, (q, S, r["kink_distance"])
    assert largest_fitting_draws(64) == (160 * 1024 - 8 * (2 * 64 * 65 + 128)) // 4 == 24064
    for q in DEGENERATE_Q:
        for make in (duplicate_inputs, zero_cov_inputs, mixed_clip_inputs):
            args = make(q)
            ok, r = kinks_are_out_of_reach(*args)
            assert ok, (make.__name__, q, r["kink_distance"])
            assert np.all(r["improving"] >= 8), (make.__name__, q, r["improving"])
            conditioned_tolerances(r, args[0], args[1], args[2], args[4])
        mean, cov, *_ = duplicate_inputs(q)
        assert np.all(cov[:, 0] == cov[:, 1]) and np.all(np.linalg.eigvalsh(cov).min(axis=1) < 1e-12)
        _, r = kinks_are_out_of_reach(*mixed_clip_inputs(q))
        # both tiny-variance points collect draws: the clipped one's diagonal adjoint would not be zero without the clip
        assert np.all(r["counts"][:, :2] >= 1) and np.all(r["gcov"][:, 0, 0] == 0.0) and np.all(r["gcov"][:, 1, 1] != 0.0)
        _, r = kinks_are_out_of_reach(*zero_cov_inputs(q))
        assert np.count_nonzero(r["counts"].sum(axis=0)) >= min(q, 8)     # many points are the arg-min of some draw
