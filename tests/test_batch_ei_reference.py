"""CPU tests of the analytic batch EI: the numpy restatement (tests/batch_ei_reference.py) against the 50-digit mpmath
goldens and against a brute-force Monte-Carlo estimate (tests of the yardstick itself), and the builder / function logic
of ``trieste_amd.acquisition.BatchExpectedImprovement`` on an oracle-backed stand-in engine (reference
tests/unit/acquisition/function/test_function.py, the ``BatchExpectedImprovement`` block)."""
import json
import os

import numpy as np
import pytest

import trieste_amd.models as M
from oracle import gp_oracle as O
from tests import batch_ei_reference as R
from tests.fakes import FakeEngine
from trieste_amd import objectives as OBJ
from trieste_amd.data import Dataset
from trieste_amd.space import Box

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_ei_goldens.json")

EPS = np.finfo(np.float64).eps
# The numpy restatement's own worst error against the goldens as a fraction of sum |summands| of the value, measured by
# the first test below on this fixture: 3.29e-13 (q = 4, near-duplicate pair; 1.2e-14 on the q = 8 near-duplicate, at
# most 2.5e-15 on the other sixteen cases).  tests/test_gpu_batch_ei.py gives the kernel 100 x this figure.
RESTATEMENT_WORST = 3.3e-13


def load_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def conditioning(cov):
    """kappa = max |cov_jk| / lambda_min(cov + 1e-6 I): forming Sigma^(i), c and R (differences and a quotient of entries
    of cov) leaves an absolute error of about eps max |cov| in their entries, and a Gaussian whose narrowest direction has
    the variance lambda_min turns an entry error delta into a CDF error of the order delta / lambda_min."""
    cov = np.asarray(cov)
    return np.abs(cov).max() / np.linalg.eigvalsh(cov + 1e-6 * np.eye(cov.shape[-1])).min()


def test_restatement_matches_the_mpmath_goldens():
    """Value (relative to sum |summands|) and every CDF (absolutely: all are <= 1, some underflow towards 0) within
    8 eps (1 + kappa) of the 50-digit figures -- a few roundings of a float64 evaluation, amplified by the conditioning of
    the q-batch -- and the value within RESTATEMENT_WORST, the figure the GPU tolerance is built on."""
    worst_v = worst_c = worst_flat = 0.0
    for n, c in enumerate(load_cases()):
        mean, cov = np.array(c["mean"])[None], np.array(c["cov"])[None]
        w1, w2 = np.array(c["w1"]).reshape(c["S"], c["q"]), np.array(c["w2"]).reshape(c["S"], c["q"] - 1)
        v, p, Phi, terms = R.batch_ei_parts(mean, cov, c["eta"], w1, w2)
        scale = np.sum(np.abs(terms))
        assert abs(scale - c["abs_terms"]) <= 1e-9 * c["abs_terms"]
        unit = EPS * (1.0 + conditioning(cov[0]))
        ev = abs(v[0] - c["value"]) / scale
        ec = max(np.abs(p[0] - np.array(c["p"])).max(), np.abs(Phi[0] - np.array(c["Phi"])).max())
        print(f"case {n:2d} q={c['q']} {c['note']:24s} value {c['value']: .6e}  error {ev:.2e} of sum |terms| = {ev / unit:.3f} units,"
              f"  CDFs {ec:.2e} = {ec / unit:.3f} units (unit {unit:.1e})")
        worst_v, worst_c, worst_flat = max(worst_v, ev / unit), max(worst_c, ec / unit), max(worst_flat, ev)
        assert ev <= 8 * unit, f"case {n} (q={c['q']}, {c['note']}): value off by {ev:.2e} of sum |terms|"
        assert ec <= 8 * unit, f"case {n} (q={c['q']}, {c['note']}): a CDF off by {ec:.2e}"
    print(f"restatement vs mpmath: value {worst_v:.3f} units, CDFs {worst_c:.3f} units; value {worst_flat:.2e} of sum |terms|")
    assert worst_flat <= RESTATEMENT_WORST


def _gpr_moments(q, B, noise, seed):
    d, N = 4, 60
    X, Y = O.synthetic_problem(O.ackley, d, N, seed=seed)
    st = O.gpr_update("matern52", 1.0, O.default_lengthscales(d), noise, float(np.mean(Y)), X, Y)
    Xq = np.random.default_rng(seed).uniform(size=(B, q, d))
    mean, cov = O.predict_joint(st, Xq)
    return mean, cov, float(np.median(mean.min(axis=1)))


# the band per q: twice what the restatement showed against the brute force at exactly these sizes and seeds (S = 200
# Sobol points against 4e5 joint samples, 12 batches), as a fraction of the largest value: measured 7.2e-5, 1.3e-4,
# 8.0e-4, 4.4e-3.  A sanity band (the closed form and the plain Monte-Carlo mean estimate the same quantity), not parity.
@pytest.mark.parametrize("q,band", [(2, 1.5e-4), (3, 2.6e-4), (5, 1.6e-3), (8, 8.9e-3)])
def test_restatement_agrees_with_a_brute_force_monte_carlo_estimate(q, band):
    mean, cov, eta = _gpr_moments(q, 12, 1e-2, seed=40 + q)
    w1, w2 = R.sobol_points(200, q, skip=11)
    got = R.batch_ei(mean, cov, eta, w1, w2)
    want = R.brute_force_qei(mean, cov, eta, 400_000, seed=q)
    assert np.count_nonzero(want > 1e-3 * want.max()) >= want.size // 2
    err = np.abs(got - want).max() / want.max()
    print(f"q={q}: closed form vs brute force: {err:.2e} of the largest value (band {band:.1e})")
    assert err <= band


# ---- the builder and the function on a stand-in engine ------------------------------------------------------------
class BatchEIFakeEngine(FakeEngine):
    """FakeEngine + the two entry points ``trieste_amd.engine.batch_ei`` / ``batch_ei_moments`` defer to:
    restatement o oracle.predict_joint."""

    calls = 0

    def batch_ei_moments(self, mean, cov, w1, w2, eta):
        mean, cov = np.asarray(mean, float), np.asarray(cov, float)
        lead, q = mean.shape[:-1], mean.shape[-1]
        return R.batch_ei(mean.reshape(-1, q), cov.reshape(-1, q, q), eta, np.asarray(w1), np.asarray(w2)).reshape(lead)

    def batch_ei(self, Xq, w1, w2, eta):
        type(self).calls += 1
        Xq = np.asarray(Xq, float)
        lead = Xq.shape[:-2]
        mean, cov = O.predict_joint(self._st(), Xq.reshape((-1,) + Xq.shape[-2:]))
        return self.batch_ei_moments(mean, cov, w1, w2, eta).reshape(lead)


@pytest.fixture
def fake_engine(monkeypatch):
    monkeypatch.setattr(M, "GPEngine", BatchEIFakeEngine)


def _model(n=12, d=2, noise=1e-3, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, d))
    data = Dataset(x, OBJ.scaled_branin(x))
    gpr = M.build_gpr(data, Box([0.0] * d, [1.0] * d), likelihood_variance=noise)
    return M.GaussianProcessRegression(gpr), data


def test_the_functions_are_exported():
    from trieste_amd.acquisition import BatchExpectedImprovement, batch_expected_improvement  # noqa: F401
    from trieste_amd.engine import batch_ei, batch_ei_moments  # noqa: F401


@pytest.mark.parametrize("sample_size", [-2, 0])
def test_builder_raises_for_invalid_sample_size(sample_size):
    from trieste_amd.acquisition import BatchExpectedImprovement

    with pytest.raises(ValueError):
        BatchExpectedImprovement(sample_size=sample_size)


def test_builder_raises_for_invalid_jitter():
    from trieste_amd.acquisition import BatchExpectedImprovement

    with pytest.raises(ValueError):
        BatchExpectedImprovement(sample_size=2, jitter=-1.0)


def test_builder_repr():
    from trieste_amd.acquisition import BatchExpectedImprovement

    assert repr(BatchExpectedImprovement(100, jitter=1e-5)) == "BatchExpectedImprovement(100, jitter=1e-05)"


def test_builder_raises_for_empty_data(fake_engine):
    from trieste_amd.acquisition import BatchExpectedImprovement

    model, _ = _model()
    builder = BatchExpectedImprovement(100)
    with pytest.raises(ValueError):
        builder.prepare_acquisition_function(model, dataset=Dataset(np.zeros((0, 2)), np.zeros((0, 1))))
    with pytest.raises(ValueError):
        builder.prepare_acquisition_function(model)


def test_update_refuses_a_foreign_function_and_redraws_the_skip(fake_engine):
    from trieste_amd.acquisition import (BatchExpectedImprovement, BatchMonteCarloExpectedImprovement,
                                         batch_expected_improvement)
    from trieste_amd.acquisition.function import SOBOL_SKIP_BOUND

    model, data = _model()
    builder = BatchExpectedImprovement(64)
    fn = builder.prepare_acquisition_function(model, data)
    assert isinstance(fn, batch_expected_improvement)
    other = BatchMonteCarloExpectedImprovement(8).prepare_acquisition_function(model, data)
    with pytest.raises(ValueError):
        builder.update_acquisition_function(other, model, data)
    with pytest.raises(ValueError):
        builder.update_acquisition_function(fn, model, None)
    skips = {fn._num_sobol_skip}
    w1 = fn.sobol(3)[0]
    for _ in range(4):
        assert builder.update_acquisition_function(fn, model, data) is fn
        skips.add(fn._num_sobol_skip)
    assert len(skips) > 1 and all(0 <= s < SOBOL_SKIP_BOUND for s in skips)
    assert not np.array_equal(w1, fn.sobol(3)[0])
    assert fn._eta == pytest.approx(float(np.min(model.engine.predict_mean(data.query_points))))


def test_function_values_are_the_reference_formula_on_the_models_posterior(fake_engine):
    """``__call__``: [..., q, D] -> [..., 1]; ONE skip for both point sets; the builder's jitter is not applied; q = 1 and
    q = 17 are refused; the value is what a brute-force estimate of the multi-point EI gives (the reference's own unit
    test compares against BatchMonteCarloExpectedImprovement at rtol 6e-2... here: the band of the test above)."""
    from trieste_amd.acquisition import BatchExpectedImprovement

    model, data = _model(n=15)
    fn = BatchExpectedImprovement(200, jitter=0.5).prepare_acquisition_function(model, data)
    rng = np.random.default_rng(3)
    x = rng.uniform(size=(6, 3, 2))
    got = fn(x)
    assert got.shape == (6, 1)
    w1, w2 = R.sobol_points(200, 3, fn._num_sobol_skip)
    np.testing.assert_array_equal(fn.sobol(3)[0], w1)
    np.testing.assert_array_equal(fn.sobol(3)[1], w2)
    mean, cov = O.predict_joint(model.engine._st(), x)
    np.testing.assert_array_equal(got[:, 0], R.batch_ei(mean, cov, fn._eta, w1, w2))
    bf = R.brute_force_qei(mean, cov, fn._eta, 200_000, seed=1)
    assert np.abs(got[:, 0] - bf).max() <= 2e-2 * max(bf.max(), 1e-12)
    assert fn(x.reshape(2, 3, 3, 2)).shape == (2, 3, 1)
    with pytest.raises(ValueError):
        fn(x[:, :1])
    with pytest.raises(ValueError):
        fn(rng.uniform(size=(2, 17, 2)))
    assert not hasattr(fn, "value_and_gradient")


def test_ego_with_batch_ei_runs_end_to_end_on_the_stand_in(fake_engine):
    """EfficientGlobalOptimization(BatchExpectedImprovement(S), num_query_points=q): no ``value_and_gradient``, so the
    joint batch is found by random search, as qEI was before its gradient existed."""
    from trieste_amd.acquisition import BatchExpectedImprovement, EfficientGlobalOptimization
    from trieste_amd.acquisition.optimizer import generate_random_search_optimizer

    model, data = _model(n=10)
    space = Box([0.0, 0.0], [1.0, 1.0])
    rule = EfficientGlobalOptimization(BatchExpectedImprovement(32), num_query_points=3,
                                       optimizer=generate_random_search_optimizer(200))
    before = BatchEIFakeEngine.calls
    pts = rule.acquire_single(space, model, dataset=data)
    assert np.asarray(pts).shape == (3, 2) and np.all(np.asarray(pts) >= 0.0) and np.all(np.asarray(pts) <= 1.0)
    assert BatchEIFakeEngine.calls > before
