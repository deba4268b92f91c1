"""GPU tests of the analytic batch EI (tgp_batch_ei / tgp_batch_ei_moments, bei_tail_kernel): against the 50-digit mpmath
goldens, against the numpy restatement of the reference's formula (tests/batch_ei_reference.py) on random moments and
behind the engine's own joint posterior, bit-identity, refusals, and the rule end to end.

Tolerance of the moments comparisons: both sides are float64 evaluations of one formula.  The restatement's own worst
error against the goldens is RESTATEMENT_WORST = 3.3e-13 of the sum of the |summands| of the value (measured by
tests/test_batch_ei_reference.py::test_restatement_matches_the_mpmath_goldens); the kernel gets 100 x that -- its Phi and
Phi^-1 are a few ulp where scipy's are below one, and an error in y_j passes through at most q - 1 further steps --
relative to sum |summands|, not to the (cancelling) total."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import batch_ei_reference as R
from tests.test_batch_ei_reference import RESTATEMENT_WORST, load_cases
from tests.util import cancellation_floor, record_margin

pytestmark = pytest.mark.gpu

KERNEL_TOL = 100.0 * RESTATEMENT_WORST


def _bare_engine(d=2):
    from trieste_amd.engine import GPEngine

    return GPEngine(d, "matern52")


def _check(got, want, tol, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    err = np.abs(got - want)
    worst = record_margin(what, err, tol)
    print(f"{what}: worst error / tolerance = {worst:.3g} over {err.size} values")
    bad = ~(err <= tol)
    if np.any(bad):
        i = int(np.argmax(err / tol))
        raise AssertionError(f"{what}: {bad.sum()} / {bad.size} differ; worst at {i}: got {got.flat[i]!r} want {want.flat[i]!r} "
                             f"err {err.flat[i]:.3e} tol {np.broadcast_to(tol, err.shape).flat[i]:.3e}")


def test_moments_entry_matches_the_mpmath_goldens():
    from trieste_amd.engine import batch_ei_moments

    eng = _bare_engine()
    for n, c in enumerate(load_cases()):
        q, S = c["q"], c["S"]
        w1, w2 = np.array(c["w1"]).reshape(S, q), np.array(c["w2"]).reshape(S, q - 1)
        got = batch_ei_moments(eng, np.array(c["mean"])[None], np.array(c["cov"])[None], w1, w2, c["eta"])
        _check(got, [c["value"]], KERNEL_TOL * c["abs_terms"], f"golden q={q} ({c['note']})")


def _random_moments(q, G, rng):
    """Moments of the kind a GPR returns: unit-scale variances, correlations from a few shared factors."""
    A = rng.standard_normal((G, q, 3))
    cov = 0.3 * (A @ A.transpose(0, 2, 1)) / 3.0
    cov[:, np.arange(q), np.arange(q)] += rng.uniform(0.02, 0.5, size=(G, q))
    mean = rng.standard_normal((G, q))
    return mean, cov, float(np.median(mean.min(axis=1)))


# q = 16 is compared at S <= 65: the restatement holds [G q^2, S, q] arrays
@pytest.mark.parametrize("q,S", [(q, S) for q in (2, 3, 5, 8, 16) for S in (1, 63, 64, 65, 500) if (q, S) != (16, 500)])
def test_moments_entry_matches_the_restatement_on_random_batches(q, S):
    from trieste_amd.engine import batch_ei_moments

    G = 2000 if q <= 5 else (256 if q == 8 else 32)
    rng = np.random.default_rng(1000 * q + S)
    mean, cov, eta = _random_moments(q, G, rng)
    w1, w2 = R.sobol_points(S, q, skip=3 * q + S)
    want, scale = R.batch_ei_scale(mean, cov, eta, w1, w2)
    assert np.count_nonzero(want > 1e-3 * want.max()) >= want.size // 2
    got = batch_ei_moments(_bare_engine(), mean, cov, w1, w2, eta)
    _check(got, want, KERNEL_TOL * scale, f"moments q={q} S={S}")


# ---- behind the engine's own posterior ------------------------------------------------------------------------------
def _ard(d, seed):
    return O.default_lengthscales(d) * (0.6 + 0.8 * np.random.default_rng(seed).uniform(size=d))


POSTERIOR_CONFIGS = [
    # (name, objective, d, kind, N, noise, ARD): the joint parity configurations (every kernel kind, d = 2 ... 16), an ARD
    # problem at d = 40 and a wide one (d = 64: the float64 JOINT sweep feeds the tail)
    ("branin_m52_N50", O.branin, 2, "matern52", 50, 1e-3, False),
    ("hartmann_rbf_N300", O.hartmann_6, 6, "rbf", 300, 1e-2, False),
    ("ackley8_m52_N1000", O.ackley, 8, "matern52", 1000, 1e-2, False),
    ("ackley8_m52_N1000_lownoise", O.ackley, 8, "matern52", 1000, 1e-5, False),
    ("ackley16_m32_N257", O.ackley, 16, "matern32", 257, 1e-3, False),
    ("ackley3_m12_N130", O.ackley, 3, "matern12", 130, 1e-3, False),
    ("ackley40_m52_ard_N200", O.ackley, 40, "matern52", 200, 1e-2, True),
    ("ackley64_rbf_N1000", O.ackley, 64, "rbf", 1000, 1e-2, False),
]


def _perturbed(mean, cov, floor, rng):
    """Moments moved by what the joint parity tests allow (1e-5 |entry| + floor per entry) with the covariance kept
    positive semi-definite: cov' = D cov D + floor z z^T, D = I + diag(+-5e-6), z = +-1; mean' = mean +- (1e-5 |mean| + floor)."""
    G, q = mean.shape
    D = 1.0 + 5e-6 * rng.choice([-1.0, 1.0], size=(G, q))
    z = rng.choice([-1.0, 1.0], size=(G, q))
    cov2 = cov * D[:, :, None] * D[:, None, :] + floor * z[:, :, None] * z[:, None, :]
    mean2 = mean + rng.choice([-1.0, 1.0], size=(G, q)) * (1e-5 * np.abs(mean) + floor)
    return mean2, cov2


@pytest.mark.parametrize("cfg", POSTERIOR_CONFIGS, ids=[c[0] for c in POSTERIOR_CONFIGS])
def test_batch_ei_behind_the_posterior_matches_the_restatement_on_the_oracles_moments(cfg, monkeypatch):
    """tgp_batch_ei vs restatement o oracle.predict_joint, G * q below and above 2048 points (the skinny product and the
    joint kernel feed the tail), q-batches with near-duplicate pairs and points next to training inputs among them.
    Tolerance 1e-5 |want| + atol, atol per q-batch = 2 x the largest change of the RESTATEMENT's value over five seeded
    perturbations of the oracle's moments of the size the joint parity tests allow; a batch whose atol exceeds 1e-2 of the
    largest value says nothing and is left out, at most one in ten."""
    from trieste_amd.engine import GPEngine, batch_ei

    _, obj, d, kind, N, noise, ard = cfg
    if kind == "matern12":   # (as tests/test_gpu_wide.py: the engine's distances are the difference form)
        monkeypatch.setattr(O, "scaled_square_dist", O.difference_form_sq_dist)
    X, Y = O.synthetic_problem(obj, d, N)
    ls = _ard(d, 17) if ard else O.default_lengthscales(d)
    c = float(np.mean(Y))
    st = O.gpr_update(kind, 1.0, ls, noise, c, X, Y)
    eng = GPEngine(d, kind)
    eng.set_hyper(1.0, ls, noise, c)
    eng.set_data(X, Y)
    floor = cancellation_floor(N, 1.0, noise)
    rng = np.random.default_rng(23)
    S = 64
    for q, G in ((2, 1100), (3, 30), (4, 40), (8, 300)):
        Xg = rng.uniform(size=(G, q, d))
        special = max(2, G // 10)
        for g in range(0, special, 2):
            Xg[g, 1] = Xg[g, 0] + 1e-3 * rng.standard_normal(d) / np.sqrt(d)          # a near-duplicate pair
            Xg[g + 1, 0] = X[g % N] + 1e-4 * rng.standard_normal(d) / np.sqrt(d)      # next to a training input
        mean, cov = O.predict_joint(st, Xg)
        eta = float(np.median(mean.min(axis=1)))
        w1, w2 = R.sobol_points(S, q, skip=5 + q)
        want = R.batch_ei(mean, cov, eta, w1, w2)
        assert np.all(np.isfinite(want))
        assert np.count_nonzero(want > 1e-3 * want.max()) >= want.size // 2
        moved = np.zeros(G)
        for seed in range(5):
            m2, c2 = _perturbed(mean, cov, floor, np.random.default_rng(100 + seed))
            moved = np.maximum(moved, np.abs(R.batch_ei(m2, c2, eta, w1, w2) - want))
        atol = 2.0 * moved
        keep = atol <= 1e-2 * want.max()
        dropped = np.flatnonzero(~keep)
        assert dropped.size <= G // 10, f"q={q}: {dropped.size} of {G} batches excluded: {dropped.tolist()}"
        got = np.asarray(batch_ei(eng, Xg, w1, w2, eta))
        assert got.shape == (G,) and np.all(np.isfinite(got))
        print(f"{cfg[0]} q={q} G={G}: atol median {np.median(atol):.2e} max {atol.max():.2e} of max(want) {want.max():.3e}; "
              f"excluded {dropped.tolist()}")
        _check(got[keep], want[keep], 1e-5 * np.abs(want[keep]) + atol[keep], f"batch EI q={q} G={G}")


def test_two_calls_two_handles_and_both_residencies_return_identical_bits():
    import torch

    from trieste_amd.engine import GPEngine, batch_ei, batch_ei_moments

    d, N = 4, 300
    X, Y = O.synthetic_problem(O.ackley, d, N)
    ls, c = O.default_lengthscales(d), float(np.mean(Y))
    engines = []
    for _ in range(2):
        eng = GPEngine(d, "matern52")
        eng.set_hyper(1.0, ls, 1e-3, c)
        eng.set_data(X, Y)
        engines.append(eng)
    rng = np.random.default_rng(5)
    for q, G, S in ((3, 50, 100), (4, 700, 130), (16, 200, 33)):
        Xg = rng.uniform(size=(G, q, d))
        w1, w2 = R.sobol_points(S, q, skip=9)
        mean, cov = engines[0].predict_joint(Xg)
        eta = float(np.median(mean.min(axis=1)))
        a = batch_ei(engines[0], Xg, w1, w2, eta)
        assert np.any(a != 0.0)
        np.testing.assert_array_equal(a, batch_ei(engines[0], Xg, w1, w2, eta))
        np.testing.assert_array_equal(a, batch_ei(engines[1], Xg, w1, w2, eta))
        dev = batch_ei(engines[0], torch.as_tensor(Xg).cuda(), torch.as_tensor(w1).cuda(), torch.as_tensor(w2).cuda(), eta)
        assert dev.is_cuda
        np.testing.assert_array_equal(a, dev.cpu().numpy())
        # the tail alone on the moments the engine returned: the same bits as the fused call
        m = batch_ei_moments(engines[1], mean, cov, w1, w2, eta)
        np.testing.assert_array_equal(a, m)
        md = batch_ei_moments(engines[0], torch.as_tensor(mean).cuda(), torch.as_tensor(cov).cuda(), w1, w2, eta)
        np.testing.assert_array_equal(a, md.cpu().numpy())
        assert batch_ei(engines[0], Xg.reshape(G // 10, 10, q, d), w1, w2, eta).shape == (G // 10, 10)


def test_refusals():
    from trieste_amd import _lib
    from trieste_amd.engine import batch_ei, batch_ei_moments

    eng = _bare_engine()
    lib, h = eng._lib, eng._h
    out = np.zeros(4)
    w = np.full((8, 17), 0.5)
    mean, cov = np.zeros((4, 17)), np.tile(np.eye(17), (4, 1, 1))
    p = lambda a: a.ctypes.data  # noqa: E731

    def moments(q, w1, w2, S):
        return lib.tgp_batch_ei_moments(h, p(mean), p(cov), 4, q, w1, w2, S, 0.0, p(out), _lib.HOST)

    assert moments(1, p(w), p(w), 8) == _lib.TGP_ERR_SHAPE
    assert b"2..16" in lib.tgp_last_error(h)
    assert moments(17, p(w), p(w), 8) == _lib.TGP_ERR_SHAPE
    assert moments(0, p(w), p(w), 8) == _lib.TGP_ERR_SHAPE
    assert moments(3, p(w), p(w), 0) == _lib.TGP_ERR_ARG
    assert moments(3, None, p(w), 8) == _lib.TGP_ERR_ARG
    assert moments(3, p(w), None, 8) == _lib.TGP_ERR_ARG
    assert lib.tgp_batch_ei_moments(h, None, p(cov), 4, 3, p(w), p(w), 8, 0.0, p(out), _lib.HOST) == _lib.TGP_ERR_ARG
    # the fused entry: same checks, and no data on the handle is a state error
    Xq = np.zeros((4, 17, 2))
    assert lib.tgp_batch_ei(h, p(Xq), 4, 1, p(w), p(w), 8, 0.0, p(out), _lib.HOST) == _lib.TGP_ERR_SHAPE
    assert lib.tgp_batch_ei(h, p(Xq), 4, 17, p(w), p(w), 8, 0.0, p(out), _lib.HOST) == _lib.TGP_ERR_SHAPE
    assert lib.tgp_batch_ei(h, p(Xq), 4, 3, p(w), p(w), 0, 0.0, p(out), _lib.HOST) == _lib.TGP_ERR_ARG
    assert lib.tgp_batch_ei(h, p(Xq), 4, 3, None, p(w), 8, 0.0, p(out), _lib.HOST) == _lib.TGP_ERR_ARG
    assert lib.tgp_batch_ei(h, p(Xq), 4, 3, p(w), p(w), 8, 0.0, p(out), _lib.HOST) == _lib.TGP_ERR_STATE
    # the Python layer
    w1, w2 = R.sobol_points(8, 3)
    with pytest.raises(ValueError):
        batch_ei_moments(eng, np.zeros((2, 1)), np.ones((2, 1, 1)), np.zeros((8, 1)), np.zeros((8, 0)), 0.0)
    with pytest.raises(ValueError):
        batch_ei_moments(eng, np.zeros((2, 17)), np.tile(np.eye(17), (2, 1, 1)), w[:, :17], w[:, :16], 0.0)
    with pytest.raises(ValueError):
        batch_ei_moments(eng, np.zeros((2, 3)), np.tile(np.eye(3), (2, 1, 1)), w1, w1, 0.0)        # w2 of the wrong width
    with pytest.raises(ValueError):
        batch_ei(eng, np.zeros((2, 3, 5)), w1, w2, 0.0)                                           # d = 5 on a d = 2 engine
    # an indefinite covariance (input data: an argument check, nothing faults) names its group
    covs = np.tile(np.eye(3), (6, 1, 1))
    covs[4] = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(_lib.NotPositiveDefiniteError, match="group 4") as ei:
        batch_ei_moments(eng, np.zeros((6, 3)), covs, w1, w2, 0.0)
    assert isinstance(ei.value, RuntimeError)
    # ... and the handle is usable afterwards
    ok = batch_ei_moments(eng, np.zeros((6, 3)), np.tile(np.eye(3), (6, 1, 1)), w1, w2, 0.0)
    assert np.all(np.isfinite(ok)) and np.all(ok > 0.0)


def _branin_setup(n, seed):
    import trieste_amd.models as M
    from trieste_amd import objectives as OBJ
    from trieste_amd.data import Dataset
    from trieste_amd.space import Box

    space = Box([0, 0], [1, 1])
    x = space.sample(n, seed=seed)
    data = Dataset(x, OBJ.scaled_branin(x))
    model = M.GaussianProcessRegression(M.build_gpr(data, space, likelihood_variance=1e-5))
    return space, data, model


def test_ego_with_batch_ei_in_an_ask_tell_loop_on_the_real_engine():
    """EfficientGlobalOptimization(BatchExpectedImprovement(100), num_query_points=3): runs, returns [3, 2] points in the
    box, and the chosen batch is the one of the largest value among the random batches the search looked at (arg-max)."""
    import trieste_amd
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import (BatchExpectedImprovement, EfficientGlobalOptimization, batch_expected_improvement,
                                         generate_random_search_optimizer)
    from trieste_amd.ask_tell_optimization import AskTellOptimizer
    from trieste_amd.data import Dataset

    trieste_amd.set_seed(11)
    space, data, model = _branin_setup(8, seed=2)
    rule = EfficientGlobalOptimization(BatchExpectedImprovement(100), num_query_points=3)   # the default optimizer
    opt = AskTellOptimizer(space, data, model, rule)
    for _ in range(2):
        pts = np.asarray(opt.ask())
        assert pts.shape == (3, 2) and np.all(pts >= space.lower) and np.all(pts <= space.upper)
        opt.tell(Dataset(pts, OBJ.scaled_branin(pts)))
    fn = rule.acquisition_function
    assert isinstance(fn, batch_expected_improvement) and not hasattr(fn, "value_and_gradient")
    # the arg-max property, with the search's candidates reproduced here from its seed
    space, data, model = _branin_setup(8, seed=3)
    rule = EfficientGlobalOptimization(BatchExpectedImprovement(100), num_query_points=3,
                                       optimizer=generate_random_search_optimizer(3000, seed=5, on_device=False))
    pts = np.asarray(AskTellOptimizer(space, data, model, rule).ask())
    assert pts.shape == (3, 2) and np.all(pts >= space.lower) and np.all(pts <= space.upper)
    fn = rule.acquisition_function
    cands = (space ** 3).sample(3000, seed=5).reshape(3000, 3, 2)
    vals = np.asarray(fn(cands))[:, 0]
    assert np.all(np.isfinite(vals))
    best = int(np.argmax(vals))                  # the returned batch IS the candidate of the largest value, hence its value
    np.testing.assert_array_equal(pts, cands[best])   # is >= that of every batch the search looked at (first index on ties)
    assert vals[best] > 0.0 and np.all(vals[best] >= vals)
    # evaluated alone the batch takes the small-call route of the posterior: the same value to the parity tolerance
    alone = float(np.asarray(fn(pts[None]))[0, 0])
    assert abs(alone - vals[best]) <= 1e-5 * abs(vals[best]) + 1e-9


@pytest.mark.slow  # as in the reference: run with --runslow yes (the step budget is tuned to ITS seeds)
def test_bayesian_optimizer_with_batch_ei_finds_minima_of_scaled_branin():
    """The reference's bar for this rule (tests/integration/test_bayesian_optimization.py:131-137,
    id="BatchExpectedImprovement": 12 steps of 3 points from 5 initial ones): best observation within 0.5 % of the scaled
    Branin minimum, best point within 5 % of a minimiser."""
    import trieste_amd
    import trieste_amd.models as M
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import BatchExpectedImprovement, EfficientGlobalOptimization
    from trieste_amd.bayesian_optimizer import BayesianOptimizer, stop_at_minimum
    from trieste_amd.data import Dataset

    trieste_amd.set_seed(1793)
    problem = OBJ.ScaledBranin
    space = problem.search_space
    initial = space.sample(5, seed=1793)
    data = Dataset(initial, problem.objective(initial))
    model = M.GaussianProcessRegression(M.build_gpr(data, space, likelihood_variance=1e-7))
    rule = EfficientGlobalOptimization(BatchExpectedImprovement(100), num_query_points=3)
    result = BayesianOptimizer(lambda x: Dataset(x, problem.objective(x)), space).optimize(
        12, data, model, rule, fit_initial_model=False,
        early_stop_callback=stop_at_minimum(problem.minimum, problem.minimizers, minimum_rtol=0.005, minimum_step_number=2))
    assert result.final_result.is_ok, result.final_result
    best_x, best_y, _ = result.try_get_optimal_point()
    minimizer_err = np.abs((best_x - problem.minimizers) / problem.minimizers)
    assert np.any(np.all(minimizer_err < 0.05, axis=-1)), (best_x, best_y)
    np.testing.assert_allclose(best_y, problem.minimum, rtol=0.005)
