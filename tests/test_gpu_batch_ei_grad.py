"""GPU tests of the analytic batch EI's gradient (tgp_batch_ei_moments_grad / tgp_batch_ei_value_grad,
bei_grad_tail_kernel): against the 50-digit directional derivatives, against the torch autograd restatement
(tests/batch_ei_grad_reference.py) on random moments and behind the engine's own posterior, against central differences of
the engine's forward entry, bit-identity, refusals, and the opt-in rule end to end.

Tolerance of the comparisons on given moments: both sides are float64 evaluations of one derivative.  The restatement's own
worst error against the goldens is GRAD_RESTATEMENT_WORST of the scale tests/test_batch_ei_grad_reference.py defines (sum
|g_i| |d_i| along a random direction; the array's largest |entry| for a single coordinate); the kernel gets 100 x that, the
project's factor for the value kernel."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import batch_ei_grad_reference as GR
from tests import batch_ei_reference as R
from tests.make_batch_ei_grad_goldens import direction_arrays
from tests.test_batch_ei_grad_reference import (GRAD_RESTATEMENT_WORST, case_arrays, direction_scale, golden_gradient,
                                                load_directions)
from tests.test_batch_ei_reference import load_cases
from tests.test_gpu_batch_ei import KERNEL_TOL, POSTERIOR_CONFIGS, _ard, _bare_engine, _branin_setup, _check, _perturbed, \
    _random_moments
from tests.test_gpu_parity import _dense_joint_vjp
from tests.util import cancellation_floor

pytestmark = pytest.mark.gpu

GRAD_TOL = 100.0 * GRAD_RESTATEMENT_WORST


def test_moments_grad_entry_matches_the_mpmath_goldens():
    """Value at the forward test's tolerance; every golden directional derivative <gmean, dm> + <gcov, dC> within GRAD_TOL of
    its scale, the scale taken with the golden's own adjoint entries where the file holds them all (q <= 4) and with the
    restatement's otherwise (q = 6, 8: three random directions do not give the entries)."""
    from trieste_amd.engine import batch_ei_moments_grad

    eng = _bare_engine()
    cases, dirs = load_cases(), load_directions()
    got = {}
    for d in dirs:
        n = d["case"]
        c = cases[n]
        q = c["q"]
        if n not in got:
            mean, cov, w1, w2 = case_arrays(c)
            v, gm, gc = batch_ei_moments_grad(eng, mean, cov, w1, w2, c["eta"])
            _check(v, [c["value"]], KERNEL_TOL * c["abs_terms"], f"golden value q={q} ({c['note']})")
            np.testing.assert_array_equal(gc[0], gc[0].T)
            gold = golden_gradient(n, q, dirs)
            if gold is None:
                _, rm, rc, _ = GR.batch_ei_value_grad(mean, cov, c["eta"], w1, w2)
                gold = (rm[0], rc[0])
            got[n] = (gm[0], gc[0], gold)
        gm, gc, gold = got[n]
        dm, dC = direction_arrays(q, d)
        have = float(gm @ dm + np.sum(gc * dC))
        _check([have], [d["deriv"]], GRAD_TOL * direction_scale(d, dm, dC, *gold),
               f"golden derivative case {n} q={q} {d['kind']} {d.get('i', '')} {d.get('j', '')}")


# q = 16 is compared at S <= 65: the restatement holds [G q^2, S, q] arrays and their autograd graph
@pytest.mark.parametrize("q,S", [(q, S) for q in (2, 3, 5, 8, 16) for S in (1, 63, 64, 65, 500) if (q, S) != (16, 500)])
def test_moments_grad_entry_matches_the_restatement_on_random_batches(q, S):
    """gmean and gcov entrywise within GRAD_TOL x the largest |entry| of that array in that q-batch (the restatement's);
    gcov exactly symmetric.  val: bit-identical to tgp_batch_ei_moments' (the new kernel repeats the forward kernel's
    arithmetic operation for operation and in the same order), and within the forward test's tolerance of the restatement."""
    from trieste_amd.engine import batch_ei_moments, batch_ei_moments_grad

    G = 200 if q <= 5 else (64 if q == 8 else 16)
    rng = np.random.default_rng(1000 * q + S)
    mean, cov, eta = _random_moments(q, G, rng)
    w1, w2 = R.sobol_points(S, q, skip=3 * q + S)
    want, wm, wc, scale = GR.batch_ei_value_grad(mean, cov, eta, w1, w2)
    assert np.count_nonzero(want > 1e-3 * want.max()) >= want.size // 2
    eng = _bare_engine()
    val, gm, gc = batch_ei_moments_grad(eng, mean, cov, w1, w2, eta)
    fwd = batch_ei_moments(eng, mean, cov, w1, w2, eta)
    np.testing.assert_array_equal(val, fwd)
    _check(val, want, KERNEL_TOL * scale, f"grad entry's value q={q} S={S}")
    np.testing.assert_array_equal(gc, gc.transpose(0, 2, 1))
    _check(gm, wm, GRAD_TOL * np.abs(wm).max(axis=1, keepdims=True) * np.ones_like(wm), f"gmean q={q} S={S}")
    _check(gc, wc, GRAD_TOL * np.abs(wc).max(axis=(1, 2), keepdims=True) * np.ones_like(wc), f"gcov q={q} S={S}")


GRAD_POSTERIOR_CONFIGS = [c for c in POSTERIOR_CONFIGS if c[0] in (
    "branin_m52_N50", "hartmann_rbf_N300", "ackley8_m52_N1000_lownoise", "ackley40_m52_ard_N200", "ackley64_rbf_N1000")]


@pytest.mark.parametrize("cfg", GRAD_POSTERIOR_CONFIGS, ids=[c[0] for c in GRAD_POSTERIOR_CONFIGS])
def test_value_grad_behind_the_posterior_matches_the_restatement_through_the_dense_vjp(cfg):
    """tgp_batch_ei_value_grad vs dense VJP o restatement's adjoints o oracle.predict_joint.  Tolerance: qEI's gradient
    tolerance (rtol 1e-5, atol max(floor 1e3 q, 1e-7 max |want|)) plus, per q-batch, 2 x the largest change of ``want`` over
    the five seeded perturbations of the oracle's moments the joint parity tests allow.  A q-batch whose extra term exceeds
    1e-2 of the median over the call of max |want| says nothing and is left out (at most one in ten; finite values and
    gradients are still asserted for it).  Special batches (a near-duplicate pair, a point next to a training input) fill
    at most the first twentieth of the call, at least two of them."""
    from trieste_amd.engine import GPEngine, batch_ei_value_grad

    _, obj, d, kind, N, noise, ard = cfg
    X, Y = O.synthetic_problem(obj, d, N)
    ls = _ard(d, 17) if ard else O.default_lengthscales(d)
    c = float(np.mean(Y))
    st = O.gpr_update(kind, 1.0, ls, noise, c, X, Y)
    eng = GPEngine(d, kind)
    eng.set_hyper(1.0, ls, noise, c)
    eng.set_data(X, Y)
    floor = cancellation_floor(N, 1.0, noise)
    rng = np.random.default_rng(29)
    S = 64
    for q, G in ((2, 60), (3, 30), (4, 40), (8, 30)):
        Xg = rng.uniform(size=(G, q, d))
        special = max(2, (G // 20) & ~1)   # an even count: pairs of rows, never past the first twentieth
        for g in range(0, special, 2):
            Xg[g, 1] = Xg[g, 0] + 1e-3 * rng.standard_normal(d) / np.sqrt(d)          # a near-duplicate pair
            Xg[g + 1, 0] = X[g % N] + 1e-4 * rng.standard_normal(d) / np.sqrt(d)      # next to a training input
        mean, cov = O.predict_joint(st, Xg)
        assert np.all(np.diagonal(cov, axis1=1, axis2=2) > 1e-12)   # no clipped variance: the restatement has no clip
        eta = float(np.median(mean.min(axis=1)))
        w1, w2 = R.sobol_points(S, q, skip=5 + q)
        wval, gm, gc, scale = GR.batch_ei_value_grad(mean, cov, eta, w1, w2)
        assert np.count_nonzero(wval > 1e-3 * wval.max()) >= G // 2
        want = _dense_joint_vjp(st, Xg, gm, gc)
        assert np.all(np.isfinite(want))
        moved = np.zeros(G)
        for seed in range(5):
            m2, c2 = _perturbed(mean, cov, floor, np.random.default_rng(100 + seed))
            _, gm2, gc2, _ = GR.batch_ei_value_grad(m2, c2, eta, w1, w2)
            moved = np.maximum(moved, np.abs(_dense_joint_vjp(st, Xg, gm2, gc2) - want).max(axis=(1, 2)))
        extra = 2.0 * moved
        per_batch = np.abs(want).max(axis=(1, 2))
        keep = extra <= 1e-2 * np.median(per_batch)
        dropped = np.flatnonzero(~keep)
        assert dropped.size <= G // 10, f"q={q}: {dropped.size} of {G} batches excluded: {dropped.tolist()}"
        val, grad = batch_ei_value_grad(eng, Xg, w1, w2, eta)
        val, grad = np.asarray(val), np.asarray(grad)
        assert val.shape == (G,) and grad.shape == (G, q, d)
        assert np.all(np.isfinite(val)) and np.all(np.isfinite(grad))
        print(f"{cfg[0]} q={q} G={G}: extra term / median max|want| median {np.median(extra) / np.median(per_batch):.2e} "
              f"max {extra.max() / np.median(per_batch):.2e}; median max|want| {np.median(per_batch):.3e}; "
              f"excluded {dropped.tolist()}")
        atol = max(floor * 1e3 * q, 1e-7 * np.abs(want).max())
        tol = 1e-5 * np.abs(want) + atol + extra[:, None, None]
        _check(grad[keep], want[keep], tol[keep], f"batch EI gradient q={q} G={G}")


def test_gradient_agrees_with_central_differences_of_the_forward_entry():
    """Ties tgp_batch_ei_value_grad to the merged tgp_batch_ei: central differences of the forward entry in a handful of
    coordinates, steps h and h / 2 with h = 1e-4 x the lengthscale.  The differences' own accuracy: truncation (twice the
    change from h to h / 2; the finer one's error is a third of it) plus the posterior's float64 noise in the moments
    (the cancellation floor per entry, weighted with the tail's own adjoints) divided by the step."""
    from trieste_amd.engine import GPEngine, batch_ei, batch_ei_moments_grad, batch_ei_value_grad

    d, N, noise = 6, 300, 1e-2
    X, Y = O.synthetic_problem(O.hartmann_6, d, N)
    ls, c = O.default_lengthscales(d), float(np.mean(Y))
    eng = GPEngine(d, "matern52")
    eng.set_hyper(1.0, ls, noise, c)
    eng.set_data(X, Y)
    floor = cancellation_floor(N, 1.0, noise)
    rng = np.random.default_rng(31)
    for q, G, S in ((2, 12, 100), (4, 12, 64), (8, 6, 64)):
        Xg = rng.uniform(size=(G, q, d))
        w1, w2 = R.sobol_points(S, q, skip=17)
        mean, cov = eng.joint_forward(Xg)
        eta = float(np.median(np.asarray(mean).min(axis=1)))
        val, grad = batch_ei_value_grad(eng, Xg, w1, w2, eta)
        _, gm, gc = batch_ei_moments_grad(eng, mean, cov, w1, w2, eta)
        noise_val = floor * (np.abs(gm).sum(axis=1) + np.abs(gc).sum(axis=(1, 2)))   # [G]
        assert np.count_nonzero(val > 1e-3 * val.max()) >= G // 2
        for _ in range(6):
            j, k = int(rng.integers(q)), int(rng.integers(d))
            h = 1e-4 * float(ls[k])
            cd = []
            for s in (h, h / 2):
                Xp, Xm = Xg.copy(), Xg.copy()
                Xp[:, j, k] += s
                Xm[:, j, k] -= s
                cd.append((batch_ei(eng, Xp, w1, w2, eta) - batch_ei(eng, Xm, w1, w2, eta)) / (2 * s))
            tol = 2.0 * np.abs(cd[0] - cd[1]) + 2.0 * noise_val / (h / 2)
            err = np.abs(grad[:, j, k] - cd[1])
            gs = np.abs(grad).max(axis=(1, 2))
            print(f"q={q} coordinate ({j}, {k}): error {err.max():.2e}, tolerance {tol.min():.2e} ... {tol.max():.2e}, "
                  f"max |grad| per batch {gs.min():.2e} ... {gs.max():.2e}")
            assert np.median(tol / gs) <= 1e-2, "the differences say nothing at this step"
            assert np.all(err <= tol), (err, tol)


def test_two_calls_two_handles_and_both_residencies_return_identical_bits():
    import torch

    from trieste_amd.engine import GPEngine, batch_ei_moments_grad, batch_ei_value_grad

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
    cu = lambda a: torch.as_tensor(np.ascontiguousarray(a)).cuda()  # noqa: E731
    for q, G, S in ((2, 40, 64), (3, 50, 100), (8, 100, 130), (16, 20, 33)):
        Xg = rng.uniform(size=(G, q, d))
        w1, w2 = R.sobol_points(S, q, skip=9)
        mean, cov = engines[0].joint_forward(Xg)
        eta = float(np.median(np.asarray(mean).min(axis=1)))
        v, g = batch_ei_value_grad(engines[0], Xg, w1, w2, eta)
        assert np.any(v != 0.0) and np.any(g != 0.0)
        for other in (batch_ei_value_grad(engines[0], Xg, w1, w2, eta), batch_ei_value_grad(engines[1], Xg, w1, w2, eta)):
            np.testing.assert_array_equal(v, other[0])
            np.testing.assert_array_equal(g, other[1])
        dv, dgr = batch_ei_value_grad(engines[0], cu(Xg), cu(w1), cu(w2), eta)
        assert dv.is_cuda and dgr.is_cuda
        np.testing.assert_array_equal(v, dv.cpu().numpy())
        np.testing.assert_array_equal(g, dgr.cpu().numpy())
        # the tail alone on the moments the engine returned
        mv, mm, mc = batch_ei_moments_grad(engines[0], mean, cov, w1, w2, eta)
        np.testing.assert_array_equal(v, mv)
        for other in (batch_ei_moments_grad(engines[0], mean, cov, w1, w2, eta),
                      batch_ei_moments_grad(engines[1], mean, cov, w1, w2, eta),
                      tuple(t.cpu().numpy() for t in batch_ei_moments_grad(engines[1], cu(mean), cu(cov), w1, w2, eta))):
            for a, b in zip((mv, mm, mc), other):
                np.testing.assert_array_equal(a, b)
        # ... and its adjoints through tgp_joint_vjp: the fused call's gradient
        np.testing.assert_array_equal(g, engines[1].joint_vjp(Xg, mm, mc))


def test_refusals():
    import torch

    from trieste_amd import _lib
    from trieste_amd.engine import GPEngine, batch_ei_moments_grad, batch_ei_value_grad

    eng = _bare_engine()
    lib, h = eng._lib, eng._h
    val, gm, gc = np.zeros(4), np.zeros((4, 17)), np.zeros((4, 17, 17))
    w = np.full((8, 17), 0.5)
    mean, cov = np.zeros((4, 17)), np.tile(np.eye(17), (4, 1, 1))
    p = lambda a: a.ctypes.data  # noqa: E731

    def moments(q, w1, w2, S, m=p(mean), v=p(val)):
        return lib.tgp_batch_ei_moments_grad(h, m, p(cov), 4, q, w1, w2, S, 0.0, v, p(gm), p(gc), _lib.HOST)

    assert moments(1, p(w), p(w), 8) == _lib.TGP_ERR_SHAPE
    assert b"2..16" in lib.tgp_last_error(h)
    assert moments(17, p(w), p(w), 8) == _lib.TGP_ERR_SHAPE
    assert moments(3, p(w), p(w), 0) == _lib.TGP_ERR_ARG
    assert moments(3, None, p(w), 8) == _lib.TGP_ERR_ARG
    assert moments(3, p(w), None, 8) == _lib.TGP_ERR_ARG
    assert moments(3, p(w), p(w), 8, m=None) == _lib.TGP_ERR_ARG
    assert moments(3, p(w), p(w), 8, v=None) == _lib.TGP_ERR_ARG
    Xq = np.zeros((4, 17, 2))
    grad = np.zeros((4, 17, 2))

    def fused(hh, G, q, w1, w2, S, v=p(val), g=p(grad)):
        return lib.tgp_batch_ei_value_grad(hh, p(Xq), G, q, w1, w2, S, 0.0, v, g, _lib.HOST)

    assert fused(h, 4, 1, p(w), p(w), 8) == _lib.TGP_ERR_SHAPE
    assert fused(h, 4, 17, p(w), p(w), 8) == _lib.TGP_ERR_SHAPE
    assert fused(h, 4, 3, p(w), p(w), 0) == _lib.TGP_ERR_ARG
    assert fused(h, 4, 3, None, p(w), 8) == _lib.TGP_ERR_ARG
    assert fused(h, 4, 3, p(w), p(w), 8, v=None) == _lib.TGP_ERR_ARG
    assert fused(h, 4, 3, p(w), p(w), 8, g=None) == _lib.TGP_ERR_ARG
    assert fused(h, 4, 3, p(w), p(w), 8) == _lib.TGP_ERR_STATE     # no data on the handle
    d, N = 2, 30
    X, Y = O.synthetic_problem(O.branin, d, N)
    full = GPEngine(d, "matern52")
    full.set_hyper(1.0, O.default_lengthscales(d), 1e-3, 0.0)
    full.set_data(X, Y)
    big = np.zeros((683, 3, 2))
    bv, bg = np.zeros(683), np.zeros((683, 3, 2))
    assert lib.tgp_batch_ei_value_grad(full._h, p(big), 683, 3, p(w), p(w), 8, 0.0, p(bv), p(bg), _lib.HOST) == _lib.TGP_ERR_SHAPE
    # the Python layer
    w1, w2 = R.sobol_points(8, 3)
    with pytest.raises(ValueError):
        batch_ei_moments_grad(eng, np.zeros((2, 1)), np.ones((2, 1, 1)), np.zeros((8, 1)), np.zeros((8, 0)), 0.0)
    with pytest.raises(ValueError):
        batch_ei_moments_grad(eng, np.zeros((2, 17)), np.tile(np.eye(17), (2, 1, 1)), w[:, :17], w[:, :16], 0.0)
    with pytest.raises(ValueError):
        batch_ei_moments_grad(eng, np.zeros((2, 3)), np.tile(np.eye(3), (2, 1, 1)), w1, w1, 0.0)      # w2 of the wrong width
    with pytest.raises(ValueError):   # mixed residency
        batch_ei_moments_grad(eng, torch.zeros((2, 3), dtype=torch.float64).cuda(), np.tile(np.eye(3), (2, 1, 1)), w1, w2, 0.0)
    with pytest.raises(ValueError):
        batch_ei_value_grad(full, np.zeros((2, 3, 5)), w1, w2, 0.0)                                  # d = 5 on a d = 2 engine
    with pytest.raises(ValueError):
        batch_ei_value_grad(full, np.zeros((2, 1, 2)), np.zeros((8, 1)), np.zeros((8, 0)), 0.0)
    with pytest.raises(ValueError):
        batch_ei_value_grad(full, np.zeros((683, 3, 2)), w1, w2, 0.0)                                # 2049 points
    with pytest.raises(ValueError):   # Sobol points on the device, the batch on the host
        batch_ei_value_grad(full, np.zeros((2, 3, 2)), torch.as_tensor(w1).cuda(), torch.as_tensor(w2).cuda(), 0.0)
    # an indefinite covariance (input data: an argument check, nothing faults) names its group
    covs = np.tile(np.eye(3), (6, 1, 1))
    covs[4] = np.array([[1.0, 2.0, 0.0], [2.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    with pytest.raises(_lib.NotPositiveDefiniteError, match="group 4"):
        batch_ei_moments_grad(eng, np.zeros((6, 3)), covs, w1, w2, 0.0)
    # ... and the handle is usable afterwards
    ok = batch_ei_moments_grad(eng, np.zeros((6, 3)), np.tile(np.eye(3), (6, 1, 1)), w1, w2, 0.0)
    assert all(np.all(np.isfinite(a)) for a in ok) and np.all(ok[0] > 0.0)


def _known_batches(space, q, n, seed):
    """A sampler callable for ``generate_continuous_optimizer``: one batch of n known candidates of space ** q."""
    cands = (space ** q).sample(n, seed=seed)

    def sampler(_space):
        yield cands

    return sampler, cands


def test_ego_with_the_differentiable_batch_ei_in_an_ask_tell_loop_on_the_real_engine():
    """EfficientGlobalOptimization(BatchExpectedImprovement(100, differentiable=True), num_query_points=3): runs, returns
    [3, 2] points in the box; and with known initial batches the value at the returned batch is >= the largest value among
    them (L-BFGS-B starts from the top-k of them, no run ends below its start, the result is the arg-max over the runs).
    The only slack: 1e-5 |value| + 1e-9 between the two posterior routes a large and a small call take."""
    import trieste_amd
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import (BatchExpectedImprovement, EfficientGlobalOptimization,
                                         differentiable_batch_expected_improvement, generate_continuous_optimizer)
    from trieste_amd.ask_tell_optimization import AskTellOptimizer
    from trieste_amd.data import Dataset

    trieste_amd.set_seed(11)
    space, data, model = _branin_setup(8, seed=2)
    rule = EfficientGlobalOptimization(BatchExpectedImprovement(100, differentiable=True), num_query_points=3)
    opt = AskTellOptimizer(space, data, model, rule)
    for _ in range(2):
        pts = np.asarray(opt.ask())
        assert pts.shape == (3, 2) and np.all(pts >= space.lower) and np.all(pts <= space.upper)
        opt.tell(Dataset(pts, OBJ.scaled_branin(pts)))
    assert isinstance(rule.acquisition_function, differentiable_batch_expected_improvement)
    # the property, on known initial batches
    trieste_amd.set_seed(12)
    space, data, model = _branin_setup(8, seed=3)
    sampler, cands = _known_batches(space, 3, 3000, seed=5)
    rule = EfficientGlobalOptimization(BatchExpectedImprovement(100, differentiable=True), num_query_points=3,
                                       optimizer=generate_continuous_optimizer(sampler, num_optimization_runs=8))
    pts = np.asarray(AskTellOptimizer(space, data, model, rule).ask())
    assert pts.shape == (3, 2) and np.all(pts >= space.lower) and np.all(pts <= space.upper)
    fn = rule.acquisition_function
    vals = np.asarray(fn(cands.reshape(3000, 3, 2)))[:, 0]
    start = float(vals.max())
    refined = float(np.asarray(fn(pts[None]))[0, 0])
    v1, g1 = fn.value_and_gradient(pts[None])
    assert abs(float(v1[0]) - refined) <= 1e-5 * abs(refined) + 1e-9
    # (random search alone over the same candidates returns their arg-max: ``start``)
    print(f"random search alone (the best of 3000 batches): {start:.6e}; refined by L-BFGS-B from the top 8: {refined:.6e}")
    assert start > 0.0 and refined >= start - (1e-5 * abs(start) + 1e-9)


@pytest.mark.slow  # as in the reference: run with --runslow yes (the step budget is tuned to ITS seeds)
def test_bayesian_optimizer_with_the_differentiable_batch_ei_finds_minima_of_scaled_branin():
    """The forward file's Branin bar (reference tests/integration/test_bayesian_optimization.py:131-137) with the opt-in
    builder: 12 steps of 3 points from 5 initial ones."""
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
    rule = EfficientGlobalOptimization(BatchExpectedImprovement(100, differentiable=True), num_query_points=3)
    result = BayesianOptimizer(lambda x: Dataset(x, problem.objective(x)), space).optimize(
        12, data, model, rule, fit_initial_model=False,
        early_stop_callback=stop_at_minimum(problem.minimum, problem.minimizers, minimum_rtol=0.005, minimum_step_number=2))
    assert result.final_result.is_ok, result.final_result
    best_x, best_y, _ = result.try_get_optimal_point()
    minimizer_err = np.abs((best_x - problem.minimizers) / problem.minimizers)
    assert np.any(np.all(minimizer_err < 0.05, axis=-1)), (best_x, best_y)
    np.testing.assert_allclose(best_y, problem.minimum, rtol=0.005)
