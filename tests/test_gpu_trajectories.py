"""The decoupled-trajectory path across its instantiations: a covering design over batch forms, padded dimensions, arg-min
edges and the RFF phase (tgp_traj_create, tgp_traj_create_rff, tgp_traj_eval, tgp_traj_argmin[_async], tgp_traj_value_grad;
csrc/tgp_kernels_traj.hip).

1. Batch forms: B in {1, 2, 3, 4, 5, 15, 16} per kernel kind takes every shared-input form of launch_traj_bp (1 exact, 4 masked,
   4 exact, 16 masked, 16 exact) and the per-trajectory form -- against the oracle at the tolerances of the parity suites, and
   BIT FOR BIT against each other: every form accumulates a column with the same fused multiply-adds in the same order, so
   column b of a size-B trajectory equals the one-column trajectory built from column b alone, and shared inputs equal the same
   inputs broadcast per trajectory.
2. B > 16 (17, 33): creation is allowed, the per-trajectory calls work, the shared-input calls refuse.
3. Padded dimensions: d in {1, 2, 5, 7, 9, 17, 32} (dp = 2, 2, 6, 8, 16, 32, 32), d = 17 on the box [1024, 1025]^17.
4. Arg-min: candidate counts around the wave and block sizes, ties, index bases, NaN rows, no candidates.
5. The RFF phase against the mpmath golden inside the bound derived in tests/traj_cases.py."""
import functools
import types

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import traj_cases as T
from tests.util import assert_close, cancellation_floor, record_margin

pytestmark = pytest.mark.gpu

KINDS = ("rbf", "matern12", "matern32", "matern52")
MEAN_C = 0.25
NOISE = 1e-2


@pytest.fixture(autouse=True)
def _difference_form_oracle():
    with O.difference_form():
        yield


def _engine(p):
    from trieste_amd.engine import GPEngine

    eng = GPEngine(p.d, p.kind)
    eng.set_hyper(p.variance, p.ls, p.noise, p.c)
    eng.set_data(p.X, p.Y)
    return eng


@functools.lru_cache(maxsize=None)
def _problem(kind, d=3, N=40, F=37, cols=16, lo=0.0, M=300, P=9, seed=0):
    """One small model with its draws: the basis W, b, `cols` columns of prior weights w and noise draws xi (a batch of size B
    takes the first B), M shared candidates (some at and next to training inputs) and P points per trajectory."""
    from trieste_amd.sampler import sample_rff_basis

    p = types.SimpleNamespace(kind=kind, d=d, N=N, F=F, variance=1.3, noise=NOISE, c=MEAN_C, lo=lo)
    U, p.Y = O.synthetic_problem(O.ackley, d, N, seed=1234 + seed)
    p.X = lo + U
    p.ls = O.default_lengthscales(d)
    p.st = O.gpr_update(kind, p.variance, p.ls, p.noise, p.c, p.X, p.Y)
    p.floor = cancellation_floor(N, p.variance, p.noise)
    rng = np.random.default_rng([d, N, F, seed])
    p.W, p.b = sample_rff_basis(kind, F, d, rng)
    p.w, p.xi, p.eps = rng.standard_normal((F, cols)), rng.standard_normal((N, cols)), rng.standard_normal((F, cols))
    Xq = lo + rng.uniform(size=(M, d))
    Xq[:3] = p.X[:3]
    Xq[3:6] = p.X[3:6] + 1e-6
    p.Xq = np.ascontiguousarray(Xq)
    p.Xp = lo + rng.uniform(size=(P, cols, d))
    p.Xp[0, 0] = p.X[3]    # r = 0: the kink of Matern-1/2
    return p


def _create(eng, p, cols, rff):
    return eng.trajectory_rff(p.W, p.b, p.eps[:, cols]) if rff else eng.trajectory(p.W, p.b, p.w[:, cols], p.xi[:, cols])


def _readings(traj, p, cols, rff, shared=True):
    """Everything a trajectory returns, for comparisons bit for bit."""
    r = types.SimpleNamespace(weights=traj.theta() if rff else traj.v(), per=traj(np.ascontiguousarray(p.Xp[:, cols])))
    if shared:
        r.vals = traj(p.Xq)
        r.amin, r.aidx = traj.argmin(p.Xq)
    return r


@functools.lru_cache(maxsize=None)
def _singles(key, rff, shared=True):
    """The one-column trajectory of every column of the problem `key` (the arguments of `_problem`)."""
    with O.difference_form():
        p = _problem(*key)
    eng = _engine(p)
    out = []
    for b in range(p.w.shape[1]):
        t = _create(eng, p, slice(b, b + 1), rff)
        out.append(_readings(t, p, slice(b, b + 1), rff, shared))
        t.close()
    eng.close()
    return out


def _against_oracle(traj, p, B, rff, shared=True):
    """Weights, values (shared and per-trajectory inputs) and gradients of a size-B trajectory against the oracle; returns
    its readings."""
    cols = slice(0, B)
    r = _readings(traj, p, cols, rff, shared)
    w, xi, eps, Xp = p.w[:, cols], p.xi[:, cols], p.eps[:, cols], np.ascontiguousarray(p.Xp[:, cols])
    if rff:
        oth = O.rff_theta(p.st, p.W, p.b, eps)
        tscale = max(1.0, np.abs(oth).max())
        assert_close(r.weights, oth, rtol=1e-6, atol=1e-9 * tscale / min(p.noise, 1.0), what=f"theta B={B}")
        wf, v = r.weights, np.zeros((p.N, B))
        ev = lambda X: O.rff_trajectory_eval(p.st, p.W, p.b, wf, X)
        rv, av, rg = 1e-9, 1e-9 * tscale, 1e-7       # the tolerances of the RFF-weight parity test
    else:
        ov = O.decoupled_weights(p.st, p.W, p.b, w, xi)
        assert_close(r.weights, ov, atol=p.floor * max(1.0, np.abs(ov).max()) / min(p.noise, 1.0), what=f"v B={B}")
        wf, v = w, r.weights
        tscale = np.sqrt(p.variance) * max(1.0, np.abs(v).max())
        ev = lambda X: O.trajectory_eval(p.st, p.W, p.b, wf, v, X)
        rv, av, rg = 1e-7, 1e-8 * tscale, 1e-6       # the tolerances of the shifted-input trajectory test
    if shared:
        assert_close(r.vals, ev(p.Xq), rtol=rv, atol=av, what=f"values, shared inputs B={B}")
        np.testing.assert_array_equal(r.aidx, np.argmin(r.vals, axis=0))
        np.testing.assert_array_equal(r.amin, r.vals[r.aidx, np.arange(B)])
    assert_close(r.per, ev(Xp), rtol=rv, atol=av, what=f"values, per-trajectory inputs B={B}")
    val, grad = traj.value_and_gradient(Xp)
    oval, ograd = O.trajectory_value_and_grad(p.st, p.W, p.b, wf, v, Xp)
    assert_close(val, oval, rtol=rv, atol=av, what=f"value of value_and_gradient B={B}")
    sl = slice(1, None) if p.kind == "matern12" and not rff else slice(None)   # d k / dx is discontinuous at r = 0
    assert_close(grad[sl], ograd[sl], rtol=rg, atol=1e-8 * np.abs(ograd).max(), what=f"gradient B={B}")
    if B == 1:  # another kernel with libm's cos: close, not bitwise
        assert_close(val, r.per, rtol=1e-10, atol=1e-9 * tscale, what="value == traj_eval")
    return r


def _columns_equal_singles(r, singles, B, shared=True):
    for b in range(B):
        s = singles[b]
        np.testing.assert_array_equal(r.weights[:, b], s.weights[:, 0], err_msg=f"weights of column {b} of {B}")
        np.testing.assert_array_equal(r.per[:, b], s.per[:, 0], err_msg=f"per-trajectory values of column {b} of {B}")
        if shared:
            np.testing.assert_array_equal(r.vals[:, b], s.vals[:, 0], err_msg=f"shared-input values of column {b} of {B}")
            assert (r.amin[b], r.aidx[b]) == (s.amin[0], s.aidx[0]), f"arg-min of column {b} of {B}"


def _shared_equals_broadcast(traj, p, B):
    Xb = np.ascontiguousarray(np.broadcast_to(p.Xq[:, None, :], (p.Xq.shape[0], B, p.d)))
    np.testing.assert_array_equal(traj(p.Xq), traj(Xb), err_msg=f"shared form vs per-trajectory form, B={B}")


# ---- 1. batch forms ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (1, 2, 3, 4, 5, 15, 16))
@pytest.mark.parametrize("kind", KINDS)
def test_batch_forms(kind, B):
    key = (kind,)
    p = _problem(*key)
    eng = _engine(p)
    traj = _create(eng, p, slice(0, B), False)
    r = _against_oracle(traj, p, B, False)
    _columns_equal_singles(r, _singles(key, False), B)
    _shared_equals_broadcast(traj, p, B)


@pytest.mark.parametrize("B", (1, 2, 4, 5, 16))
@pytest.mark.parametrize("F", (23, 47), ids=("design", "gram"))
def test_batch_forms_rff(F, B):
    """The RFF weight posterior in design space (F < N) and gram space (F >= N): theta, values, arg-min, gradient."""
    key = ("matern52", 3, 40, F)
    p = _problem(*key)
    eng = _engine(p)
    traj = _create(eng, p, slice(0, B), True)
    r = _against_oracle(traj, p, B, True)
    _columns_equal_singles(r, _singles(key, True), B)
    _shared_equals_broadcast(traj, p, B)
    with pytest.raises(RuntimeError):
        traj.v()


# ---- 2. more than 16 trajectories -------------------------------------------------------------------------------------------------
def _shared_calls_refuse(traj, p):
    import torch

    for call in (lambda: traj(p.Xq), lambda: traj.argmin(p.Xq), lambda: traj.argmin_pairs(torch.from_numpy(p.Xq).cuda())):
        with pytest.raises(ValueError, match="B <= 16"):
            call()


@pytest.mark.parametrize("stale_scratch", (False, True), ids=("fresh", "after-predict"))
@pytest.mark.parametrize("B", (17, 33))
def test_more_than_16_trajectories(B, stale_scratch):
    """tgp_traj_create projects Phi_Z w for ALL B columns (its shared-input projection holds 16 per launch): every column of v
    against the oracle and against its one-column trajectory, also when the handle's output scratch holds the values of an
    earlier call (a `predict` of more than N B points) where columns 16 .. B - 1 of the projection would land."""
    key = ("matern52", 3, 40, 37, 33)
    p = _problem(*key)
    eng = _engine(p)
    if stale_scratch:
        mean, _ = eng.predict(np.random.default_rng(5).uniform(size=(p.N * B + 64, p.d)))
        assert np.all(np.isfinite(mean)) and np.abs(mean).max() > 1e-3
    traj = _create(eng, p, slice(0, B), False)
    r = _against_oracle(traj, p, B, False, shared=False)
    _columns_equal_singles(r, _singles(key, False, False), B, shared=False)
    _shared_calls_refuse(traj, p)


@pytest.mark.parametrize("B", (17, 33))
def test_more_than_16_rff_trajectories(B):
    key = ("matern52", 3, 40, 23, 33)
    p = _problem(*key)
    eng = _engine(p)
    traj = _create(eng, p, slice(0, B), True)
    r = _against_oracle(traj, p, B, True, shared=False)
    _columns_equal_singles(r, _singles(key, True, False), B, shared=False)
    _shared_calls_refuse(traj, p)


def test_parallel_thompson_sampling_of_20_points():
    """ParallelContinuousThompsonSampling through EGO with 20 query points: the sampler's 20 trajectories carry the canonical
    weights of the oracle for its own draws (replayed from its seed), and the 20 points are finite points of the box."""
    import trieste_amd.models as M
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import (EfficientGlobalOptimization, ParallelContinuousThompsonSampling,
                                         generate_continuous_optimizer)
    from trieste_amd.data import Dataset
    from trieste_amd.sampler import DecoupledTrajectorySampler, sample_rff_basis
    from trieste_amd.space import Box

    q, n, F, noise, seed = 20, 30, 64, 1e-2, 4242
    space = Box([0, 0], [1, 1])
    x = space.sample(n, seed=1)
    data = Dataset(x, OBJ.scaled_branin(x))
    gpr = M.build_gpr(data, space, likelihood_variance=noise)
    model = M.GaussianProcessRegression(gpr, num_rff_features=F)
    model.trajectory_sampler = lambda: DecoupledTrajectorySampler(model, F, seed=seed)
    k = gpr.kernel
    st = O.gpr_update(k.kind, k.variance, k.lengthscales, noise, gpr.mean_function.c, x, data.observations[:, 0])
    opt = generate_continuous_optimizer(num_initial_samples=400, num_optimization_runs=2)
    rule = EfficientGlobalOptimization(ParallelContinuousThompsonSampling(), optimizer=opt, num_query_points=q)
    pts = rule.acquire_single(space, model, dataset=data)
    assert pts.shape == (q, 2) and np.all(np.isfinite(pts)) and all(pt in space for pt in pts)
    rng = np.random.default_rng(seed)    # the sampler's draws, in its order: basis, then w, then xi
    W, b = sample_rff_basis(k.kind, F, 2, rng)
    w, xi = rng.standard_normal((F, q)), rng.standard_normal((n, q))
    held = rule.acquisition_function.trajectory._traj
    assert held.B == q
    ov = O.decoupled_weights(st, W, b, w, xi)
    floor = cancellation_floor(n, k.variance, noise)
    assert_close(held.v(), ov, atol=floor * max(1.0, np.abs(ov).max()) / min(noise, 1.0), what="v of the 20 trajectories")


# ---- 3. padded dimensions ---------------------------------------------------------------------------------------------------------
DIMS = [("matern52", d) for d in (1, 2, 5, 7, 9, 17, 32)] + [("matern12", 17)]


@pytest.mark.parametrize("kind,d", DIMS, ids=[f"{k}-d{d}" for k, d in DIMS])
def test_padded_dimensions(kind, d):
    """d < dp wherever a padded width allows it; d = 17 on [1024, 1025]^17, where the canonical part is centred on the first
    training input and the RFF phase is not, so a padded column that is not an exact zero would show."""
    B = 3
    p = _problem(kind, d, 33, 20, 3, 1024.0 if d == 17 else 0.0)
    eng = _engine(p)
    traj = _create(eng, p, slice(0, B), False)
    _against_oracle(traj, p, B, False)
    _shared_equals_broadcast(traj, p, B)


# ---- 4. arg-min edges -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def amin():
    with O.difference_form():
        p = _problem("matern52", 3, 40, 37, 16, 0.0, 600)
    eng = _engine(p)
    traj = _create(eng, p, slice(0, 5), False)
    yield types.SimpleNamespace(p=p, eng=eng, traj=traj, B=5)
    traj.close()
    eng.close()


def _argmin_is_first_minimum(a, Xq, index_base=0):
    got = a.traj(Xq)
    vals, idx = a.traj.argmin(Xq, index_base)
    want = np.nanargmin(got, axis=0)   # the first of equal minima, NaN rows never
    np.testing.assert_array_equal(idx, index_base + want)
    np.testing.assert_array_equal(vals, got[want, np.arange(a.B)])
    return vals, idx


@pytest.mark.parametrize("M", (1, 63, 64, 65, 255, 256, 257, 513))
def test_argmin_candidate_counts(amin, M):
    """Around one wave (64), one block (256) and two blocks: the wave reduce, the 4-wave reduce in LDS, the reduce over
    blocks."""
    _argmin_is_first_minimum(amin, amin.p.Xq[:M])


PLACES = {"same wave": (5, 40, 130, 300), "later lane first": (40, 130, 300), "other wave first": (130, 300),
          "blocks only": (300, 520), "last block first": (520, 599)}


@pytest.mark.parametrize("places", sorted(PLACES))
def test_argmin_ties_go_to_the_first_index(amin, places):
    """Column 0's minimiser row copied to a later lane of the same wave (5, 40), another wave of the block (130) and other
    blocks (300, 520, 599): the earliest copy wins, whichever stage of the reduce meets the tie."""
    p = amin.p
    j0 = int(np.argmin(amin.traj(p.Xq)[:, 0]))
    Xs = p.Xq.copy()
    Xs[j0] = p.Xq[(j0 + 1) % len(Xs)]
    Xs[list(PLACES[places])] = p.Xq[j0]
    _, idx = _argmin_is_first_minimum(amin, Xs)
    assert idx[0] == min(PLACES[places])


def test_argmin_index_base_and_device_pairs(amin):
    import torch

    p = amin.p
    v0, i0 = _argmin_is_first_minimum(amin, p.Xq)
    Xd = torch.from_numpy(p.Xq).cuda()
    for base in (0, 7, 2 ** 40 + 3):
        v, i = _argmin_is_first_minimum(amin, p.Xq, base)
        np.testing.assert_array_equal(v, v0)
        np.testing.assert_array_equal(i, i0 + base)
        pairs = amin.traj.argmin_pairs(Xd, base)
        amin.eng.synchronize()
        np.testing.assert_array_equal(pairs[0].cpu().numpy(), v0)
        np.testing.assert_array_equal(pairs[1].contiguous().view(torch.int64).cpu().numpy(), i0 + base)


def test_argmin_never_picks_a_nan_row(amin):
    p = amin.p
    j = np.argmin(amin.traj(p.Xq), axis=0)
    Xs = p.Xq.copy()
    Xs[[0, int(j[0]), int(j[1]), 255, 256, 599]] = np.nan   # the first row, two columns' minimisers, block edges, the last row
    got = amin.traj(Xs)
    assert np.all(np.isnan(got[0])) and np.isfinite(got[1]).all()
    _argmin_is_first_minimum(amin, Xs)


def test_no_candidates_give_an_empty_array(amin):
    out = amin.traj(np.empty((0, amin.p.d)))
    assert out.shape == (0, amin.B)


# ---- 5. the RFF phase at its own resolution ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", T.REGIMES)
def test_rff_phase_within_its_derived_bound(regime):
    """trajectory_rff with mean_const = 0 (no canonical part) on the golden's exact inputs, theta read back and treated as
    data: the device's values against the mpmath phases inside the bound of tests/traj_cases.py, d in {1, 8} x F in {1, 24}
    (design space at F = 1, gram space at F = 24 >= N = 20), three columns."""
    from trieste_amd.engine import GPEngine

    worst = {}
    for c in T.load_goldens()["phase"]:
        if c["regime"] != regime:
            continue
        d, F = c["d"], c["F"]
        x, ls, b = np.array(c["x"]), np.array(c["ls"]), np.array(c["b"])
        W = np.array(c["W"]).reshape(F, d)
        rng = np.random.default_rng([d, F, 11])
        eng = GPEngine(d, T.KIND)
        eng.set_hyper(c["variance"], ls, NOISE, 0.0)
        eng.set_data(c["lo"] + rng.uniform(size=(20, d)), rng.standard_normal(20))
        traj = eng.trajectory_rff(W, b, rng.standard_normal((F, 3)))
        theta = traj.theta()
        assert np.all(np.isfinite(theta)) and np.abs(theta).max() > 0
        err = T.rff_errors(traj(x), c["cos"], c["scale"], theta)
        bound = T.rff_bound(x, ls, W, b, theta, c["variance"])
        worst[f"d{d}-F{F}"] = record_margin(f"rff phase {regime} d={d} F={F}", err, bound)
        traj.close()
        eng.close()
    print(f"rff phase, {regime}: worst error / bound {worst}")
    assert len(worst) == 4 and max(worst.values()) <= 1.0, f"worst error / bound per case, {regime} regime: {worst}"
