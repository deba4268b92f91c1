"""CPU: the integrated variance reduction's two restatements (tests/ivr_reference.py) against the 50-digit goldens and against
each other, the weights against scipy, the tolerance helpers the GPU tests rely on, five planted defects each rejected by
that tolerance, and the host layer (builder and function object) on an oracle-backed engine stand-in."""
import json
import os

import numpy as np
import pytest

import trieste_amd.models as M
from oracle import gp_oracle as O
from tests import ivr_reference as R
from tests.fakes import FakeEngine
from tests.util import EPS, cancellation_floor
from trieste_amd import engine as E
from trieste_amd import objectives as OBJ
from trieste_amd.acquisition import IntegratedVarianceReduction, integrated_variance_reduction
from trieste_amd.data import Dataset
from trieste_amd.space import Box

GOLDENS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ivr_goldens.json")


def load_goldens():
    with open(GOLDENS) as f:
        return json.load(f)


def state_of(case):
    return O.gpr_update(case["kind"], case["variance"], np.array(case["lengthscales"]), case["noise"], case["mean_const"],
                        np.array(case["X"]), np.array(case["Y"]))


def golden_weights(case):
    return None if case["weights"] is None else np.array([float(v) for v in case["weights"]])


# ---- goldens ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", load_goldens()["full"], ids=lambda c: c["name"])
def test_both_routes_agree_with_the_full_goldens(case):
    st, Z, Xq = state_of(case), np.array(case["Z"]), np.array(case["Xq"])[None]
    w = golden_weights(case)
    gout, gred, gc0 = float(case["out"]), float(case["reduction"]), float(case["c0"])
    cov, cross, var_old = R.oracle_moments(st, Z, Xq)
    # the float64 moments are within the posterior's cancellation floor of the exact ones: the propagated tolerance
    f = cancellation_floor(st.N, st.variance, st.noise)
    atol = R.reduction_atol(cov, cross, w, st.noise, f)[0] + R.tail_bound(cov, cross, w, st.noise)[0]
    wmean = 1.0 if w is None else float(np.mean(w))
    out_o = R.oracle_route(st, Z, Xq, w)[0]
    out_f, red_f, c0_f = R.factored_route(st, Z, Xq, w)
    assert out_f[0] == red_f[0] - c0_f
    assert abs(red_f[0] - gred) <= 1e-9 * gred + atol, (red_f[0], gred, atol)
    assert abs(c0_f - gc0) <= 1e-9 * gc0 + f * wmean
    for out in (out_o, out_f[0]):
        assert abs(out - gout) <= 1e-9 * abs(gout) + atol + f * wmean, (out, gout)
    assert abs(R.oracle_reduction(st, Z, Xq, w)[0] - gred) <= 1e-9 * gred + atol
    # the weights themselves, as the function object computes them
    if w is not None:
        mean_old, _ = O.predict(st, Z)
        np.testing.assert_allclose(R.weights_of(mean_old, var_old, case["threshold"]), w, rtol=1e-6, atol=1e-300)


@pytest.mark.parametrize("case", load_goldens()["moments"], ids=lambda c: c["name"])
def test_tail_restatement_is_inside_a_quarter_of_the_counted_bound(case):
    cov, cross, w = np.array(case["cov"]), np.array(case["cross"]), case["weights"]
    gold = np.array([float(v) for v in case["reduction"]])
    red = R.tail_restatement(cov, cross, w, case["noise"])
    bound = R.tail_bound(cov, cross, w, case["noise"])
    assert np.all(bound > 0.0) and np.all(bound <= 1e-6 * gold), (bound, gold)   # the bound is a rounding bound, not a licence
    assert np.all(np.abs(red - gold) <= 0.25 * bound), (np.abs(red - gold) / bound)


def test_the_goldens_cover_what_they_claim():
    doc = load_goldens()
    full, mom = doc["full"], doc["moments"]
    assert {len(c["X"]) for c in full} >= {2, 5, 8} and {len(c["Z"]) for c in full} >= {1, 3, 7}
    assert {len(c["Xq"]) for c in full} >= {1, 2, 3} and {c["kind"] for c in full} == {"rbf", "matern52"}
    assert min(c["noise"] for c in full) == 1e-7 and max(c["noise"] for c in full) == 1e-1
    assert {None if c["threshold"] is None else len(c["threshold"]) for c in full} == {None, 1, 2}
    assert {np.array(c["cov"]).shape[-1] for c in mom} >= {1, 2, 5, 16}
    conds = [np.linalg.cond(np.array(c["cov"])[0] + c["noise"] * np.eye(np.array(c["cov"]).shape[-1])) for c in mom]
    assert 1e6 < max(conds) <= 1.5e7
    ws = np.concatenate([np.array(c["weights"]) for c in mom if c["weights"] is not None])
    assert ws.max() == 1.0 and 0.0 < ws[ws > 0].min() <= 1e-300 and np.any(ws == 0.0)
    assert all((np.array(c["cross"]) > 0).any() and (np.array(c["cross"]) < 0).any() for c in mom)
    assert any(0.0 < float(v) < 1e-200 for c in mom for v in c["reduction"])
    assert os.path.getsize(GOLDENS) < 100 * 1024


# ---- the three prototype models ---------------------------------------------------------------------------------------------------------
PROTOTYPES = {   # name -> (objective, d, N, kernel, noise)
    "branin-50": (O.branin, 2, 50, "matern52", 1e-3),
    "hartmann6-rbf-300": (O.hartmann_6, 6, 300, "rbf", 1e-3),
    "ackley8-386-noise1e-5": (O.ackley, 8, 386, "matern52", 1e-5),
}
_STATES = {}


def prototype(name):
    if name not in _STATES:
        obj, d, N, kernel, noise = PROTOTYPES[name]
        X, Y = O.synthetic_problem(obj, d, N)
        Y = (Y - Y.mean()) / Y.std()
        st = O.gpr_update(kernel, 1.0, O.default_lengthscales(d), noise, 0.0, X, Y)
        rng = np.random.default_rng(7)
        Z = rng.uniform(size=(130, d))
        mean_old, var_old = O.predict(st, Z)
        _STATES[name] = (st, Z, mean_old, var_old)
    return _STATES[name]


def thresholds_for(mean_old):
    lo, hi = np.quantile(mean_old, [0.3, 0.7])
    return {"none": None, "one": [float(lo)], "two": [float(lo), float(hi)]}


@pytest.mark.parametrize("name", sorted(PROTOTYPES))
@pytest.mark.parametrize("q", [1, 3, 16])
def test_the_factored_form_reproduces_the_reference_route(name, q):
    st, Z, mean_old, var_old = prototype(name)
    Xq = np.random.default_rng(100 + q).uniform(size=(6, q, st.d))
    for form, th in thresholds_for(mean_old).items():
        w = R.weights_of(mean_old, var_old, th)
        out_o = R.oracle_route(st, Z, Xq, w)
        out_f, red, c0 = R.factored_route(st, Z, Xq, w)
        np.testing.assert_array_equal(out_f, red - c0)
        cov, cross, _ = R.oracle_moments(st, Z, Xq)
        # two float64 orders of the same sums: P-term sums of magnitude c0, and the tail's own rounding
        tol = 2.0 * R.gamma(len(Z) + 2) * c0 + 2.0 * R.tail_bound(cov, cross, w, st.noise)
        assert np.all(np.abs(out_o - out_f) <= tol), (form, np.abs(out_o - out_f) / tol)
        assert np.all(red >= 0.0) and np.all(red < c0)


# ---- weights ----------------------------------------------------------------------------------------------------------------------------
def test_weight_formulas_agree_with_scipy():
    from scipy.stats import norm

    rng = np.random.default_rng(3)
    mean, var = rng.normal(size=50), rng.uniform(1e-12, 2.0, size=50)
    assert R.weights_of(mean, var, None) is None
    np.testing.assert_allclose(R.weights_of(mean, var, [0.3]), norm.pdf(0.3, mean, np.sqrt(var)), rtol=1e-13, atol=1e-300)
    two = norm.cdf(0.9, mean, np.sqrt(var)) - norm.cdf(-0.2, mean, np.sqrt(var))
    np.testing.assert_allclose(R.weights_of(mean, var, [-0.2, 0.9]), two, rtol=1e-12, atol=1e-16)


# ---- tolerance helpers ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROTOTYPES))
@pytest.mark.parametrize("q", [1, 3, 16])
def test_reduction_atol_covers_moments_perturbed_by_the_floor(name, q):
    st, Z, mean_old, var_old = prototype(name)
    Xq = np.random.default_rng(200 + q).uniform(size=(4, q, st.d))
    cov, cross, _ = R.oracle_moments(st, Z, Xq)
    f = cancellation_floor(st.N, st.variance, st.noise)
    rng = np.random.default_rng(5)
    for th in thresholds_for(mean_old).values():
        w = R.weights_of(mean_old, var_old, th)
        base = R.tail_restatement(cov, cross, w, st.noise)
        atol = R.reduction_atol(cov, cross, w, st.noise, f)
        for _ in range(20):
            dc = f * rng.choice([-1.0, 1.0], size=cov.shape)
            dc = np.tril(dc) + np.swapaxes(np.tril(dc, -1), -1, -2)
            dx = f * rng.choice([-1.0, 1.0], size=cross.shape)
            moved = R.tail_restatement(cov + dc, cross + dx, w, st.noise)
            assert np.all(np.abs(moved - base) <= atol), (np.abs(moved - base) / atol).max()


# ---- planted defects --------------------------------------------------------------------------------------------------------------------
def _defect_setting(defect):
    """A model, integration points, batches and weights on which the defect moves the reduction by >= 10 tol."""
    rng = np.random.default_rng(11)
    d, N, P = 2, 12, 70   # P = 70: a last tile of 6 lanes, 128 padded
    X = rng.uniform(size=(N, d))
    Y = np.sin(4.0 * X.sum(axis=1))
    st = O.gpr_update("matern52", 1.0, np.array([0.3, 0.4]), 1e-2, 0.0, X, Y)
    Z = rng.uniform(size=(P, d))
    Xq = rng.uniform(size=(5, 2, d))
    w = rng.uniform(0.2, 1.0, size=P)
    if defect == "weights_after_sum":
        w[P // 2:] *= 1e-3
    return st, Z, Xq, w


@pytest.mark.parametrize("defect", [d for d in R.DEFECTS if d != "unclipped_c0"])
def test_the_tolerance_rejects_each_planted_defect_of_the_reduction(defect):
    st, Z, Xq, w = _defect_setting(defect)
    cov, cross, _ = R.oracle_moments(st, Z, Xq)
    f = cancellation_floor(st.N, st.variance, st.noise)
    _, good, _ = R.factored_route(st, Z, Xq, w)
    _, bad, _ = R.factored_route(st, Z, Xq, w, defect=defect)
    tol = 1e-5 * good + R.reduction_atol(cov, cross, w, st.noise, f)
    assert np.all(np.abs(R.oracle_reduction(st, Z, Xq, w) - good) <= tol)      # the sound form passes ...
    assert np.all(np.abs(bad - good) >= 10.0 * tol), (defect, np.abs(bad - good) / tol)   # ... every group of the defect fails by 10 x


def test_the_tolerance_rejects_an_unclipped_variance_in_c0():
    """var_old below the floor: with a training input among the integration points and noise far below the floor's scale the
    unclipped variance is negative or ~1e-16-small where the posterior's is 1e-12.  The tolerance on out is
    1e-5 (|ref| + c0) + atol; the defect is visible where c0 itself is of the order of the clip, i.e. ALL integration points
    are training inputs."""
    rng = np.random.default_rng(12)
    X = rng.uniform(size=(6, 2))
    st = O.gpr_update("rbf", 1.0, np.array([0.5, 0.5]), 1e-14, 0.0, X, np.cos(3.0 * X[:, 0]))
    Z, Xq = X.copy(), rng.uniform(size=(3, 1, 2))
    out, red, c0 = R.factored_route(st, Z, Xq, None)
    out_bad, _, c0_bad = R.factored_route(st, Z, Xq, None, defect="unclipped_c0")
    assert c0 >= 1e-12
    cov, cross, _ = R.oracle_moments(st, Z, Xq)
    f = cancellation_floor(st.N, st.variance, st.noise)
    tol = 1e-5 * np.abs(out) + 1e-5 * c0 + R.reduction_atol(cov, cross, None, st.noise, f)
    assert np.all(np.abs(out_bad - out) >= 10.0 * tol), (np.abs(out_bad - out) / tol, c0, c0_bad)


# ---- the host layer on an engine stand-in --------------------------------------------------------------------------------------------------
class IvrFakeEngine(FakeEngine):
    """FakeEngine with the two engine calls of the integrated variance reduction, by the oracle route."""

    installs = 0

    def set_integration_points(self, Z, weights=None):
        self._ivr_owner = None
        IvrFakeEngine.installs += 1
        self._ivr = None if Z is None or len(Z) == 0 else (np.array(Z, float), None if weights is None else np.array(weights, float))

    def ivr_values(self, Xq, with_reduction=False):
        if getattr(self, "_ivr", None) is None:
            raise RuntimeError("no integration points set: call tgp_set_integration_points first")
        Z, w = self._ivr
        Xq = np.asarray(Xq, float)
        lead, q = Xq.shape[:-2], Xq.shape[-2]
        flat = Xq.reshape(-1, q, self.d)
        out = R.oracle_route(self._st(), Z, flat, w).reshape(lead)
        if not with_reduction:
            return out
        return out, R.oracle_reduction(self._st(), Z, flat, w).reshape(lead)


@pytest.fixture()
def fake_engine(monkeypatch):
    monkeypatch.setattr(M, "GPEngine", IvrFakeEngine)


def _model(n=12, d=2, noise=1e-3, seed=0):
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, d))
    data = Dataset(x, OBJ.scaled_branin(x))
    gpr = M.build_gpr(data, Box([0.0] * d, [1.0] * d), likelihood_variance=noise)
    return M.GaussianProcessRegression(gpr), data


def test_builder_and_function_validate_their_arguments(fake_engine):
    model, data = _model()
    Z = np.random.default_rng(1).uniform(size=(9, 2))
    assert repr(IntegratedVarianceReduction(Z, [0.1, 0.2])) == "IntegratedVarianceReduction(threshold=[0.1, 0.2])"
    assert repr(IntegratedVarianceReduction(Z)) == "IntegratedVarianceReduction(threshold=None)"

    class NoFastUpdate:
        engine = model.engine

        def predict(self, x):
            return model.predict(x)

    with pytest.raises(NotImplementedError):
        IntegratedVarianceReduction(Z).prepare_acquisition_function(NoFastUpdate())

    class NoEngine:
        def conditional_predict_f(self, *a):
            raise AssertionError

    with pytest.raises(TypeError):
        IntegratedVarianceReduction(Z).prepare_acquisition_function(NoEngine())
    for bad_z in (Z[0], Z[None], np.empty((0, 2)), np.ones((4, 3))):
        with pytest.raises(ValueError):
            integrated_variance_reduction(model, bad_z)
    for bad_t in ([[0.1, 0.2]], [0.1, 0.2, 0.3], [], [0.5, 0.1], "high"):
        with pytest.raises(ValueError):
            integrated_variance_reduction(model, Z, bad_t)
    fn = IntegratedVarianceReduction(Z, 0.5).prepare_acquisition_function(model, data)
    for q in (0, E.IVR_MAX_Q + 1):
        with pytest.raises(ValueError):
            fn(np.zeros((3, q, 2)))
    with pytest.raises(ValueError):
        fn(np.zeros(2))
    assert not hasattr(fn, "value_and_gradient")   # what routes it to the random search


def test_function_values_weights_and_update(fake_engine):
    model, data = _model()
    st = model.engine._st()
    Z = np.random.default_rng(2).uniform(size=(11, 2))
    x = np.random.default_rng(3).uniform(size=(4, 5, 3, 2))
    mean_old, var_old = O.predict(st, Z)
    for th in (None, 0.4, [0.4], (0.2, 0.8)):
        builder = IntegratedVarianceReduction(Z, th)
        fn = builder.prepare_acquisition_function(model, data)
        w = R.weights_of(mean_old, var_old, None if th is None else np.atleast_1d(th))
        if th is None:
            assert fn.weights is None
        else:
            np.testing.assert_allclose(fn.weights, w, rtol=1e-12, atol=1e-300)
        val, red = fn(x), fn.reduction(x)
        assert val.shape == (4, 5, 1) and red.shape == (4, 5, 1)
        np.testing.assert_allclose(val[..., 0].reshape(-1), R.oracle_route(st, Z, x.reshape(-1, 3, 2), w), rtol=1e-12)
        assert np.all(red >= 0.0)
        assert builder.update_acquisition_function(fn, model, data) is fn


def test_function_reinstalls_its_points_after_another_function_used_the_engine(fake_engine):
    model, data = _model()
    rng = np.random.default_rng(4)
    Z1, Z2, x = rng.uniform(size=(7, 2)), rng.uniform(size=(5, 2)), rng.uniform(size=(3, 2, 2))
    f1 = integrated_variance_reduction(model, Z1)
    f2 = integrated_variance_reduction(model, Z2, [0.3])
    n0 = IvrFakeEngine.installs
    a1 = f1(x)
    assert IvrFakeEngine.installs == n0 + 1
    np.testing.assert_array_equal(f1(x), a1)
    assert IvrFakeEngine.installs == n0 + 1      # still the owner: nothing re-sent
    a2 = f2(x)
    assert IvrFakeEngine.installs == n0 + 2 and not np.array_equal(a1, a2)
    np.testing.assert_array_equal(f1(x), a1)     # f1 re-sets its own points
    assert IvrFakeEngine.installs == n0 + 3
    E.set_integration_points(model.engine, Z2)   # a direct call clears the owner mark
    np.testing.assert_array_equal(f1.reduction(x), f1.reduction(x))
    assert IvrFakeEngine.installs == n0 + 5
    # the weights are frozen at construction, the model-dependent part follows the model
    w_before = f2.weights.copy()
    model.update(Dataset(np.concatenate([data.query_points, x[0]]), np.concatenate([data.observations, OBJ.scaled_branin(x[0])])))
    np.testing.assert_array_equal(f2.weights, w_before)
    st = model.engine._st()
    np.testing.assert_allclose(f2(x)[..., 0], R.oracle_route(st, Z2, x, w_before), rtol=1e-12)
