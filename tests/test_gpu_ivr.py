"""GPU: the integrated variance reduction on the device (tgp_set_integration_points, tgp_ivr_values, tgp_ivr_moments;
trieste_amd/csrc/tgp_kernels_ivr.hip) against the 50-digit goldens, the kernel-order restatement and the oracle's route
(tests/ivr_reference.py, where both tolerances are derived): the tail across its widths, behind the posterior of every kernel
kind, across its chunk boundary, its handle state, its refusals, and the rule end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import ivr_reference as R
from tests import ivr_tour as T
from tests.util import cancellation_floor, record_margin

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = os.path.join(ROOT, "tests", "golden", "ivr_goldens.json")


def load_goldens():
    with open(GOLDENS) as f:
        return json.load(f)


def within(what, got, want, tol):
    err = np.abs(np.asarray(got) - np.asarray(want))
    worst = record_margin(what, err, tol)
    print(f"{what}: worst error / tolerance {worst:.3e}")
    assert np.all(err <= tol), f"{what}: worst error / tolerance {worst:.3e}"


def engine_of(st):
    from trieste_amd.engine import GPEngine

    eng = GPEngine(st.d, st.kind)
    eng.set_hyper(st.variance, st.lengthscales, st.noise, st.mean_const)
    eng.set_data(st.X, st.Y)
    return eng


def bare_engine():
    from trieste_amd.engine import GPEngine

    return GPEngine(2, "matern52")


# ---- goldens ---------------------------------------------------------------------------------------------------------------------------
def test_moments_entry_against_the_moments_goldens():
    from trieste_amd import engine as E

    eng = bare_engine()
    for case in load_goldens()["moments"]:
        cov, cross, w = np.array(case["cov"]), np.array(case["cross"]), case["weights"]
        gold = np.array([float(v) for v in case["reduction"]])
        got = E.ivr_moments(eng, cov, cross, w, case["noise"])
        within(f"moments golden {case['name']}", got, gold, R.tail_bound(cov, cross, w, case["noise"]))


def test_values_against_the_full_goldens():
    from trieste_amd import engine as E

    for case in load_goldens()["full"]:
        st = O.gpr_update(case["kind"], case["variance"], np.array(case["lengthscales"]), case["noise"], case["mean_const"],
                          np.array(case["X"]), np.array(case["Y"]))
        Z, Xq = np.array(case["Z"]), np.array(case["Xq"])[None]
        w = None if case["weights"] is None else np.array([float(v) for v in case["weights"]])
        gout, gred, gc0 = float(case["out"]), float(case["reduction"]), float(case["c0"])
        eng = engine_of(st)
        E.set_integration_points(eng, Z, w)
        out, red = E.ivr_values(eng, Xq, with_reduction=True)
        cov, cross, _ = R.oracle_moments(st, Z, Xq)
        atol = R.reduction_atol(cov, cross, w, st.noise, cancellation_floor(st.N, st.variance, st.noise))
        within(f"full golden {case['name']} reduction", red, [gred], 1e-5 * gred + atol)
        within(f"full golden {case['name']} out", out, [gout], 1e-5 * abs(gout) + 1e-5 * gc0 + atol)
        np.testing.assert_array_equal(E.ivr_values(eng, Xq), out)     # with and without the second output


# ---- the tail across its widths ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 2, 3, 5, 8, 16])
def test_tail_across_its_widths(q):
    """Random positive definite moments, G = 300, P on both sides of the tile width, against the kernel-order restatement inside
    the counted bound; the weights carry exact zeros, some of them in the last partial tile."""
    from trieste_amd import engine as E

    eng = bare_engine()
    rng = np.random.default_rng(40 + q)
    G = 300
    B = rng.standard_normal((G, q, q))
    cov = B @ np.swapaxes(B, -1, -2) / q + 10.0 ** rng.uniform(-6, 0, size=(G, 1, 1)) * np.eye(q)
    for P in (1, 63, 64, 65, 130, 1000):
        cross = rng.standard_normal((G, q, P)) * 10.0 ** rng.uniform(-3, 1, size=(G, 1, 1))
        w = rng.uniform(size=P)
        w[rng.uniform(size=P) < 0.2] = 0.0
        if P > 1:
            w[-1] = 0.0
        noise = 1e-3
        want = R.tail_restatement(cov, cross, w, noise)
        bound = R.tail_bound(cov, cross, w, noise)
        got = E.ivr_moments(eng, cov, cross, w, noise)
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0)
        within(f"tail q={q} P={P}", got, want, bound)
        unweighted = E.ivr_moments(eng, cov, cross, None, noise)
        within(f"tail q={q} P={P} unweighted", unweighted, R.tail_restatement(cov, cross, None, noise), R.tail_bound(cov, cross, None, noise))
    import torch

    dev = [torch.as_tensor(a, device="cuda") for a in (cov, cross, w)]
    np.testing.assert_array_equal(E.ivr_moments(eng, *dev, noise).cpu().numpy(), got)   # device residency: the same bits


# ---- behind the posterior -----------------------------------------------------------------------------------------------------------------
def _ard(d, seed):
    return O.default_lengthscales(d) * (0.6 + 0.8 * np.random.default_rng(seed).uniform(size=d))


POSTERIOR_CONFIGS = [
    # (name, objective, d, kind, N, noise, ARD): every kernel kind, d = 2 ... 16, an ARD problem at d = 40, a wide one at d = 64
    ("branin_m52_N50", O.branin, 2, "matern52", 50, 1e-3, False),
    ("hartmann_rbf_N300", O.hartmann_6, 6, "rbf", 300, 1e-2, False),
    ("ackley8_m52_N1000", O.ackley, 8, "matern52", 1000, 1e-2, False),
    ("ackley8_m52_N386_lownoise", O.ackley, 8, "matern52", 386, 1e-5, False),
    ("ackley16_m32_N257", O.ackley, 16, "matern32", 257, 1e-3, False),
    ("ackley3_m12_N130", O.ackley, 3, "matern12", 130, 1e-3, False),
    ("ackley40_m52_ard_N200", O.ackley, 40, "matern52", 200, 1e-2, True),
    ("ackley64_rbf_N1000", O.ackley, 64, "rbf", 1000, 1e-2, False),
]


@pytest.mark.parametrize("cfg", POSTERIOR_CONFIGS, ids=[c[0] for c in POSTERIOR_CONFIGS])
def test_values_behind_the_posterior_match_the_oracle_route(cfg, monkeypatch):
    """tgp_ivr_values against conditional_predict_f's arithmetic on the oracle's moments, P = 130, q = 1, 3, 16, the three
    threshold forms; tolerance 1e-5 |ref| + reduction_atol (+ 1e-5 c0 on out).  The reduction must stand above its own
    tolerance for at least half the groups, or the comparison says nothing."""
    from trieste_amd import engine as E

    _, obj, d, kind, N, noise, ard = cfg
    if kind == "matern12":   # (as tests/test_gpu_wide.py: the engine's distances are the difference form)
        monkeypatch.setattr(O, "scaled_square_dist", O.difference_form_sq_dist)
    X, Y = O.synthetic_problem(obj, d, N)
    ls = _ard(d, 17) if ard else O.default_lengthscales(d)
    c = float(np.mean(Y))
    st = O.gpr_update(kind, 1.0, ls, noise, c, X, Y)
    eng = engine_of(st)
    f = cancellation_floor(N, 1.0, noise)
    rng = np.random.default_rng(29)
    Z = rng.uniform(size=(130, d))
    mean_old, var_old = O.predict(st, Z)
    lo, hi = np.quantile(mean_old, [0.3, 0.7])
    for q in (1, 3, 16):
        G = 24
        Xq = rng.uniform(size=(G, q, d))
        Xq[0, 0] = X[3] + 1e-4 * rng.standard_normal(d) / np.sqrt(d)     # next to a training input
        if q > 1:
            Xq[1, 1] = Xq[1, 0] + 1e-3 * rng.standard_normal(d) / np.sqrt(d)   # a near-duplicate pair
        cov, cross, _ = R.oracle_moments(st, Z, Xq)
        for form, th in (("none", None), ("one", [lo]), ("two", [lo, hi])):
            w = R.weights_of(mean_old, var_old, th)
            want_out, want_red = R.route_on_moments(cov, cross, var_old, w, noise)
            c0 = R.c0_of(var_old, w)
            atol = R.reduction_atol(cov, cross, w, noise, f)
            E.set_integration_points(eng, Z, w)
            out, red = E.ivr_values(eng, Xq, with_reduction=True)
            tol = 1e-5 * want_red + atol
            within(f"{cfg[0]} q={q} {form} reduction", red, want_red, tol)
            within(f"{cfg[0]} q={q} {form} out", out, want_out, 1e-5 * np.abs(want_out) + 1e-5 * c0 + atol)
            above = np.count_nonzero(want_red > tol)
            print(f"{cfg[0]} q={q} {form}: reduction above its tolerance for {above} of {G} groups; "
                  f"median reduction / tolerance {np.median(want_red / tol):.3e}, c0 / median reduction {c0 / np.median(want_red):.3e}")
            assert above >= G // 2


# ---- chunk boundary -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 3, 16])
def test_values_across_the_chunk_boundary(q):
    """2048 // q + 3 groups: two chunks, the second partial.  The last groups agree with a call on those groups alone inside the
    tolerance (a group's bits may depend on its chunk's size: the products split k by their tile count), and with the oracle."""
    from trieste_amd import engine as E

    X, Y = O.synthetic_problem(O.branin, 2, 50)
    st = O.gpr_update("matern52", 1.0, O.default_lengthscales(2), 1e-3, float(np.mean(Y)), X, Y)
    eng = engine_of(st)
    rng = np.random.default_rng(50 + q)
    Z, w = rng.uniform(size=(130, 2)), rng.uniform(size=130)
    G = 2048 // q + 3
    Xq = rng.uniform(size=(G, q, 2))
    E.set_integration_points(eng, Z, w)
    out, red = E.ivr_values(eng, Xq, with_reduction=True)
    assert np.all(np.isfinite(out)) and np.all(red > 0.0)
    last = slice(G - 5, G)    # the second chunk's three groups and the first chunk's last two
    out_l, red_l = E.ivr_values(eng, Xq[last], with_reduction=True)
    cov, cross, var_old = R.oracle_moments(st, Z, Xq[last])
    want_out, want_red = R.route_on_moments(cov, cross, var_old, w, st.noise)
    atol = R.reduction_atol(cov, cross, w, st.noise, cancellation_floor(st.N, 1.0, st.noise))
    tol = 1e-5 * want_red + atol
    within(f"chunk boundary q={q}: whole call vs the last groups alone", red[last], red_l, tol)
    within(f"chunk boundary q={q}: whole call vs oracle", red[last], want_red, tol)
    within(f"chunk boundary q={q}: out vs oracle", out[last], want_out, 1e-5 * np.abs(want_out) + 1e-5 * R.c0_of(var_old, w) + atol)
    np.testing.assert_array_equal(out_l, E.ivr_values(eng, Xq[last]))
    import torch

    dout, dred = E.ivr_values(eng, torch.as_tensor(Xq, device="cuda"), with_reduction=True)     # device residency: the same bits
    np.testing.assert_array_equal(dout.cpu().numpy(), out)
    np.testing.assert_array_equal(dred.cpu().numpy(), red)


def test_a_breakdown_in_the_second_chunk_is_reported_with_its_global_index():
    """On given moments (the chunked body and the report are the ones tgp_ivr_values runs through): q = 16 and P = 16384 make
    chunks of 2^28 / (8 q P) = 128 groups; group 129 of 131 has a negative definite covariance and no noise to mend it."""
    from trieste_amd import engine as E
    from trieste_amd._lib import NotPositiveDefiniteError

    eng = bare_engine()
    q, P, G = 16, E.IVR_MAX_P, 131
    cov = np.tile(np.eye(q), (G, 1, 1))
    cross = np.zeros((G, q, P))
    cross[:, 0, ::1000] = 1.0
    red = E.ivr_moments(eng, cov, cross, None, 0.0)
    np.testing.assert_array_equal(red, np.full(G, len(range(0, P, 1000)) / P))
    cov[129] = -np.eye(q)
    with pytest.raises(NotPositiveDefiniteError, match=r"group 129\b"):
        E.ivr_moments(eng, cov, cross, None, 0.0)
    cov[5] = -np.eye(q)   # the first chunk's report comes first
    with pytest.raises(NotPositiveDefiniteError, match=r"group 5\b"):
        E.ivr_moments(eng, cov, cross, None, 0.0)


# ---- state ----------------------------------------------------------------------------------------------------------------------------------
def _check_tour(t):
    for name in ("small", "two-tiles", "q1"):
        np.testing.assert_array_equal(t[f"{name} again"], np.stack([t[f"{name} first value"], t[f"{name} first reduction"]]))
        np.testing.assert_array_equal(t[f"{name} appended"], t[f"{name} appended fresh"])
        np.testing.assert_array_equal(t[f"{name} refit"], t[f"{name} refit fresh"])
        # the derived arrays were rebuilt, not kept: the values moved with the model
        assert not np.array_equal(t[f"{name} appended"][1], t[f"{name} first reduction"])
        assert not np.array_equal(t[f"{name} refit"][1], t[f"{name} appended"][1])
    assert all(np.all(np.isfinite(v)) for v in t.values())


def test_values_follow_the_model_and_ignore_the_handles_history():
    _check_tour(T.tour())


def test_tour_under_poisoned_allocations():
    """TGP_POISON=1 fills every fresh device allocation of the library with NaNs: the tour in a fresh child process under it,
    and here, must agree bit for bit.  The child's timeout is a safety cap; a child that hangs or dies on a signal ends the
    session, so that nothing else is started on a GPU that has just faulted."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tour.npz")
        env = dict(os.environ, TGP_POISON="1")
        try:
            child = subprocess.run([sys.executable, "-m", "tests.ivr_tour", out], env=env, cwd=ROOT, timeout=120,
                                   capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.exit(f"the poisoned tour hung (120 s cap); stderr:\n{(e.stderr or b'')[-4000:]}", returncode=1)
        if child.returncode < 0 or child.returncode in (134, 139):
            pytest.exit(f"the poisoned tour died with {child.returncode}; stderr:\n{child.stderr[-4000:]}", returncode=1)
        assert child.returncode == 0, f"poisoned tour exited with {child.returncode}:\n{child.stderr[-4000:]}"
        with np.load(out) as z:
            poisoned = {k: z[k] for k in z.files}
    _check_tour(poisoned)
    plain = T.tour()
    assert sorted(plain) == sorted(poisoned)
    for k in plain:
        np.testing.assert_array_equal(plain[k], poisoned[k], err_msg=k)


def test_clearing_and_cloning():
    from trieste_amd import engine as E

    X, Y = O.synthetic_problem(O.branin, 2, 30)
    st = O.gpr_update("matern52", 1.0, O.default_lengthscales(2), 1e-3, 0.0, X, Y)
    eng = engine_of(st)
    rng = np.random.default_rng(3)
    Z, Xq = rng.uniform(size=(9, 2)), rng.uniform(size=(4, 2, 2))
    E.set_integration_points(eng, Z)
    a = E.ivr_values(eng, Xq)
    twin = eng.clone()
    with pytest.raises(RuntimeError, match="integration points"):     # a clone has no setting
        E.ivr_values(twin, Xq)
    E.set_integration_points(twin, Z)
    np.testing.assert_array_equal(E.ivr_values(twin, Xq), a)
    E.set_integration_points(eng, None)                                # P == 0 clears
    with pytest.raises(RuntimeError, match="integration points"):
        E.ivr_values(eng, Xq)
    E.set_integration_points(eng, np.empty((0, 2)))
    with pytest.raises(RuntimeError, match="integration points"):
        E.ivr_values(eng, Xq)
    # cloning INTO a handle that has a setting keeps the setting and rebuilds what depends on the model
    other = engine_of(O.gpr_update("matern52", 1.0, O.default_lengthscales(2), 1e-3, 0.0, X[:20], Y[:20]))
    E.set_integration_points(other, Z)
    b = E.ivr_values(other, Xq)
    other.clone_from(twin)
    np.testing.assert_array_equal(E.ivr_values(other, Xq), a)
    assert not np.array_equal(a, b)


def test_refusals():
    import ctypes as C

    from trieste_amd import _lib
    from trieste_amd import engine as E

    X, Y = O.synthetic_problem(O.branin, 2, 20)
    eng = engine_of(O.gpr_update("matern52", 1.0, O.default_lengthscales(2), 1e-3, 0.0, X, Y))
    lib = eng._lib
    rng = np.random.default_rng(4)
    Z = rng.uniform(size=(5, 2))
    p = lambda a: a.ctypes.data
    E.set_integration_points(eng, Z)
    out = np.empty(3)
    for q in (0, 17):
        Xq = np.zeros((3, max(q, 1), 2))
        assert lib.tgp_ivr_values(eng._h, p(Xq), 3, q, p(out), None, _lib.HOST) == _lib.TGP_ERR_SHAPE
        cov, cross = np.zeros((3, max(q, 1), max(q, 1))), np.zeros((3, max(q, 1), 5))
        assert lib.tgp_ivr_moments(eng._h, p(cov), p(cross), None, 3, q, 5, 0.0, p(out), _lib.HOST) == _lib.TGP_ERR_SHAPE
    with pytest.raises(ValueError):
        E.ivr_values(eng, np.zeros((3, 17, 2)))
    Xq = rng.uniform(size=(3, 2, 2))
    assert lib.tgp_ivr_values(eng._h, p(Xq), 3, 2, None, None, _lib.HOST) == _lib.TGP_ERR_ARG      # both outputs NULL
    assert lib.tgp_ivr_values(eng._h, p(Xq), 3, 2, None, p(out), _lib.HOST) == _lib.TGP_OK         # either alone is fine
    big = np.zeros((E.IVR_MAX_P + 1, 2))
    assert lib.tgp_set_integration_points(eng._h, p(big), len(big), None, _lib.HOST) == _lib.TGP_ERR_SHAPE
    assert lib.tgp_set_integration_points(eng._h, p(big), -1, None, _lib.HOST) == _lib.TGP_ERR_SHAPE
    with pytest.raises(ValueError):
        E.set_integration_points(eng, big)
    E.ivr_values(eng, Xq)                                        # a refused setting leaves the earlier one in place
    for bad in (-1e-300, np.nan, np.inf):
        w = np.ones(5)
        w[2] = bad
        with pytest.raises(ValueError, match="weights"):
            E.set_integration_points(eng, Z, w)
        import torch

        with pytest.raises(ValueError, match="weights"):
            E.set_integration_points(eng, torch.as_tensor(Z, device="cuda"), torch.as_tensor(w, device="cuda"))
    with pytest.raises(RuntimeError, match="integration points"):   # a setting refused for its weights is no setting
        E.ivr_values(eng, Xq)
    with pytest.raises(ValueError):
        E.set_integration_points(eng, np.zeros((5, 3)))
    with pytest.raises(ValueError):
        E.set_integration_points(eng, Z, np.ones(4))
    nodata = bare_engine()
    nodata.set_hyper(1.0, [0.5, 0.5], 1e-3, 0.0)
    E.set_integration_points(nodata, Z)
    with pytest.raises(RuntimeError, match="no data"):
        E.ivr_values(nodata, Xq)
    with pytest.raises(RuntimeError, match="integration points"):
        E.ivr_values(engine_of(O.gpr_update("matern52", 1.0, O.default_lengthscales(2), 1e-3, 0.0, X, Y)), Xq)
    with pytest.raises(ValueError):
        E.ivr_moments(eng, np.zeros((3, 2, 2)), np.zeros((3, 3, 5)))
    with pytest.raises(ValueError):
        E.ivr_moments(eng, np.tile(np.eye(2), (3, 1, 1)), np.zeros((3, 2, 5)), noise=-1.0)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 3])
def test_the_rule_acquires_batches_that_reduce_the_integrated_variance(q):
    """EfficientGlobalOptimization(IntegratedVarianceReduction(Z), num_query_points = q) on scaled Branin: 20 Sobol points, 500
    Sobol integration points, 3 steps at fixed hyper-parameters.  By the oracle: every acquired batch's reduction is at least
    the 90th percentile of 200 random batches', and the mean predictive variance over Z falls at every step."""
    from scipy.stats import qmc

    import trieste_amd.models as M
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import EfficientGlobalOptimization, IntegratedVarianceReduction
    from trieste_amd.data import OBJECTIVE, Dataset
    from trieste_amd.space import Box

    space = Box([0.0, 0.0], [1.0, 1.0])
    x0 = qmc.Sobol(d=2, scramble=False).random(32)[1:21]
    Z = qmc.Sobol(d=2, scramble=True, seed=5).random(512)[:500]
    data = Dataset(x0, OBJ.scaled_branin(x0))
    model = M.GaussianProcessRegression(M.build_gpr(data, space, likelihood_variance=1e-4))
    rule = EfficientGlobalOptimization(IntegratedVarianceReduction(Z), num_query_points=q)
    rng = np.random.default_rng(8)

    def oracle_state():
        g = model.model
        return O.gpr_update(g.kernel.kind, g.kernel.variance, np.broadcast_to(g.kernel.lengthscales, (2,)), g.likelihood_variance,
                            g.mean_function.c, g.data[0], g.data[1])

    previous = None
    for step in range(3):
        st = oracle_state()
        mean_var = float(np.mean(O.predict(st, Z)[1]))
        if previous is not None:
            assert mean_var < previous, (step, mean_var, previous)
        previous = mean_var
        points = np.asarray(rule.acquire(space, {OBJECTIVE: model}, {OBJECTIVE: data}))
        assert points.shape == (q, 2) and np.all((points >= 0.0) & (points <= 1.0))
        random = R.oracle_reduction(st, Z, rng.uniform(size=(200, q, 2)))
        got = R.oracle_reduction(st, Z, points[None])[0]
        print(f"q={q} step {step}: acquired reduction {got:.4e}; random batches' 90th percentile {np.quantile(random, 0.9):.4e}, "
              f"best {random.max():.4e}; mean variance over Z {mean_var:.4e}")
        assert got >= np.quantile(random, 0.9)
        data = data + Dataset(points, OBJ.scaled_branin(points))
        model.update(data)
    assert float(np.mean(O.predict(oracle_state(), Z)[1])) < previous
