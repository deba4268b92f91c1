"""The difference-form oracle (oracle/gp_oracle.py ``difference_form``): the reference the GPU tests of general models
(tests/test_gpu_general.py) compare against, pinned on the CPU.

The default oracle follows gpflow and forms r^2 = |a|^2 + |b|^2 - 2 a.b of the scaled inputs.  Its rounding error is about
eps (|a|^2 + |b|^2), so on inputs far from the origin it is not a reference at all.  The difference form errs relative to
r^2 itself.  These tests show that it agrees with the 50-digit goldens, that it does not care where the inputs sit, that the
default form does, and that both commute exactly with power-of-two scaling of inputs and lengthscales."""
import contextlib

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import test_oracle_golden as G
from tests.util import assert_close, cancellation_floor

SHIFT = 1024.0  # X in [0, 1]^d -> X + t in [t, 2t]: (X + t) - t is exact


@pytest.mark.parametrize("c", G.CASES, ids=[c["name"] for c in G.CASES])
def test_difference_form_matches_mpmath(c):
    """(a) The goldens' own checks, unchanged tolerances, with every K and K* in the difference form."""
    with O.difference_form():
        G.test_oracle_matches_mpmath(c)
        G.test_oracle_greedy_batch_pieces_match_mpmath(c)
        G.test_oracle_entropy_tails_match_mpmath(c)
        if c["noise"] >= 1e-3:
            G.test_oracle_ei_and_qei_end_to_end(c)
    assert O.scaled_square_dist is not O.difference_form_sq_dist  # the default is back after the block


def test_difference_form_context_restores_default_on_error():
    with pytest.raises(RuntimeError):
        with O.difference_form():
            assert O.kernel_matrix("rbf", 1.0, 1.0, np.zeros((1, 1)), np.ones((1, 1)))[0, 0] == np.exp(-0.5)
            raise RuntimeError
    X = np.random.default_rng(0).uniform(size=(5, 3))
    np.testing.assert_array_equal(O.kernel_matrix("rbf", 1.0, 0.3, X), O.kernel_from_r2(
        "rbf", 1.0, O.scaled_square_dist(X, X, np.full(3, 0.3))))


def _general_problem(kind="matern52", d=4, N=60, seed=11):
    """ARD lengthscales over a decade in shuffled order, variance 2.5, noise scaled with it, Y = a f + b with mean 37.5;
    inputs on the unit cube (the test shifts them)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N, d))
    f = O.ackley(X)
    Y = 3.0 * (f - f.mean()) / f.std() + 37.5
    ls = rng.permutation(np.geomspace(0.15, 1.5, d))
    variance, noise = 2.5, 2.5e-3
    Xq = rng.uniform(size=(40, d))
    Xq[:4] = X[:4]
    Xq[4:8] = X[4:8] + 1e-6
    Xg = rng.uniform(size=(3, 5, d))
    return kind, variance, ls, noise, float(np.mean(Y)), X, Y, Xq, Xg


def _outputs(kind, variance, ls, noise, c, X, Y, Xq, Xg):
    st = O.gpr_update(kind, variance, ls, noise, c, X, Y)
    mean, var = O.predict(st, Xq)
    jm, jc = O.predict_joint(st, Xg)
    eta = O.eta_min_mean(st)
    ei = O.expected_improvement(mean, var, eta)
    nl, ng = O.nlml_and_grad(st)
    av, ag = O.acq_value_and_grad(st, "ei", eta, Xq)
    return dict(mean=mean, var=var, joint_mean=jm, joint_cov=jc, eta=eta, ei=ei, nlml=nl, nlml_grad=ng, acq=av,
                acq_grad=ag)


_MEAN_LIKE = ("mean", "joint_mean", "eta")  # the parity tests' convention: ten floors on quantities of the size of Y


def _shift_errors(kind, form):
    """Worst error / (1e-10 relative + cancellation floor) per output: `form` on the shifted inputs against the
    difference-form oracle on the exact centred copies."""
    kind, variance, ls, noise, c, X, Y, Xq, Xg = _general_problem(kind)
    floor = cancellation_floor(X.shape[0], variance, noise)
    Xt, Xqt, Xgt = X + SHIFT, Xq + SHIFT, Xg + SHIFT
    X, Xq, Xg = Xt - SHIFT, Xqt - SHIFT, Xgt - SHIFT   # the exact centred copies (the shifted points' own values)
    assert np.array_equal(X + SHIFT, Xt) and np.array_equal(Xq + SHIFT, Xqt)
    with O.difference_form():
        want = _outputs(kind, variance, ls, noise, c, X, Y, Xq, Xg)
    with form():
        got = _outputs(kind, variance, ls, noise, c, Xt, Y, Xqt, Xgt)
    gmax = float(np.max(np.abs(want["nlml_grad"])))
    ratios = {}
    for k in want:
        atol = floor * (10 if k in _MEAN_LIKE else 1)
        if k == "nlml_grad":
            atol = 1e-10 * gmax
        elif k == "acq_grad":
            atol = floor * 10 / float(np.min(ls))
        err = np.abs(np.asarray(got[k]) - np.asarray(want[k]))
        ratios[k] = (err, 1e-10 * np.abs(np.asarray(want[k])) + atol)
    return ratios


@pytest.mark.parametrize("kind", ["rbf", "matern12", "matern32", "matern52"])
def test_difference_form_does_not_see_a_shift(kind):
    """(b) t = 1024: predict, the joint covariance, EI, NLML and its gradient and the acquisition gradient on the shifted
    inputs equal the centred problem's to 1e-10 relative plus the cancellation floor."""
    for k, (err, tol) in _shift_errors(kind, O.difference_form).items():
        assert_close(err, np.zeros_like(err), rtol=0.0, atol=tol, what=f"shifted {k}")


def test_dot_product_form_does_see_a_shift():
    """(c) Why the reference had to change: the default (dot-product) oracle on the same shifted problem (N = 60, d = 4,
    Matern-5/2) misses the centred answer by far more than the tolerance above.  Measured worst error / tolerance: mean 37,
    variance 29, joint covariance 23, EI 14, NLML 86, NLML gradient 339, acquisition gradient 18 (its K* is in the
    difference form, the factor is not).  The error grows with (offset / lengthscale)^2 and with N / noise."""
    ratios = {k: float(np.max(err / tol)) for k, (err, tol) in _shift_errors("matern52", contextlib.nullcontext).items()}
    print("dot-product oracle on shifted inputs, worst error / tolerance:", {k: f"{v:.3g}" for k, v in ratios.items()})
    for k in ("mean", "var", "joint_cov", "ei", "nlml", "nlml_grad", "acq_grad"):
        assert ratios[k] > 10.0, (k, ratios[k])


@pytest.mark.parametrize("form", [contextlib.nullcontext, O.difference_form], ids=["dot", "difference"])
@pytest.mark.parametrize("k", [-3, 5])
def test_power_of_two_scaling_is_exact(form, k):
    """(d) X, Xq and the lengthscales times 2^k leave x / ls bit-identical: predict, EI and the NLML are bit-identical, the
    derivatives w.r.t. x and the lengthscales are exactly 2^-k times the unscaled ones, the others identical."""
    kind, variance, ls, noise, c, X, Y, Xq, Xg = _general_problem("matern52")
    s = 2.0 ** k
    with form():
        a = _outputs(kind, variance, ls, noise, c, X, Y, Xq, Xg)
        b = _outputs(kind, variance, ls * s, noise, c, X * s, Y, Xq * s, Xg * s)
    for key in ("mean", "var", "joint_mean", "joint_cov", "eta", "ei", "nlml", "acq"):
        np.testing.assert_array_equal(b[key], a[key], err_msg=key)
    d = X.shape[1]
    np.testing.assert_array_equal(b["acq_grad"], a["acq_grad"] / s)
    np.testing.assert_array_equal(b["nlml_grad"][:d], a["nlml_grad"][:d] / s)
    np.testing.assert_array_equal(b["nlml_grad"][d:], a["nlml_grad"][d:])
