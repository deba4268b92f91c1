"""CPU: the arithmetic of the gradient of the expected hypervolume improvement with respect to the moments, re-derived.  The
numpy restatement (tests/ehvi_grad_reference.py) against 50-digit goldens on the cases of the value's goldens; against central
differences of the value's restatement; the single cell as the product rule over expected improvements; and the host layer
that routes the differentiable function to the continuous optimizer."""
import json
import os

import numpy as np
import pytest
from scipy.stats import norm

from tests import ehvi_grad_reference as G
from tests import ehvi_reference as R
from tests.test_ehvi_reference import front_2d, front_3d, load_cases
from trieste_amd.acquisition.multi_objective import prepare_default_non_dominated_partition_bounds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ehvi_grad_goldens.json")

# The numpy restatement's own worst error against the goldens, as a fraction of the case's scale (scale_m for d / d mean,
# scale_v for d / d var: the same sums with the signs of their terms removed), over the cases that are not flagged ``tail``:
# measured by the first test below on this fixture: 3.41e-15 (d / d var of "P=4, narrow marginals"; d / d mean is at most
# 6.6e-16 on those 29 cases).  In the tail the plain restatement loses z^2 ulp: 6.24e-14 at 36 sigma, which the kernel's
# corrected pdf and cdf avoid.  tests/test_gpu_ehvi_grad.py gives the kernel 100 x this figure, tails included.
GRAD_RESTATEMENT_WORST = 3.41e-15


def load_grad_cases():
    """The value's cases (moments, cells) with ``gmean``, ``gvar``, ``scale_m``, ``scale_v`` [P] from the gradient goldens."""
    with open(GOLDEN) as f:
        grads = json.load(f)["cases"]
    cases = load_cases()
    assert len(grads) == len(cases) == 39
    for c, g in zip(cases, grads):
        assert c["note"] == g["note"] and c["tail"] == g["tail"]
        for k in ("gmean", "gvar", "scale_m", "scale_v"):
            c[k] = np.array([float(v) for v in g[k]], dtype=np.float64)
            assert c[k].shape == c["mean"].shape
    return cases


def grad_errors(c, gmean, gvar):
    """The errors of (gmean, gvar) [P] against case c's goldens as fractions of its scales; a zero scale demands an exactly
    zero result (inf otherwise)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        em = np.where(c["scale_m"] > 0, np.abs(gmean - c["gmean"]) / c["scale_m"], np.where(gmean == 0.0, 0.0, np.inf))
        ev = np.where(c["scale_v"] > 0, np.abs(gvar - c["gvar"]) / c["scale_v"], np.where(gvar == 0.0, 0.0, np.inf))
    return em, ev


def _args(c):
    return c["mean"][None], c["var"][None], c["lb"], c["ub"]


def test_restatement_matches_the_mpmath_goldens():
    cases = load_grad_cases()
    assert sum(c["tail"] for c in cases) == 10
    zero_scale = [c["note"] for c in cases if np.any(c["scale_v"] == 0.0)]
    assert zero_scale == ["P=2, var 1e-12, inside"]   # pdf has flushed at every bound: exactly zero, scale and derivative
    worst, worst_tail = (0.0, ""), (0.0, "")
    for n, c in enumerate(cases):
        assert np.all(c["scale_m"] > 0.0) and np.all(np.abs(c["gmean"]) <= c["scale_m"]) and np.all(np.abs(c["gvar"]) <= c["scale_v"])
        assert np.all(c["gmean"] < 0.0)   # a larger mean (minimisation) never improves the hypervolume
        gm, gv = G.g_difference_grad(*_args(c))
        sm, sv = G.grad_scales(*_args(c))
        assert np.all(np.abs(sm[0] - c["scale_m"]) <= 1e-12 * c["scale_m"]), (n, c["note"])
        assert np.all(np.abs(sv[0] - c["scale_v"]) <= 1e-12 * c["scale_v"]), (n, c["note"])
        em, ev = grad_errors(c, gm[0], gv[0])
        e = max(em.max(), ev.max())
        print(f"case {n:2d} {c['note']:50s} tail={c['tail']!s:5s} d/dmean {em.max():.2e} d/dvar {ev.max():.2e} of the scales")
        if c["tail"]:
            worst_tail = max(worst_tail, (e, c["note"]))
        else:
            worst = max(worst, (e, c["note"]))
    print(f"numpy restatement vs mpmath: worst {worst[0]:.3e} of the scales ({worst[1]}); in the tail {worst_tail[0]:.3e} "
          f"({worst_tail[1]})")
    assert worst[0] <= 2.0 * GRAD_RESTATEMENT_WORST
    assert worst_tail[0] <= 1e-13   # (z^2 ulp at 36 sigma: 6.2e-14)


def test_restatement_agrees_with_central_differences_of_the_value():
    """d / d mean and d / d var of ``ehvi_reference.g_difference_form`` by central differences at two step sizes on random
    moments (means in [0, 1], standard deviations 0.1 .. 1): the tolerance is twice the difference between the two
    estimates (their truncation error falls by four from one to the other) plus the value's rounding over the step."""
    rng = np.random.default_rng(11)
    for front, ref in (front_2d(), front_3d()):
        lb, ub = prepare_default_non_dominated_partition_bounds(ref, front)
        P = front.shape[1]
        mean, var = rng.uniform(0.0, 1.0, (40, P)), rng.uniform(0.1, 1.0, (40, P)) ** 2
        gm, gv = G.g_difference_grad(mean, var, lb, ub)
        noise = 8 * np.finfo(float).eps * R.scale(mean, var, lb, ub)
        for which, got in ((0, gm), (1, gv)):
            for j in range(P):
                est = []
                for h in (2e-4, 1e-4):
                    step = np.zeros(P)
                    step[j] = h
                    if which == 0:
                        est.append((R.g_difference_form(mean + step, var, lb, ub) - R.g_difference_form(mean - step, var, lb, ub)) / (2 * h))
                    else:
                        hv = h * var[:, j]
                        up, dn = var.copy(), var.copy()
                        up[:, j] += hv
                        dn[:, j] -= hv
                        est.append((R.g_difference_form(mean, up, lb, ub) - R.g_difference_form(mean, dn, lb, ub)) / (2 * hv))
                        noise_j = noise / (1e-4 * var[:, j])
                tol = 2.0 * np.abs(est[0] - est[1]) + (noise / 1e-4 if which == 0 else noise_j)
                assert np.all(np.abs(got[:, j] - est[1]) <= tol), (P, which, j, np.max(np.abs(got[:, j] - est[1]) / tol))
                assert np.median(np.abs(est[1])) > 100 * np.median(tol)   # the differences say something


def test_single_cell_gradient_is_the_product_rule_over_expected_improvements():
    """With the one cell [-1e10, reference] EHVI = prod_j EI_j, EI_j = (r - m) cdf(z) + s pdf(z): d EI / d m = -cdf(z),
    d EI / d v = pdf(z) / (2 s)."""
    rng = np.random.default_rng(12)
    for P in (2, 3, 4):
        ref = rng.uniform(0.5, 1.5, P)
        lb, ub = prepare_default_non_dominated_partition_bounds(ref, None)
        mean, var = rng.uniform(0.0, 2.0, (50, P)), 10.0 ** rng.uniform(-4, 0, (50, P))
        sd = np.sqrt(var)
        z = (ref - mean) / sd
        ei = (ref - mean) * norm.cdf(z) + sd * norm.pdf(z)
        gm, gv = G.g_difference_grad(mean, var, lb, ub)
        for j in range(P):
            others = np.prod(np.delete(ei, j, axis=1), axis=1)
            np.testing.assert_allclose(gm[:, j], -others * norm.cdf(z[:, j]), rtol=1e-13, atol=0)
            np.testing.assert_allclose(gv[:, j], others * norm.pdf(z[:, j]) / (2 * sd[:, j]), rtol=1e-13, atol=0)


def test_a_clipped_factor_contributes_no_derivative():
    """A cell whose upper bound lies below its lower bound in one objective has a factor the max clips to zero: that
    objective's derivative of the cell is zero (the function as computed), and the others' vanish with the product."""
    mean, var = np.array([[0.3, 0.4]]), np.array([[0.04, 0.09]])
    lb, ub = np.array([[0.5, -1e10], [-1e10, 0.2]]), np.array([[0.2, 1.0], [0.5, 0.9]])   # cell 0 is inverted in objective 0
    gm, gv = G.g_difference_grad(mean, var, lb, ub)
    gm1, gv1 = G.g_difference_grad(mean, var, lb[1:], ub[1:])
    assert np.array_equal(gm, gm1) and np.array_equal(gv, gv1)


def test_tile_width_rule():
    from trieste_amd.engine import ehvi_grad_tile_width

    for P in (2, 3, 4):
        for V in range(1, 513):
            C = ehvi_grad_tile_width(P, V)
            assert C in (1, 2, 4, 8) and 24 * P * V * C <= 160 * 1024 and (C == 8 or 24 * P * V * 2 * C > 160 * 1024)
    assert ehvi_grad_tile_width(4, 512) == 2 and ehvi_grad_tile_width(2, 2) == 8


def test_builder_builds_the_differentiable_function_and_the_selector_routes_it():
    """``ExpectedHypervolumeImprovement(differentiable=True)`` builds the subclass with ``value_and_gradient`` (the default
    stays value-only), ``update_acquisition_function`` accepts both, and ``value_and_gradient`` installs the partition
    like ``__call__``, chunks at 2048 points and refuses anything but [R, D]."""
    import trieste_amd.acquisition.multi_objective.ehvi as ehvi_mod
    from trieste_amd.acquisition import (ExpectedHypervolumeImprovement, differentiable_expected_hv_improvement,
                                         expected_hv_improvement)
    from trieste_amd.acquisition.multi_objective import differentiable_expected_hv_improvement as exported

    assert exported is differentiable_expected_hv_improvement
    assert not hasattr(expected_hv_improvement, "value_and_gradient")
    assert "differentiable=True" in repr(ExpectedHypervolumeImprovement(differentiable=True))
    assert "differentiable" not in repr(ExpectedHypervolumeImprovement())
    assert repr(ExpectedHypervolumeImprovement([1.0, 2.0], differentiable=True)).endswith(", differentiable=True)")

    class Engine:
        device, d = 0, 3

    class Member:
        def __init__(self):
            self._engine = Engine()

    class Stack:
        _models = [Member(), Member()]

        def predict(self, x):
            x = np.asarray(x)
            return np.stack([x[:, 0], 1.0 - x[:, 0]], axis=1), np.ones((len(x), 2))

    calls = []

    def fake_value_grad(engines, Xq):
        calls.append((len(engines), Xq.shape))
        return Xq.sum(axis=1), 2.0 * Xq

    installed = []
    saved = ehvi_mod._require_engine, ehvi_mod._engine_mod.ehvi_value_grad, ehvi_mod._engine_mod.ehvi_set_partition_tables
    ehvi_mod._require_engine = lambda m, who: m._engine
    ehvi_mod._engine_mod.ehvi_value_grad = fake_value_grad
    ehvi_mod._engine_mod.ehvi_set_partition_tables = lambda e, *t: installed.append(e)
    try:
        from trieste_amd.data import Dataset

        data = Dataset(np.array([[0.2, 0.0, 0.0], [0.7, 0.0, 0.0]]), np.array([[0.2, 0.8], [0.7, 0.3]]))
        stack = Stack()
        plain = ExpectedHypervolumeImprovement([1.1, 1.1]).prepare_acquisition_function(stack, data)
        assert type(plain) is expected_hv_improvement
        builder = ExpectedHypervolumeImprovement([1.1, 1.1], differentiable=True)
        fn = builder.prepare_acquisition_function(stack, data)
        assert type(fn) is differentiable_expected_hv_improvement and isinstance(fn, expected_hv_improvement)
        assert builder.update_acquisition_function(fn, stack, data) is fn
        assert ExpectedHypervolumeImprovement([1.1, 1.1]).update_acquisition_function(fn, stack, data) is fn
        with pytest.raises(ValueError):
            builder.update_acquisition_function(lambda x: x, stack, data)
        x = np.random.default_rng(0).uniform(size=(2048 + 5, 3))
        v, g = fn.value_and_gradient(x)
        assert calls == [(2, (2048, 3)), (2, (5, 3))] and len(installed) == 1
        assert np.array_equal(v, x.sum(axis=1)) and np.array_equal(g, 2.0 * x)
        with pytest.raises(ValueError, match=r"\[R, D\]"):
            fn.value_and_gradient(np.zeros((4, 2, 3)))
    finally:
        ehvi_mod._require_engine, ehvi_mod._engine_mod.ehvi_value_grad, ehvi_mod._engine_mod.ehvi_set_partition_tables = saved
