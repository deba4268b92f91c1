"""CPU checks of tests/traj_cases.py: the restatement of traj_cos_halfturns against mpmath, and the bound on the RFF phase --
that a float64 evaluation can meet it, that the faithful restatement of the kernel meets it, and that a restatement with
one defect leaves it (tests/golden/traj_phase_goldens.json; no GPU)."""
import types
from fractions import Fraction

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import traj_cases as T


@pytest.fixture(scope="module")
def gold():
    return T.load_goldens()


def _ident(c):
    return f"{c['regime']}-d{c['d']}-F{c['F']}"


def _arrays(c):
    return np.array(c["x"]), np.array(c["ls"]), np.array(c["W"]).reshape(c["F"], c["d"]), np.array(c["b"])


def _theta(c, B=3):
    rng = np.random.default_rng([c["d"], c["F"], 7])
    return rng.standard_normal((c["F"], B)) * np.array([1.0, 1e-3, 40.0])[:B]


def _ratio(c, values, theta):
    x, ls, W, b = _arrays(c)
    err = T.rff_errors(values, c["cos"], c["scale"], theta)
    return float(np.max(err / T.rff_bound(x, ls, W, b, theta, c["variance"])))


def test_halfturn_cosine_restated_is_within_two_eps_of_mpmath(gold):
    """f P(f^2) with exact fused multiply-adds on [-1/2, 1/2], +-50 half turns, y = k, y = k + 1/2 (the ties of rint) and
    their neighbours, tiny y: absolute error at most POLY_ABS_ERR = 2 * 2^-52, the figure tests/traj_cases.py puts into the
    bound (worst over these 428 points: 0.83 * 2^-52, next to f = 1/2; 1.05 * 2^-52 over 3620 points of the same design)."""
    h = gold["halfturn"]
    worst, at = 0.0, None
    for y, (hi, lo) in zip(h["y"], h["sinpi"]):
        err = float(abs(Fraction(T.halfturn_cos(y)) - (Fraction(hi) + Fraction(lo))))
        if err > worst:
            worst, at = err, y
    assert worst <= T.POLY_ABS_ERR, (worst / 2.0 ** -52, at)
    assert worst >= 0.25 * 2.0 ** -52, "the polynomial cannot be more exact than its last rounding"
    # the edges themselves: whole half turns are exact zeros, quarter turns +-1 to the last place
    for k in range(-50, 51):
        assert T.halfturn_cos(float(k)) == 0.0
        assert abs(T.halfturn_cos(k + 0.5) - (-1.0) ** k) <= 2.0 ** -52
    assert T.halfturn_cos(1e-300) == pytest.approx(np.pi * 1e-300, rel=1e-15)


def test_every_regime_is_the_one_it_claims(gold):
    far = 0.0
    for c in gold["phase"]:
        x, ls, W, b = _arrays(c)
        arg = np.abs((x / ls) @ W.T + b)
        if c["regime"] == "small":
            assert arg.max() < 1.0
        elif c["regime"] == "far":
            assert c["lo"] == 1024.0 and np.all(ls == 0.05) and np.median(arg) > 5e3
            far = max(far, arg.max())
        else:
            assert c["lo"] == 0.0 and np.allclose(ls, O.default_lengthscales(c["d"]))
    assert far > 1e5
    assert len(gold["phase"]) == len(T.REGIMES) * len(T.DIMS) * len(T.FEATURES)


def test_float64_oracle_lies_inside_the_bound(gold):
    """The bound is not tighter than a plain float64 evaluation (numpy's cos of the phase in radians) can meet."""
    for c in gold["phase"]:
        x, ls, W, b = _arrays(c)
        theta = _theta(c)
        st = types.SimpleNamespace(variance=c["variance"], lengthscales=ls, mean_const=0.0)
        r = _ratio(c, O.rff_trajectory_eval(st, W, b, theta, x), theta)
        assert r <= 1.0, (_ident(c), r)


def test_restated_kernel_lies_inside_the_bound(gold):
    for c in gold["phase"]:
        x, ls, W, b = _arrays(c)
        theta = _theta(c)
        r = _ratio(c, T.rff_restated(x, ls, W, b, theta, c["variance"]), theta)
        assert r <= 1.0, (_ident(c), r)


def _off(index, rel=1e-12):
    co = list(T.COEFFS)
    co[index] *= 1.0 + rel
    return tuple(co)


DEFECTS = {
    "leading coefficient off by 1e-12": dict(coeffs=_off(8)),
    "parity of n ignored": dict(parity=False),
    "b / pi without the half turn": dict(half=0.0),
}


@pytest.mark.parametrize("defect", sorted(DEFECTS))
def test_one_defect_leaves_the_bound(gold, defect):
    """Teeth: in the typical regime (where the bound is what an ordinary call is held to) each planted defect is outside it,
    at every d and F of the cases.  (The parity of n can only be seen where some phase has an odd n: one feature over 4
    points may have none, so that defect is asked of the cases that have one -- at least three of the four, both F = 24.)"""
    asked = []
    for c in gold["phase"]:
        if c["regime"] != "typical":
            continue
        x, ls, W, b = _arrays(c)
        if "parity" in DEFECTS[defect]:
            n = np.rint((x / ls) @ (W * T.INV_PI).T + (b * T.INV_PI + 0.5))
            if not np.any(n % 2 == 1):
                continue
        asked.append(_ident(c))
        theta = _theta(c)
        r = _ratio(c, T.rff_restated(x, ls, W, b, theta, c["variance"], **DEFECTS[defect]), theta)
        assert r > 1.0, (_ident(c), defect, r)
    assert len(asked) >= 3 and {"typical-d1-F24", "typical-d8-F24"} <= set(asked), asked


def test_second_coefficient_off_is_seen_where_one_feature_stands_alone(gold):
    """The z^1 coefficient moves the value by |f|^3 5.2e-12 at most: visible against the bound of a single feature (F = 1)."""
    for c in gold["phase"]:
        if c["regime"] != "typical" or c["F"] != 1:
            continue
        x, ls, W, b = _arrays(c)
        theta = _theta(c)
        r = _ratio(c, T.rff_restated(x, ls, W, b, theta, c["variance"], coeffs=_off(7)), theta)
        assert r > 1.0, (_ident(c), r)
