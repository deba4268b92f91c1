"""A CPU restatement of the device's fast math (csrc/tgp_dev.hpp: fast_exp_nonpos, traj_exp2, fast_sqrt_pos, traj_sqrt)
with exact fused multiply-adds (rational arithmetic, one rounding), against the 32-digit references of
tests/golden/kernel_resolution_goldens.json ("scalar").  It states, reproducibly, what the header claims (<= 2 ulp) and what
a comparison at the resolution of tests/test_gpu_kernel_resolution.py (eps (8 + B s)) can and cannot see of a change to
these functions:
* the LAST printed digit of a polynomial coefficient moves the result by less than eps / 2 (one rounding step at most), and the second residual step
  of fast_sqrt_pos by one rounding step at most (one step already rounds correctly) -- below what any float64 comparison resolves;
* a coefficient wrong from its 13th digit, or a lost coupled Goldschmidt step, is far outside the bound.
The constants are copied from the header; v_rsq_f64 is stood in for by 1 / sqrt(x) (1 +- 2^-23): the instruction set guide
gives the instruction 2^29 ulp."""
import json
import math
import os
from fractions import Fraction

import pytest

EPS = 2.0 ** -52
EXP_C = [2.5110037605963777e-08, 2.763263963904103e-07, 2.755724091857897e-06, 2.4801485482328494e-05,
         0.00019841269890047113, 0.0013888888952314775, 0.008333333333319601, 0.0416666666664881, 0.1666666666666668,
         0.5000000000000019, 1.0, 1.0]
EXP2_C = [4.456675463639861e-10, 7.074194562613105e-09, 1.0178051192117847e-07, 1.3215432534254118e-06,
          1.5252733856295574e-05, 0.00015403530463727982, 0.001333355814639035, 0.009618129107587253, 0.0555041086648217,
          0.24022650695910158, 0.6931471805599453, 1.0]


def fma(a, b, c):
    return float(Fraction(a) * Fraction(b) + Fraction(c))   # int / int division rounds correctly


def fast_exp_nonpos(x, C=EXP_C):
    x = max(x, -745.5)
    n = float(round(x * 1.4426950408889634))
    r = fma(n, -6.93147180369123816490e-01, x)
    r = fma(n, -1.90821492927058770002e-10, r)
    p = C[0]
    for c in C[1:]:
        p = fma(p, r, c)
    return math.ldexp(p, int(n))


def traj_exp2(t, C=EXP2_C):
    n = float(round(t))
    f = t - n
    p = C[0]
    for c in C[1:]:
        p = fma(p, f, c)
    return math.ldexp(p, int(n))


def _rsq(x, sign):
    return (1.0 / math.sqrt(x)) * (1.0 + sign * 2.0 ** -23)


def fast_sqrt_pos(x, sign=1.0, residual_steps=2, coupled_step=True):
    y = _rsq(x, sign)
    g, h = x * y, 0.5 * y
    if coupled_step:
        r = fma(-h, g, 0.5)
        g, h = fma(g, r, g), fma(h, r, h)
    for _ in range(residual_steps):
        g = fma(fma(-g, g, x), h, g)
    return g


def traj_sqrt(x, sign=1.0):
    y = _rsq(x, sign)
    g, h = x * y, 0.5 * y
    return fma(g, fma(-h, g, 0.5), g)


@pytest.fixture(scope="module")
def ref():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_resolution_goldens.json")
    with open(path) as f:
        return json.load(f)["scalar"]


def _ulps(got, hilo):
    want = Fraction(hilo[0]) + Fraction(hilo[1])
    return float(abs(Fraction(got) - want) / want) / EPS


def _last_digit(c):
    """c with the last digit of its shortest decimal form raised by one."""
    mant, _, exp = repr(c).partition("e")
    digits = len(mant.split(".")[1]) if "." in mant else 0
    return float(f"{mant}e{exp or 0}") + float(f"1e{int(exp or 0) - digits}")


def test_restated_functions_hold_the_claimed_two_ulp(ref):
    """fast_exp_nonpos, traj_exp2 and fast_sqrt_pos within the 2 ulp the header claims (measured 0.49, 0.47, 0.43 eps).
    traj_sqrt's one coupled Goldschmidt step turns a seed error e into 3/2 e^2: 1.5 * 2^-46 = 96 eps at the documented
    e = 2^-23, plus the roundings of x * y and of the two fused multiply-adds (1/2 eps each at most): 97.5 eps is its bound.
    (On an MI355X the trajectory's Matern values sit 8 eps s from mpmath at s = 680, i.e. a seed near 2^-25 there;
    tests/test_gpu_kernel_resolution.py.)"""
    worst = dict(
        exp=max(_ulps(fast_exp_nonpos(x), r) for x, r in zip(ref["x"], ref["exp"])),
        exp2=max(_ulps(traj_exp2(x), r) for x, r in zip(ref["x"], ref["exp2"])),
        sqrt=max(_ulps(fast_sqrt_pos(y, s), r) for y, r in zip(ref["y"], ref["sqrt"]) for s in (-1.0, 1.0)),
        traj_sqrt=max(_ulps(traj_sqrt(y, s), r) for y, r in zip(ref["y"], ref["sqrt"]) for s in (-1.0, 1.0)))
    print("worst error in eps:", worst)
    assert max(worst["exp"], worst["exp2"], worst["sqrt"]) <= 2.0 and worst["traj_sqrt"] <= 97.5, worst


def test_what_a_comparison_at_eight_eps_can_and_cannot_see(ref):
    xs = ref["x"][::4]
    for name, fn, C in (("fast_exp_nonpos", fast_exp_nonpos, EXP_C), ("traj_exp2", traj_exp2, EXP2_C)):
        for i in range(len(C) - 2):             # the trailing 1.0s are exact
            Cm = list(C)
            Cm[i] = _last_digit(C[i])
            moved = max(abs(fn(x, Cm) - fn(x, C)) / fn(x, C) for x in xs) / EPS
            assert moved <= 1.0, (name, i, moved)                      # at most one rounding step of the result ...
            true = abs(Cm[i] - C[i]) * 0.5 ** (len(C) - 1 - i) / 0.7      # |r|, |f| <= 1/2, the polynomial >= 0.7
            assert true / EPS < 0.5, (name, i, true / EPS)             # ... from a change below half an eps
        Cm = list(C)
        Cm[-3] = C[-3] * (1.0 + 1e-12)          # wrong from the 13th digit
        key = "exp" if fn is fast_exp_nonpos else "exp2"
        assert max(_ulps(fn(x, Cm), r) for x, r in zip(ref["x"], ref[key])) > 16.0, name
    ys = ref["y"][::4]
    moved = max(abs(fast_sqrt_pos(y, s, 1) - fast_sqrt_pos(y, s, 2)) / fast_sqrt_pos(y, s, 2) for y in ys for s in (-1.0, 1.0))
    assert moved / EPS <= 1.0
    worst_one_step = max(_ulps(fast_sqrt_pos(y, s, 1), r) for y, r in zip(ref["y"], ref["sqrt"]) for s in (-1.0, 1.0))
    assert worst_one_step <= 0.55, worst_one_step                       # one residual step already rounds correctly
    lost = max(_ulps(fast_sqrt_pos(y, s, 0, coupled_step=False), r) for y, r in zip(ref["y"], ref["sqrt"]) for s in (-1.0, 1.0))
    assert lost > 1e6, lost
