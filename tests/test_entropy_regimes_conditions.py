"""What tests/test_gpu_entropy_regimes.py stands on, checked without a GPU: the float64 reference of tests/entropy_regimes.py
against 50-digit values, the regime cells and the sensitivity condition on the oracle's moments, and a numpy restatement of the
device's tail (csrc/tgp_dev.hpp: mills_cf, log_normal_cdf, entropy_tail) -- operation for operation, but with a * b + c for
the fused multiply-adds of mills_cf (one more rounding in sums of positive terms) -- which passes the comparison the GPU
suite makes, and fails it in the regime of each of the four defects of the reference's float64 formulas once that defect is
put back:
  (a) log(Phi(-gamma)) as the logarithm of 1 - 1e-15                    gamma in [-8, -6.5]
  (b) GIBBON's 1 + rho^2 h (gamma - h) rounds to 1                       gamma < -8
  (c) log Phi by the order-3 asymptotic series (tfp's log_ndtr)          gamma > 20
  (d) -gamma h / 2 - log Phi(-gamma) as a difference of two gamma^2 / 2  gamma > 1e3
"""
import json
import math
import os

import numpy as np
import pytest
from scipy.special import erfc

from tests import acq_regimes as R
from tests import entropy_regimes as E

KEYS = ("mes", "dmes", "gib", "dgib", "dgib_drho2")
C = 0.9189385332046727
U0 = 6.0


@pytest.fixture(scope="module")
def goldens():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entropy_tail_goldens.json")
    with open(path) as f:
        cases = json.load(f)["cases"]
    return {k: np.array([c[k] for c in cases]) for k in ("gamma", "rho2") + KEYS}


def test_goldens_cover_the_grid(goldens):
    from tests.make_entropy_tail_goldens import GAMMAS, RHO2S

    assert goldens["gamma"].size == len(GAMMAS) * len(RHO2S) == 128
    assert sorted(set(goldens["gamma"])) == sorted(GAMMAS) and sorted(set(goldens["rho2"])) == sorted(RHO2S)
    assert all(np.all(goldens[k] > 0.0) for k in KEYS)


def test_reference_matches_the_goldens_to_1e7(goldens):
    """Required: 1e-7 relative (1 % of the comparison's 1e-5) for the five functions on gamma in [-37.5, 4e7] x rho^2 up to
    1 - 1e-10.  Measured worst cases: mes 4.3e-16, dmes 1.1e-14, gib 1.0e-14, dgib 2.6e-13, dgib_drho2 3.0e-14 (the last four
    at gamma = 3, where erfcx feeds delta = h - gamma).  The goldens are functions of the double rho^2 in the file: against the
    functions of the real number 1 - 1e-10 the same reference is 6.6e-8 off at gamma >= 1e5, which is the rounding of rho^2
    (5.5e-17 of 1 - rho^2 = 1e-10), not of the reference."""
    t = E.sample_terms(goldens["gamma"], goldens["rho2"])
    worst = {k: float(np.max(np.abs(t[k] - goldens[k]) / goldens[k])) for k in KEYS}
    print("worst relative error of the reference:", worst)
    assert max(worst.values()) <= 1e-7, worst


# ---- the device's tail, restated --------------------------------------------------------------------------------------
def normal_cdf(z):
    return 0.5 * erfc(-z * 0.7071067811865476)


def normal_pdf(z):
    return 0.3989422804014327 * np.exp(-0.5 * z * z)


def mills_cf(u):
    x = 1.0 / u
    x2 = x * x
    qa, qb = np.ones_like(u), np.zeros_like(u)
    for k in range(16, 4, -1):
        qa, qb = float(k + 1) * x2 * qb + qa, qa
    q4 = 5.0 * x2 * qb + qa
    q3 = 4.0 * x2 * qa + q4
    q2 = 3.0 * x2 * q4 + q3
    q1 = 2.0 * x2 * q3 + q2
    return x * q2 / q1, 2.0 * x * q3 / q2, x * (3.0 * q4 * q2 - 2.0 * q3 * q3) / (q3 * q2)


def log_normal_cdf(x):
    xl = np.minimum(x, -U0)
    return np.where(x >= 0.0, np.log1p(-normal_cdf(-np.maximum(x, 0.0))),
                    np.where(x >= -U0, np.log(normal_cdf(np.clip(x, -U0, 0.0))),
                             -0.5 * xl * xl - C - np.log(mills_cf(-xl)[0] - xl)))


def series_log_normal_cdf(x):
    """The reference's log_ndtr: -ndtr(-x) above 8, log(ndtr(x)) down to -20, the order-3 asymptotic series below."""
    x2 = np.square(np.minimum(x, -20.0))
    return np.where(x > 8.0, -normal_cdf(-x), np.where(x >= -20.0, np.log(normal_cdf(np.clip(x, -20.0, 8.0))),
                    -0.5 * x2 - np.log(-np.minimum(x, -20.0)) - C + np.log(1.0 - 1.0 / x2 + 3.0 / x2 ** 2 - 15.0 / x2 ** 3)))


def device_terms(u, rho2, nrho2, defect=None):
    """entropy_tail's loop body for one sample: (f_mes, fu_mes, f_gib, fu_gib, acc_rho term), with one of the defects (a) to (d)
    put back (module docstring)."""
    with np.errstate(all="ignore"):
        big = u > U0
        ub, us = np.where(big, u, 2.0 * U0), np.where(big, 0.0, u)
        delta, t2, t32 = mills_cf(ub)
        hb = ub + delta
        wb = delta * (t2 - delta)
        fb = -0.5 * ub * delta + C + np.log(hb)
        if defect == "d":                                    # the two gamma^2 / 2 terms, from a log Phi that is itself accurate
            lmc = log_normal_cdf(-ub)
            hb = np.exp(-0.5 * ub * ub - C - lmc)
            fb = -0.5 * ub * hb - lmc
            wb = 1.0 + hb * (ub - hb)
        lq = log_normal_cdf(-us)
        hs = normal_pdf(us) / normal_cdf(-us)
        if defect == "a":                                    # log_ndtr's middle branch up to x = 8, the ratio through it
            lq = np.where(-us > 8.0, -normal_cdf(us), np.log(normal_cdf(-us)))
            hs = np.exp(-0.5 * us * us - C - lq)
        ds = hs - us
        hds = hs * ds
        ws = 1.0 - hds
        fs = -0.5 * us * hs - lq
        h = np.where(big, hb, hs)
        hd = np.where(big, 1.0 - wb, hds)
        w = np.where(big, wb, ws)
        one_ud = np.where(big, t2 * delta, 1.0 - us * ds)
        dhd = np.where(big, hb * delta * delta * t2 * t32, hs * (ds * ds - ws))
        fmes = np.where(big, fb, fs)
        if defect == "c":                                    # the parent's arithmetic above gamma = 20
            lmc = series_log_normal_cdf(-u)
            r = np.exp(-0.5 * u * u - C - lmc)
            far = u > 20.0
            h, fmes = np.where(far, r, h), np.where(far, -0.5 * u * r - lmc, fmes)
            hd = np.where(far, r * (r - u), hd)
            w = np.where(far, 1.0 - hd, w)
            one_ud = np.where(far, 1.0 - u * (r - u), one_ud)
            dhd = np.where(far, -(-r * (u - r) * (u - r) + r - r * r * (r - u)), dhd)
        inner = nrho2 + rho2 * w
        fgib = np.where(hd < 0.5, -0.5 * np.log1p(-rho2 * np.minimum(hd, 0.5)), -0.5 * np.log(inner))
        if defect == "b":
            fgib = -0.5 * np.log(1.0 + rho2 * -hd)
        return fmes, 0.5 * h * one_ud, fgib, 0.5 * rho2 * dhd / inner, 0.5 * hd / inner


def test_restated_device_tail_matches_the_goldens_to_1e5(goldens):
    """Measured: 2e-12 for the values and 2e-10 for the derivatives, both just below the switch to the continued fraction at
    gamma = 6 (the eps gamma^2 and eps gamma^6 of the differences taken there)."""
    got = device_terms(goldens["gamma"], goldens["rho2"], 1.0 - goldens["rho2"])
    worst = {k: float(np.max(np.abs(g - goldens[k]) / goldens[k])) for k, g in zip(KEYS, got)}
    print("worst relative error of the restated device tail:", worst)
    assert max(worst.values()) <= 1e-5, worst


@pytest.mark.parametrize("name", E.IDS)
def test_cells_and_sensitivity_on_the_oracles_moments(name):
    """>= 20 asserted (candidate, sample) pairs in every cell the model can populate, and the 8-ulp sensitivity term below
    1e-6 |ref| for every asserted pair -- on the oracle's moments; the GPU suite asserts both again on the engine's."""
    p = E.problem(name)
    for acq in E.ACQS:
        E.assert_cells(p, acq, E.cell_counts(p, acq, p.params, p.om, p.ov))
        pairs = 0
        for s in p.params:
            ref = E.tails(p, acq, [s], p.om, p.ov)
            ok = np.abs(ref) >= R.TINY
            sens = E.sensitivity(p, acq, [s], p.om, p.ov)
            assert np.all(sens[ok] <= 1e-6 * np.abs(ref[ok])), (acq, s, float(np.max(sens[ok] / np.abs(ref[ok]))))
            pairs += int(ok.sum())
        assert pairs >= 100000, (acq, pairs)


def _failures(p, defect):
    """{acq: failures per gamma-bin} of the restated tail on the model's (candidate, sample) pairs, under the GPU suite's
    tolerance: 1e-5 |ref| + the 8-ulp sensitivity; a NaN or a negative value fails."""
    out = {acq: np.zeros(len(E.G_BINS), dtype=np.int64) for acq in E.ACQS}
    den = p.ov + p.noise
    for s in p.params:
        g = E.gammas([s], p.om, p.ov)[:, 0]
        fm, _, fg, _, _ = device_terms(g, p.ov / den, p.noise / den, defect)
        gb = E.g_bin(g)
        for acq, got in (("mes", fm), ("gibbon", fg)):
            ref = E.tails(p, acq, [s], p.om, p.ov)
            tol = R.RTOL * np.abs(ref) + E.sensitivity(p, acq, [s], p.om, p.ov)
            bad = (np.abs(ref) >= R.TINY) & (gb >= 0) & ~((np.abs(got - ref) <= tol) & (got >= 0.0))
            np.add.at(out[acq], gb[bad], 1)
    return out


def test_each_defect_is_caught_in_its_regime():
    """On the low-noise model (oracle's moments, every sample of the list alone): the restated tail has no failure in any bin;
    with one defect put back it fails in the bins that defect lives in and in none on the other side of them.  ((c) is the
    parent's whole arithmetic above gamma = 20, so it carries (d) with it.)  Failures counted on 2100 candidates x 195 samples:
    (a) mes 9450 in [-8,8] (GIBBON's share of that regime is (b): 1 + 4e-14 at gamma = -8); (b) gibbon 48611, 65265, 8125 in the three bins up to 8 (every pair below -8);
    (c) gibbon 12924 of 14571 in (20,37]; (d) mes 1325 of 1331 in (1e3,1e5] and 2712 of 2712 in (1e5,1e8]."""
    p = E.problem(E.NEW)
    bins = {n: i for i, n in enumerate(E.G_BIN_NAMES)}
    clean = _failures(p, None)
    assert all(not f.any() for f in clean.values()), clean
    fails = {d: _failures(p, d) for d in "abcd"}
    print({d: {a: f.tolist() for a, f in v.items()} for d, v in fails.items()})
    assert fails["a"]["mes"][bins["[-8,8]"]] > 0, ("(a) not caught in [-8,8]", fails["a"]["mes"])
    assert not fails["a"]["mes"][[i for i in range(8) if i != bins["[-8,8]"]]].any(), fails["a"]["mes"]
    for b in ("[-37,-20)", "[-20,-8)"):
        assert fails["b"]["gibbon"][bins[b]] > 0, (f"(b) not caught in {b}", fails["b"]["gibbon"])
    assert not fails["b"]["gibbon"][3:].any() and not fails["b"]["mes"].any(), fails["b"]
    assert fails["c"]["gibbon"][bins["(20,37]"]] > 0, ("(c) not caught in (20,37]", fails["c"]["gibbon"])
    assert not fails["c"]["gibbon"][:4].any() and not fails["c"]["mes"][:4].any(), fails["c"]
    for acq in E.ACQS:
        for b in ("(1e3,1e5]", "(1e5,1e8]"):
            assert fails["d"][acq][bins[b]] > 0, (f"(d) not caught in {b}", acq, fails["d"][acq])
        assert not fails["d"][acq][:5].any(), fails["d"][acq]
