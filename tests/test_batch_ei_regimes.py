"""CPU tests of the two batch-EI yardsticks away from unit scale and from the median threshold: the numpy restatement
(tests/batch_ei_reference.py) and the torch autograd restatement (tests/batch_ei_grad_reference.py) against the 50-digit
values and directional derivatives of tests/golden/batch_ei_regime_goldens.json -- output scales 1e-4 ... 1e6, thresholds
12 posterior standard deviations below the smallest mean ... 6 above it, q = 3, 5, 9, near-duplicate pairs at scale 1e3.
The bounds are the two constants the GPU tolerances are built on, unchanged: RESTATEMENT_WORST of sum |summands| for a
value, GRAD_RESTATEMENT_WORST of the scale of tests/test_batch_ei_grad_reference.py for a directional derivative.

``regime_moments`` is the generator of random moments in one regime that tests/test_gpu_batch_ei_regimes.py runs the device
kernels on."""
import functools

import numpy as np

from tests import batch_ei_grad_reference as GR
from tests import batch_ei_reference as R
from tests import make_batch_ei_regime_goldens as MK
from tests.make_batch_ei_grad_goldens import direction_arrays
from tests.test_batch_ei_grad_reference import GRAD_RESTATEMENT_WORST, case_arrays, direction_scale, golden_gradient
from tests.test_batch_ei_reference import RESTATEMENT_WORST


@functools.lru_cache(maxsize=None)
def load_regime_goldens():
    """(cases, directions) in the layout of the two older golden files."""
    return MK.load()


def regime_moments(q, G, s, t, rng):
    """G q-batches of the unit-scale kind (three shared factors, own variances 0.02 ... 0.5) with the means offset by + 5,
    scaled to the output scale s; eta by the rule of the goldens, ``min(mean) + t mean(sd)``, applied to every q-batch, the
    median of the G figures taken (one eta per call, as the entry points take it)."""
    A = rng.standard_normal((G, q, 3))
    cov = 0.3 * (A @ A.transpose(0, 2, 1)) / 3.0
    cov[:, np.arange(q), np.arange(q)] += rng.uniform(0.02, 0.5, size=(G, q))
    mean = (rng.standard_normal((G, q)) + 5.0) * s
    cov = cov * (s * s)
    per_batch = mean.min(axis=1) + t * np.sqrt(np.diagonal(cov, axis1=1, axis2=2)).mean(axis=1)
    return mean, cov, float(np.median(per_batch))


def test_the_file_holds_the_grid_of_regimes():
    cases, dirs = load_regime_goldens()
    grid = {(c["q"], c["S"], c["s"], c["t"]) for c in cases if c["base"] == f"q{c['q']}"}
    assert grid >= {(q, S, s, t) for q, S in MK.SIZES for s in MK.SCALES for t in MK.SHIFTS}
    assert {(9, 65, 1.0, 0.0), (9, 65, 1.0, -6.0)} <= grid
    assert sorted(c["q"] for c in cases if c["base"].endswith("pair") and c["s"] == 1e3) == [3, 5, 9]
    assert len(cases) == 65
    assert len(dirs) == sum(c["q"] + c["q"] * (c["q"] + 1) // 2 if c["q"] <= 4 else 3 for c in cases)
    for c in cases:   # the threshold rule, on the moments as the tests read them
        assert c["eta"] == MK.threshold(np.array(c["mean"]), np.array(c["cov"]), c["t"])
        assert np.isfinite(c["value"]) and c["abs_terms"] > 1e-250


def test_numpy_restatement_value_matches_the_regime_goldens():
    cases, _ = load_regime_goldens()
    worst = (0.0, None)
    for n, c in enumerate(cases):
        mean, cov, w1, w2 = case_arrays(c)
        v, p, Phi, terms = R.batch_ei_parts(mean, cov, c["eta"], w1, w2)
        scale = float(np.sum(np.abs(terms)))
        assert abs(scale - c["abs_terms"]) <= 1e-9 * c["abs_terms"], (n, c["note"])
        ev = abs(v[0] - c["value"]) / c["abs_terms"]
        # p and Phi are stored to 9 significant digits: a coarse check that the pieces, not only their sum, are right
        np.testing.assert_allclose(p[0], np.array(c["p"]), rtol=1e-8, atol=1e-300, err_msg=c["note"])
        np.testing.assert_allclose(Phi[0], np.array(c["Phi"]), rtol=1e-8, atol=1e-300, err_msg=c["note"])
        if ev > 1e-14:
            print(f"case {n:2d} q={c['q']} S={c['S']} {c['note']:36s} value {c['value']: .6e} error {ev:.2e} of sum |terms|")
        worst = max(worst, (ev, c["note"]))
        assert ev <= RESTATEMENT_WORST, (n, c["note"], ev)
    print(f"numpy restatement vs the regime goldens: worst {worst[0]:.3e} of sum |summands| ({worst[1]})")


def test_torch_restatement_value_and_gradient_match_the_regime_goldens():
    cases, dirs = load_regime_goldens()
    worst_v, worst_g = (0.0, None), (0.0, None)
    grads = {}
    for d in dirs:
        n = d["case"]
        c = cases[n]
        if n not in grads:
            mean, cov, w1, w2 = case_arrays(c)
            v, gm, gc, sc = GR.batch_ei_value_grad(mean, cov, c["eta"], w1, w2)
            assert abs(sc[0] - c["abs_terms"]) <= 1e-9 * c["abs_terms"], (n, c["note"])
            ev = abs(v[0] - c["value"]) / c["abs_terms"]
            worst_v = max(worst_v, (ev, c["note"]))
            assert ev <= RESTATEMENT_WORST, (n, c["note"], ev)
            np.testing.assert_array_equal(gc[0], gc[0].T)
            grads[n] = (gm[0], gc[0], golden_gradient(n, c["q"], dirs))
        gm, gc, gold = grads[n]
        dm, dC = direction_arrays(c["q"], d)
        got = float(gm @ dm + np.sum(gc * dC))
        scale = direction_scale(d, dm, dC, *(gold if gold is not None else (gm, gc)))
        assert np.isfinite(scale) and scale > 1e-250, (n, c["note"], scale)
        ratio = abs(got - d["deriv"]) / scale
        if ratio > 1e-13:
            print(f"case {n:2d} q={c['q']} {c['note']:36s} {d['kind']:6s} {d.get('i', '')} {d.get('j', '')}: "
                  f"derivative {d['deriv']: .6e} error {ratio:.2e} of the scale {scale:.3e}")
        worst_g = max(worst_g, (ratio, c["note"]))
        assert ratio <= GRAD_RESTATEMENT_WORST, (n, c["note"], d["kind"], d.get("i"), d.get("j"), ratio)
    print(f"torch restatement vs the regime goldens: value worst {worst_v[0]:.3e} of sum |summands| ({worst_v[1]}); "
          f"derivatives worst {worst_g[0]:.3e} of the scale ({worst_g[1]}) over {len(dirs)} directions")
