"""The fp64 oracle against mpmath where the GPU tests lean on it hardest: the acquisition tails deep below the
improvement threshold (a relative comparison of the engine's tails, down to 1e-290, takes them as its reference:
tests/acq_regimes.py) and the kernel functions at ulp resolution.  The goldens are written by
tests/make_acq_tail_goldens.py and tests/make_kernel_resolution_goldens.py; nothing here needs mpmath or a GPU."""
import json
import os

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.kernel_resolution import A_COEF, A_GRAD, B_DIFF
from tests.util import EPS

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    with open(os.path.join(GOLDEN_DIR, name)) as f:
        return json.load(f)


def test_oracle_tails_match_mpmath_to_1e8():
    """EI, PI and AEI on z in {-37.5, -37, -36, -30, -20, -10, -5, -1, 0, 1, 5, 8, 20} x sigma in {1e-6, 1e-3, 0.3, 1, 1e3}
    to 1e-8 relative.  Measured worst cases: EI and AEI 1.6e-10, both at z = -37.5, sigma = 1e-3 (a subnormal value,
    1.2e-312) and at z = -37, sigma = 1e-6 among the normal ones (1.5e-307); PI 2.2e-13 at z = -36.  The loss is the
    eps z^4 cancellation of diff Phi(z) + sigma phi(z), which the reference implementation shares, and the rounding of
    subnormal terms.  1e-8 is more than an order of magnitude above that."""
    cases = _load("acq_tail_goldens.json")["cases"]
    assert len(cases) == 13 * 5
    worst = {}
    for c in cases:
        got = dict(ei=O.expected_improvement(c["mean"], c["var"], c["eta"]),
                   pi=O.probability_of_improvement(c["mean"], c["var"], c["eta"]),
                   aei=O.augmented_expected_improvement(c["mean"], c["var"], c["eta"], c["noise"]))
        for acq, v in got.items():
            assert c[acq] > 0.0
            rel = abs(float(v) - c[acq]) / c[acq]
            worst[acq] = max(worst.get(acq, 0.0), rel)
            assert rel <= 1e-8, (acq, c["z"], c["sigma"], float(v), c[acq], rel)
    print("worst relative error of the oracle's tails:", worst)


@pytest.mark.parametrize("kind", O.KERNEL_KINDS)
def test_oracle_kernels_match_mpmath_to_an_ulp(kind):
    """``O.kernel_from_r2`` on the single-point design (r^2 the nearest double of the exact one): within eps (1 + s) of
    mpmath, s the argument of the exponential.  Measured on these probes: 0.50, 0.55, 0.99, 1.0 of that bound for rbf,
    matern12, matern32, matern52, the worst at small s, where 1 + s, the exponential and two products round a value just
    below 1."""
    g = _load("kernel_resolution_goldens.json")
    b = g["single"][kind]
    k, s = np.array(b["k"]), np.array(b["s"])
    K = O.kernel_from_r2(kind, g["variance"], np.array(b["r2"]))
    assert np.all(k >= 1e-300) and s.max() <= 680.0 * (1 + 1e-12)
    assert np.all(np.abs(K - k) <= EPS * (1.0 + s) * k), float(np.max(np.abs(K - k) / (EPS * (1.0 + s) * k)))


@pytest.mark.parametrize("kind", O.KERNEL_KINDS)
def test_oracle_kernel_matrix_and_gradient_on_every_design(kind):
    """The oracle in the difference form from the points themselves -- the reference of the parity tests -- on the three
    designs of the goldens, and its input gradient (``acq_value_and_grad`` of -LCB at beta = 0 on the single-point design is
    -dk/dx).  Bound: eps (A + B s), the one derived for the device in tests/kernel_resolution.py with sqrt and exp at
    2 ulp -- numpy's are at least that accurate.  Measured: at most 1.05 eps (1 + s) on every design."""
    g = _load("kernel_resolution_goldens.json")
    ls, B = np.array(g["lengthscales"]), B_DIFF[kind]
    bound = lambda s, A=A_COEF[kind]: EPS * (A + B * np.asarray(s))
    R, D, b = g["rows"], g["dense"], g["single"][kind]
    X = np.tile(np.array(g["X0"]), (R["N"], 1))
    X[:, 0] += R["spacing"] * np.arange(R["N"])
    with O.difference_form():
        for i in R["rows"]:
            blk = R[kind][str(i)]
            K = O.kernel_matrix(kind, g["variance"], ls, np.array(blk["x"]), X)
            k = np.array(blk["k"])
            assert np.count_nonzero(K) == k.size, "a kernel value 4096 lengthscales away is not exactly 0"
            assert np.all(np.abs(K[:, i] - k) <= bound(blk["s"]) * k), (i, float(np.max(np.abs(K[:, i] - k) / k)) / EPS)
        Kd, kd = O.kernel_matrix(kind, g["variance"], ls, np.array(D["x"]), np.array(D["X"])), np.array(D[kind]["K"])
        assert np.all(np.abs(Kd - kd) <= bound(D[kind]["s"]) * kd)
        st = O.gpr_update(kind, g["variance"], ls, g["noise"], 0.0, np.array([g["X0"]]), np.array([4.0]))
    assert st.L[0, 0] == 2.0
    val, grad = O.acq_value_and_grad(st, "nlcb", 0.0, np.array(b["x"]))
    k, dk = np.array(b["k"]), np.array(b["dk"])
    assert np.all(np.abs(-val - k) <= bound(b["s"]) * k)
    assert np.all(np.abs(-grad - dk) <= (bound(b["s"], A_GRAD[kind]) * np.abs(dk).max(axis=1))[:, None])
