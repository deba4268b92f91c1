"""The conditions a relative comparison of the engine's acquisition tails (tests/acq_regimes.py) relies on, checked on the oracle's own moments without a GPU: every
(z-bin x sigma-class) cell a model can populate holds at least 20 asserted candidates over its parameter list, the
sensitivity of every asserted reference value and gradient row to 8 ulp of the moments stays below 1e-6 of it, the
chain-rule reference of the gradients reproduces the oracle's gradient, and the deep-tail candidate set of the arg-max test
is below 1e-100 and normal.

Cells that cannot be populated: the ``clipped`` class exists only where the noise is below the 1e-12 clip
(m52_d8_N200_lownoise_tiny: noise 3.7e-14); with noise 1e-2 sigma^2 the variance at a training input stays near the noise,
far above 1e-12, so the four other models have no clipped candidate (``EMPTY``).  Every other cell of every model is
populated (the smallest holds 200 asserted candidate-parameter pairs)."""
import numpy as np
import pytest

from tests import acq_regimes as R

# (model, sigma class) pairs no candidate of the model can fall into
EMPTY = {(name, "clipped") for name in R.IDS if name != "m52_d8_N200_lownoise_tiny"}


@pytest.mark.parametrize("name", R.IDS)
def test_cells_are_populated_and_sensitivity_is_small(name):
    p = R.problem(name)
    cls = R.sigma_class(p, p.ov)
    present = [int(np.sum(cls == k)) for k in range(4)]
    print(name, "candidates per sigma class", dict(zip(R.SIGMA_CLASSES, present)), "parameters", len(p.params))
    for acq in ("ei", "pi", "aei"):
        counts = R.cell_counts(p, acq, p.params, p.om, p.ov)
        print(acq, "\n", counts)
        for k in range(4):
            if (name, R.SIGMA_CLASSES[k]) in EMPTY:
                assert present[k] == 0
                continue
            for b in range(len(R.Z_BINS)):
                assert counts[b, k] >= R.MIN_CELL, (name, acq, R.Z_BIN_NAMES[b], R.SIGMA_CLASSES[k], int(counts[b, k]))
        for param in p.params:
            *_, problems = R.value_check(p, acq, param, R.tails(p, acq, param, p.om, p.ov), p.om, p.ov)
            assert not problems, problems
    for beta in R.BETAS:
        *_, problems = R.value_check(p, "nlcb", beta, R.tails(p, "nlcb", beta, p.om, p.ov), p.om, p.ov)
        assert not problems, problems


@pytest.mark.parametrize("name", R.IDS)
def test_deep_tail_candidate_set_is_below_1e_100_and_normal(name):
    p = R.problem(name)
    param, idx = R.deep_tail(p, p.om, p.ov)
    assert idx.size >= 200 and np.all(idx[-40:] >= R.M - 40), "the far field belongs to the set"
    for acq in ("ei", "pi", "aei"):
        v = R.tails(p, acq, param, p.om[idx], p.ov[idx])
        assert np.all((v >= 1e-280) & (v < 1e-100)), (acq, float(v.min()), float(v.max()))


@pytest.mark.parametrize("name", R.IDS)
def test_gradient_reference_and_its_sensitivity(name):
    """The chain-rule reference of the gradient comparison, at the oracle's own moments, is the oracle's gradient to
    1e-5 |grad|_inf per row; its sensitivity to 8 ulp of the moments stays below 1e-6 |grad|_inf on every asserted row; and
    at least 20 asserted rows per tail lie at z < -10, where an absolute tolerance would compare nothing."""
    from oracle import gp_oracle as O

    p = R.problem(name)
    sub = R.grad_subset(p)
    Xs = np.ascontiguousarray(p.Xq[sub])
    mean, var = p.om[sub], p.ov[sub]
    dmean_dx, dvar_dx = R.moment_gradients(p, Xs)
    wide = R.grad_rows(p, var)
    assert wide.sum() >= 150
    j = int(np.flatnonzero((R.sigma_class(p, var) == 1) & wide)[0])
    for acq in ("ei", "pi", "aei", "nlcb"):
        deep = 0
        for param in (R.BETAS if acq == "nlcb" else R.grad_params(p, mean, var, j)):
            _, grad = O.acq_value_and_grad(p.st, acq, float(param), Xs)
            err, tol, rows, _, problems = R.gradient_check(p, acq, float(param), grad, mean, var, dmean_dx, dvar_dx)
            assert not problems, problems
            deep += int(np.sum(rows & ((param - mean) / np.sqrt(var) < -10.0)))
        if acq != "nlcb":
            print(name, acq, "asserted gradient rows at z < -10:", deep)
        assert acq == "nlcb" or deep >= R.MIN_CELL, (name, acq, deep)
