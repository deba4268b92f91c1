"""The entropy-search tails (entropy_tail in csrc/tgp_dev.hpp: entropy_tail_kernel behind values, arg-max and top-k, the tail
of grad_finish_kernel behind ``acq_value_grad``) compared RELATIVELY in every regime of gamma = (sample - mean) / sd.

The parity suites compare MES and GIBBON with the float64 oracle at rtol 1e-6 plus an absolute term and only where
gamma <= 30, and the oracle used to repeat the device's arithmetic line for line.  Here a single min-value sample steers gamma
as ``param`` steers z in tests/test_gpu_acq_regimes.py (same models, candidates and lists; one low-noise model more, whose
near-data candidates reach gamma = 4e6), the reference is the stable float64 restatement of tests/entropy_regimes.py (within
3e-13 of 50-digit values: tests/test_entropy_regimes_conditions.py) evaluated AT THE ENGINE'S OWN MOMENTS (``predict`` with
the sweep forced), and the tolerance is 1e-5 |ref| plus the first-order sensitivity of the tail to 8 ulp of those moments: no
absolute floor.  Values must be finite and >= 0 wherever |ref| >= 1e-290, finite and at most 1e-290 below.  The tail kernel
runs after the sweep, whatever the sweep's launch policy: the default variant only.

Asserted inside the tests on the engine's moments: >= 20 asserted (candidate, sample) pairs in every (gamma-bin x sigma-class)
cell the model can populate (``entropy_regimes.populated``); the sensitivity term <= 1e-6 |ref| for every asserted pair.

Measured on an MI355X (profiles/r24_entropy_tails.txt): the values use at most 3.5e-7 of the tolerance (worst relative error
6e-14 for MES, 3.4e-12 for GIBBON, both in [-8,8]), the gradients 1.6e-4, the repulsion 2.2e-4.  Against the arithmetic this
suite was written to replace (log_ndtr's three branches, the ratio through exp(log pdf - log cdf), log(1 + rho^2 h (gamma - h)))
17 of the 29 tests fail; on the low-noise model the value test fails for MES in 9448 pairs of [-8,8] (gamma <= -6.5), 1328 of
1331 in (1e3,1e5] and all 2712 in (1e5,1e8] (worst relative error 1.8e8), for GIBBON in every pair below gamma = -8 (48611
and 65267, the value returned is 0), 8123 in [-8,8], 12932 of 14571 in (20,37], 953 in (37,1e3] and every pair above 1e3, 2013
of them NaN; the five other models fail in the same bins as far as they reach."""
import math

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import acq_regimes as R
from tests import entropy_regimes as E
from tests.util import cancellation_floor, record_margin

pytestmark = pytest.mark.gpu


def _engine(p, variant=0):
    from trieste_amd.engine import GPEngine

    eng = GPEngine(p.d, p.kind)
    eng.set_variant(variant)
    eng.set_hyper(p.variance, p.ls, p.noise, p.c)
    eng.set_data(p.X, p.Y)
    return eng


def _moments(p, Xq):
    mean, var = _engine(p, 1024).predict(Xq)
    return np.asarray(mean), np.asarray(var)


@pytest.mark.parametrize("name", E.IDS)
def test_tail_values_in_every_regime(name):
    """One sample per call, every sample of the model's list, MES and GIBBON on the 2100 candidates; margins per acquisition,
    gamma-bin and sigma class."""
    p = E.problem(name)
    mean, var = _moments(p, p.Xq)
    samples = p.params
    cls = R.sigma_class(p, var)
    eng = _engine(p)
    problems = []
    for acq in E.ACQS:
        counts = np.zeros((len(E.G_BINS), 4), dtype=np.int64)
        errs, tols, keys = [], [], []
        for s in samples:
            eng.set_min_value_samples([s])
            got = eng.acq_values(acq, 0.0, p.Xq)
            err, tol, asserted, probs = E.value_check(p, acq, [s], got, mean, var)
            problems += probs
            gb = E.g_bin(E.gammas([s], mean, var)[:, 0])
            ok = asserted & (gb >= 0)
            np.add.at(counts, (gb[ok], cls[ok]), 1)
            errs.append(err[ok])
            tols.append(tol[ok])
            keys.append(gb[ok] * 4 + cls[ok])
        errs, tols, keys = np.concatenate(errs), np.concatenate(tols), np.concatenate(keys)
        for key in np.unique(keys):
            record_margin(f"{acq} values {E.G_BIN_NAMES[key // 4]} ({R.SIGMA_CLASSES[key % 4]})", errs[keys == key],
                          tols[keys == key], R.RTOL)
        E.assert_cells(p, acq, counts)
    assert not problems, f"{len(problems)} problem(s):\n" + "\n".join(problems[:12])


@pytest.mark.parametrize("S", [5, 64, 4096])
@pytest.mark.parametrize("name", ["m52_d8_N300", E.NEW])
def test_sample_counts_mix_the_regimes(name, S):
    """S samples from every part of the list at once (4096: the list, and uniform draws over its range): the mean of the
    per-sample reference; 4097 samples are refused and leave the samples in place."""
    p = E.problem(name)
    Xs = np.ascontiguousarray(p.Xq[R.grad_subset(p)])      # 300 candidates of every sigma class: the sample loop is per candidate
    mean, var = _moments(p, Xs)
    params = p.params
    if S <= params.size:
        samples = params[np.linspace(0, params.size - 1, S).astype(int)]
    else:
        rng = np.random.default_rng(S)
        samples = rng.permutation(np.concatenate([params, rng.uniform(params[0], params[-1], S - params.size)]))
    g = E.gammas(samples, mean, var)
    assert len({int(b) for b in E.g_bin(g).ravel() if b >= 0}) >= 6
    eng = _engine(p)
    eng.set_min_value_samples(samples)
    problems = []
    for acq in E.ACQS:
        got = eng.acq_values(acq, 0.0, Xs)
        err, tol, asserted, probs = E.value_check(p, acq, samples, got, mean, var)
        assert asserted.sum() >= 250
        record_margin(f"{acq} values S={S}", err[asserted], tol[asserted], R.RTOL)
        problems += probs
    if S == 4096:
        with pytest.raises(ValueError):
            eng.set_min_value_samples(np.concatenate([samples, samples[:1]]))
        np.testing.assert_array_equal(eng.acq_values("gibbon", 0.0, Xs), got)
    assert not problems, "\n".join(problems[:12])


@pytest.mark.parametrize("name", E.IDS)
def test_value_and_gradient_per_candidate(name):
    """``acq_value_grad`` on 300 candidates, one sample per call at gamma in ``GRAD_G`` of the far field's moments and of one
    near-data candidate's: the chain rule a dmean/dx + b dvar/dx with (a, b) from the stable reference (GIBBON's b includes the
    rho^2 term) at the engine's moments and the oracle's moment gradients, under ``acq_regimes.gradient_check``'s row rule
    and tolerance."""
    p = E.problem(name)
    Xs = np.ascontiguousarray(p.Xq[R.grad_subset(p)])
    eng = _engine(p)
    mean, var = (np.asarray(a) for a in eng.predict(Xs))      # 300 points: the skinny product the gradient call forms too
    cls = R.sigma_class(p, var)
    dmean_dx, dvar_dx = R.moment_gradients(p, Xs)
    wide = R.grad_rows(p, var)
    assert wide.sum() >= 150
    j = int(np.flatnonzero((cls == 1) & wide)[0])
    problems = []
    for acq in E.ACQS:
        high = low = 0
        for s in E.grad_samples(p, mean, var, j):
            eng.set_min_value_samples([s])
            val, grad = (np.asarray(a) for a in eng.acq_value_grad(acq, 0.0, Xs))
            err, tol, asserted, probs = E.value_check(p, acq, [s], val, mean, var)
            record_margin(f"{acq} acq_value_grad value", err[asserted], tol[asserted], R.RTOL)
            problems += probs
            gerr, gtol, rows, _, probs = E.gradient_check(p, acq, [s], grad, mean, var, dmean_dx, dvar_dx)
            record_margin(f"{acq} acq_value_grad gradient", gerr[rows], gtol[rows], R.RTOL)
            problems += probs
            g = E.gammas([s], mean, var)[:, 0]
            high += int(np.sum(rows & (g > 1e3)))
            low += int(np.sum(rows & (g < -10.0)))
        assert low >= R.MIN_CELL, (acq, low)
        assert name != E.NEW or high >= R.MIN_CELL, (acq, high)
    assert not problems, f"{len(problems)} problem(s):\n" + "\n".join(problems[:12])


@pytest.mark.parametrize("above", [0.1, 1.0])
def test_argmax_and_topk_with_gamma_up_to_1e5(above):
    """The low-noise model with one sample 0.1 (1.0) above the smallest near-data mean: gamma reaches 9e3 (9e4) at the
    candidates the model already knows (sd = 1e-5).  The fused arg-max and top-k equal the arg-max / stable descending sort of
    the engine's own values, the winner agrees with the reference's to 1e-5 relative, and no value exceeds
    log(gamma_max) + 1 (f_GIB <= f_MES = log gamma + 0.42 - O(1 / gamma^2) for gamma > 1): a tail that cancels at eps gamma^4
    is off by 0.6 (6e3) there."""
    p = E.problem(E.NEW)
    mean, var = _moments(p, p.Xq)
    near = R.sigma_class(p, var) == 1
    s = float(mean[near].min() + above)
    gmax = float(E.gammas([s], mean, var).max())
    assert 5e3 <= gmax <= 2e5, gmax
    eng = _engine(p)
    eng.set_min_value_samples([s])
    for acq in E.ACQS:
        got = np.asarray(eng.acq_values(acq, 0.0, p.Xq))
        assert np.all(np.isfinite(got)) and np.all(got >= 0.0) and got.max() <= math.log(gmax) + 1.0, (acq, got.min(), got.max())
        val, i, x = eng.acq_argmax(acq, 0.0, p.Xq)
        assert i == int(np.argmax(got)) and val == got[i], (acq, i, int(np.argmax(got)))
        np.testing.assert_array_equal(x, p.Xq[i])
        want = E.tails(p, acq, [s], mean, var)
        oi = int(np.argmax(want))
        assert i == oi or abs(want[oi] - want[i]) <= 1e-5 * want[oi], (acq, i, oi, want[i], want[oi])
        assert abs(val - want[oi]) <= 1e-5 * want[oi] + E.sensitivity(p, acq, [s], mean, var)[i], (acq, val, want[oi])
        tv, ti = eng.acq_topk(acq, 0.0, p.Xq, 17)
        ov_, oi_ = O.top_k(got, 17)
        np.testing.assert_array_equal(ti, oi_)
        np.testing.assert_array_equal(tv, ov_)


@pytest.mark.parametrize("m", [1, 16, 17])
@pytest.mark.parametrize("name", ["m52_d8_N300", "rbf_d2_N100_tiny", "m12_d40_N130"])
def test_repulsion_is_the_log_ratio_of_the_two_engines_variances(name, m):
    """gibbon(with a twin of m appended points) - gibbon(without) = w / 2 (log(v_twin + noise) - log(v + noise)) with v and
    v_twin from the two engines' own ``predict``, within cancellation_floor(N + m) / noise; m <= 16 takes the rank-m
    correction of this model's variance (where the kernel sums have an instantiation), m = 17 the twin's own sweep.
    Candidate 500 sits exactly at the first appended point."""
    p = E.problem(name)
    rng = np.random.default_rng(100 + m)
    pending = rng.uniform(size=(m, p.d))
    pending[0] = p.Xq[500]
    w = 1.0 / m ** 2
    eng = _engine(p)
    eng.set_min_value_samples(p.params[::40])
    without = np.asarray(eng.acq_values("gibbon", 0.0, p.Xq))
    twin = eng.clone()
    twin.append_data(pending, np.full(m, p.c))
    eng.set_repulsion(twin, w)
    with_twin = np.asarray(eng.acq_values("gibbon", 0.0, p.Xq))
    eng.set_repulsion(None)
    np.testing.assert_array_equal(eng.acq_values("gibbon", 0.0, p.Xq), without)
    base = _engine(p, 1024)
    tw = base.clone()
    tw.append_data(pending, np.full(m, p.c))
    tw.set_variant(1024)
    v, vt = np.asarray(base.predict(p.Xq)[1]), np.asarray(tw.predict(p.Xq)[1])
    ref = 0.5 * w * (np.log(vt + p.noise) - np.log(v + p.noise))
    tol = cancellation_floor(p.N + m, p.variance, p.noise) / p.noise
    err = np.abs((with_twin - without) - ref)
    record_margin(f"gibbon repulsion m={m}", err, np.full_like(err, tol), 0.0, tol)
    floor = cancellation_floor(p.N + m, p.variance, p.noise)
    # one noisy observation at the candidate itself leaves v noise / (v + noise); further points only lower it
    assert np.all(np.isfinite(with_twin)) and vt[500] <= v[500] * p.noise / (v[500] + p.noise) + floor, (v[500], vt[500])
    assert np.all(err <= tol), (float(err.max()), tol, int(np.argmax(err)))
