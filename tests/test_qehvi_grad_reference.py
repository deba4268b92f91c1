"""CPU: the arithmetic of the gradient of the batch Monte-Carlo expected hypervolume improvement w.r.t. the joint moments,
re-derived.  The numpy restatement (tests/qehvi_grad_reference.py) against 50-digit central differences of a 50-digit value
(tests/make_qehvi_grad_goldens.py); its d / d mean at zero draws against the derivative of an exact rational hypervolume of the
union; and the host layer that builds the differentiable function and routes it to the continuous optimizer."""
import functools
import json
import os
from fractions import Fraction

import numpy as np
import pytest

from tests import qehvi_grad_reference as GR
from tests import qehvi_reference as R
from tests.fakes import FakeEngine
from tests.test_qehvi_reference import sphere_front
from trieste_amd.acquisition.multi_objective import prepare_default_non_dominated_partition_bounds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qehvi_grad_goldens.json")
U = 2.0 ** -53

# The numpy restatement's own worst error against the goldens, as a fraction of the entry's scale (the same sums with every
# term's sign removed; for gcov propagated through the factor's absolute values), measured by the first test below on this
# fixture: 5.33e-15 (d / d cov of "P=4 q=2 correlation 0.99"; the four cases with correlation 0.99 give 3.2e-15 .. 5.3e-15 there,
# LAPACK's factor of a nearly singular covariance moved through the adjoint; d / d cov is at most 1.9e-15 and d / d mean at
# most 1.4e-15 on the other cases).  tests/test_gpu_qehvi_grad.py gives the kernel 100 x this figure (the kernel's fma chains
# against numpy's order).
GRAD_RESTATEMENT_WORST = 5.33e-15


def _symmetric(tri, q):
    out = np.zeros((q, q))
    out[np.tril_indices(q)] = tri
    return out + np.tril(out, -1).T


def load_grad_cases():
    """The cases with mean [P, q], cov / gcov [P, q, q] (from their lower triangles), eps [P, q, S], lb / ub [K, P], gmean
    [P, q], value."""
    with open(GOLDEN) as f:
        doc = json.load(f)
    cases = doc["cases"]
    for c in cases:
        c["mean"], c["eps"] = np.array(c["mean"], np.float64), np.array(c["eps"], np.float64)
        P, q = c["mean"].shape
        part = doc["partitions"][str(P)]
        c["lb"], c["ub"] = np.array(part["lb"], np.float64), np.array(part["ub"], np.float64)
        c["cov"] = np.stack([_symmetric(np.array(t, np.float64), q) for t in c["cov"]])
        c["gcov"] = np.stack([_symmetric(np.array([float(v) for v in t]), q) for t in c["gcov"]])
        c["gmean"] = np.array([[float(v) for v in row] for row in c["gmean"]])
        c["value"] = float(c["value"])
    return cases


def restate(c):
    """``moment_adjoints`` of a golden case as a call of one group."""
    return GR.moment_adjoints(c["mean"][:, None], c["cov"][:, None], c["eps"], c["jitter"], c["lb"], c["ub"])


def grad_errors(got, want, scale):
    """|got - want| as fractions of ``scale``; a zero scale demands an exactly zero result (inf otherwise)."""
    got, want, scale = (np.asarray(a, np.float64) for a in (got, want, scale))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(scale > 0, np.abs(got - want) / scale, np.where(got == 0.0, 0.0, np.inf))


def test_restatement_matches_the_mpmath_goldens():
    cases = load_grad_cases()
    assert 24 <= len(cases) <= 32
    assert {c["mean"].shape[0] for c in cases} == {2, 3, 4} and {c["mean"].shape[1] for c in cases} == {1, 2, 3, 5, 8}
    assert all(c["eps"].shape[2] <= 8 and len(c["lb"]) <= 12 and c["kink"] >= 1e-6 for c in cases)
    assert sum(c["zero"] for c in cases) == 2 and sum("far below" in c["note"] for c in cases) == 2
    assert sum("correlation 0.99" in c["note"] for c in cases) >= 3
    assert os.path.getsize(GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(GOLDEN), "qehvi_goldens.json"))
    worst = (0.0, "")
    for n, c in enumerate(cases):
        P, q = c["mean"].shape
        r = restate(c)
        samples = r["samples"]
        assert GR.kink_distance(samples, c["lb"], c["ub"])[0] >= 1e-6
        if c["zero"]:
            assert c["value"] == 0.0 and not np.any(c["gmean"]) and not np.any(c["gcov"])
            for k in ("value", "gmean", "gcov", "gmean_scale", "gcov_scale"):
                assert not np.any(r[k]), (c["note"], k)
            continue
        off = ~np.eye(q, dtype=bool)
        assert np.any(c["gmean"] != 0.0) and (q == 1 or np.any(c["gcov"][:, off] != 0.0)), c["note"]
        assert np.all(c["gmean"] <= 0.0)   # a larger sample (minimisation) never improves the hypervolume
        assert np.all(np.abs(c["gmean"]) <= r["gmean_scale"][:, 0] * (1 + 1e-12))
        em = grad_errors(r["gmean"][:, 0], c["gmean"], r["gmean_scale"][:, 0]).max()
        ec = grad_errors(r["gcov"][:, 0], c["gcov"], r["gcov_scale"][:, 0]).max()
        print(f"case {n:2d} {c['note']:48s} d/dmean {em:.2e} d/dcov {ec:.2e} of the scales")
        worst = max(worst, (max(em, ec), c["note"]))
    print(f"numpy restatement vs mpmath: worst {worst[0]:.3e} of the scales ({worst[1]})")
    assert worst[0] <= 2.0 * GRAD_RESTATEMENT_WORST


ZERO_DRAW_SHAPES = [(2, 1), (2, 3), (2, 5), (3, 2), (3, 4)]


@functools.lru_cache(maxsize=None)
def zero_draw_problem(P, q):
    """(mean [P, G, q], cov, lb, ub, exact [P, G, q] of Fractions): G = 4 batches whose means lie on multiples of 2^-10, add
    volume to a sphere front and keep more than 2^-19 from every kink (seeds are redrawn until they do), with the exact
    derivative of the hypervolume of the union w.r.t. every coordinate: the volume is piecewise linear in any single
    coordinate, so its central difference with the step 2^-20, below the kink distance, IS the derivative, in exact rationals
    (``exact_union``: no cells, no inclusion-exclusion).  Shared with tests/test_gpu_qehvi_grad.py; nobody changes it."""
    front, ref = sphere_front(P, 12 if P == 2 else 8, seed=20 + P)
    lb, ub = prepare_default_non_dominated_partition_bounds(ref, front)
    G, delta = 4, Fraction(1, 2 ** 20)
    for seed in range(1000 * P + q, 1000 * P + q + 200):
        rng = np.random.default_rng(seed)
        pts = rng.integers(-102, 1127, (8 * G, q, P)) / 1024.0                                    # about [-0.1, 1.1]
        samples = pts[:, None]                                                                     # [8 G, S = 1, q, P]
        adds = np.any(GR.sample_adjoints(samples, lb, ub) != 0.0, axis=(1, 2, 3))
        clear = GR.kink_distance(samples, lb, ub) > 2.0 ** -19
        keep = np.flatnonzero(adds & clear)[:G]
        if len(keep) == G:
            break
    assert len(keep) == G
    pts = pts[keep]
    assert np.all(GR.kink_distance(pts[:, None], lb, ub) > 2.0 * float(delta))                    # the gap condition
    mean = np.ascontiguousarray(np.transpose(pts, (2, 0, 1)))                                      # [P, G, q]
    cov = np.broadcast_to(0.1 * np.eye(q), (P, G, q, q)).copy()
    exact = np.empty((P, G, q), object)
    for g in range(G):
        for i in range(q):
            for j in range(P):
                up, dn = pts[g].copy(), pts[g].copy()
                up[i, j] += float(delta)                # (exact: a step of 2^-20 on a multiple of 2^-10)
                dn[i, j] -= float(delta)
                assert Fraction(float(up[i, j])) - Fraction(float(dn[i, j])) == 2 * delta
                exact[j, g, i] = (R.exact_union(up, front, ref) - R.exact_union(dn, front, ref)) / (2 * delta)
    for a in (mean, cov, lb, ub, exact):
        a.setflags(write=False)
    return mean, cov, lb, ub, exact


def exact_errors(got, exact):
    """|got - exact| elementwise, ``exact`` an array of Fractions."""
    return np.array([float(abs(Fraction(float(v)) - e)) for v, e in zip(np.ravel(got), np.ravel(exact))]).reshape(np.shape(got))


@pytest.mark.parametrize("P,q", ZERO_DRAW_SHAPES)
def test_gmean_at_zero_draws_is_the_exact_rational_derivative(P, q):
    """eps = 0 and S = 1: the samples are the means, and gmean is the derivative of the hypervolume the q means add to the
    front (``zero_draw_problem``).  Tolerance: the roundings of the restatement's sum -- 2 P - 3 per partial product, numpy's
    sum over the K cells, the at most 2^(q-1) subsets in which a point can own an objective -- times u times the scale.  (A
    derivative that cancels to zero may leave the terms' rounding: no exact zero is asked for.)"""
    mean, cov, lb, ub, exact = zero_draw_problem(P, q)
    r = GR.moment_adjoints(mean, cov, np.zeros((P, q, 1)), 1e-6, lb, ub)
    count = (2 * P - 3) + len(lb) + 2 ** (q - 1)
    err, tol = exact_errors(r["gmean"], exact), count * U * r["gmean_scale"]
    assert np.all(err <= tol), float(np.max(err / np.maximum(tol, 1e-300)))
    print(f"P={P} q={q} K={len(lb)}: gmean vs the exact derivative, worst {np.max(err / np.maximum(tol, 1e-300)):.3f} of "
          f"{count} u scale")
    assert np.any(r["gmean"] != 0.0) and any(e != 0 for e in exact.ravel())


def test_restatement_is_consistent_with_differences_of_the_value_restatement():
    """Central differences of ``qehvi_reference.value_from_moments`` along a mean and along a symmetric covariance
    perturbation, at two steps: the tolerance is twice their difference plus the value's rounding over the step."""
    front, ref = sphere_front(3, 8, seed=23)
    lb, ub = prepare_default_non_dominated_partition_bounds(ref, front)
    rng = np.random.default_rng(5)
    P, G, q, S = 3, 6, 3, 4
    a = rng.standard_normal((P, G, q, q))
    mean, cov = rng.uniform(0.0, 0.9, (P, G, q)), 0.05 * (a @ np.swapaxes(a, -1, -2) / q + 0.05 * np.eye(q))
    eps = rng.standard_normal((P, q, S))
    r = GR.moment_adjoints(mean, cov, eps, 1e-6, lb, ub)
    far = GR.kink_distance(r["samples"], lb, ub) > 1e-3
    assert far.sum() >= 3
    noise = 64 * U * R.abs_terms_from_moments(mean, cov, eps, 1e-6, lb, ub)
    checked = 0
    for j, i, b in ((0, 0, 0), (1, 2, 1), (2, 1, 0)):
        for what in ("mean", "cov"):
            est = []
            for h in (2e-5, 1e-5):
                up_m, dn_m, up_c, dn_c = mean.copy(), mean.copy(), cov.copy(), cov.copy()
                if what == "mean":
                    up_m[j, :, i] += h
                    dn_m[j, :, i] -= h
                else:
                    for m_, sgn in ((up_c, h), (dn_c, -h)):
                        m_[j, :, i, b] += sgn
                        if i != b:
                            m_[j, :, b, i] += sgn
                est.append((R.value_from_moments(up_m, up_c, eps, 1e-6, lb, ub) - R.value_from_moments(dn_m, dn_c, eps, 1e-6, lb, ub))
                           / (2 * h))
            got = r["gmean"][j, :, i] if what == "mean" else (r["gcov"][j, :, i, b] * (1.0 if i == b else 2.0))
            tol = 2.0 * np.abs(est[0] - est[1]) + noise / 1e-5
            assert np.all(np.abs(got - est[1])[far] <= tol[far]), (what, j, i, b, np.abs(got - est[1])[far], tol[far])
            checked += int(np.sum(np.abs(est[1])[far] > 100 * tol[far]))
    assert checked >= 6   # the differences say something


def test_kink_distance():
    lb, ub = np.array([[-np.inf, 0.5], [0.25, -np.inf]]), np.array([[0.25, 1.0], [1.0, 0.5]])
    samples = np.array([[[[0.3, 0.7], [0.6, 0.71]]], [[[0.9, 0.1], [0.1, 0.9]]]])    # [G = 2, S = 1, q = 2, P = 2]
    np.testing.assert_allclose(GR.kink_distance(samples, lb, ub), [0.01, 0.1], rtol=1e-12)
    assert GR.kink_distance(samples[:, :, :1], lb, ub)[0] == pytest.approx(0.05)


# ---- the seeded inputs of the GPU shape test, and their kink distances ----------------------------------------------------------
SHAPE_CASES = [(P, q) for P in (2, 3, 4) for q in (1, 2, 3, 8)]
SHAPE_GROUPS = (1, 2, 65, 300)


def cells_of(part):
    """(lb, ub) [K, P] of the tables ``tests.ehvi_tour.table_partition`` returns."""
    bounds, _, lo, hi = part
    cols = np.arange(bounds.shape[0])[None]
    return bounds[cols, lo], bounds[cols, hi]


def shape_inputs(P, q):
    """(mean, cov) of 300 groups and an iterator over (S, K, eps, partition tables): sample counts around the wave width and
    the gradient kernel's sample chunk C_g, cell counts around the slice count, every S with every K."""
    from tests.ehvi_tour import table_partition
    from tests.qehvi_tour import random_moments
    from trieste_amd.engine import qehvi_grad_sample_chunk

    chunk = qehvi_grad_sample_chunk(P, q)
    rng = np.random.default_rng(200 * P + q)
    mean, cov = random_moments(rng, P, SHAPE_GROUPS[-1], q)

    def pairs():
        for S in sorted({1, 63, 64, 65, chunk - 1, chunk, chunk + 1}):
            eps = rng.standard_normal((P, q, S))
            for K in (1, 2, 3, 5):
                yield S, K, eps, table_partition(rng, P, 6, K)

    return mean, cov, pairs()


def test_no_compared_group_of_the_shape_test_lies_at_a_kink():
    """tests/test_gpu_qehvi_grad.py leaves a group out of its comparison with the restatement when its kink distance is below
    the samples' tolerance: over the seeded inputs the restatement alone leaves out none."""
    from tests.test_gpu_qehvi import _sample_atol

    left_out = checked = 0
    for P, q in SHAPE_CASES:
        mean, cov, pairs = shape_inputs(P, q)
        m, c = np.ascontiguousarray(mean[:, [0, -1]]), np.ascontiguousarray(cov[:, [0, -1]])
        for S, K, eps, part in pairs:
            lb, ub = cells_of(part)
            samples = R.samples_from_moments(m, c, eps, 1e-6)
            left_out += int(np.sum(GR.kink_distance(samples, lb, ub) <= _sample_atol(m, c, eps, 1e-6)))
            checked += 2
    print(f"{left_out} of {checked} groups lie within the samples' tolerance of a kink")
    assert left_out == 0 and checked >= 2 * 4 * 4 * len(SHAPE_CASES)


# ---- the host layer ----------------------------------------------------------------------------------------------------------
def test_grad_sample_chunk_rule():
    from trieste_amd.engine import QEHVI_GRAD_MAX_POINTS, QEHVI_SLICES, qehvi_grad_sample_chunk, qehvi_grad_sum_roundings

    def bytes_(P, q, C):
        return 8 * ((QEHVI_SLICES + 1) * P * q * C + P * (2 * q * q + q + q * (q + 3) // 2))

    for P in (2, 3, 4):
        for q in range(1, 9):
            C = qehvi_grad_sample_chunk(P, q)
            assert C % 64 == 0 and 64 <= C <= 512 and bytes_(P, q, C) <= 160 * 1024
            assert C == 512 or bytes_(P, q, C + 64) > 160 * 1024
    assert qehvi_grad_sample_chunk(4, 8) == 64 and qehvi_grad_sample_chunk(2, 2) == 512 and qehvi_grad_sample_chunk(2, 8) == 192
    assert QEHVI_GRAD_MAX_POINTS == 2048
    assert qehvi_grad_sum_roundings(2, 1, 1, 1) == 1 + 2 + 3 + 1 + 6 + 1 + 2


@pytest.fixture()
def stack(monkeypatch):
    import trieste_amd.models as M
    from trieste_amd.data import Dataset

    monkeypatch.setattr(M, "GPEngine", FakeEngine)
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 1, (12, 2))
    Y = np.stack([np.sin(3 * X[:, 0]) + X[:, 1], np.cos(2 * X[:, 1]) - X[:, 0]], axis=1)

    def member(j, kernel):
        m = M.GaussianProcessRegression(M.GPR((X, Y[:, j:j + 1]), kernel, M.Constant(0.1 * j), 1e-3))
        m.update(Dataset(X, Y[:, j:j + 1]))
        return m

    models = [member(0, M.Matern52(1.0, [0.4, 0.6])), member(1, M.SquaredExponential(0.7, 0.5))]
    return M.TrainablePredictJointReparamModelStack(*[(m, 1) for m in models]), Dataset(X, Y)


def test_default_builder_stays_value_only_and_the_option_builds_the_gradient(stack, monkeypatch):
    """The default builder builds a ``batch_ehvi`` without ``value_and_gradient``; ``differentiable=True`` builds the subclass,
    whose ``value_and_gradient`` installs the partition like ``__call__``, chunks at 2048 // B groups, hands the sampler's draws
    over and refuses anything but [R, B, D]."""
    from trieste_amd import engine as engine_mod
    from trieste_amd.acquisition import BatchMonteCarloExpectedHypervolumeImprovement, batch_ehvi, differentiable_batch_ehvi
    from trieste_amd.acquisition.multi_objective import differentiable_batch_ehvi as exported

    model, data = stack
    assert exported is differentiable_batch_ehvi and issubclass(differentiable_batch_ehvi, batch_ehvi)
    assert not hasattr(batch_ehvi, "value_and_gradient")
    plain = BatchMonteCarloExpectedHypervolumeImprovement(16).prepare_acquisition_function(model, data)
    assert type(plain) is batch_ehvi and not hasattr(plain, "value_and_gradient")
    assert "differentiable" not in repr(BatchMonteCarloExpectedHypervolumeImprovement(16))
    builder = BatchMonteCarloExpectedHypervolumeImprovement(16, differentiable=True)
    assert repr(builder) == "BatchMonteCarloExpectedHypervolumeImprovement(16, get_reference_point, jitter=1e-06, differentiable=True)"
    assert repr(BatchMonteCarloExpectedHypervolumeImprovement(4, [1.0, 2.0], differentiable=True)).endswith(", differentiable=True)")
    fn = builder.prepare_acquisition_function(model, data)
    assert type(fn) is differentiable_batch_ehvi
    calls, installed = [], []

    def fake_value_grad(engines, Xq, eps, jitter):
        calls.append((len(engines), Xq.shape, eps.shape, jitter))
        return Xq.sum(axis=(1, 2)), 2.0 * Xq

    monkeypatch.setattr(engine_mod, "qehvi_value_grad", fake_value_grad)
    monkeypatch.setattr(engine_mod, "ehvi_set_partition_tables", lambda e, *t: installed.append(e))
    B = 3
    x = np.random.default_rng(0).uniform(size=(2048 // B + 5, B, 2))
    v, g = fn.value_and_gradient(x)
    assert calls == [(2, (2048 // B, B, 2), (2, B, 16), 1e-6), (2, (5, B, 2), (2, B, 16), 1e-6)] and len(installed) == 1
    assert np.array_equal(v, x.sum(axis=(1, 2))) and np.array_equal(g, 2.0 * x)
    with pytest.raises(ValueError, match=r"\[R, B, D\]"):
        fn.value_and_gradient(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="at most 8 points"):
        fn.value_and_gradient(np.zeros((2, 9, 2)))
