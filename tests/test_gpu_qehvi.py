"""GPU: the batch Monte-Carlo expected hypervolume improvement -- the tail kernel against 50-digit goldens, an exact rational
hypervolume of the union and the numpy restatement of the reference's loop, across the shapes at which it changes path; purity
(bit-identity across calls, permutations, sub-ranges and poisoned allocations); composition with every engine's own
``predict_joint``; the function object; the refusals; the ownership of the partition; and the rule end to end.

Tolerance of a comparison on given moments:  tol = c_sum u abs_terms + Lip sample_atol,  u = 2^-53, where

  c_sum        counts the roundings of the kernel's documented summation (``engine.qehvi_sum_roundings``):
               P + 1 per product; then the longest chain of additions a term passes through: the 2^q - 1 terms of its
               (sample, cell) in the walk's accumulator, the ceil(K / 4) cells of the lane's slice times the ceil(S / 64)
               samples of the lane in the lane's accumulator, 3 additions over the four slices, 6 of the butterfly over the
               lanes, and the division by S
  abs_terms    the sum with every sign positive (tests/qehvi_reference.py)
  sample_atol  ``tests.util.reparam_sample_atol`` with the backward error of two float64 Cholesky factorisations (the kernel's
               and the yardstick's), 2 (q + 1) u max|cov + jitter I| (Higham, Accuracy and Stability, theorem 10.3), as the
               floor of the covariance entries, plus the q + 1 roundings of each side's dot product
  Lip          the largest (P - 1)-dimensional cross-section of the box spanned by the samples and the top of the cells: the
               hypervolume is Lipschitz in each coordinate by that area."""
import os
import subprocess
import sys
from fractions import Fraction

import numpy as np
import pytest

from tests import qehvi_reference as R
from tests import qehvi_tour as T
from tests.ehvi_tour import table_partition
from tests.test_qehvi_reference import load_cases, sphere_front
from tests.util import record_margin, reparam_sample_atol

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def _E():
    from trieste_amd import engine as E

    return E


def _bare_engine(d=2):
    return _E().GPEngine(d, "matern52", device=0)


def _sample_atol(mean, cov, eps, jitter):
    q = cov.shape[-1]
    covs = cov.reshape(-1, q, q)
    floor = 2.0 * (q + 1) * U * float(np.max(np.abs(covs + jitter * np.eye(q))))
    dot = 2.0 * (q + 1) * U * (float(np.max(np.abs(mean))) + q * float(np.sqrt(np.max(np.abs(covs)) + jitter)) * float(np.max(np.abs(eps))))
    return reparam_sample_atol(covs, floor, eps, jitter) + dot


def _lipschitz(samples, ub):
    """samples [..., P], cell tops ub [K, P] -> the largest cross-section of the box [min samples, max ub]."""
    P = samples.shape[-1]
    lengths = np.maximum(np.max(ub, axis=0) - np.minimum(samples.reshape(-1, P).min(axis=0), np.max(ub, axis=0)), 0.0)
    return max(float(np.prod(np.delete(lengths, j))) for j in range(P))


def _check(what, got, want, tol):
    got, want, tol = (np.asarray(a, np.float64) for a in (got, want, tol))
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    err = np.abs(got - want)
    worst = record_margin(what, err, tol)
    print(f"{what}: worst {worst:.3f} of the tolerance")
    assert np.all(err <= tol), (what, float(np.max(err)), float(np.min(tol)))


def _moments_tolerance(E, mean, cov, eps, jitter, lb, ub, groups):
    """(want, tol) of the groups ``groups`` of a call on given moments, by the formula of the module docstring."""
    P, _, q = mean.shape
    S, K = eps.shape[2], len(lb)
    m, c = np.ascontiguousarray(mean[:, groups]), np.ascontiguousarray(cov[:, groups])
    samples = R.samples_from_moments(m, c, eps, jitter)
    want, scale = R.reference_form(samples, lb, ub), R.abs_terms(samples, lb, ub)
    tol = E.qehvi_sum_roundings(P, q, S, K) * U * scale + _lipschitz(samples, ub) * _sample_atol(m, c, eps, jitter)
    return want, tol


# ---- goldens and exact yardstick -------------------------------------------------------------------------------------------
def test_moments_entry_matches_the_mpmath_goldens():
    E = _E()
    eng = _bare_engine()
    for n, c in enumerate(load_cases()):
        P, q = c["mean"].shape
        mean, cov = c["mean"][:, None, :], c["cov"][:, None, :, :]
        E.ehvi_set_partition(eng, c["lb"], c["ub"])
        got = E.qehvi_moments(eng, mean, cov, c["eps"], c["jitter"])
        print(f"case {n:2d} {c['note']:45s} value {c['value']: .6e} device {got[0]: .6e}")
        samples = R.samples_from_moments(mean, cov, c["eps"], c["jitter"])
        tol = E.qehvi_sum_roundings(P, q, c["eps"].shape[2], len(c["lb"])) * U * c["abs_terms"] \
            + _lipschitz(samples, c["ub"]) * _sample_atol(mean, cov, c["eps"], c["jitter"])
        _check(f"golden {n} ({c['note']})", got, [c["value"]], [tol])
        assert (got[0] > 0.0) == (c["value"] > 0.0), c["note"]


@pytest.mark.parametrize("P,q", [(P, q) for P in (2, 3) for q in (1, 2, 5, 8)])
def test_zero_draws_give_the_exact_union_of_the_means(P, q):
    """eps = 0 and S = 1: the samples are the means exactly, and the value is the hypervolume the q means add to the front,
    held to c_sum u abs_terms against exact rationals (coordinate compression: no cells, no inclusion-exclusion)."""
    from trieste_amd.acquisition import prepare_default_non_dominated_partition_bounds

    E = _E()
    front, ref = sphere_front(P, 12 if P == 2 else 8, seed=20 + P)
    lb, ub = prepare_default_non_dominated_partition_bounds(ref, front)
    rng = np.random.default_rng(1000 * P + q)
    G = 6
    # points uniform in [-0.1, 1.1]^P; of 8 G drawn batches, 4 that add volume (some point below the reference point that no
    # front point dominates) and 2 that add none
    drawn = rng.uniform(-0.1, 1.1, (P, 8 * G, q))
    pts = np.transpose(drawn, (1, 2, 0))                                                       # [8 G, q, P]
    dominated = np.any(np.all(front[None, None] <= pts[:, :, None, :], axis=-1), axis=-1)      # [8 G, q]
    adds = np.any(~dominated & np.all(pts < ref, axis=-1), axis=-1)
    keep = np.concatenate([np.flatnonzero(adds)[:4], np.flatnonzero(~adds)[:2]])
    assert len(keep) == G or q >= 5    # (large batches nearly always add volume)
    keep = np.concatenate([keep, np.setdiff1d(np.arange(8 * G), keep)])[:G]
    mean = np.ascontiguousarray(drawn[:, keep])
    cov =np.broadcast_to(0.1 * np.eye(q), (P, G, q, q)).copy()
    exact = [R.exact_union(mean[:, g, :].T, front, ref) for g in range(G)]
    share = sum(e > 0 for e in exact) / G
    print(f"P={P} q={q} K={len(lb)}: {100 * share:.0f} % of the batches have a positive exact value")
    assert share >= 0.5
    eng = _bare_engine()
    E.ehvi_set_partition(eng, lb, ub)
    got = E.qehvi_moments(eng, mean, cov, np.zeros((P, q, 1)))
    scale = R.abs_terms(np.transpose(mean, (1, 2, 0))[:, None], lb, ub)
    c_sum = E.qehvi_sum_roundings(P, q, 1, len(lb))
    err = np.array([float(abs(Fraction(float(v)) - e)) for v, e in zip(got, exact)])
    tol = c_sum * U * scale
    worst = record_margin(f"exact union P={P} q={q}", err, np.maximum(tol, 1e-300))
    print(f"exact union P={P} q={q}: worst {worst:.3f} of c_sum u abs_terms (c_sum = {c_sum})")
    assert np.all(err <= tol)
    assert all((v > 0.0) == (e > 0) for v, e in zip(got, exact))


# ---- shapes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P,q", [(P, q) for P in (2, 3, 4) for q in (1, 2, 3, 7, 8)])
def test_shapes_where_the_kernel_changes_path(P, q):
    """Sample counts around the wave width and the sample chunk, cell counts around the slice count, group counts up to 1000:
    against the numpy restatement on the first and the last group of the largest call, and every smaller call bit-equal to the
    head of the largest."""
    E = _E()
    chunk = E.qehvi_sample_chunk(P, q)
    assert chunk == min(512, (32 * 1024 // (8 * P * q)) // 64 * 64)   # the documented rule
    eng = _bare_engine()
    rng = np.random.default_rng(100 * P + q)
    Gs = (1, 2, 65, 1000)
    mean, cov = T.random_moments(rng, P, Gs[-1], q)
    for S in sorted({1, 63, 64, 65, chunk - 1, chunk, chunk + 1}):
        eps = rng.standard_normal((P, q, S))
        for K in (1, 2, E.QEHVI_SLICES - 1, E.QEHVI_SLICES + 1):
            bounds, nb, lo, hi = table_partition(rng, P, 6, K)
            E.ehvi_set_partition_tables(eng, bounds, nb, lo, hi)
            cols = np.arange(P)[None]
            lb, ub = bounds[cols, lo], bounds[cols, hi]
            full = E.qehvi_moments(eng, mean, cov, eps)
            want, tol = _moments_tolerance(E, mean, cov, eps, 1e-6, lb, ub, [0, Gs[-1] - 1])
            _check(f"P={P} q={q} S={S} K={K}", full[[0, -1]], want, tol)
            for G in Gs[:-1]:
                part = E.qehvi_moments(eng, np.ascontiguousarray(mean[:, :G]), np.ascontiguousarray(cov[:, :G]), eps)
                np.testing.assert_array_equal(part, full[:G], err_msg=f"P={P} q={q} S={S} K={K} G={G}")


# ---- purity --------------------------------------------------------------------------------------------------------------
def test_values_do_not_depend_on_the_call():
    """Identical calls, a permutation of the batches, a sub-range, device-resident inputs: the same bits per batch."""
    import torch

    E = _E()
    rng = np.random.default_rng(31)
    for P, q, S, K in ((2, 3, 70, 7), (4, 6, 40, 5)):
        eng = _bare_engine()
        E.ehvi_set_partition_tables(eng, *table_partition(rng, P, 6, K))
        mean, cov = T.random_moments(rng, P, 333, q)
        eps = rng.standard_normal((P, q, S))
        base = E.qehvi_moments(eng, mean, cov, eps)
        assert np.any(base > 0.0)
        np.testing.assert_array_equal(E.qehvi_moments(eng, mean, cov, eps), base)
        perm = rng.permutation(333)
        np.testing.assert_array_equal(E.qehvi_moments(eng, mean[:, perm], cov[:, perm], eps), base[perm])
        np.testing.assert_array_equal(E.qehvi_moments(eng, mean[:, 100:177], cov[:, 100:177], eps), base[100:177])
        dev = [torch.as_tensor(a).to("cuda:0") for a in (mean, cov, eps)]
        np.testing.assert_array_equal(E.qehvi_moments(eng, *dev).cpu().numpy(), base)
        # leading dimensions of the moments
        lead = E.qehvi_moments(eng, mean.reshape(P, 3, 111, q), cov.reshape(P, 3, 111, q, q), eps)
        np.testing.assert_array_equal(lead, base.reshape(3, 111))


def test_tour_under_poisoned_allocations():
    """TGP_POISON=1 fills every fresh device allocation of the library with NaNs: the tour of tests/qehvi_tour.py in a fresh
    child process under it, and here, must agree bit for bit.  The child's timeout is a safety cap; a child that hangs or
    dies on a signal ends the session, so that nothing else is started on a GPU that has just faulted."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tour.npz")
        env = dict(os.environ, TGP_POISON="1")
        try:
            child = subprocess.run([sys.executable, "-m", "tests.qehvi_tour", out], env=env, cwd=ROOT, timeout=120,
                                   capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.exit(f"the poisoned tour hung (120 s cap); stderr:\n{(e.stderr or b'')[-4000:]}", returncode=1)
        if child.returncode < 0 or child.returncode in (134, 139):
            pytest.exit(f"the poisoned tour died with {child.returncode}; stderr:\n{child.stderr[-4000:]}", returncode=1)
        assert child.returncode == 0, f"poisoned tour exited with {child.returncode}:\n{child.stderr[-4000:]}"
        with np.load(out) as z:
            poisoned = {k: z[k] for k in z.files}
    plain = T.tour()
    assert sorted(plain) == sorted(poisoned) and len(plain) >= 11
    for key, value in plain.items():
        assert np.all(np.isfinite(value)), key
        np.testing.assert_array_equal(poisoned[key], value, err_msg=key)


# ---- composition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernels", [("matern52", "rbf"), ("matern32", "matern52", "matern12")])
def test_values_compose_every_engines_own_predict_joint(kernels):
    """qehvi_values(engines, Xq) == qehvi_moments of each engine's predict_joint(Xq), bit for bit, at G q = 2048 (the
    small-product path) and at the first G beyond it (the joint kernel).  The posterior itself is pinned by the parity suites."""
    import torch

    E = _E()
    P, q, d = len(kernels), 4, 3
    engines = T.mixed_stack(kernels, 90, d, seed=40 + P)
    rng = np.random.default_rng(41 + P)
    E.ehvi_set_partition_tables(engines[0], *table_partition(rng, P, 8, 15))
    eps = rng.standard_normal((P, q, 48))
    for G in (512, 513):
        Xq = rng.uniform(size=(G, q, d))
        moments = [eng.predict_joint(Xq) for eng in engines]
        mean, cov = np.stack([m for m, _ in moments]), np.stack([c for _, c in moments])
        want = E.qehvi_moments(engines[0], mean, cov, eps)
        got = E.qehvi_values(engines, Xq, eps)
        np.testing.assert_array_equal(got, want, err_msg=f"G={G}")
        assert np.all(np.isfinite(got)) and np.any(got > 0.0)
        s, t = E.ehvi_last_ms(engines[0])
        assert s > 0.0 and t > 0.0
    dev = E.qehvi_values(engines, torch.as_tensor(Xq).to("cuda:0"), torch.as_tensor(eps).to("cuda:0"))
    np.testing.assert_array_equal(dev.cpu().numpy(), want)


# ---- the function object ---------------------------------------------------------------------------------------------------
def _vlmop2_stack(n=10):
    import trieste_amd.models as M
    from trieste_amd import objectives as OBJ
    from trieste_amd.data import Dataset
    from trieste_amd.space import Box

    space = Box([-2.0, -2.0], [2.0, 2.0])
    x = space.sample_sobol(n, skip=0)
    data = Dataset(x, OBJ.vlmop2(x, 2))
    members = [M.GaussianProcessRegression(M.build_gpr(Dataset(x, data.observations[:, j:j + 1]), space,
                                                       likelihood_variance=1e-5)) for j in range(2)]
    return space, data, M.TrainablePredictJointReparamModelStack(*[(m, 1) for m in members])


def test_function_object_equals_the_reference_form_of_the_samplers_samples():
    """batch_ehvi(x) against the reference's loop applied to ``sampler.sample(x)`` of the SAME sampler, for the leading shapes
    [G], [G1, G2] and the flattened [M, 1, q d] that ``batchify_joint`` passes."""
    import trieste_amd
    from trieste_amd.acquisition import BatchMonteCarloExpectedHypervolumeImprovement, batchify_joint

    E = _E()
    trieste_amd.set_seed(7)
    space, data, stack = _vlmop2_stack()
    q, S = 3, 24
    fn = BatchMonteCarloExpectedHypervolumeImprovement(S).prepare_acquisition_function(stack, data)
    x = space.sample(60 * q, seed=5).reshape(60, q, 2)
    got = fn(x)
    assert got.shape == (60, 1) and np.any(got > 0.0)
    samples = fn._sampler.sample(x, jitter=1e-6)                      # [60, S, q, 2]
    assert samples.shape == (60, S, q, 2)
    lb, ub = fn._lb_points, fn._ub_points
    want, scale = R.reference_form(samples, lb, ub), R.abs_terms(samples, lb, ub)
    mean, cov = stack.predict_joint(x)                                 # [60, q, 2], [60, 2, q, q]
    atol = _sample_atol(np.moveaxis(mean, -1, 0), np.moveaxis(cov, -3, 0), fn._sampler.eps(q), 1e-6)
    tol = E.qehvi_sum_roundings(2, q, S, len(lb)) * U * scale + _lipschitz(samples, ub) * atol
    _check("function object [G]", got[:, 0], want, tol)
    np.testing.assert_array_equal(fn(x.reshape(6, 10, q, 2)), got.reshape(6, 10, 1))
    seen = {}

    def one_point_optimizer(expanded, f):
        flat = x.reshape(60, 1, q * 2)
        seen["values"] = f(flat)
        return flat[:1, 0, :]

    points = batchify_joint(one_point_optimizer, q)(space, fn)
    assert points.shape == (q, 2)
    np.testing.assert_array_equal(seen["values"], got)


def test_ehvi_and_qehvi_functions_over_one_stack_keep_their_own_cells():
    import trieste_amd
    from trieste_amd.acquisition import BatchMonteCarloExpectedHypervolumeImprovement, ExpectedHypervolumeImprovement

    trieste_amd.set_seed(8)
    space, data, stack = _vlmop2_stack()
    single = ExpectedHypervolumeImprovement().prepare_acquisition_function(stack, data)
    batch = BatchMonteCarloExpectedHypervolumeImprovement(16, [5.0, 5.0]).prepare_acquisition_function(stack, data)
    assert not np.array_equal(single._ub_points, batch._ub_points)
    pts = space.sample(120, seed=6)
    alone_single = single(pts[:, None, :])
    alone_single_again = single(pts[:, None, :])
    alone_batch = batch(pts.reshape(40, 3, 2))
    alone_batch_again = batch(pts.reshape(40, 3, 2))
    np.testing.assert_array_equal(alone_single, alone_single_again)
    np.testing.assert_array_equal(alone_batch, alone_batch_again)
    for _ in range(3):
        np.testing.assert_array_equal(single(pts[:, None, :]), alone_single)
        np.testing.assert_array_equal(batch(pts.reshape(40, 3, 2)), alone_batch)
    assert np.any(alone_single > 0.0) and np.any(alone_batch > 0.0)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_carry_their_code_and_leave_the_handle_as_it_was():
    E = _E()
    L = E._lib
    lib = L.load()
    rng = np.random.default_rng(50)
    P, q, S, G, d = 2, 3, 10, 7, 3
    engines = T.mixed_stack(("matern52", "rbf"), 40, d, seed=51)
    lead = engines[0]
    E.ehvi_set_partition_tables(lead, *table_partition(rng, P, 6, 9))
    mean, cov = T.random_moments(rng, P, G, q)
    eps = rng.standard_normal((P, q, S))
    Xq = rng.uniform(size=(G, q, d))
    out = np.empty(G)
    base_m, base_v = E.qehvi_moments(lead, mean, cov, eps), E.qehvi_values(engines, Xq, eps)

    def unchanged():
        np.testing.assert_array_equal(E.qehvi_moments(lead, mean, cov, eps), base_m)
        np.testing.assert_array_equal(E.qehvi_values(engines, Xq, eps), base_v)

    def moments_rc(eng, q_=q, S_=S, jitter=1e-6):
        return lib.tgp_qehvi_moments(eng._h, mean.ctypes.data, cov.ctypes.data, G, q_, eps.ctypes.data, S_, jitter,
                                     out.ctypes.data, L.HOST)

    def values_rc(engs, q_=q, S_=S, jitter=1e-6):
        _, hs = E._handles(engs)
        return lib.tgp_qehvi_values(hs, len(engs), Xq.ctypes.data, G, q_, eps.ctypes.data, S_, jitter, out.ctypes.data, L.HOST)

    def message(eng):
        return lib.tgp_last_error(eng._h).decode()

    for call, eng in ((lambda **k: moments_rc(lead, **k), lead), (lambda **k: values_rc(engines, **k), lead)):
        for kwargs, code in ((dict(q_=0), L.TGP_ERR_SHAPE), (dict(q_=9), L.TGP_ERR_SHAPE), (dict(S_=0), L.TGP_ERR_ARG),
                             (dict(jitter=-1e-9), L.TGP_ERR_ARG)):
            assert call(**kwargs) == code and message(eng).strip(), kwargs
            unchanged()
    with pytest.raises(ValueError):   # the wrappers turn both codes into ValueError
        E.qehvi_moments(lead, *T.random_moments(rng, P, 2, 9), rng.standard_normal((P, 9, 4)))
    # no partition
    bare = _bare_engine(d)
    assert moments_rc(bare) == L.TGP_ERR_STATE and "partition" in message(bare)
    with pytest.raises(RuntimeError):
        E.qehvi_moments(bare, mean, cov, eps)
    others = T.mixed_stack(("matern52", "rbf"), 30, d, seed=52)
    assert values_rc(others) == L.TGP_ERR_STATE and "partition" in message(others[0])
    # P different from the partition's
    three = engines + [others[0]]
    assert values_rc(three) == L.TGP_ERR_ARG and "objectives" in message(lead)
    unchanged()
    # a handle without data; handles of different d
    empty = E.GPEngine(d, "matern52", device=0)
    assert values_rc([lead, empty]) == L.TGP_ERR_STATE and "no data" in message(lead)
    unchanged()
    narrow = T.mixed_stack(("matern52",), 30, d - 1, seed=53)[0]
    assert values_rc([lead, narrow]) == L.TGP_ERR_ARG and "dimension" in message(lead)
    unchanged()
    # two identical points in batch 4, jitter = 0: rows 0 and 2 of its covariances coincide (entries chosen so that the
    # factorisation's pivot is exactly 0: 0.25 = 0.5^2)
    bad = cov.copy()
    for j in range(P):
        c = 0.1 + 0.01 * j
        bad[j, 4] = [[0.25, c, 0.25], [c, 0.5, c], [0.25, c, 0.25]]
    rc = lib.tgp_qehvi_moments(lead._h, mean.ctypes.data, bad.ctypes.data, G, q, eps.ctypes.data, S, 0.0, out.ctypes.data, L.HOST)
    assert rc == L.TGP_ERR_NOT_PD and "group 4" in message(lead), message(lead)
    with pytest.raises(L.NotPositiveDefiniteError, match="group 4"):
        E.qehvi_moments(lead, mean, bad, eps, jitter=0.0)
    assert np.all(np.isfinite(E.qehvi_moments(lead, mean, bad, eps, jitter=1e-6)))   # (with the jitter it factorises)
    unchanged()


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_ego_with_batch_ehvi_on_vlmop2():
    """EfficientGlobalOptimization(BatchMonteCarloExpectedHypervolumeImprovement(64), num_query_points=3) in the Ask-Tell loop
    for three rounds on VLMOP2 (d = 2) from 10 Sobol points, through ``batchify_joint`` and the default optimizer."""
    import trieste_amd
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import BatchMonteCarloExpectedHypervolumeImprovement, EfficientGlobalOptimization, Pareto
    from trieste_amd.ask_tell_optimization import AskTellOptimizer
    from trieste_amd.data import Dataset

    trieste_amd.set_seed(4321)
    space, data, stack = _vlmop2_stack()
    rule = EfficientGlobalOptimization(BatchMonteCarloExpectedHypervolumeImprovement(64), num_query_points=3)
    opt = AskTellOptimizer(space, data, stack, rule)
    ref = np.array([1.1, 1.1])
    hv = [Pareto(data.observations).hypervolume_indicator(ref)]
    for _ in range(3):
        batch = opt.ask()
        assert batch.shape == (3, 2) and np.all(space.lower <= batch) and np.all(batch <= space.upper)
        fn = rule.acquisition_function
        value = float(fn(batch[None])[0, 0])
        observed = opt.dataset.query_points
        copies = fn(np.repeat(observed[:, None, :], 3, axis=1))[:, 0]      # three copies of every observed point
        print(f"value at the batch {value:.5f}; best batch of three copies of an observed point {copies.max():.5f}")
        assert np.isfinite(value) and value >= copies.max()
        opt.tell(Dataset(batch, OBJ.vlmop2(batch, 2)))
        hv.append(Pareto(opt.dataset.observations).hypervolume_indicator(ref))
    print("hypervolume per round:", " ".join(f"{h:.4f}" for h in hv))
    assert all(b >= a - 1e-15 for a, b in zip(hv, hv[1:]))
