"""GPU: the expected hypervolume improvement -- the tail kernel against 50-digit goldens and the numpy restatement of the
reference's formula, across the shapes at which it changes path, purity (bit-identity across calls, sub-ranges and poisoned
allocations), composition with every engine's own ``predict``, the arg-max, the refusals, and the rule end to end.

Tolerance of the comparisons on given moments: both sides are float64 evaluations of one formula.  The restatement's own
worst error against the goldens is RESTATEMENT_WORST of ``abs_terms`` (tests/test_ehvi_reference.py); the kernel gets 100 x
that -- its erfc and exp are a few ulp where scipy's are below one, and there are at most four factors -- relative to the
scale, not to the (cancelling) value.

C below is the kernel's documented tile width: the largest power of two <= 64 with 8 P V C bytes <= 160 KiB; its 1024 threads
are C lanes x S = 1024 / C slices of the cell list."""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import ehvi_reference as R
from tests import ehvi_tour as T
from tests.test_ehvi_reference import RESTATEMENT_WORST, front_2d, front_3d, load_cases
from tests.util import record_margin

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL_TOL = 100.0 * RESTATEMENT_WORST


def _E():
    from trieste_amd import engine as E

    return E


def _bare_engine(d=2):
    return _E().GPEngine(d, "matern52", device=0)


def _check(what, got, want, scale):
    got, want, scale = (np.asarray(a, np.float64) for a in (got, want, scale))
    assert got.shape == want.shape and np.all(np.isfinite(got))
    err, tol = np.abs(got - want), KERNEL_TOL * scale
    worst = record_margin(what, err, tol)
    print(f"{what}: worst {worst:.3f} of the tolerance ({KERNEL_TOL:.1e} of the scale)")
    assert np.all(err <= tol), (what, float(np.max(err / scale)))


# ---- goldens and restatement ---------------------------------------------------------------------------------------------
def test_moments_entry_matches_the_mpmath_goldens():
    """Every golden, the tail cases included (values down to 1e-288)."""
    E = _E()
    eng = _bare_engine()
    for n, c in enumerate(load_cases()):
        E.ehvi_set_partition(eng, c["lb"], c["ub"])
        got = E.ehvi_moments(eng, c["mean"][:, None], c["var"][:, None])
        print(f"case {n:2d} {c['note']:50s} value {c['value']: .6e} device {got[0]: .6e}")
        _check(f"golden {n} ({c['note']})", got, [c["value"]], [c["abs_terms"]])
        assert got[0] > 0.0


def test_moments_entry_matches_the_restatement_on_random_moments():
    """The reference's own formula as the yardstick, on moments that are not in the tail by construction."""
    from trieste_amd.acquisition import prepare_default_non_dominated_partition_bounds

    E = _E()
    eng = _bare_engine()
    rng = np.random.default_rng(21)
    for front, ref in (front_2d(), front_3d()):
        lb, ub = prepare_default_non_dominated_partition_bounds(ref, front)
        mean, var, kept = R.random_moments(rng, front, ref, 700, lb, ub)
        print(f"P={front.shape[1]}: {100 * kept:.0f} % of the draws kept")
        assert kept >= 0.2
        assert np.all(R.within_sigmas_of_front(mean, var, front, 4.0))
        E.ehvi_set_partition(eng, lb, ub)
        got = E.ehvi_moments(eng, mean.T, var.T)
        _check(f"restatement P={front.shape[1]} K={len(lb)}", got, R.reference_form(mean, var, lb, ub), R.scale(mean, var, lb, ub))


# ---- shapes --------------------------------------------------------------------------------------------------------------
def _dense_reference(bounds, lo, hi, mean, var):
    cols = np.arange(bounds.shape[0])[None]
    lb, ub = bounds[cols, lo], bounds[cols, hi]
    return R.g_difference_form(mean.T, var.T, lb, ub), R.scale(mean.T, var.T, lb, ub)


# per P: two small tables, both sides of the first change of tile width (C = 64 -> 32), and the largest table
SHAPES = [(P, V) for P, edge in ((2, 160), (3, 106), (4, 80)) for V in (2, 3, 64, 65, edge, edge + 1, 512)]


@pytest.mark.parametrize("P,V", SHAPES)
def test_shapes_where_the_kernel_changes_path(P, V):
    """Cell counts around the slice count S (a slice with no cell, one cell, two), candidate counts around the tile width C
    and the wave width, several workgroups: against the numpy g-difference form (pinned by the goldens, tails included), and
    every smaller call bit-equal to the head of the largest."""
    E = _E()
    C = 64
    while 8 * P * V * C > 160 * 1024:   # the documented rule
        C //= 2
    assert C == E.ehvi_tile_width(P, V) and C in ((64,) if V <= 64 else (8, 16, 32, 64))
    S = 1024 // C
    eng = _bare_engine()
    rng = np.random.default_rng(100 * P + V)
    Ms = sorted({1, 63, 64, 65, max(C - 1, 1), C + 1, 257, 5000})
    # (standard deviations of 0.1 .. 1 against bounds and means in [0, 1]: at most 10 sigma out, where the float64 yardstick --
    # scipy's erfc is off by 1e-14 relatively at 36 sigma -- is good to 1e-15 and no product passes through subnormals;
    # the far tails are the goldens' to test)
    mean, var = rng.uniform(0.0, 1.0, (P, 5000)), 10.0 ** rng.uniform(-2, 0, (P, 5000))
    for K in (1, 2, S - 1, S + 1):
        bounds, nb, lo, hi = T.table_partition(rng, P, V, K)
        E.ehvi_set_partition_tables(eng, bounds, nb, lo, hi)
        full = E.ehvi_moments(eng, mean, var)
        want, scale = _dense_reference(bounds, lo, hi, mean, var)
        assert np.all(np.isfinite(scale)) and scale.min() > 1e-250
        _check(f"P={P} V={V} K={K} M=5000", full, want, scale)
        for M in Ms[:-1]:
            part = E.ehvi_moments(eng, np.ascontiguousarray(mean[:, :M]), np.ascontiguousarray(var[:, :M]))
            np.testing.assert_array_equal(part, full[:M], err_msg=f"P={P} V={V} K={K} M={M}")


@pytest.mark.parametrize("P,n,ref", [(3, 40, 1.1), (4, 12, 1.1)])
def test_partitions_of_real_fronts(P, n, ref):
    """A 3-D front of about 40 points (about 1 500 cells, every slice many cells deep) and a 4-D front of 12 points."""
    from trieste_amd.acquisition import Pareto, prepare_default_non_dominated_partition_bounds

    E = _E()
    rng = np.random.default_rng(P)
    w = rng.dirichlet(np.ones(P), size=4 * n)
    front = Pareto(0.1 + 0.8 * w ** 2 / np.sum(w ** 2, axis=1, keepdims=True)).front[:n]
    reference = np.full(P, ref)
    lb, ub = prepare_default_non_dominated_partition_bounds(reference, front)
    print(f"P={P}: front of {len(front)} points, {len(lb)} cells")
    assert len(front) == n and (P != 3 or 500 <= len(lb) <= 5000)
    eng = _bare_engine()
    E.ehvi_set_partition(eng, lb, ub)
    M = 300
    mean, var = rng.uniform(0.0, 1.2, (M, P)), 10.0 ** rng.uniform(-2, 0, (M, P))   # (at most 12 sigma out, as above)
    assert R.scale(mean, var, lb, ub).min() > 1e-250
    got = E.ehvi_moments(eng, mean.T, var.T)
    _check(f"front P={P} K={len(lb)}", got, R.g_difference_form(mean, var, lb, ub), R.scale(mean, var, lb, ub))


# ---- purity --------------------------------------------------------------------------------------------------------------
def test_values_are_pure_functions_of_moments_and_partition():
    """A sub-range of the candidates, taken anywhere, equals the corresponding slice of the whole call bit for bit; so does a
    repeated call."""
    E = _E()
    eng = _bare_engine()
    rng = np.random.default_rng(7)
    for P, V, K in ((2, 30, 50), (3, 120, 900), (4, 512, 300)):
        E.ehvi_set_partition_tables(eng, *T.table_partition(rng, P, V, K))
        mean, var = rng.uniform(0.0, 1.0, (P, 3000)), 10.0 ** rng.uniform(-5, 0, (P, 3000))
        full = E.ehvi_moments(eng, mean, var)
        np.testing.assert_array_equal(E.ehvi_moments(eng, mean, var), full)
        for a, b in ((0, 1), (1, 66), (37, 2999), (1500, 1564), (2936, 3000)):
            sub = E.ehvi_moments(eng, np.ascontiguousarray(mean[:, a:b]), np.ascontiguousarray(var[:, a:b]))
            np.testing.assert_array_equal(sub, full[a:b], err_msg=f"P={P} [{a}, {b})")


def test_tour_under_poisoned_allocations():
    """TGP_POISON=1 fills every fresh device allocation of the library with NaNs: the tour of tests/ehvi_tour.py in a fresh
    child process under it, and here, must agree bit for bit.  The child's timeout is a safety cap; a child that hangs or
    dies on a signal ends the session, so that nothing else is started on a GPU that has just faulted."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tour.npz")
        env = dict(os.environ, TGP_POISON="1")
        try:
            child = subprocess.run([sys.executable, "-m", "tests.ehvi_tour", out], env=env, cwd=ROOT, timeout=120,
                                   capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:
            pytest.exit(f"the poisoned tour hung (120 s cap); stderr:\n{(e.stderr or b'')[-4000:]}", returncode=1)
        if child.returncode < 0 or child.returncode in (134, 139):
            pytest.exit(f"the poisoned tour died with {child.returncode}; stderr:\n{child.stderr[-4000:]}", returncode=1)
        assert child.returncode == 0, f"poisoned tour exited with {child.returncode}:\n{child.stderr[-4000:]}"
        with np.load(out) as z:
            poisoned = {k: z[k] for k in z.files}
    plain = T.tour()
    assert sorted(plain) == sorted(poisoned) and len(plain) >= 13
    for key, value in plain.items():
        assert np.all(np.isfinite(value)), key
        np.testing.assert_array_equal(poisoned[key], value, err_msg=key)


# ---- composition ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d,kernel,P", [(40, 2, "matern52", 2), (300, 6, "rbf", 3), (300, 2, "rbf", 2), (40, 6, "matern52", 4)])
def test_values_compose_every_engines_own_predict(N, d, kernel, P):
    """ehvi_values(engines, Xq) == ehvi_moments of each engine's predict(Xq), bit for bit: at 100 points (the small-product
    path), 2049 and 5000 (the sweep).  The posterior itself is pinned by the parity suites."""
    E = _E()
    engines = T.stack_engines(P, N, d, kernel, seed=N + d)
    rng = np.random.default_rng(N * d)
    E.ehvi_set_partition_tables(engines[0], *T.table_partition(rng, P, 30, 120))
    for M in (100, 2049, 5000):
        Xq = rng.uniform(size=(M, d))
        moments = [eng.predict(Xq) for eng in engines]
        mean, var = np.stack([m for m, _ in moments]), np.stack([v for _, v in moments])
        want = E.ehvi_moments(engines[0], mean, var)
        got = E.ehvi_values(engines, Xq)
        np.testing.assert_array_equal(got, want, err_msg=f"M={M}")
        assert np.all(np.isfinite(got)) and np.any(got > 0.0)
    import torch

    Xd = torch.as_tensor(Xq).to("cuda:0")   # device-resident candidates: a CUDA tensor comes back
    np.testing.assert_array_equal(E.ehvi_values(engines, Xd).cpu().numpy(), want)


# ---- arg-max -------------------------------------------------------------------------------------------------------------
def test_argmax_is_the_first_maximum_of_the_values():
    E = _E()
    engines = T.stack_engines(2, 50, 3, "matern52", seed=9)
    rng = np.random.default_rng(9)
    E.ehvi_set_partition_tables(engines[0], *T.table_partition(rng, 2, 12, 40))
    for M in (1, 200, 5000):
        Xq = rng.uniform(size=(M, 3))
        vals = E.ehvi_values(engines, Xq)
        w = int(np.argmax(vals))
        v, i, x = E.ehvi_argmax(engines, Xq)
        assert (v, i) == (vals[w], w)
        np.testing.assert_array_equal(x, Xq[w])
        v2, i2, x2 = E.ehvi_argmax(engines, Xq, index_base=1000)
        assert (v2, i2) == (v, 1000 + w)
        np.testing.assert_array_equal(x2, Xq[w])
        # the winner duplicated behind and in front of the set: the first index wins
        dup = np.concatenate([Xq[w:w + 1], Xq, Xq[w:w + 1]])
        vd, idd, _ = E.ehvi_argmax(engines, dup)
        assert (vd, idd) == (v, 0) and int(np.argmax(E.ehvi_values(engines, dup))) == 0
        tail = np.concatenate([Xq, Xq[w:w + 1]])
        assert E.ehvi_argmax(engines, tail)[1] == w
    with pytest.raises(ValueError):
        E.ehvi_argmax(engines, np.zeros((0, 3)))


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
    return space, data, M.TrainableModelStack(*[(m, 1) for m in members])


def test_function_object_on_the_device():
    """__call__ against the engine entry, argmax against the values, argmax_sampled against argmax on the same Philox sample,
    update returning new values on the same object, and the optimizers finding the fused path."""
    import trieste_amd
    from trieste_amd.acquisition import (ExpectedHypervolumeImprovement, automatic_optimizer_selector,
                                         generate_random_search_optimizer)

    E = _E()
    space, data, stack = _vlmop2_stack()
    builder = ExpectedHypervolumeImprovement()
    fn = builder.prepare_acquisition_function(stack, data)
    engines = [m.engine for m in stack._models]
    assert fn._engine is engines[0]
    pts = space.sample(500, seed=3)
    vals = fn(pts[:, None, :])
    assert vals.shape == (500, 1) and np.all(vals >= 0.0) and np.any(vals > 0.0)
    np.testing.assert_array_equal(vals[:, 0], E.ehvi_values(engines, pts))
    assert fn(pts.reshape(5, 100, 1, 2)).shape == (5, 100, 1)
    v, i, x = fn.argmax(pts)
    assert (v, i) == (vals.max(), int(np.argmax(vals[:, 0])))
    sampled = fn.argmax_sampled(17, 3000, space.lower, space.upper)
    box = engines[0].sample_box(17, 0, 3000, space.lower, space.upper)
    direct = fn.argmax(box)
    assert sampled[:2] == direct[:2]
    np.testing.assert_array_equal(sampled[2], direct[2])
    # a second function object over the same stack takes the engine's partition; the first reinstalls its own
    other = ExpectedHypervolumeImprovement([5.0, 5.0]).prepare_acquisition_function(stack, data)
    assert np.any(other(pts[:, None, :]) != vals)
    np.testing.assert_array_equal(fn(pts[:, None, :]), vals)
    assert builder.update_acquisition_function(fn, stack, data) is fn
    trieste_amd.set_seed(1)
    for optimizer in (generate_random_search_optimizer(2000, seed=4), automatic_optimizer_selector):
        point = optimizer(space, fn)
        assert point.shape == (1, 2) and np.all(space.lower <= point) and np.all(point <= space.upper)
        assert fn(point[:, None, :])[0, 0] >= np.quantile(vals, 0.9)


def test_a_new_function_object_never_inherits_a_dropped_ones_partition():
    """Function objects built, used and dropped one after another inside a helper (CPython hands the next one the same id):
    each evaluates on its OWN partition -- equal to the engine entry with that partition installed by hand -- and a partition
    installed by hand behind a live object's back is replaced by the object's on its next call."""
    import gc

    from trieste_amd.acquisition import expected_hv_improvement, prepare_default_non_dominated_partition_bounds

    E = _E()
    space, data, stack = _vlmop2_stack()
    engines = [m.engine for m in stack._models]
    pts = space.sample(300, seed=8)
    front = np.array([[0.3, 0.8], [0.6, 0.5], [0.9, 0.2]])

    def step(ref):
        fn = expected_hv_improvement(stack, prepare_default_non_dominated_partition_bounds(np.full(2, ref), front))
        return fn(pts[:, None, :])[:, 0], fn.argmax(pts)[:2]

    results = []
    for ref in (1.0, 2.0, 3.0, 4.0):
        results.append(step(ref))
        gc.collect()
    for ref, (vals, best) in zip((1.0, 2.0, 3.0, 4.0), results):
        E.ehvi_set_partition(engines[0], *prepare_default_non_dominated_partition_bounds(np.full(2, ref), front))
        want = E.ehvi_values(engines, pts)
        np.testing.assert_array_equal(vals, want, err_msg=f"reference point {ref}")
        assert best == (want.max(), int(np.argmax(want)))
    assert all(np.any(results[i][0] != results[i + 1][0]) for i in range(3))
    fn = expected_hv_improvement(stack, prepare_default_non_dominated_partition_bounds(np.full(2, 1.5), front))
    own = fn(pts[:, None, :])
    E.ehvi_set_partition(engines[0], *prepare_default_non_dominated_partition_bounds(np.full(2, 4.0), front))
    np.testing.assert_array_equal(fn(pts[:, None, :]), own)


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals_carry_a_message():
    E = _E()
    lib = E._lib.load()
    rng = np.random.default_rng(0)

    def refused(exc, call, *args):
        with pytest.raises(exc) as info:
            call(*args)
        assert str(info.value).strip(), (call, args)

    eng = _bare_engine()
    for P in (1, 5):   # objectives outside 2 .. 4
        b, n, lo, hi = T.table_partition(rng, P, 4, 3)
        refused(ValueError, E.ehvi_set_partition_tables, eng, b, n, lo, hi)
    b, n, lo, hi = T.table_partition(rng, 2, 513, 3)   # 513 bounds per objective
    refused(ValueError, E.ehvi_set_partition_tables, eng, b, n, lo, hi)
    b, n, lo, hi = T.table_partition(rng, 3, 6, 5)
    bad = hi.copy()
    bad[2, 1] = 6                                       # an index out of range
    refused(ValueError, E.ehvi_set_partition_tables, eng, b, n, lo, bad)
    bad = lo.copy()
    bad[0, 0] = -1
    refused(ValueError, E.ehvi_set_partition_tables, eng, b, n, bad, hi)
    refused(ValueError, E.ehvi_set_partition_tables, eng, b, n, hi, lo)   # lower above upper
    unsorted = b.copy()
    unsorted[1, 2:4] = unsorted[1, 3:1:-1]
    refused(ValueError, E.ehvi_set_partition_tables, eng, unsorted, n, lo, hi)
    # no partition set (a refused call leaves none behind; K = 0 clears one)
    mean, var = np.zeros((3, 4)), np.ones((3, 4))
    refused(RuntimeError, E.ehvi_moments, eng, mean, var)
    E.ehvi_set_partition_tables(eng, b, n, lo, hi)
    assert E.ehvi_moments(eng, mean, var).shape == (4,)
    E.ehvi_set_partition(eng, None, None)
    refused(RuntimeError, E.ehvi_moments, eng, mean, var)
    # stacks: no partition on the leading handle, a handle without data, handles of different d, the wrong count
    engines = T.stack_engines(3, 20, 2, "matern52", seed=1)
    Xq = rng.uniform(size=(10, 2))
    refused(RuntimeError, E.ehvi_values, engines, Xq)
    refused(RuntimeError, E.ehvi_argmax, engines, Xq)
    E.ehvi_set_partition_tables(engines[0], b, n, lo, hi)
    assert E.ehvi_values(engines, Xq).shape == (10,)
    refused(RuntimeError, E.ehvi_values, [engines[0], _bare_engine(2), engines[2]], Xq)
    refused(ValueError, E.ehvi_values, [engines[0], engines[1], T.stack_engines(1, 20, 3, "matern52", seed=2)[0]], Xq)
    refused(ValueError, E.ehvi_values, engines[:2], Xq)
    refused(ValueError, E.ehvi_values, engines[:1], Xq)
    refused(ValueError, E.ehvi_values, engines + engines[:2], Xq)
    assert lib.tgp_last_error(engines[0]._h)


# ---- end to end ----------------------------------------------------------------------------------------------------------
def test_ego_with_ehvi_on_vlmop2():
    """EfficientGlobalOptimization(ExpectedHypervolumeImprovement()) in the Ask-Tell loop for 10 steps on VLMOP2 (d = 2) from
    10 Sobol points: the hypervolume of the observations against the fixed reference point [1.1, 1.1] never decreases (true of
    any growing set), ends strictly above where it started, and the function object is one instance throughout."""
    import trieste_amd
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import EfficientGlobalOptimization, ExpectedHypervolumeImprovement, Pareto
    from trieste_amd.ask_tell_optimization import AskTellOptimizer
    from trieste_amd.data import Dataset

    trieste_amd.set_seed(1234)
    space, data, stack = _vlmop2_stack()
    rule = EfficientGlobalOptimization(ExpectedHypervolumeImprovement())
    opt = AskTellOptimizer(space, data, stack, rule)
    ref = np.array([1.1, 1.1])
    hv = [Pareto(data.observations).hypervolume_indicator(ref)]
    functions = set()
    for _ in range(10):
        q = opt.ask()
        assert q.shape == (1, 2)
        functions.add(id(rule.acquisition_function))
        opt.tell(Dataset(q, OBJ.vlmop2(q, 2)))
        hv.append(Pareto(opt.dataset.observations).hypervolume_indicator(ref))
    print("hypervolume per step:", " ".join(f"{h:.4f}" for h in hv))
    assert all(b >= a - 1e-15 for a, b in zip(hv, hv[1:]))
    assert hv[-1] > hv[0]
    assert len(functions) == 1
