"""CPU: the multi-objective host layer -- the non-dominated filter, the Pareto set and its hypervolume, both partitions of
the non-dominated region (covering property, volumes), the default reference point, the error cases, the model stacks
(over engine-backed models with the engine replaced by tests/fakes.py::FakeEngine) and the VLMOP2 objective."""
import numpy as np
import pytest

import trieste_amd.models as M
from tests.fakes import FakeEngine
from trieste_amd import objectives as OBJ
from trieste_amd.acquisition import (DividedAndConquerNonDominated, ExactPartition2dNonDominated,
                                     ExpectedHypervolumeImprovement, Pareto, expected_hv_improvement, get_reference_point,
                                     non_dominated, prepare_default_non_dominated_partition_bounds)
from trieste_amd.data import Dataset
from trieste_amd.engine import ehvi_partition_tables, ehvi_tile_width
from trieste_amd.space import Box


@pytest.fixture(autouse=True)
def fake_engine(monkeypatch):
    monkeypatch.setattr(M, "GPEngine", FakeEngine)


# ---- dominance ---------------------------------------------------------------------------------------------------------
def test_non_dominated_on_hand_made_sets():
    obs = np.array([[0.0, 1.0], [1.0, 0.0], [0.5, 0.5], [0.5, 0.5], [0.6, 0.6], [0.0, 1.0], [0.0, 2.0], [2.0, 0.0], [1.0, 1.0]])
    front, mask = non_dominated(obs)
    # duplicates of a non-dominated point stay; a tie in one objective with a worse other objective is dominated
    assert mask.tolist() == [True, True, True, True, False, True, False, False, False]
    np.testing.assert_array_equal(front, obs[mask])
    one, m1 = non_dominated(np.array([[3.0, 4.0, 5.0]]))
    assert one.shape == (1, 3) and m1.tolist() == [True]
    same, ms = non_dominated(np.ones((4, 3)))
    assert same.shape == (4, 3) and ms.all()
    chain, mc = non_dominated(np.array([[1.0, 1.0, 1.0], [2.0, 2.0, 2.0], [1.0, 1.0, 2.0]]))
    assert mc.tolist() == [True, False, False]
    rng = np.random.default_rng(0)
    pts = rng.uniform(size=(200, 3))
    front, mask = non_dominated(pts)
    brute = np.array([not np.any(np.all(pts <= p, axis=1) & np.any(pts < p, axis=1)) for p in pts])
    assert mask.tolist() == brute.tolist()
    with pytest.raises(ValueError):
        non_dominated(np.zeros(3))


# ---- partitions ----------------------------------------------------------------------------------------------------------
def _front(P, n, seed):
    """A front of exactly n points: points of the unit sphere's positive orthant (a <= b componentwise and a != b would
    give |a| < |b|, so none dominates another), scaled into [0.1, 0.9]."""
    g = np.abs(np.random.default_rng(seed).standard_normal((n, P)))
    front = 0.1 + 0.8 * g / np.linalg.norm(g, axis=1, keepdims=True)
    assert np.all(non_dominated(front)[1])
    return front


FRONTS = [(P, n) for P in (2, 3) for n in (1, 2, 7, 25)] + [(4, n) for n in (1, 2, 7, 12)]


@pytest.mark.parametrize("P,n", FRONTS)
def test_partitions_cover_the_non_dominated_region_exactly_once(P, n):
    """Over 2e4 uniform points of the box [anti-reference, reference]: a point the front dominates lies in no cell, every
    other point in exactly one (half-open cells [lb, ub)); and the cells' volumes add up to the box minus the dominated
    hypervolume.  The divide-and-conquer partition is checked for P = 2 as well, against the exact one."""
    front = _front(P, n, seed=10 * P + n)
    assert len(front) == n
    ref, anti = np.full(P, 1.05), np.full(P, -0.25)
    partitions = [prepare_default_non_dominated_partition_bounds(ref, front, anti)]
    if P == 2:
        partitions.append(DividedAndConquerNonDominated(front).partition_bounds(anti, ref))
        np.testing.assert_array_equal(partitions[0][0], ExactPartition2dNonDominated(front).partition_bounds(anti, ref)[0])
    rng = np.random.default_rng(n)
    pts = rng.uniform(anti, ref, size=(20000, P))
    dominated = np.any(np.all(front[None] <= pts[:, None, :], axis=-1), axis=-1)
    assert 0 < dominated.sum() < len(pts)
    hv = Pareto(front).hypervolume_indicator(ref)
    for lb, ub in partitions:
        assert lb.shape == ub.shape and lb.shape[1] == P and np.all(lb <= ub)
        inside = np.zeros(len(pts), dtype=int)
        for lo, up in zip(lb, ub):
            inside += np.all((lo <= pts) & (pts < up), axis=-1)
        assert np.all(inside[dominated] == 0)
        assert np.all(inside[~dominated] == 1)
        box = np.prod(ref - anti)
        assert abs(np.sum(np.prod(ub - lb, axis=1)) - (box - hv)) <= 1e-12 * box
        # every bound is a pseudo-front value: at most F + 2 distinct ones per objective (what the device tables rest on)
        bounds, nb, li, ui = ehvi_partition_tables(lb, ub)
        assert np.all(nb <= len(front) + 2) and np.all(li <= ui)
        np.testing.assert_array_equal(bounds[np.arange(P)[None], li], lb)
        np.testing.assert_array_equal(bounds[np.arange(P)[None], ui], ub)


def test_two_objective_hypervolume_is_the_staircase_sum():
    front = _front(2, 25, seed=3)
    ref = np.array([1.2, 1.1])
    s = front[np.argsort(front[:, 0])]
    heights = np.concatenate([[ref[1]], s[:-1, 1]]) - s[:, 1]
    staircase = np.sum((ref[0] - s[:, 0]) * heights)
    assert abs(Pareto(front).hypervolume_indicator(ref) - staircase) <= 1e-13
    assert Pareto(np.array([[0.0, 0.0]])).hypervolume_indicator([2.0, 3.0]) == pytest.approx(6.0, abs=1e-14)
    # dominated observations do not change it; already_non_dominated takes the set as it is
    extra = np.concatenate([front, front + 0.01])
    assert Pareto(extra).hypervolume_indicator(ref) == pytest.approx(staircase, abs=1e-13)
    np.testing.assert_array_equal(Pareto(front, already_non_dominated=True).front, front)
    np.testing.assert_array_equal(Pareto(extra, already_non_dominated=True).front, extra)   # taken as it is, unfiltered


def test_threshold_drops_small_undecided_boxes():
    front = _front(3, 25, seed=4)
    ref, anti = np.full(3, 1.05), np.full(3, -0.25)
    exact = DividedAndConquerNonDominated(front).partition_bounds(anti, ref)
    coarse = DividedAndConquerNonDominated(front, threshold=1e-2).partition_bounds(anti, ref)
    assert 0 < len(coarse[0]) < len(exact[0])
    assert np.sum(np.prod(coarse[1] - coarse[0], axis=1)) < np.sum(np.prod(exact[1] - exact[0], axis=1))


def test_get_reference_point_on_a_known_front():
    obs = np.array([[1.0, 4.0], [2.0, 2.0], [4.0, 1.0], [3.0, 3.0], [5.0, 5.0]])
    # front: the first three; max + 2 (max - min) / 3
    np.testing.assert_allclose(get_reference_point(obs), [4.0 + 2.0, 4.0 + 2.0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(get_reference_point(np.array([[1.0, 2.0, 3.0]])), [1.0, 2.0, 3.0])
    with pytest.raises(ValueError, match="empty observations"):
        get_reference_point(np.zeros((0, 2)))


def test_empty_branches_and_error_cases():
    ref = np.array([1.0, 2.0, 3.0])
    for obs in (None, np.zeros((0, 3))):
        lb, ub = prepare_default_non_dominated_partition_bounds(ref, obs)
        np.testing.assert_array_equal(lb, [[-1e10] * 3])
        np.testing.assert_array_equal(ub, [ref])
    lb, ub = prepare_default_non_dominated_partition_bounds(ref, None, np.array([0.0, 0.0, 0.0]))
    np.testing.assert_array_equal(lb, [[0.0] * 3])
    with pytest.raises(ValueError, match="larger than reference"):
        prepare_default_non_dominated_partition_bounds(ref, None, np.array([0.0, 5.0, 0.0]))
    with pytest.raises(ValueError, match="below default anti-reference"):
        prepare_default_non_dominated_partition_bounds(np.array([1.0, -2e10]), None)
    with pytest.raises(ValueError, match="below default anti-reference"):
        prepare_default_non_dominated_partition_bounds(np.array([1.0, 1.0]), np.array([[0.5, -2e10]]))
    with pytest.raises(ValueError):
        prepare_default_non_dominated_partition_bounds(np.ones((2, 2)), None)
    with pytest.raises(ValueError):
        prepare_default_non_dominated_partition_bounds(np.ones(2), None, np.zeros((1, 2)))
    front = np.array([[0.2, 0.8], [0.8, 0.2]])
    with pytest.raises(ValueError):   # a front point beyond the reference point
        prepare_default_non_dominated_partition_bounds(np.array([0.5, 1.0]), front)
    with pytest.raises(ValueError):   # ... or below the anti-reference point
        ExactPartition2dNonDominated(front).partition_bounds(np.array([0.5, 0.0]), np.array([1.0, 1.0]))
    for cls in (ExactPartition2dNonDominated, DividedAndConquerNonDominated):
        with pytest.raises(ValueError, match="contains dominated points"):
            cls(np.array([[0.2, 0.2], [0.5, 0.5]]))
    with pytest.raises(ValueError):
        ExactPartition2dNonDominated(np.array([[0.1, 0.2, 0.3]]))
    with pytest.raises(ValueError):
        Pareto(np.zeros((3,)))
    with pytest.raises(ValueError):
        Pareto(np.zeros((3, 1)))
    with pytest.raises(ValueError, match="empty front"):
        Pareto(np.zeros((0, 2))).hypervolume_indicator(np.ones(2))


def test_tile_width_rule():
    """The largest power of two <= 64 whose table of 8 P V C bytes fits 160 KiB."""
    assert [ehvi_tile_width(2, V) for V in (2, 160, 161, 320, 321, 512)] == [64, 64, 32, 32, 16, 16]
    assert [ehvi_tile_width(3, V) for V in (106, 107, 213, 214, 512)] == [64, 32, 32, 16, 8]
    assert [ehvi_tile_width(4, V) for V in (80, 81, 160, 161, 320, 321, 512)] == [64, 32, 32, 16, 16, 8, 8]


# ---- model stacks --------------------------------------------------------------------------------------------------------
def _gpr(y, x, noise=1e-3):
    data = Dataset(x, y)
    return M.GaussianProcessRegression(M.build_gpr(data, Box([0.0, 0.0], [1.0, 1.0]), likelihood_variance=noise))


def _stack(n=10, seed=0, cls=M.TrainableModelStack):
    rng = np.random.default_rng(seed)
    x = rng.uniform(size=(n, 2))
    y = np.concatenate([OBJ.scaled_branin(x), OBJ.simple_quadratic(x), np.sin(3.0 * x[:, :1])], axis=1)
    members = [_gpr(y[:, j:j + 1], x) for j in range(3)]
    return cls(*[(m, 1) for m in members]), members, Dataset(x, y)


def test_model_stack_concatenates_in_order():
    stack, members, data = _stack(cls=M.ModelStack)
    q = np.random.default_rng(1).uniform(size=(4, 5, 2))
    mean, var = stack.predict(q)
    assert mean.shape == var.shape == (4, 5, 3)
    for j, m in enumerate(members):
        mj, vj = m.predict(q)
        np.testing.assert_array_equal(mean[..., j:j + 1], mj)
        np.testing.assert_array_equal(var[..., j:j + 1], vj)
    import trieste_amd

    trieste_amd.set_seed(7)
    s = stack.sample(q[0], 6)
    assert s.shape == (6, 5, 3)
    trieste_amd.set_seed(7)
    np.testing.assert_array_equal(s[..., :1], members[0].sample(q[0], 6))
    assert stack.log(data) is None
    assert not hasattr(stack, "update")


def test_trainable_stack_splits_observations():
    stack, members, data = _stack()
    rng = np.random.default_rng(2)
    x2 = np.concatenate([data.query_points, rng.uniform(size=(3, 2))])
    y2 = np.concatenate([data.observations, rng.normal(size=(3, 3))])
    stack.update(Dataset(x2, y2))
    for j, m in enumerate(members):
        got = m.get_internal_data()
        np.testing.assert_array_equal(got.query_points, x2)
        np.testing.assert_array_equal(got.observations, y2[:, j:j + 1])
    results = stack.optimize(Dataset(x2, y2))
    assert len(results) == 3 and all(hasattr(r, "x") for r in results)
    with pytest.raises(ValueError, match="columns"):
        stack.update(Dataset(x2, y2[:, :2]))


def test_stack_refuses_other_event_sizes():
    _, members, _ = _stack()
    with pytest.raises(ValueError, match="event size"):
        M.ModelStack((members[0], 1), (members[1], 2))
    with pytest.raises(ValueError, match="event size"):
        M.TrainableModelStack((members[0], 3))


# ---- builder and function object: what needs no device -------------------------------------------------------------------
def test_builder_refusals_and_repr():
    stack, members, data = _stack()
    builder = ExpectedHypervolumeImprovement()
    assert repr(builder) == "ExpectedHypervolumeImprovement(get_reference_point)"
    assert "1.1" in repr(ExpectedHypervolumeImprovement([1.1, 1.1]))
    with pytest.raises(ValueError, match="populated"):
        builder.prepare_acquisition_function(stack, None)
    with pytest.raises(ValueError, match="populated"):
        builder.prepare_acquisition_function(stack, Dataset(np.zeros((0, 2)), np.zeros((0, 3))))
    lb, ub = prepare_default_non_dominated_partition_bounds(np.ones(3), None)
    with pytest.raises(TypeError, match="no CPU evaluation path"):   # not a stack
        expected_hv_improvement(members[0], (lb, ub))

    class NoEngine:
        def predict(self, q):
            return np.zeros(q.shape[:-1] + (1,)), np.ones(q.shape[:-1] + (1,))

    with pytest.raises(TypeError, match="no CPU evaluation path"):   # a stack of models without engines
        expected_hv_improvement(M.ModelStack((NoEngine(), 1), (NoEngine(), 1), (NoEngine(), 1)), (lb, ub))
    with pytest.raises(ValueError, match="objectives"):               # partition and stack disagree
        expected_hv_improvement(stack, (lb[:, :2], ub[:, :2]))
    fn = expected_hv_improvement(stack, (lb, ub))
    assert fn._engine is members[0].engine and not hasattr(fn, "value_and_gradient")
    for bad in (np.zeros((5, 2)), np.zeros((5, 2, 2))):
        with pytest.raises(ValueError, match="only supports batch sizes of one"):
            fn(bad)
    with pytest.raises(ValueError):
        builder.update_acquisition_function(lambda x: x, stack, data)


def test_every_function_object_installs_its_own_partition(monkeypatch):
    """Function objects built and dropped one after another (CPython reuses their ids) each install their own tables on the
    leading engine before evaluating; one that stays alive installs once per partition, and again after someone else did."""
    import gc

    import trieste_amd.engine as E

    stack, members, data = _stack()
    installs = []

    def record(engine, bounds, n_bounds, lower_idx, upper_idx):
        engine._ehvi_owner = None
        installs.append((engine, float(bounds[0, -1])))

    monkeypatch.setattr(E, "ehvi_set_partition_tables", record)

    def step(ref):
        fn = expected_hv_improvement(stack, prepare_default_non_dominated_partition_bounds(np.full(3, ref), None))
        return fn._engines()

    for ref in (1.0, 2.0, 3.0, 4.0):
        assert step(ref)[0] is members[0].engine
        gc.collect()
    assert [r for _, r in installs] == [1.0, 2.0, 3.0, 4.0] and all(e is members[0].engine for e, _ in installs)
    fn = expected_hv_improvement(stack, prepare_default_non_dominated_partition_bounds(np.full(3, 5.0), None))
    fn._engines(), fn._engines()
    assert [r for _, r in installs][4:] == [5.0]
    fn.update(prepare_default_non_dominated_partition_bounds(np.full(3, 6.0), None))
    fn._engines(), fn._engines()
    assert [r for _, r in installs][5:] == [6.0]
    record(members[0].engine, np.array([[0.0, 7.0]]), None, None, None)   # installed behind the object's back
    fn._engines()
    assert [r for _, r in installs][6:] == [7.0, 6.0]


def test_vlmop2():
    x = np.array([[0.0, 0.0], [2 ** -0.5, 2 ** -0.5], [-(2 ** -0.5), -(2 ** -0.5)]])
    y = OBJ.vlmop2(x, 2)
    assert y.shape == (3, 2)
    np.testing.assert_allclose(y[0], [1 - np.exp(-1.0), 1 - np.exp(-1.0)], rtol=1e-15)
    np.testing.assert_allclose(y[1], [0.0, 1 - np.exp(-4.0)], atol=1e-15)
    np.testing.assert_allclose(y[2], [1 - np.exp(-4.0), 0.0], atol=1e-15)
    assert OBJ.vlmop2(np.zeros((4, 5, 3)), 3).shape == (4, 5, 2)
    with pytest.raises(ValueError):
        OBJ.vlmop2(np.zeros((4, 3)), 2)
