"""CPU: the numpy side of the pruned EI arg-max on general models, and the planted defects only such models can see.

tests/prune_cases.CONFIGS has equal lengthscales, variance 1, mean 0 and the unit cube: there sigma^2, sigma and 1 are one
number, a dropped mean changes nothing and ls[0] is every lengthscale -- and the bounds the arg-max prunes by are made of
exactly these.  tests/prune_cases.GENERAL departs in all four ways at once (and one exact twin of a unit model, its
outputs scaled by 2^-10).  Every oracle call on them runs in the difference form (tests/prune_cases.form).

1. The table tests/test_gpu_prune_general.py reads (S.RECORDED_GENERAL, R.SHARE_CASE_GENERAL) is what the functions give.
2. Seed, screen and checkpoints keep the oracle's arg-max on every general model, threshold, order and lag.
3. |mean32 - mean| <= E against the long-double mean, and the restated pre-screen drops only what the exact screen drops.
4. Four planted defects, each invisible on every model of CONFIGS (bit-identical decisions) and caught by a general model
   (the oracle's winner lost, or mean32 outside E): the evidence that the GPU tests on these models can fail.
5. Which (model, threshold) pairs may carry a share condition."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import prescreen_cases as R
from tests import prune_cases as PC
from tests import prune_screen_cases as S

BOUND_M = 4096
NBLK_SAMPLE = -(-S.SAMPLE // PC.CAND_BLOCK)
GENERAL = pytest.mark.parametrize("name", PC.GENERAL_IDS)
needs_long_double = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="the reference needs an extended long double")


# ---- 1. the recorded table -------------------------------------------------------------------------------------------
def test_general_models_depart_in_every_way():
    for name in PC.GENERAL_IDS:
        p = PC.problem(name)
        assert 256 < p.N <= 768 and p.variance != 1.0 and abs(p.mean_const) > 30.0
        assert int(np.argmin(p.ls / p.width)) != 0 and np.ptp(p.ls / p.width) > 0.0
        assert np.abs(p.lo).max() >= 40.0 and p.noise == p.rel_noise * p.variance
        Xq = PC.candidates(name)
        assert Xq.shape == (PC.M, p.d) and np.all(Xq >= p.lo) and np.all(Xq <= p.lo + p.width)
    assert {R.dpad(PC.problem(n).d) for n in PC.GENERAL_IDS} >= {4, 6, 8, 16}


def test_unit_thresholds_keep_their_bits():
    p = PC.problem("m52_N512_d8")
    for eta in (-2.7182818284590451, 0.3, 1e-3):
        assert S.thresholds(p, eta) == {"eta": eta, "eta+0.5": eta + 0.5, "eta+3": eta + 3.0, "-1e6": -1e6}


def test_twin_is_the_unit_model_scaled():
    p, q = PC.problem(PC.TWIN), PC.problem(PC.TWIN_OF)
    assert np.array_equal(p.X / p.ls, q.X / q.ls) and np.array_equal(PC.candidates(PC.TWIN) / p.ls, PC.candidates(PC.TWIN_OF) / q.ls)
    assert np.array_equal(p.Y * 2.0 ** 10, q.Y) and (p.variance * 4.0 ** 10, p.noise * 4.0 ** 10, p.mean_const) == (1.0, q.noise, 0.0)
    for label in S.THRESHOLDS:
        assert S.thresholds(p, 0.37 * 2.0 ** -10)[label] * 2.0 ** 10 == S.thresholds(q, 0.37)[label]


@GENERAL
def test_recorded_general_table_is_what_the_oracle_gives(name):
    """Slow for a CPU test (means and variances of 131 149 candidates); the GPU test reads the table instead."""
    rec = S.RECORDED_GENERAL[name]
    p = PC.problem(name)
    got = {label: S.oracle_screened(name, label) for label in S.THRESHOLDS}
    print(name, got)
    assert got == rec["screened"]
    assert S.top_seed_candidate(name, "eta+3") == rec["top_seed"]
    b = S.blocks_screened_against_top_seed(name, "eta+3")
    assert (int(b[b >= S.DUP_FLOOR][0]), int(b[-1])) == rec["dup_blocks"]
    assert rec["top_seed"] // PC.CAND_BLOCK not in set(b.tolist())
    assert abs(PC.oracle_state(name)[1] - rec["eta"]) <= 1e-9 * np.sqrt(p.variance)
    idx, val = S.oracle_winner(name, "eta+0.5")
    assert idx == rec["winner"][0] and abs(val - rec["winner"][1]) <= 1e-7 * rec["winner"][1]
    assert rec["screened"]["-1e6"] == 0


def test_recorded_general_share_case():
    """On the whole plain set of the recorded case the restatement dismisses at least half of the blocks the oracle screens."""
    name, label = R.SHARE_CASE_GENERAL
    ub32, prebest, _, E = R.restated_blocks(name, label, PC.candidates(name))
    n = int(R.dismissed(ub32, prebest).sum())
    assert n == R.SHARE_DISMISSED_GENERAL
    assert 2 * n >= S.RECORDED_GENERAL[name]["screened"][label] > 0
    # what a cap E <= variance made of this model: no candidate passed it
    assert not np.any(E <= PC.problem(name).variance)


# ---- 2. the screen keeps the arg-max ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lag", [1, 256])
@pytest.mark.parametrize("order", ["identity", "reversed", "shuffled"])
@pytest.mark.parametrize("label", S.THRESHOLDS)
@GENERAL
def test_screen_keeps_the_argmax_on_general_models(name, label, order, lag):
    st, _ = PC.oracle_state(name)
    eta = S.threshold(name, label)
    mean, var = S.sample_moments(name)
    val, idx, given, screened, seed = S.sweep_with_screen(mean, var, eta, st.variance, S.orders(NBLK_SAMPLE)[order], lag)
    full = PC.ei_tail(eta - mean, var[-1])
    want = int(O.argmax_first(full))
    assert (val, idx) == (float(full[want]), want)
    assert not (screened & ~given).any()
    if seed.max() > 0.0:
        assert not screened[int(np.argmax(seed))]
    pos = eta - mean > 0.0
    assert np.all((eta - mean)[pos] <= (1.0 + S.SEED_RTOL) * full[pos])
    if label == "-1e6":
        assert not given.any() and not np.any(full > 0.0)
    if lag >= NBLK_SAMPLE:
        assert not screened.any()
    elif label == "eta+3":
        assert screened.any()                     # not vacuous: with the others' seeds known the screen acts


# ---- 3. the restated pre-screen --------------------------------------------------------------------------------------
def _bound_quantities(name, ls=None, bound_variance=None):
    """-> (m32, E, an) of the first BOUND_M plain candidates; ``ls`` / ``bound_variance`` plant defects (c) / (d)."""
    p = PC.problem(name)
    alpha = R.model_alpha(name)
    Xq = PC.candidates(name)[:BOUND_M]
    m32, an = R.restate(p.kind, p.variance, p.ls if ls is None else ls, p.X, alpha, p.mean_const, Xq)
    if ls is not None:   # the candidates' norms belong to the bound, which defect (c) leaves alone
        a = np.sqrt(R.SCALE[p.kind]) * (Xq / p.ls - (p.X / p.ls)[0])
        an = np.sqrt((a * a).sum(1))
    xmax, x0 = R.model_extent(p.kind, p.ls, p.X)
    npad = -(-p.N // PC.ROW_BLOCK) * PC.ROW_BLOCK
    E = R.bound(p.kind, p.d, npad, np.abs(alpha).sum(), p.variance if bound_variance is None else bound_variance,
                an, xmax, x0, m32, 0.0)
    return m32, E


def _true_error(name, m32):
    p = PC.problem(name)
    mean = R.true_mean(p.kind, p.variance, p.ls, p.X, R.model_alpha(name), p.mean_const, PC.candidates(name)[:BOUND_M])
    return np.abs((m32 - mean).astype(np.float64))


@needs_long_double
@pytest.mark.parametrize("name", PC.GENERAL_IDS + [PC.TWIN])
def test_restated_mean32_stays_within_its_bound(name):
    m32, E = _bound_quantities(name)
    err = _true_error(name, m32)
    sd = np.sqrt(PC.problem(name).variance)
    print(f"{name}: worst |mean32 - mean| {err.max():.3e}  E / sd {E.min() / sd:.3e} .. {E.max() / sd:.3e}  "
          f"worst error / E {(err / E).max():.3e}")
    assert np.all(np.isfinite(E)) and np.all(err <= E)
    assert np.all(E * E <= PC.problem(name).variance)      # the homogeneous cap passes every candidate of these models


@pytest.mark.parametrize("label", S.THRESHOLDS)
@GENERAL
def test_restated_screen_drops_only_what_the_exact_screen_drops_on_general_models(name, label):
    st, _ = PC.oracle_state(name)
    eta = S.threshold(name, label)
    mean, _ = S.sample_moments(name)
    ub32, prebest, m32, E = R.restated_blocks(name, label, PC.candidates(name)[: S.SAMPLE])
    assert np.all(np.abs(m32 - mean) <= E)
    ub = S.screen_bound(eta, mean, st.variance)
    nblk = ub32.shape[0]
    ub = np.concatenate([ub, np.full(nblk * PC.CAND_BLOCK - ub.shape[0], -np.inf)]).reshape(nblk, PC.CAND_BLOCK).max(1)
    best = float(S.block_seeds(eta, mean).max())
    assert np.all(ub32 >= ub) and prebest <= best
    exact = np.array([best > PC.MIN_BEST and u * PC.MARGIN < best for u in ub])
    pre = R.dismissed(ub32, prebest)
    print(f"{name} {label}: exact screen drops {exact.sum()} of {nblk}, pre-screen {pre.sum()}; prebest {prebest:.6g} best {best:.6g}")
    assert not np.any(pre & ~exact)
    if label == "-1e6":
        assert not pre.any()
    elif label == "eta+3":
        assert pre.any()                          # not vacuous on any general model


def test_restated_twin_decides_as_the_unit_model():
    """Scaling the outputs by 2^-10 scales mean32, E, the bounds and the lower seed exactly and moves no decision; under a
    cap E <= variance the twin passed no candidate."""
    for label in S.THRESHOLDS:
        Xq, Xt = PC.candidates(PC.TWIN_OF)[: S.SAMPLE], PC.candidates(PC.TWIN)[: S.SAMPLE]
        ub, prebest, m32, E = R.restated_blocks(PC.TWIN_OF, label, Xq)
        # the twin at the unit model's threshold scaled (the oracle's own eta differs by a rounding of its factorisation)
        p = PC.problem(PC.TWIN)
        eta = S.threshold(PC.TWIN_OF, label) * PC.TWIN_Y
        alpha = R.model_alpha(PC.TWIN_OF) / PC.TWIN_Y
        parts = [R.restate(p.kind, p.variance, p.ls, p.X, alpha, 0.0, Xt[lo: lo + 4096]) for lo in range(0, S.SAMPLE, 4096)]
        m32t, an = (np.concatenate(x) for x in zip(*parts))      # (in the chunks of R.restated_blocks: the same sums)
        xmax, x0 = R.model_extent(p.kind, p.ls, p.X)
        Et = R.bound(p.kind, p.d, 512, np.abs(alpha).sum(), p.variance, an, xmax, x0, m32t, eta)
        ubt, prebest_t = R.block_quantities(eta, p.variance, m32t, Et)
        assert np.array_equal(m32t, m32 * PC.TWIN_Y) and np.array_equal(Et, E * PC.TWIN_Y)
        assert np.array_equal(R.dismissed(ubt, prebest_t), R.dismissed(ub, prebest))
        assert not np.any(Et <= p.variance)
        if label == "eta":
            assert R.dismissed(ubt, prebest_t).sum() > 0


# ---- 4. planted defects ----------------------------------------------------------------------------------------------
SWEEPS = [("identity", 1), ("shuffled", 1), ("reversed", 256)]


def _sweep(name, label, order, lag, bound_variance=None, drop_mean_const=False):
    """The numpy sweep over the sample; -> (its decisions, the oracle's arg-max of the sample).
    (a) ``bound_variance``: screen and checkpoints at it; (b) ``drop_mean_const``: seeds and bounds at mean - mean_const."""
    st, _ = PC.oracle_state(name)
    eta = S.threshold(name, label)
    mean, var = S.sample_moments(name, bound_variance)
    out = S.sweep_with_screen(mean, var, eta, st.variance if bound_variance is None else bound_variance,
                              S.orders(NBLK_SAMPLE)[order], lag, bound_mean=mean - st.mean_const if drop_mean_const else None)
    full = PC.ei_tail(eta - mean, var[-1])
    want = int(O.argmax_first(full))
    return out, (float(full[want]), want)


def _same_decisions(a, b):
    return a[:2] == b[:2] and all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))


def _sweep_defect(defect):
    """A defect of the sweep: invisible on every unit model, and the general (model, threshold, order, lag) that lose the winner."""
    for name in PC.IDS:
        for label in S.THRESHOLDS:
            for order, lag in SWEEPS:
                assert _same_decisions(_sweep(name, label, order, lag, **defect)[0], _sweep(name, label, order, lag)[0]), (name, label)
    lost = []
    for name in PC.GENERAL_IDS:
        for label in S.THRESHOLDS:
            for order, lag in SWEEPS:
                out, want = _sweep(name, label, order, lag, **defect)
                assert _sweep(name, label, order, lag)[0][:2] == want
                if out[:2] != want:
                    lost.append((name, label, order, lag))
    return lost


def test_defect_a_bounds_at_variance_one():
    """Screen and checkpoint bound taken at variance 1: too low a bound wherever the variance is above 1 (below 1 it is
    merely loose, and costs no winner)."""
    lost = _sweep_defect(dict(bound_variance=1.0))
    print("winner lost on", sorted({(n, t) for n, t, _, _ in lost}))
    assert lost and all(PC.problem(n).variance > 1.0 for n, _, _, _ in lost)


def test_defect_b_mean_const_left_out_of_seed_and_bound():
    """Seeds and bounds at mean - mean_const: at mean_const = 37.5 every seed gains 37.5 and the blocks are compared by their
    means alone."""
    lost = _sweep_defect(dict(drop_mean_const=True))
    print("winner lost on", sorted({(n, t) for n, t, _, _ in lost}))
    assert lost


@needs_long_double
def test_defect_c_first_lengthscale_for_every_coordinate():
    for name in PC.IDS:
        p = PC.problem(name)
        for x, y in zip(_bound_quantities(name, ls=np.full(p.d, p.ls[0])), _bound_quantities(name)):
            assert np.array_equal(x, y), name
    caught = []
    for name in PC.GENERAL_IDS:
        p = PC.problem(name)
        m32, E = _bound_quantities(name, ls=np.full(p.d, p.ls[0]))
        ratio = (_true_error(name, m32) / E).max()
        print(f"{name}: worst error / E {ratio:.3e}")
        caught += [name] * bool(ratio > 1.0)
    assert caught == PC.GENERAL_IDS


@needs_long_double
def test_defect_d_variance_left_out_of_the_bound():
    for name in PC.IDS:
        for x, y in zip(_bound_quantities(name, bound_variance=1.0), _bound_quantities(name)):
            assert np.array_equal(x, y), name
    caught = []
    for name in PC.GENERAL_IDS:
        m32, E = _bound_quantities(name, bound_variance=1.0)
        ratio = (_true_error(name, m32) / E).max()
        print(f"{name}: worst error / E {ratio:.3e}")
        caught += [name] * bool(ratio > 1.0)
    assert "g_m32_d4_N520_var1e4" in caught


# ---- 5. the share condition ------------------------------------------------------------------------------------------
def test_share_cases_qualify_and_cover_every_general_model():
    """A GPU test asks the engine for half of the oracle's screened count only on these pairs: the oracle screens at least
    half of the blocks there.  Every general model has one (eta + 3 sd)."""
    print(S.SHARE_CASES_GENERAL)
    assert {n for n, _ in S.SHARE_CASES_GENERAL} == set(PC.GENERAL_IDS)
    assert all((n, "eta+3") in S.SHARE_CASES_GENERAL for n in PC.GENERAL_IDS)
    assert all(2 * S.RECORDED_GENERAL[n]["screened"][t] >= S.NBLK for n, t in S.SHARE_CASES_GENERAL)
    assert not any(t == "-1e6" for _, t in S.SHARE_CASES_GENERAL)
    assert R.SHARE_CASE_GENERAL in S.SHARE_CASES_GENERAL
