"""GPU: the pruned EI arg-max on general models -- ARD lengthscales, variances from 1e-4 to 1e4, constant means of 37.5 and
-1000, boxes far from the origin, padded dimensions 4, 6, 8 and 16 (tests/prune_cases.GENERAL).

The other prune suites (test_gpu_prune*.py) run on models where sigma^2, sigma and 1 are one number, a dropped mean changes
nothing and ls[0] is every lengthscale: the quantities every pruning bound is made of.  A wrong bound produces no wrong
number; it drops the true winner, on some models only.  tests/test_prune_general_cases.py plants four such defects in the
numpy side and shows that these models see them and the unit models do not.

The unpruned launch (tgp_set_variant bit 11) is anchored to the oracle's recorded winner (difference form, computed on the
CPU: S.RECORDED_GENERAL); everything else is compared with that launch bit for bit.  Thresholds are eta + k sd for k = 0,
0.5, 3 and -1e6 sd + mean (S.thresholds).  One engine per model (test_gpu_prune_screen._shared); helpers of
test_gpu_prune_screen.py and test_gpu_prune_prescreen.py."""
import functools

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import prescreen_cases as R
from tests import prune_cases as PC
from tests import prune_screen_cases as S
from tests import test_gpu_prune_prescreen as Pre
from tests import test_gpu_prune_screen as G
from tests.util import cancellation_floor

pytestmark = pytest.mark.gpu

NBLK = S.NBLK
NO_PRESCREEN = Pre.NO_PRESCREEN
VARIANTS = [0, G.NO_SCREEN, G.STATIC, NO_PRESCREEN, G.NO_SCREEN | G.STATIC]
VARIANT_IDS = ["default", "no-screen", "static-blocks", "no-pre-screen", "no-screen-static"]
SPLITS = [(0, 0), (-1, 0)]
MODELS = pytest.mark.parametrize("name", PC.GENERAL_IDS)
BOUND_M = 4096


def _param(name, label):
    """The threshold from the ENGINE's eta, as tests/test_gpu_prune_screen._param takes it on the unit models."""
    return S.thresholds(PC.problem(name), G._shared(name)[1])[label]


@functools.lru_cache(maxsize=None)
def _plain_unpruned(name, label):
    """The unpruned winner of the plain set at a threshold: computed once, shared by the cases."""
    return G._unpruned(name, _param(name, label), PC.candidates(name))


def _floor(name):
    p = PC.problem(name)
    return cancellation_floor(p.N, p.variance, p.noise)


@MODELS
def test_unpruned_winner_is_the_oracles(name):
    """The anchor of every comparison below: the launch with nothing given up returns the oracle's recorded arg-max at
    eta + 0.5 sd -- the same index, or one whose oracle value is within 1e-5 |max| + cancellation_floor of the oracle's
    largest (_argmax_agrees of tests/test_gpu_general.py; the two oracle values then come from the CPU, two candidates)."""
    p = PC.problem(name)
    rec = S.RECORDED_GENERAL[name]
    eta = G._shared(name)[1]
    assert abs(eta - rec["eta"]) <= 10 * _floor(name), (eta, rec["eta"])
    val, idx = _plain_unpruned(name, "eta+0.5")
    oi, ov = rec["winner"]
    print(f"{name}: engine ({val!r}, {idx}) oracle ({ov!r}, {oi}); eta {eta!r} against {rec['eta']!r}")
    assert val > 0.0
    if idx != oi:
        st, _ = PC.oracle_state(name)
        with PC.form(name):
            at = O.ei_values(st, PC.candidates(name)[[oi, idx]], _param(name, "eta+0.5"))
        assert abs(at[0] - at[1]) <= 1e-5 * abs(at[0]) + _floor(name), (idx, oi, at)


def _check_counters(name, label, variant, out, pre):
    """The invariants of tests/test_gpu_prune_screen._check_counters, the share condition from the general table."""
    blocks, given, skipped = out["counters"]
    screened = out["screened"]
    nrb = -(-PC.problem(name).N // PC.ROW_BLOCK)
    assert blocks == NBLK and 0 <= pre <= screened <= given <= NBLK
    assert given <= skipped <= given * (nrb - 1)
    if label == "-1e6":
        assert (given, skipped, screened, pre) == (0, 0, 0, 0)
    if variant & G.NO_SCREEN:
        assert (screened, pre) == (0, 0)
    elif (name, label) in S.SHARE_CASES_GENERAL:
        # the oracle screens at least half of the blocks by the seeds alone, each block knowing those a round before it
        want = S.RECORDED_GENERAL[name]["screened"][label]
        assert 2 * screened >= want > 0 and given > 0, (screened, want)
    if variant & NO_PRESCREEN:
        assert pre == 0
    elif not variant & G.NO_SCREEN and (name, label) == R.SHARE_CASE_GENERAL:
        # phase 0 is live: the restatement dismisses R.SHARE_DISMISSED_GENERAL blocks here (none under a cap E <= variance)
        assert pre > 0


@MODELS
@pytest.mark.parametrize("label", S.THRESHOLDS)
@pytest.mark.parametrize("variant", VARIANTS, ids=VARIANT_IDS)
@pytest.mark.parametrize("split", SPLITS, ids=["never-split", "default-split"])
def test_pruned_is_the_unpruned_launch(name, label, variant, split):
    want = _plain_unpruned(name, label)
    eng, _ = G._shared(name)
    out, pre = Pre._launch(eng, variant, _param(name, label), PC.candidates(name), split)
    print(f"{name} {label} variant {variant} split {split}: blocks, given up, row blocks skipped = {out['counters']}, screened = "
          f"{out['screened']}, pre-screened = {pre}, (survivors, items) = {out['split']} (oracle, seeds alone: "
          f"{S.RECORDED_GENERAL[name]['screened'][label]})")
    assert out["winner"] == (G._bits(want[0]), want[1]), (out["winner"], want)
    _check_counters(name, label, variant, out, pre)
    if split[0] == 0:
        assert out["split"][1] == 0
    if label == "-1e6":
        assert out["winner"] == (G._bits(0.0), 0)
    else:
        assert want[0] > 0.0


@MODELS
@pytest.mark.parametrize("label", S.THRESHOLDS)
def test_pre_screen_changes_no_counter(name, label):
    """With phase 0 and without it (bit 14): winner, the three counters, screened, (survivors, items) all equal."""
    eng, _ = G._shared(name)
    got, pre = Pre._compare(eng, _param(name, label), PC.candidates(name))
    want = _plain_unpruned(name, label)
    assert got["winner"] == (G._bits(want[0]), want[1])


def _winner_moved_to(name, label, index):
    """The plain set with its winner at the threshold moved to `index` (its old place takes a copy of the point behind it)."""
    _, old = _plain_unpruned(name, label)
    Xq = PC.candidates(name).copy()
    x = Xq[old].copy()
    Xq[old] = Xq[(old + 1) % PC.M]
    Xq[index] = x
    return Xq


@MODELS
@pytest.mark.parametrize("where", [G.FIRST, G.LAST_FULL, G.RAGGED], ids=["first-block", "last-full-block", "ragged-tail"])
def test_winner_planted(name, where):
    val, _ = _plain_unpruned(name, "eta+0.5")
    Xq = _winner_moved_to(name, "eta+0.5", where)
    param = _param(name, "eta+0.5")
    want = G._unpruned(name, param, Xq)
    got, _, _ = G._pruned(name, param, Xq)
    G._same(got, want)
    assert got == (val, where)


@MODELS
@pytest.mark.parametrize("which", [0, 1], ids=["copy-below", "copy-above"])
def test_duplicated_winner_in_a_screened_block(name, which):
    """A copy of the winner in a block whose other 127 candidates the oracle screens against the largest seed: the lower of
    the two indices wins, with phase 0 and without it."""
    val, w = _plain_unpruned(name, "eta+3")
    at = S.RECORDED_GENERAL[name]["dup_blocks"][which] * PC.CAND_BLOCK + (5, 9)[which]
    assert at // PC.CAND_BLOCK != w // PC.CAND_BLOCK
    Xq = PC.candidates(name).copy()
    Xq[at] = Xq[w]
    param = _param(name, "eta+3")
    want = G._unpruned(name, param, Xq)
    for variant in (0, G.STATIC):
        got, _, _ = G._pruned(name, param, Xq, variant)
        G._same(got, want)
        assert got == (val, min(w, at))
    got, _ = Pre._compare(G._shared(name)[0], param, Xq)
    assert got["winner"] == (G._bits(val), min(w, at))


@MODELS
def test_nan_and_inf_coordinates_in_the_block_of_the_largest_seed(name):
    top = S.RECORDED_GENERAL[name]["top_seed"]
    blk0 = top // PC.CAND_BLOCK * PC.CAND_BLOCK
    Xq = PC.candidates(name).copy()
    for i in (top, blk0, blk0 + 1, blk0 + PC.CAND_BLOCK - 1, 0, G.RAGGED, 300 * PC.CAND_BLOCK + 3):
        Xq[i, i % Xq.shape[1]] = np.nan
    Xq[blk0 + 2, 0] = np.inf
    Xq[77 * PC.CAND_BLOCK + 5, Xq.shape[1] - 1] = -np.inf
    param = _param(name, "eta+3")
    want = G._unpruned(name, param, Xq)
    got, counters, screened = G._pruned(name, param, Xq)
    G._same(got, want)
    assert got[0] == got[0] and np.all(np.isfinite(Xq[got[1]]))
    assert 0 <= screened <= counters[1] <= NBLK
    both, _ = Pre._compare(G._shared(name)[0], param, Xq)
    assert both["winner"] == (G._bits(want[0]), want[1])


@MODELS
def test_index_base(name):
    val, idx = _plain_unpruned(name, "eta+0.5")
    base = (1 << 40) + 7
    param = _param(name, "eta+0.5")
    want = G._unpruned(name, param, PC.candidates(name), base)
    got, _, _ = G._pruned(name, param, PC.candidates(name), index_base=base)
    G._same(got, want)
    assert got == (val, base + idx)


@pytest.mark.parametrize("name", PC.GENERAL_IDS + [PC.TWIN])
def test_device_mean32_stays_within_the_device_bound(name):
    """|mean32 - mean| <= E with both from the device, on every general model; on the first two the device's E is
    tests/prescreen_cases.bound (rtol 1e-6 as in test_device_bound_is_the_restated_bound: the two sum |alpha| in another
    order) -- the first comparison of its ARD and x0 terms."""
    from trieste_amd.engine import prescreen_means

    eng, _ = G._shared(name)
    p = PC.problem(name)
    Xq = PC.candidates(name)[:BOUND_M]
    m32, E = prescreen_means(eng, Xq)
    err = np.abs(m32 - eng.predict_mean(Xq))
    print(f"{name}: worst |mean32 - mean| {err.max():.3e}  E {E.min():.3e} .. {E.max():.3e}  worst error / E {(err / E).max():.3e}")
    assert np.all(np.isfinite(E)) and np.all(E > 0.0)
    assert np.all(err <= E)
    assert np.all(E * E <= p.variance)          # none of these models is capped
    if name in ("g_m52_d8_N512_at1024", "g_rbf_d6_N700_at100"):
        alpha = R.model_alpha(name)
        a =np.sqrt(R.SCALE[p.kind]) * (Xq / p.ls - (p.X / p.ls)[0])
        xmax, x0 = R.model_extent(p.kind, p.ls, p.X)
        npad = -(-p.N // PC.ROW_BLOCK) * PC.ROW_BLOCK
        want = R.bound(p.kind, p.d, npad, np.abs(alpha).sum(), p.variance, np.sqrt((a * a).sum(1)), xmax, x0, m32, 0.0)
        np.testing.assert_allclose(E, want, rtol=1e-6)


def test_twin_scaled_by_a_power_of_two_decides_as_the_unit_model():
    """g_twin_m52_N512_d8 is m52_N512_d8 with X and ls times 4, Y times 2^-10, variance and noise times 4^-10: every
    operation of the engine commutes exactly with these scalings (test_output_scaling_by_a_power_of_two_is_exact), so at the
    scaled thresholds the winner has the unit model's index and exactly 2^-10 times its value, and phase 0 dismisses the
    same blocks.  (Under the cap E <= variance, a length against its square, the twin pre-screened nothing.)  Two identical
    static-blocks launches of the unit model reproduce every counter on an MI355X, so under that variant all of them are
    required equal as well; with drawn blocks the others are printed."""
    unit, eta = G._shared(PC.TWIN_OF)
    twin, eta_t = G._shared(PC.TWIN)
    assert eta_t == eta * PC.TWIN_Y
    for label in S.THRESHOLDS:
        pu, pt = G._param(PC.TWIN_OF, label), _param(PC.TWIN, label)
        assert pt == pu * PC.TWIN_Y
        for variant in (0, G.STATIC):
            a, pre_a = Pre._launch(unit, variant, pu, PC.candidates(PC.TWIN_OF))
            b, pre_b = Pre._launch(twin, variant, pt, PC.candidates(PC.TWIN))
            print(f"{label} variant {variant}: unit {a} pre-screened {pre_a}; twin {b} pre-screened {pre_b}")
            va, vb = (np.frombuffer(x["winner"][0], dtype="<f8")[0] for x in (a, b))
            assert b["winner"][1] == a["winner"][1]
            assert G._bits(vb * 2.0 ** 10) == a["winner"][0], (va, vb)
            assert pre_b == pre_a
            if label != "-1e6":
                assert pre_a > 0
            if variant == G.STATIC:
                again, pre_again = Pre._launch(unit, variant, pu, PC.candidates(PC.TWIN_OF))
                assert (again, pre_again) == (a, pre_a)
                assert {k: b[k] for k in ("counters", "screened", "split")} == {k: a[k] for k in ("counters", "screened", "split")}
