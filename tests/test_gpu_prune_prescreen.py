"""GPU: the float32 pre-screen (phase 0) of the pruned EI arg-max changes no bit and no counter, and its bound holds.

Phase 0 (the numpy side is tests/prescreen_cases.py, checked on the CPU by tests/test_prescreen_cases.py)
forms every candidate's mean in float32 with a bound E and lets the exact mean pass skip the blocks it can dismiss.
tgp_set_variant bit 14 runs without it: every case compares winner value bits and index, the three counters, the screened
count and (survivors, items) with that launch, and the winner with the unpruned launch (bit 11).  Models, candidate sets
and helpers are those of tests/prune_cases.py and tests/test_gpu_prune_screen.py."""
import functools

import numpy as np
import pytest

from tests import prescreen_cases as R
from tests import prune_cases as PC
from tests import prune_screen_cases as S
from tests import test_gpu_prune_screen as G

pytestmark = pytest.mark.gpu

NO_PRESCREEN = 16384
CONFIGS = pytest.mark.parametrize("name", PC.IDS)
BOUND_M = 4096


def _launch(eng, variant, param, Xq, split=(-1, 0)):
    """-> everything the pre-screen must leave alone, and its own count, of one arg-max under `variant`."""
    from trieste_amd import engine as E

    eng.set_variant(variant)
    E.set_prune_split(eng, *split)
    v, i, _ = eng.acq_argmax("ei", param, Xq)
    out = dict(winner=(G._bits(v), i), counters=E.prune_counters(eng), screened=E.prune_screened(eng), split=E.prune_split(eng))
    pre = E.prune_prescreened(eng)
    E.set_prune_split(eng)
    eng.set_variant(0)
    return out, pre


def _compare(eng, param, Xq, variant=0, split=(-1, 0)):
    """The launch with phase 0 against the one without; -> (what they share, blocks pre-screened)."""
    want, pre0 = _launch(eng, variant | NO_PRESCREEN, param, Xq, split)
    got, pre = _launch(eng, variant, param, Xq, split)
    assert got == want, (got, want)
    assert pre0 == 0 and 0 <= pre <= got["screened"]
    return got, pre


@CONFIGS
@pytest.mark.parametrize("label", S.THRESHOLDS)
def test_same_bits_and_counters_as_without(name, label):
    eng, _ = G._shared(name)
    got, pre = _compare(eng, G._param(name, label), PC.candidates(name))
    v, i = G._plain_unpruned(name, label)
    print(f"{name} {label}: {got}; pre-screened {pre}")
    assert got["winner"] == (G._bits(v), i)
    if label == "-1e6" or PC.problem(name).N <= PC.ROW_BLOCK:
        assert pre == 0
    if (name, label) == R.SHARE_CASE:
        # tests/prescreen_cases.py: the restatement dismisses SHARE_DISMISSED blocks here, over half of the oracle's screened ones
        assert pre > 0


@CONFIGS
@pytest.mark.parametrize("variant", [G.NO_SCREEN, G.STATIC], ids=["no-screen", "static-blocks"])
def test_under_the_other_knock_outs(name, variant):
    eng, _ = G._shared(name)
    got, pre = _compare(eng, G._param(name, "eta+0.5"), PC.candidates(name), variant)
    v, i = G._plain_unpruned(name, "eta+0.5")
    assert got["winner"] == (G._bits(v), i)
    if variant & G.NO_SCREEN:
        assert (got["screened"], pre) == (0, 0)


@CONFIGS
@pytest.mark.parametrize("split", [(0, 0), (-1, 0)], ids=["never-split", "default-split"])
def test_under_the_split_knobs(name, split):
    eng, _ = G._shared(name)
    got, _ = _compare(eng, G._param(name, "eta+3"), PC.candidates(name), split=split)
    v, i = G._plain_unpruned(name, "eta+3")
    assert got["winner"] == (G._bits(v), i)
    if split[0] == 0:
        assert got["split"][1] == 0


@CONFIGS
@pytest.mark.parametrize("m", [PC.M - 77, PC.M - 77 - 5, 4 * 256 * PC.CAND_BLOCK + 1], ids=["full-blocks", "ragged-123", "one-over"])
def test_candidate_counts(name, m):
    eng, _ = G._shared(name)
    Xq = PC.candidates(name)[:m]
    param = G._param(name, "eta+0.5")
    got, _ = _compare(eng, param, Xq)
    v, i = G._unpruned(name, param, Xq)
    assert got["winner"] == (G._bits(v), i)


@CONFIGS
def test_nan_candidates(name):
    top = S.RECORDED[name]["top_seed"]
    blk0 = top // PC.CAND_BLOCK * PC.CAND_BLOCK
    Xq = PC.candidates(name).copy()
    for i in (top, blk0 + 1, 0, G.RAGGED, 300 * PC.CAND_BLOCK + 3):
        Xq[i, i % Xq.shape[1]] = np.nan
    Xq[77 * PC.CAND_BLOCK + 5, 0] = np.inf
    eng, _ = G._shared(name)
    param = G._param(name, "eta+3")
    got, _ = _compare(eng, param, Xq)
    v, i = G._unpruned(name, param, Xq)
    assert got["winner"] == (G._bits(v), i)


@CONFIGS
@pytest.mark.parametrize("which", [0, 1], ids=["copy-below", "copy-above"])
def test_winner_duplicated_into_a_dismissed_block(name, which):
    val, w = G._plain_unpruned(name, "eta+3")
    at = S.RECORDED[name]["dup_blocks"][which] * PC.CAND_BLOCK + (5, 9)[which]
    Xq = PC.candidates(name).copy()
    Xq[at] = Xq[w]
    eng, _ = G._shared(name)
    got, _ = _compare(eng, G._param(name, "eta+3"), Xq)
    assert got["winner"] == (G._bits(val), min(w, at))


def _bound_models():
    """The recorded models, then two built for the bound: the m52_N512_d8 box moved to 1e3, and that model at noise 1e-5."""
    return list(PC.IDS) + ["shifted-box", "low-noise"]


@functools.lru_cache(maxsize=None)
def _bound_engine(which):
    if which in PC.IDS:
        return G._shared(which)[0], PC.candidates(which)[:BOUND_M]
    from trieste_amd.engine import GPEngine

    p = PC.problem("m52_N512_d8")
    off = 1e3 if which == "shifted-box" else 0.0
    eng = GPEngine(p.d, p.kind, device=0)
    eng.set_hyper(p.variance, p.ls, 1e-5 if which == "low-noise" else p.noise, p.mean_const)
    eng.set_data(p.X + off, p.Y)
    return eng, PC.candidates("m52_N512_d8")[:BOUND_M] + off


@pytest.mark.parametrize("which", _bound_models())
def test_device_mean32_stays_within_its_bound(which):
    from trieste_amd.engine import prescreen_means

    eng, Xq = _bound_engine(which)
    m32, E = prescreen_means(eng, Xq)
    err = np.abs(m32 - eng.predict_mean(Xq))
    print(f"{which}: worst |mean32 - mean| {err.max():.3e}  E {E.min():.3e} .. {E.max():.3e}  worst error / E {(err / E).max():.3e}")
    assert np.all(np.isfinite(E)) and np.all(E > 0.0)
    assert np.all(err <= E)


def test_device_bound_is_the_restated_bound():
    """E as the device forms it against tests/prescreen_cases.bound on the same model (the two sum |alpha| in another order)."""
    from trieste_amd.engine import prescreen_means

    name = "m52_N512_d8"
    eng, Xq = _bound_engine(name)
    m32, E = prescreen_means(eng, Xq)
    p = PC.problem(name)
    alpha = R.model_alpha(name)
    _, an = R.restate(p.kind, p.variance, p.ls, p.X, alpha, p.mean_const, Xq)
    xmax, x0 = R.model_extent(p.kind, p.ls, p.X)
    want = R.bound(p.kind, p.d, 512, np.abs(alpha).sum(), p.variance, an, xmax, x0, m32, 0.0)
    np.testing.assert_allclose(E, want, rtol=1e-6)


@pytest.mark.parametrize("scale", [1e9, 1e300], ids=["E-above-the-variance", "E-not-finite"])
def test_a_useless_bound_pre_screens_nothing(scale):
    """Targets (and with them alpha) blown up until E exceeds the variance, then until |alpha|_1 overflows: phase 0 dismisses
    nothing and the launch returns what it returns without it."""
    from trieste_amd.engine import GPEngine, prescreen_means

    p = PC.problem("m52_N512_d8")
    eng = GPEngine(p.d, p.kind, device=0)
    eng.set_hyper(p.variance, p.ls, p.noise, p.mean_const)
    eng.set_data(p.X, p.Y * scale)
    Xq = PC.candidates(p.name)
    _, E = prescreen_means(eng, Xq[:BOUND_M])
    assert not np.any(E <= p.variance)
    for param in (eng.eta(), 0.0):
        got, pre = _compare(eng, param, Xq)
        assert pre == 0
        eng.set_variant(G.NO_PRUNE)
        v, i, _ = eng.acq_argmax("ei", param, Xq)
        eng.set_variant(0)
        assert got["winner"] == (G._bits(v), i)
    eng.close()
