"""GPU: the three-phase pruned EI arg-max returns the unpruned sweep's winner, bit for bit, in both regimes.

Models of more than one row block run the mean pass of every block first, screen the blocks against the best word that
holds every seed, and then either cut the few survivors into ranges of row blocks over all workgroups (split regime: the
accumulators of every row block are dumped and folded by a third kernel) or run every survivor whole.
Every case compares value bits and index with tgp_set_variant bit 11 (nothing given up).  The knob
``set_prune_split(max_survivors, max_groups)`` forces either regime; ``prune_split`` reports the survivors S of the list
screen and the split work items (0: whole-block regime).

Models: those of tests/prune_cases.py at N = 512 and 768 (2 and 3 row blocks; d in {2, 8, 16}; all four kernels at
N = 512) and two of its own at N = 1024 and 1280 (4 and 5 row blocks: the smallest sizes at which a block can be cut into
fewer ranges than it has row blocks).  131072 + 77 candidates: the fused path needs 4 x #CU blocks, one block is ragged.

A launch splits only while S <= max_survivors AND S <= #workgroups (one compute unit each): the dump area is bounded by
the K* slabs the launch holds, one per workgroup.  Where a case forces max_survivors = S it therefore expects items > 0
exactly when S <= #CU."""
import functools
import struct
import types

import numpy as np
import pytest

from tests import prune_cases as PC

pytestmark = pytest.mark.gpu

NO_PRUNE, NO_SCREEN, STATIC = 2048, 4096, 8192
NBLK = -(-PC.M // PC.CAND_BLOCK)
OWN = {"m52_N1024_d8": ("matern52", 1024, 8), "m52_N1280_d2": ("matern52", 1280, 2)}
NAMES = ["m52_N512_d8", "rbf_N512_d8", "m12_N512_d8", "m32_N512_d8", "m52_N512_d2", "m52_N768_d8", "m32_N768_d16",
         "m52_N1024_d8", "m52_N1280_d2"]
SOME = ["m52_N512_d2", "m32_N768_d16", "m52_N1024_d8", "m52_N1280_d2"]   # one per row-block count, every d
THRESHOLDS = ["eta", "eta+0.5", "eta+3", "-1e6"]
FIRST, LAST_FULL, RAGGED = 5, (NBLK - 2) * PC.CAND_BLOCK + 17, (NBLK - 1) * PC.CAND_BLOCK + 40
CONFIGS = pytest.mark.parametrize("name", NAMES)
WHOLE, DEFAULT = (0, 0), (-1, 0)


@functools.lru_cache(maxsize=None)
def _problem(name):
    if name not in OWN:
        return PC.problem(name)
    from oracle import gp_oracle as O

    kind, N, d = OWN[name]
    p = types.SimpleNamespace(name=name, kind=kind, N=N, d=d, noise=1e-2, variance=1.0, mean_const=0.0)
    p.X, p.Y = O.synthetic_problem(O.ackley, d, N)
    p.ls = O.default_lengthscales(d)
    return p


@functools.lru_cache(maxsize=None)
def _candidates(name):
    if name not in OWN:
        return PC.candidates(name)
    Xq = np.random.default_rng(977).uniform(size=(PC.M, _problem(name).d))
    Xq.setflags(write=False)
    return Xq


def _engine(name):
    from trieste_amd.engine import GPEngine

    p = _problem(name)
    eng = GPEngine(p.d, p.kind, device=0)
    eng.set_hyper(p.variance, p.ls, p.noise, p.mean_const)
    eng.set_data(p.X, p.Y)
    return eng


@functools.lru_cache(maxsize=None)
def _shared(name):
    eng = _engine(name)
    return eng, eng.eta()


@functools.lru_cache(maxsize=None)
def _num_cu():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _nrb(name):
    return -(-_problem(name).N // PC.ROW_BLOCK)


def _param(name, label):
    eta = _shared(name)[1]
    return {"eta": eta, "eta+0.5": eta + 0.5, "eta+3": eta + 3.0, "-1e6": -1e6}[label]


def _bits(v):
    return struct.pack("<d", v)


def _unpruned(name, param, Xq, index_base=0):
    eng, _ = _shared(name)
    eng.set_variant(NO_PRUNE)
    v, i, _ = eng.acq_argmax("ei", param, Xq, index_base)
    eng.set_variant(0)
    return v, i


@functools.lru_cache(maxsize=None)
def _plain_unpruned(name, label):
    """The unpruned winner of the plain set at a threshold: computed once, shared by the cases."""
    return _unpruned(name, _param(name, label), _candidates(name))


def _pruned(name, param, Xq, knob=DEFAULT, variant=0, eng=None):
    """-> ((value, index), (blocks, given up, row blocks skipped), screened, (survivors, items)) under `knob`, `variant`."""
    from trieste_amd.engine import prune_counters, prune_screened, prune_split, set_prune_split

    eng = _shared(name)[0] if eng is None else eng
    eng.set_variant(variant)
    set_prune_split(eng, *knob)
    v, i, _ = eng.acq_argmax("ei", param, Xq)
    out = (v, i), prune_counters(eng), prune_screened(eng), prune_split(eng)
    set_prune_split(eng, *DEFAULT)
    eng.set_variant(0)
    return out


def _same(got, want):
    assert (_bits(got[0]), got[1]) == (_bits(want[0]), want[1]), (got, want)


def _check_counters(name, variant, counters, screened, split):
    blocks, given, skipped = counters
    survivors, items = split
    nrb = _nrb(name)
    assert blocks == NBLK and 0 <= screened <= given <= NBLK
    assert given <= skipped <= given * (nrb - 1)
    assert survivors + screened == blocks      # every block is either screened by the list or a survivor
    assert items == 0 or (1 <= survivors <= _num_cu() and items % survivors == 0 and survivors <= items <= survivors * nrb)
    if items:
        assert given == screened               # split survivors run to the end
    if variant & NO_SCREEN:
        assert screened == 0 and survivors == blocks


def _splits_by_default(S):
    return 1 <= S <= _num_cu() // 2


@CONFIGS
@pytest.mark.parametrize("label", THRESHOLDS)
def test_regimes(name, label):
    want = _plain_unpruned(name, label)
    param, Xq = _param(name, label), _candidates(name)
    got, counters, screened, (S, items) = _pruned(name, param, Xq)
    print(f"{name} {label}: {got}; counters {counters} screened {screened} survivors {S} items {items}")
    _same(got, want)
    _check_counters(name, 0, counters, screened, (S, items))
    assert (items > 0) == _splits_by_default(S)
    if label == "-1e6":
        assert (S, items, counters) == (NBLK, 0, (NBLK, 0, 0)) and (_bits(got[0]), got[1]) == (_bits(0.0), 0)
    else:
        assert got[0] > 0.0 and S >= 1
    for knob in (WHOLE, (S, 0), (S - 1, 0), (-1, 1), (-1, 2)):
        got, counters, screened, (S2, items) = _pruned(name, param, Xq, knob)
        _same(got, want)
        _check_counters(name, 0, counters, screened, (S2, items))
        assert S2 == S, (knob, S2, S)
        if knob == WHOLE or knob == (S - 1, 0):
            assert items == 0, (knob, items)
        elif knob == (S, 0):
            assert (items > 0) == (S <= _num_cu()), (knob, S, items)
        else:
            assert (items > 0) == _splits_by_default(S), (knob, S, items)
            if items:   # ranges per block: at most max_groups, never more than #workgroups / S
                assert items == S * min(knob[1], _num_cu() // S), (knob, S, items)


@pytest.mark.parametrize("name", SOME)
def test_same_call_twice_same_survivors_and_bits(name):
    param = _param(name, "eta+0.5")
    a = _pruned(name, param, _candidates(name))
    b = _pruned(name, param, _candidates(name))
    _same(a[0], b[0])
    assert a[3] == b[3] and a[2] == b[2]
    _same(a[0], _plain_unpruned(name, "eta+0.5"))


def _winner_moved_to(name, label, index):
    """The plain set with its winner at the threshold moved to `index` (its old place takes a copy of the point behind it)."""
    _, old = _plain_unpruned(name, label)
    Xq = _candidates(name).copy()
    x = Xq[old].copy()
    Xq[old] = Xq[(old + 1) % PC.M]
    Xq[index] = x
    return Xq


@CONFIGS
@pytest.mark.parametrize("where", [FIRST, LAST_FULL, RAGGED], ids=["first-block", "last-full-block", "ragged-tail"])
def test_winner_planted(name, where):
    val, _ = _plain_unpruned(name, "eta+0.5")
    Xq = _winner_moved_to(name, "eta+0.5", where)
    param = _param(name, "eta+0.5")
    want = _unpruned(name, param, Xq)
    S = _pruned(name, param, Xq)[3][0]
    for knob, splits in ((WHOLE, False), ((S, 0), S <= _num_cu())):
        got, _, _, (_, items) = _pruned(name, param, Xq, knob)
        _same(got, want)
        assert got == (val, where) and (items > 0) == splits


@pytest.mark.parametrize("name", SOME)
@pytest.mark.parametrize("which", ["copy-below", "copy-above"])
def test_duplicated_winner_in_a_second_surviving_block(name, which):
    """A copy of the winner makes its block a survivor (its bound is at least the winner's value): the lower index wins."""
    val, _ = _plain_unpruned(name, "eta+0.5")
    w = (NBLK // 2) * PC.CAND_BLOCK + 17       # the winner in the middle, its copy in block 3 or in the last full block
    at = (3 if which == "copy-below" else NBLK - 2) * PC.CAND_BLOCK + 9
    Xq = _winner_moved_to(name, "eta+0.5", w)
    Xq[at] = Xq[w]
    param = _param(name, "eta+0.5")
    want = _unpruned(name, param, Xq)
    S = _pruned(name, param, Xq)[3][0]
    assert S >= 2
    for knob in ((S, 0), WHOLE, (1, 0)):
        got, _, _, (S2, items) = _pruned(name, param, Xq, knob)
        _same(got, want)
        assert got == (val, min(w, at)) and S2 == S
        assert (items > 0) == (knob == (S, 0) and S <= _num_cu())


@pytest.mark.parametrize("name", SOME)
def test_nan_coordinates(name):
    """NaN coordinates in the block of the largest seed (the lowest mean) and in the ragged block: a NaN never wins and the
    bound of a block that holds one is stored as +inf, so the block is never screened -- the list can only grow."""
    eng, _ = _shared(name)
    param = _param(name, "eta+3")
    Xc = _candidates(name)
    mean, _ = eng.predict(Xc)
    top = int(np.argmin(mean))
    blk0 = top // PC.CAND_BLOCK * PC.CAND_BLOCK
    S_clean = _pruned(name, param, Xc)[3][0]
    Xq = Xc.copy()
    others = [i for i in (blk0, blk0 + 1, blk0 + PC.CAND_BLOCK - 1) if i != top]
    for i in others + [RAGGED]:   # the top seed itself stays: the best word is the clean run's
        Xq[i, i % Xq.shape[1]] = np.nan
    want = _unpruned(name, param, Xq)
    for knob in (DEFAULT, WHOLE):
        got, counters, screened, (S, items) = _pruned(name, param, Xq, knob)
        _same(got, want)
        assert got[0] == got[0] and not np.isnan(Xq[got[1]]).any()
        assert S_clean <= S <= S_clean + 1     # the top seed's block survives anyway; the ragged block now does too
        _check_counters(name, 0, counters, screened, (S, items))
    Xq[top, 0] = np.nan                        # ... and with the top seed itself gone
    want = _unpruned(name, param, Xq)
    for knob in (DEFAULT, WHOLE):
        got = _pruned(name, param, Xq, knob)[0]
        _same(got, want)
        assert got[0] == got[0] and not np.isnan(Xq[got[1]]).any()


@pytest.mark.parametrize("name", SOME)
def test_handle_reuse(name):
    """A call with eta = 1e6, then an ordinary one; a call over all candidates, then one over fewer: the later call equals
    a fresh handle's -- stale list entries, means and dumps are not read."""
    eng, eta = _shared(name)
    Xq = _candidates(name)
    short = Xq[: 131072 - PC.CAND_BLOCK * 5]
    fresh = _engine(name)
    want_all = _pruned(name, eta, Xq, eng=fresh)
    fresh.close()
    fresh = _engine(name)
    want_short = _pruned(name, eta, short, eng=fresh)
    fresh.close()
    huge = _pruned(name, 1e6, Xq)
    assert huge[0][0] > 1e5
    for knob in (DEFAULT, WHOLE):
        _pruned(name, 1e6, Xq, knob)
        second = _pruned(name, eta, Xq, knob)
        _same(second[0], want_all[0])
        assert second[3][0] == want_all[3][0] and second[2] == want_all[2]
        third = _pruned(name, eta, short, knob)
        _same(third[0], want_short[0])
        assert third[3][0] == want_short[3][0] and third[2] == want_short[2]
    _same(want_all[0], _plain_unpruned(name, "eta"))
    _same(want_short[0], _unpruned(name, eta, short))


@CONFIGS
@pytest.mark.parametrize("variant", [NO_SCREEN, STATIC, NO_SCREEN | STATIC])
def test_existing_variants_under_the_default_knob(name, variant):
    for label in ("eta+0.5", "-1e6"):
        got, counters, screened, split = _pruned(name, _param(name, label), _candidates(name), DEFAULT, variant)
        _same(got, _plain_unpruned(name, label))
        _check_counters(name, variant, counters, screened, split)
