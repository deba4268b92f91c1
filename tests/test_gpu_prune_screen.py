"""GPU: seed, mean screen and drawn blocks of the pruned EI arg-max return the unpruned sweep's winner, bit for bit.

Once a candidate block's means are known the kernel posts the block's largest eta - mean as a seed of the launch's best
word and gives the block up before its first row block when EI at the prior variance cannot win (the
numpy side is tests/prune_screen_cases.py, checked against the oracle by tests/test_prune_screen_bound.py).  Every case
compares value bits and index with tgp_set_variant bit 11 (nothing given up).  Bit 12 runs without seed and screen, bit 13
deals the blocks statically.  Models and the plain candidate set are those of tests/prune_cases.py (N <= 768, 131072 + 77
candidates: the fused path needs >= 4 x #CU blocks)."""
import functools
import struct

import numpy as np
import pytest

from tests import prune_cases as PC
from tests import prune_screen_cases as S

pytestmark = pytest.mark.gpu

NO_PRUNE, NO_SCREEN, STATIC = 2048, 4096, 8192
VARIANTS = [0, NO_SCREEN, STATIC, NO_SCREEN | STATIC]
NBLK = S.NBLK
FIRST, LAST_FULL, RAGGED = 5, (NBLK - 2) * PC.CAND_BLOCK + 17, (NBLK - 1) * PC.CAND_BLOCK + 40
CONFIGS = pytest.mark.parametrize("name", PC.IDS)


def _engine(name):
    from trieste_amd.engine import GPEngine

    p = PC.problem(name)
    eng = GPEngine(p.d, p.kind, device=0)
    eng.set_hyper(p.variance, p.ls, p.noise, p.mean_const)
    eng.set_data(p.X, p.Y)
    return eng


@functools.lru_cache(maxsize=None)
def _shared(name):
    """One engine per configuration and its eta."""
    eng = _engine(name)
    return eng, eng.eta()


def _param(name, label):
    eta = _shared(name)[1]
    return {"eta": eta, "eta+0.5": eta + 0.5, "eta+3": eta + 3.0, "-1e6": -1e6}[label]


def _bits(v):
    return struct.pack("<d", v)


def _unpruned(name, param, Xq, index_base=0):
    eng, _ = _shared(name)
    eng.set_variant(NO_PRUNE)
    v, i, _ = eng.acq_argmax("ei", param, Xq, index_base)
    return v, i


@functools.lru_cache(maxsize=None)
def _plain_unpruned(name, label):
    """The unpruned winner of the plain set at a threshold: computed once, shared by the cases."""
    return _unpruned(name, _param(name, label), PC.candidates(name))


def _pruned(name, param, Xq, variant=0, index_base=0):
    """-> ((value, index), (blocks, given up, row blocks skipped), screened) of the pruned launch under `variant`."""
    from trieste_amd.engine import prune_counters, prune_screened

    eng, _ = _shared(name)
    eng.set_variant(variant)
    v, i, _ = eng.acq_argmax("ei", param, Xq, index_base)
    counters, screened = prune_counters(eng), prune_screened(eng)
    eng.set_variant(0)
    return (v, i), counters, screened


def _same(got, want):
    assert (_bits(got[0]), got[1]) == (_bits(want[0]), want[1]), (got, want)


def _check_counters(name, label, variant, counters, screened):
    blocks, given, skipped = counters
    nrb = -(-PC.problem(name).N // PC.ROW_BLOCK)
    assert blocks == NBLK and 0 <= screened <= given <= NBLK
    assert given <= skipped <= given * max(nrb - 1, 0)
    if label == "-1e6" or nrb == 1:
        assert (given, skipped, screened) == (0, 0, 0)
    if variant & NO_SCREEN:
        assert screened == 0
    elif (name, label) in S.SHARE_CASES:
        # the oracle screens at least half of the blocks by the seeds alone, each block knowing those a round before it
        assert 2 * screened >= S.RECORDED[name]["screened"][label], (screened, S.RECORDED[name]["screened"][label])


@CONFIGS
@pytest.mark.parametrize("label", S.THRESHOLDS)
@pytest.mark.parametrize("variant", VARIANTS)
def test_thresholds_and_knock_outs(name, label, variant):
    want = _plain_unpruned(name, label)
    got, counters, screened = _pruned(name, _param(name, label), PC.candidates(name), variant)
    print(f"{name} {label} variant {variant}: {got}; blocks, given up, row blocks skipped = {counters}, screened = {screened}"
          f" (oracle, seeds alone: {S.RECORDED[name]['screened'][label]})")
    _same(got, want)
    _check_counters(name, label, variant, counters, screened)
    if label == "-1e6":
        assert (_bits(got[0]), got[1]) == (_bits(0.0), 0)
    else:
        assert got[0] > 0.0


def _winner_moved_to(name, label, index):
    """The plain set with its winner at the threshold moved to `index` (its old place takes a copy of the point behind it)."""
    _, old = _plain_unpruned(name, label)
    Xq = PC.candidates(name).copy()
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
    got, _, _ = _pruned(name, param, Xq)
    _same(got, want)
    assert got == (val, where)


@CONFIGS
@pytest.mark.parametrize("which", [0, 1], ids=["copy-below", "copy-above"])
def test_duplicated_winner_in_a_screened_block(name, which):
    """A copy of the winner in a block whose other 127 candidates the oracle screens against the largest seed -- one such
    block behind the first round and low, one at the end: the lower of the two indices wins."""
    val, w = _plain_unpruned(name, "eta+3")
    at = S.RECORDED[name]["dup_blocks"][which] * PC.CAND_BLOCK + (5, 9)[which]
    assert at // PC.CAND_BLOCK != w // PC.CAND_BLOCK
    Xq = PC.candidates(name).copy()
    Xq[at] = Xq[w]
    param = _param(name, "eta+3")
    want = _unpruned(name, param, Xq)
    for variant in (0, STATIC):
        got, _, _ = _pruned(name, param, Xq, variant)
        _same(got, want)
        assert got == (val, min(w, at))


@CONFIGS
def test_nan_coordinates_in_the_block_of_the_largest_seed(name):
    top = S.RECORDED[name]["top_seed"]
    blk0 = top // PC.CAND_BLOCK * PC.CAND_BLOCK
    Xq = PC.candidates(name).copy()
    for i in (top, blk0, blk0 + 1, blk0 + PC.CAND_BLOCK - 1, 0, RAGGED):
        Xq[i, i % Xq.shape[1]] = np.nan
    param = _param(name, "eta+3")
    want = _unpruned(name, param, Xq)
    got, counters, screened = _pruned(name, param, Xq)
    _same(got, want)
    assert got[0] == got[0] and not np.isnan(Xq[got[1]]).any()
    assert 0 <= screened <= counters[1] <= NBLK


@CONFIGS
def test_index_base(name):
    val, idx = _plain_unpruned(name, "eta+0.5")
    base = (1 << 40) + 7
    param = _param(name, "eta+0.5")
    want = _unpruned(name, param, PC.candidates(name), base)
    got, _, _ = _pruned(name, param, PC.candidates(name), index_base=base)
    _same(got, want)
    assert got == (val, base + idx)


@CONFIGS
def test_a_huge_call_leaves_nothing_behind(name):
    """eta = 1e6 (every seed about 1e6), then an ordinary call on the same handle: it equals a fresh handle's; then a call
    that can give nothing up: its counters are those of a launch that started from zero."""
    eng, eta = _shared(name)
    huge, _, _ = _pruned(name, 1e6, PC.candidates(name))
    assert huge[0] > 1e5
    second, counters, screened = _pruned(name, eta, PC.candidates(name))
    fresh = _engine(name)
    want = fresh.acq_argmax("ei", eta, PC.candidates(name))[:2]
    fresh.close()
    _same(second, want)
    _same(second, _plain_unpruned(name, "eta"))
    _check_counters(name, "eta", 0, counters, screened)
    _, counters, screened = _pruned(name, -1e6, PC.candidates(name))
    assert (counters, screened) == ((NBLK, 0, 0), 0)


@CONFIGS
def test_same_call_twice_same_bits(name):
    param = _param(name, "eta+0.5")
    a, _, _ = _pruned(name, param, PC.candidates(name))
    b, _, _ = _pruned(name, param, PC.candidates(name))
    _same(a, b)
    _same(a, _plain_unpruned(name, "eta+0.5"))
