"""GPU: the pruned EI arg-max returns the unpruned sweep's winner, bit for bit.

``acq_argmax("ei", ...)`` over >= 4 x #CU candidate blocks gives a block up at a row-block boundary once no candidate of
it can still win (the rule is restated in tests/prune_cases.py and checked against the oracle on the CPU
by tests/test_prune_bound.py).  tgp_set_variant bit 11 runs the same launch without giving anything up: every case
compares the two (value bits and index).  Models and candidate sets come from tests/prune_cases.py: N in {256 (one row
block: no checkpoint), 512, 700 (pads to 768), 768}, d in {2, 8, 16}, noise 1e-2 and 1e-5, all four kernels at N = 512;
131072 + 77 candidates are 4 x 256 full blocks and a ragged one."""
import functools
import struct

import numpy as np
import pytest

from tests import prune_cases as PC

pytestmark = pytest.mark.gpu

NO_PRUNE = 2048
NBLK = -(-PC.M // PC.CAND_BLOCK)
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


def _bits(v):
    return struct.pack("<d", v)


def _both(name, Xq, acq="ei", param=None, index_base=0):
    """-> ((value, index) pruned, counters, (value, index) unpruned), after asserting that the two are the same bits."""
    from trieste_amd.engine import prune_counters

    eng, eta = _shared(name)
    param = eta if param is None else param
    eng.set_variant(NO_PRUNE)
    wv, wi, _ = eng.acq_argmax(acq, param, Xq, index_base)
    assert prune_counters(eng) == (0, 0, 0)
    eng.set_variant(0)
    gv, gi, _ = eng.acq_argmax(acq, param, Xq, index_base)
    counters = prune_counters(eng)
    print(f"{name}: value {gv!r} index {gi} (unpruned {wv!r} {wi}); blocks, given up, row blocks skipped = {counters}")
    assert (_bits(gv), gi) == (_bits(wv), wi)
    return (gv, gi), counters, (wv, wi)


@functools.lru_cache(maxsize=None)
def _plain(name):
    """The plain set's winner (both ways, compared) and its point: the planted-winner cases move it around."""
    Xq = PC.candidates(name)
    got, counters, _ = _both(name, Xq)
    return got, counters, Xq[got[1]].copy()


def _winner_moved_to(name, index):
    """The plain set with its winner moved to `index` (its old place takes a copy of the point behind it)."""
    (_, old), _, x = _plain(name)
    Xq = PC.candidates(name).copy()
    Xq[old] = Xq[(old + 1) % PC.M]
    Xq[index] = x
    return Xq


@CONFIGS
def test_plain_candidates(name):
    (val, idx), (blocks, given, skipped), _ = _plain(name)
    assert blocks == NBLK and val > 0.0 and 0 <= idx < PC.M
    nrb = -(-PC.problem(name).N // PC.ROW_BLOCK)
    assert 0 <= given <= NBLK and given <= skipped <= given * max(nrb - 1, 0)   # N = 256: no checkpoint, nothing given up


@CONFIGS
@pytest.mark.parametrize("where", [FIRST, LAST_FULL, RAGGED], ids=["first-block", "last-full-block", "ragged-tail"])
def test_winner_planted(name, where):
    (val, _), _, _ = _plain(name)
    got, _, _ = _both(name, _winner_moved_to(name, where))
    assert got == (val, where)


@CONFIGS
@pytest.mark.parametrize("pair", [(2 * 128 + 3, 700 * 128 + 9), (250 * 128 + 1, 260 * 128 + 2), (1000 * 128 + 5, RAGGED)],
                         ids=["rounds-0-and-2", "neighbouring-rounds", "last-round-and-tail"])
def test_duplicated_winner_lower_index_wins(name, pair):
    """The winner at two indices in different blocks -- the lower one finished long before the higher one starts, the two in
    flight at about the same time, both late: the lower index wins."""
    (val, _), _, _ = _plain(name)
    Xq = _winner_moved_to(name, pair[0])
    Xq[pair[1]] = Xq[pair[0]]
    got, _, _ = _both(name, Xq)
    assert got == (val, pair[0])


@CONFIGS
def test_index_base(name):
    (val, idx), _, _ = _plain(name)
    base = (1 << 40) + 7
    got, _, _ = _both(name, PC.candidates(name), index_base=base)
    assert got == (val, base + idx)


@CONFIGS
def test_nan_coordinates(name):
    Xq = PC.candidates(name).copy()
    for i in (0, 77, 128 * 300 + 5, LAST_FULL, RAGGED, PC.M - 1):
        Xq[i, i % Xq.shape[1]] = np.nan
    (val, idx), _, _ = _both(name, Xq)
    assert val == val and not np.isnan(Xq[idx]).any()


@CONFIGS
def test_eta_so_low_that_every_ei_is_zero(name):
    (val, idx), (blocks, given, skipped), _ = _both(name, PC.candidates(name), param=-1e6)
    assert (_bits(val), idx) == (_bits(0.0), 0)
    assert (blocks, given, skipped) == (NBLK, 0, 0)


@CONFIGS
def test_second_call_does_not_see_the_first_calls_best(name):
    """A call whose EI values are huge, then an ordinary one on the same handle: the second equals a fresh handle's."""
    eng, eta = _shared(name)
    eng.set_variant(0)
    huge, _, _ = eng.acq_argmax("ei", 1e6, PC.candidates(name))
    assert huge > 1e5
    second = eng.acq_argmax("ei", eta, PC.candidates(name))[:2]
    fresh = _engine(name)
    want = fresh.acq_argmax("ei", eta, PC.candidates(name))[:2]
    fresh.close()
    assert (_bits(second[0]), second[1]) == (_bits(want[0]), want[1]) == (_bits(_plain(name)[0][0]), _plain(name)[0][1])


@CONFIGS
@pytest.mark.parametrize("acq,param", [("pi", None), ("nlcb", 1.96), ("aei", None)])
def test_other_tails_are_not_pruned(name, acq, param):
    _, counters, _ = _both(name, PC.candidates(name), acq=acq, param=param)
    assert counters == (0, 0, 0)


@CONFIGS
def test_planted_first_block_gives_blocks_up(name):
    """The candidate PLANT_DISTANCE lengthscales from the training minimum in the first block: blocks are given up, and at
    N >= 512 at least half of those behind the first round (tests/test_prune_bound.py: the oracle's side of that share)."""
    _, (blocks, given, skipped), _ = _both(name, PC.planted(name, FIRST))
    assert blocks == NBLK
    if name in PC.SHARE_IDS:
        assert given > 0 and skipped >= given
        assert 2 * given >= NBLK - PC.FIRST_ROUND, (given, NBLK - PC.FIRST_ROUND)
    else:
        assert (given, skipped) == (0, 0)
