"""GPU: cutting the few-blocks path's wave tiles into halves and quarters changes no bit and no counter.

While the tile items of a launch leave SIMDs idle, prune_tile_kernel cuts every 64 x 32 wave tile into parts of its eight
accumulator fragments: quarters (one fm pair, one fn) while S nb 64 parts fit the device's SIMDs and the
grid, halves (one fm pair) while S nb 32 do, whole items beyond.  Each accumulator keeps its MFMA sequence and its dump word,
so nothing may move.  tgp_set_variant bit 18 (262144) keeps whole items: every case compares the default with it by winner
value bits, index, every counter and ``prune_tiles`` (which counts wave tiles, S nb 16, however they are cut), with bit 15
(no few-blocks path) by everything but ``prune_tiles``, and with bit 11 (no pruning) by the winner.

Models: those of tests/test_gpu_prune_tiles.py (2, 3 and 5 row blocks) and two of N = 512 and 1024 (2 and 4 row blocks).
Under bit 12 every block survives, S = P, so on the 1024 SIMDs of an MI355X the counts P below sit on every side of the
rule: nb = 2 cuts quarters up to S = 8 and halves up to 16, nb = 4 quarters up to 4 and halves up to 8, nb = 5 quarters up
to 3 and halves up to 6.  A count ends in a ragged block where `ragged` says so.  (On a device with another number of SIMDs the
thresholds move; the comparison holds wherever they are.)

What this file proves is equality, not that a cut took place: no counter says which cut ran, and with the rule never cutting
every comparison would still hold.  That the cuts are taken shows in the kernel's time and in the planted defect
(profiles/r31_prescreen_issue.txt): a part writing its fm pair to the other half's dump words, built once into a library of its
own, fails 16 of the 22 cases here (11 of test_every_block_survives, 5 of test_screened_launches) by the winner's value bits --
not all of them, since the fold adds the squares of all of a column's fm words and the defect only reorders that sum."""
import functools

import numpy as np
import pytest

from tests import prune_cases as PC
from tests import test_gpu_prune_tiles as T

pytestmark = pytest.mark.gpu

WHOLE = 262144                                   # tgp_set_variant bit 18
MODELS = dict(T.MODELS, m52_N512_d8=("matern52", 512, 8), rbf_N1024_d6=("rbf", 1024, 6))
COUNTS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17)     # blocks; the split cap of every launch is 64, the path's own cap 32
CONFIGS = pytest.mark.parametrize("name", list(MODELS))


@functools.lru_cache(maxsize=None)
def _model(name):
    """-> (engine, eta, candidates [17 blocks, d], read-only)."""
    from oracle import gp_oracle as O
    from trieste_amd.engine import GPEngine

    kind, N, d = MODELS[name]
    X, Y = O.synthetic_problem(O.ackley, d, N)
    eng = GPEngine(d, kind, device=0)
    eng.set_hyper(1.0, O.default_lengthscales(d), 1e-2, 0.0)
    eng.set_data(X, Y)
    Xq = np.random.default_rng(1231).uniform(size=(max(COUNTS) * PC.CAND_BLOCK, d))
    Xq.setflags(write=False)
    return eng, eng.eta(), Xq


def _launch(name, variant, param, Xq):
    from trieste_amd import engine as E

    eng = _model(name)[0]
    eng.set_variant(variant | T.NO_SPLIT)
    E.set_prune_split(eng, 64, 0)
    v, i, _ = eng.acq_argmax("ei", param, np.ascontiguousarray(Xq))
    out = dict(winner=(T._bits(v), i), counters=E.prune_counters(eng), screened=E.prune_screened(eng),
               prescreened=E.prune_prescreened(eng), split=E.prune_split(eng))
    tiles = E.prune_tiles(eng)
    E.set_prune_split(eng)
    eng.set_variant(0)
    return out, tiles


def _compare(name, variant, param, Xq):
    nrb = -(-MODELS[name][1] // PC.ROW_BLOCK)
    got, tiles = _launch(name, variant, param, Xq)
    whole, whole_tiles = _launch(name, variant | WHOLE, param, Xq)
    old, off = _launch(name, variant | T.NO_FEW, param, Xq)
    plain, _ = _launch(name, T.NO_PRUNE, param, Xq)
    print(f"{name} M={len(Xq)} variant={variant}: {got}; (pre-listed, tile items) {tiles}")
    assert (got, tiles) == (whole, whole_tiles), (got, tiles, whole, whole_tiles)
    assert got == old and off == (0, 0), (got, old, off)
    assert got["winner"] == plain["winner"], (got, plain)
    assert tiles[1] == got["split"][0] * nrb * 16 > 0   # the path ran, and its count is in wave tiles whatever the cut
    return got


@CONFIGS
@pytest.mark.parametrize("ragged", [False, True], ids=["full", "ragged"])
def test_every_block_survives(name, ragged):
    """Bit 12: S = P on both sides of the quarters' and of the halves' rule."""
    _, eta, Xq = _model(name)
    for P in COUNTS:
        got = _compare(name, T.NO_SCREEN, eta + 0.5, Xq[: P * PC.CAND_BLOCK - (37 if ragged else 0)])
        assert got["split"][0] == P


@CONFIGS
def test_screened_launches(name):
    """The default launch: the screen leaves S <= P of the pre-listed blocks, at two thresholds."""
    _, eta, Xq = _model(name)
    for P in (1, 2, 9, 17):
        for param in (eta, eta + 0.5):
            _compare(name, 0, param, Xq[: P * PC.CAND_BLOCK - 5])


def test_the_bit_alone_changes_nothing():
    """Without the few-blocks path (bit 15) bit 18 names nothing: the launch is the same launch."""
    name = "m52_N512_d8"
    _, eta, Xq = _model(name)
    assert _launch(name, T.NO_FEW, eta + 0.5, Xq[:389]) == _launch(name, T.NO_FEW | WHOLE, eta + 0.5, Xq[:389])
