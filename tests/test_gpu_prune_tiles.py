"""GPU: the few-blocks path of the pruned EI arg-max changes no bit and no counter.

When the float32 pre-screen leaves a handful of blocks (P <= its cap), the launch generates the K* of each ONCE into a
slab, forms the means from the slab, and cuts every survivor's row blocks into 64 x 32 wave tiles over all compute units
(DESIGN.md 4.1).  tgp_set_variant bit 15 runs without the path, bit 11 without pruning: every case compares winner value
bits and index with both, and blocks / given up / skipped, screened, pre-screened and (survivors, items) with bit 15.
``prune_tiles`` reports (blocks pre-listed, tile items); items is 0 when the path was not taken.

Shapes: N = 257, 600 and 1100 (2, 3 and 5 row blocks), all four kernel kinds, padded dimensions 2, 4, 6, 8 and 16,
M in {1, 127, 128, 129, 3 * 128 + 5}.  Launches this small reach the fused kernels only under variant bit 0 (no row-group
split), and their derived split cap is #blocks / 2: the cases run under the derived cap and under a cap of #blocks, where
every block may take the path.

Which test catches which planted fault in prune_tile_kernel (both show in the winner's value bits; neither changes a
counter, the counters are decided before the tiles run):
  * a wrong dump word (fn ^ 1 in the store: the two 16-column fragments of a wave tile exchanged): test_same_bits_and_counters
    at every M >= 127 (at M = 1 the columns past M repeat candidate 0, so the exchanged column holds the same value),
    test_both_sides_of_the_cap, test_a_small_launch_after_a_large_one and test_an_exact_tie -- 33 of the 48 cases;
  * a dropped last k-step (the item's last tile_step skipped; it carries the diagonal of W): the same tests and
    test_same_bits_and_counters at M = 1 on four of the five models -- 37 of the 48 cases."""
import functools
import types

import numpy as np
import pytest

from tests import prune_cases as PC

pytestmark = pytest.mark.gpu

NO_SPLIT, NO_PRUNE, NO_SCREEN, NO_FEW = 1, 2048, 4096, 32768
FEW_MAX = 32          # PRUNE_FEW_MAX of trieste_amd/csrc/tgp_internal.hpp
MODELS = {
    "m52_N257_d8": ("matern52", 257, 8),      # dp 8, 2 row blocks
    "rbf_N600_d5": ("rbf", 600, 5),           # dp 6, 3 row blocks
    "m32_N600_d3": ("matern32", 600, 3),      # dp 4
    "m12_N1100_d2": ("matern12", 1100, 2),    # dp 2, 5 row blocks
    "m52_N1100_d16": ("matern52", 1100, 16),  # dp 16
}
COUNTS = [1, 127, 128, 129, 3 * 128 + 5]
CONFIGS = pytest.mark.parametrize("name", list(MODELS))


@functools.lru_cache(maxsize=None)
def _problem(name):
    from oracle import gp_oracle as O

    kind, N, d = MODELS[name]
    p = types.SimpleNamespace(name=name, kind=kind, N=N, d=d, noise=1e-2, variance=1.0, mean_const=0.0)
    p.X, p.Y = O.synthetic_problem(O.ackley, d, N)
    p.ls = O.default_lengthscales(d)
    return p


@functools.lru_cache(maxsize=None)
def _shared(name):
    from trieste_amd.engine import GPEngine

    p = _problem(name)
    eng = GPEngine(p.d, p.kind, device=0)
    eng.set_hyper(p.variance, p.ls, p.noise, p.mean_const)
    eng.set_data(p.X, p.Y)
    return eng, eng.eta()


@functools.lru_cache(maxsize=None)
def _candidates(name):
    """FEW_MAX + 1 blocks, uniform on the unit box; read-only, the cases slice or copy it."""
    Xq = np.random.default_rng(977).uniform(size=((FEW_MAX + 1) * PC.CAND_BLOCK, _problem(name).d))
    Xq.setflags(write=False)
    return Xq


def _nrb(name):
    return -(-_problem(name).N // PC.ROW_BLOCK)


def _bits(v):
    return np.float64(v).tobytes()


def _launch(name, variant, param, Xq, cap=-1, eng=None):
    """One arg-max under `variant` (always without the row-group split) and a split cap -> everything compared."""
    from trieste_amd import engine as E

    eng = _shared(name)[0] if eng is None else eng
    eng.set_variant(variant | NO_SPLIT)
    E.set_prune_split(eng, cap, 0)
    v, i, _ = eng.acq_argmax("ei", param, Xq)
    out = dict(winner=(_bits(v), i), counters=E.prune_counters(eng), screened=E.prune_screened(eng),
               prescreened=E.prune_prescreened(eng), split=E.prune_split(eng))
    tiles = E.prune_tiles(eng)
    E.set_prune_split(eng)
    eng.set_variant(0)
    return out, tiles


def _compare(name, param, Xq, variant=0, cap=-1, eng=None):
    """The launch with the few-blocks path against bit 15 (everything) and bit 11 (the winner) -> (shared, tiles)."""
    want, off = _launch(name, variant | NO_FEW, param, Xq, cap, eng)
    plain, _ = _launch(name, NO_PRUNE, param, Xq, cap, eng)
    got, tiles = _launch(name, variant, param, Xq, cap, eng)
    print(f"{name} M={len(Xq)} variant={variant} cap={cap}: {got}; (pre-listed, tile items) {tiles}")
    assert off == (0, 0)
    assert got == want, (got, want)
    assert got["winner"] == plain["winner"], (got, plain)
    # the path is taken exactly when 1 <= P <= min(FEW_MAX, split cap, #workgroups = #blocks), and every survivor is cut
    # into 16 wave tiles per row block
    nblk = -(-len(Xq) // PC.CAND_BLOCK)
    few_max = min(FEW_MAX, nblk // 2 if cap < 0 else cap, nblk)
    P, items = tiles
    assert P == (nblk - got["prescreened"] if few_max > 0 else 0)
    assert items == (got["split"][0] * _nrb(name) * 16 if 1 <= P <= few_max else 0)
    return got, tiles


@CONFIGS
@pytest.mark.parametrize("m", COUNTS)
def test_same_bits_and_counters(name, m):
    """Screened (some pre-listed blocks do not survive) and under bit 12 (every block survives); derived cap and cap = #blocks."""
    Xq = _candidates(name)[:m]
    eta = _shared(name)[1]
    nblk = -(-m // PC.CAND_BLOCK)
    taken = 0
    for variant, param in ((0, eta + 0.5), (0, eta), (NO_SCREEN, eta + 0.5)):
        for cap in (-1, nblk):
            _, tiles = _compare(name, param, Xq, variant, cap)
            taken += tiles[1] > 0
    assert taken >= 3   # cap = #blocks lets every launch with a block left take the path


def test_both_sides_of_the_cap():
    """Bit 12, M = 128 P for P = 1 .. FEW_MAX + 1 under a split cap of 64: tile items are non-zero exactly up to FEW_MAX."""
    name = "rbf_N600_d5"
    eta = _shared(name)[1]
    for P in range(1, FEW_MAX + 2):
        got, tiles = _compare(name, eta + 0.5, _candidates(name)[: P * PC.CAND_BLOCK], NO_SCREEN, 64)
        assert got["split"][0] == P and tiles[0] == P
        assert (tiles[1] > 0) == (P <= FEW_MAX)


@CONFIGS
def test_never_split_switches_the_path_off(name):
    got, tiles = _compare(name, _shared(name)[1] + 0.5, _candidates(name)[:389], cap=0)
    assert tiles == (0, 0) and got["split"][1] == 0


@CONFIGS
def test_the_same_launch_twice(name):
    Xq = _candidates(name)[:389]
    param = _shared(name)[1] + 0.5
    first = _launch(name, NO_SCREEN, param, Xq, 4)
    assert first[1][1] > 0
    assert _launch(name, NO_SCREEN, param, Xq, 4) == first


@pytest.mark.parametrize("name", ["m52_N257_d8", "m12_N1100_d2"])
def test_a_small_launch_after_a_large_one(name):
    """Slabs, means and dump of a 16-block launch stay behind; the 3-block launch after it reads none of them."""
    from trieste_amd.engine import GPEngine

    p = _problem(name)
    eng = GPEngine(p.d, p.kind, device=0)
    eng.set_hyper(p.variance, p.ls, p.noise, p.mean_const)
    eng.set_data(p.X, p.Y)
    param = _shared(name)[1] + 0.5
    big, small = _candidates(name)[: 16 * PC.CAND_BLOCK], _candidates(name)[20 * PC.CAND_BLOCK : 23 * PC.CAND_BLOCK - 9]
    want = _launch(name, NO_SCREEN, param, small, 16)      # on the shared handle, whatever its history
    assert _launch(name, NO_SCREEN, param, big, 16, eng)[1][1] > 0
    assert _launch(name, NO_SCREEN, param, small, 16, eng) == want
    _compare(name, param, small, NO_SCREEN, 16, eng)
    eng.close()


@CONFIGS
@pytest.mark.parametrize("which", ["next-block", "block-after-next"])
def test_an_exact_tie(name, which):
    """The winner's coordinates copied into another block: the same value bits twice, and the smaller index wins."""
    Xq = _candidates(name)[:389].copy()
    param = _shared(name)[1] + 0.5
    vb, w = _launch(name, NO_PRUNE, param, Xq)[0]["winner"]
    wblk = w // PC.CAND_BLOCK
    at = ((wblk + 1) % 3) * PC.CAND_BLOCK + 7 if which == "next-block" else ((wblk + 2) % 3) * PC.CAND_BLOCK + 11
    assert at // PC.CAND_BLOCK != wblk
    Xq[at] = Xq[w]
    for variant in (0, NO_SCREEN):
        got, tiles = _compare(name, param, Xq, variant, 4)
        assert tiles[1] > 0
        assert got["winner"] == (vb, min(w, at))
