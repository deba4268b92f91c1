"""GPU: the packed pre-screen (two candidates per thread) keeps every bit of the scalar one.

Phase 0 of the pruned EI arg-max holds two candidates of a block, columns j and j + 64, as the halves of a 2-vector and forms
their distances with the packed float32 instructions; tgp_set_variant bit 16 (65536) runs the earlier kernel, one candidate
per thread.  Per half a packed instruction is the scalar one, so nothing may move: mean32 and E are compared as 64-bit
patterns (NaN patterns included), and a launch by its winner's value bits and index and by every counter it leaves.

Models: N = 512 (two row blocks, the smallest at which phase 0 runs), Ackley targets as tests/prune_cases.py builds them, for
every kernel kind at d = 2, 8, 16 (exact) and d = 3, 5 (padded to 4 and 6): the twenty instantiations of the kernel.
Candidate counts: around the half boundary (63, 64, 65), the block boundary (127, 128, 129), the pair boundary (255, 256, 257),
an odd number of blocks (1, 129, 257, 384, 385) and M_PASSES, at which a workgroup of the read-back launch takes a second pair.

Planted defects (each built once into a library of its own, this file of 64 cases run against it):
  * the two halves written back exchanged (the high half's sum to column j, the low half's to column j + 64): 40 cases fail --
    every test_mean32_and_bound_bit_for_bit and every test_pair_mates_do_not_leak case.  The launches cannot see it: a block's
    bound and seed are maxima over its columns;
  * the high half taking the low half's row coordinate with its sign dropped (t.y = x.y + b where t.y = x.y - b stands): 48 cases
    fail -- the same 40, test_launch_keeps_its_bits at d = 2 and 3 (rbf, matern32, matern52) and test_pre_screening_at_scale on
    matern52 d = 8 and rbf d = 5."""
import functools
import struct

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import prescreen_cases as R
from tests import prune_cases as PC

pytestmark = pytest.mark.gpu

SCALAR = 65536                                   # tgp_set_variant bit 16
NO_PRUNE, NO_SCREEN, STATIC, NO_FEW = 2048, 4096, 8192, 32768
NO_SPLIT = 1                                     # a launch of a few blocks stays on the fused (pruned) kernels
N = 512
DIMS = (2, 3, 5, 8, 16)
MS = (1, 63, 64, 65, 127, 128, 129, 255, 256, 257, 384, 385)
# the read-back launch has at most two workgroups per compute unit, each taking a pair of blocks per pass: past four blocks
# per compute unit of the largest part (256) some workgroup makes a second pass; the odd count leaves its last pair half empty
M_PASSES = (4 * 256 + 2) * PC.CAND_BLOCK + 5
MODELS = pytest.mark.parametrize("kind,d", [(k, d) for k in R.KINDS for d in DIMS], ids=lambda v: str(v))


@functools.lru_cache(maxsize=None)
def _model(kind, d):
    """-> (engine, eta, candidates [M_PASSES, d], read-only) of the N = 512 model of (kind, d)."""
    from trieste_amd.engine import GPEngine

    X, Y = O.synthetic_problem(O.ackley, d, N)
    eng = GPEngine(d, kind, device=0)
    eng.set_hyper(1.0, O.default_lengthscales(d), 1e-2, 0.0)
    eng.set_data(X, Y)
    Xq = np.random.default_rng(977 + d).uniform(size=(M_PASSES, d))
    Xq.setflags(write=False)
    return eng, eng.eta(), Xq


def _means(eng, variant, Xq):
    from trieste_amd.engine import prescreen_means

    eng.set_variant(variant)
    m32, E = prescreen_means(eng, np.ascontiguousarray(Xq))
    eng.set_variant(0)
    return np.asarray(m32), np.asarray(E)


def _same_patterns(got, want, what):
    bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} differ, first at {bad[:8]}: {got[bad[:4]]} vs {want[bad[:4]]}"


def _launch(eng, variant, param, Xq):
    """-> everything an arg-max leaves behind under `variant` (never the row-group split of small launches, which has no
    phase 0: bit 0 in every launch, on both sides of every comparison)."""
    from trieste_amd import engine as E

    eng.set_variant(variant | NO_SPLIT)
    v, i, _ = eng.acq_argmax("ei", param, np.ascontiguousarray(Xq))
    out = dict(winner=(struct.pack("<d", v), i), counters=E.prune_counters(eng), screened=E.prune_screened(eng),
               prescreened=E.prune_prescreened(eng), split=E.prune_split(eng), tiles=E.prune_tiles(eng))
    eng.set_variant(0)
    return out


@MODELS
def test_mean32_and_bound_bit_for_bit(kind, d):
    eng, _, Xq = _model(kind, d)
    for m in MS + (M_PASSES,):
        got_m, got_e = _means(eng, 0, Xq[:m])
        want_m, want_e = _means(eng, SCALAR, Xq[:m])
        assert np.all(np.isfinite(want_m)) and np.all(want_e > 0.0)
        _same_patterns(got_m, want_m, f"mean32 at M = {m}")
        _same_patterns(got_e, want_e, f"E at M = {m}")


# (M, the bad candidate, its pair-mate): low half and high half of a full block; the last valid column of a partial block
LEAKS = [(256, 3, 67), (256, 128 + 67, 128 + 3), (200, 199, 135)]


@MODELS
def test_pair_mates_do_not_leak(kind, d):
    eng, eta, Xq0 = _model(kind, d)
    for m, j, mate in LEAKS:
        clean_m, clean_e = _means(eng, SCALAR, Xq0[:m])
        for bad in (np.nan, np.inf):
            Xq = Xq0[:m].copy()
            Xq[j, j % d] = bad
            got_m, got_e = _means(eng, 0, Xq)
            want_m, want_e = _means(eng, SCALAR, Xq)
            _same_patterns(got_m, want_m, f"mean32, {bad} in candidate {j} of {m}")
            _same_patterns(got_e, want_e, f"E, {bad} in candidate {j} of {m}")
            # the mate, and everyone else, is what it was without the bad coordinate
            keep = np.arange(m) != j
            _same_patterns(got_m[keep], clean_m[keep], f"mean32 beside candidate {j} of {m}")
            _same_patterns(got_e[keep], clean_e[keep], f"E beside candidate {j} of {m}")
            assert np.isfinite(got_m[mate]) and np.isfinite(got_e[mate])
            # the block's bound is +inf under both: the kernel's rule (prescreen_cases.block_quantities) on what either form
            # returned for the candidate, and an arg-max that pre-screens the same blocks under both
            assert not (np.isfinite(got_m[j]) and np.isfinite(got_e[j]))
            for mm, ee in ((got_m, got_e), (want_m, want_e)):
                ub, _ = R.block_quantities(eta, 1.0, mm, ee)
                assert np.isposinf(ub[j // PC.CAND_BLOCK]) and np.all(np.isfinite(np.delete(ub, j // PC.CAND_BLOCK)))
            assert _launch(eng, 0, eta + 3.0, Xq) == _launch(eng, SCALAR, eta + 3.0, Xq)


@MODELS
def test_launch_keeps_its_bits(kind, d):
    eng, eta, Xq = _model(kind, d)
    for m in (129, 255, 256, 257, 384, 385):
        unpruned = _launch(eng, NO_PRUNE, eta, Xq[:m])["winner"]
        for other in (0, NO_SCREEN, STATIC, NO_FEW):
            got, want = _launch(eng, other, eta, Xq[:m]), _launch(eng, other | SCALAR, eta, Xq[:m])
            assert got == want, (m, other, got, want)
            assert got["winner"] == unpruned
            assert got["counters"][0] == -(-m // PC.CAND_BLOCK)


@pytest.mark.parametrize("kind,d", [("matern52", 8), ("rbf", 5), ("matern32", 16)])
def test_pre_screening_at_scale(kind, d):
    """Enough blocks that phase 0 dismisses some (a block count where every workgroup of the arg-max takes several pairs)."""
    eng, eta, Xq = _model(kind, d)
    got, want = _launch(eng, 0, eta, Xq), _launch(eng, SCALAR, eta, Xq)
    print(f"{kind} d = {d}: {got}")
    assert got == want
    assert got["winner"] == _launch(eng, NO_PRUNE, eta, Xq)["winner"]
    if (kind, d) == ("matern52", 8):   # the model of prescreen_cases.SHARE_CASE, where the restatement dismisses blocks at eta
        assert got["prescreened"] > 0


def test_variant_bit_alone_changes_nothing():
    """Bit 16 names the form of phase 0 and nothing else: with phase 0 off (bit 14) the launch is the same launch."""
    eng, eta, Xq = _model("matern52", 8)
    assert _launch(eng, 16384, eta, Xq[:385]) == _launch(eng, 16384 | SCALAR, eta, Xq[:385])
