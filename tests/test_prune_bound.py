"""CPU: the give-up rule of the pruned EI arg-max (tests/prune_cases.py states it) against the numpy restatement of the
engine's EI tail, and against the oracle on whole sweeps.

1. The rule's margin covers what the tail's own rounding can do to its monotonicity in the variance: over z from -38 to 8
   and variances from VAR_FLOOR to 1, with the second variance 1 ulp to a factor 2 above the first, the value at the
   larger variance is never below the value at the smaller one by more than MARGIN (wherever the rule can act at all:
   above MIN_BEST).
2. On a 512-point model the block-stop rule never discards the arg-max, ties included, however late a block learns of the
   others' maxima.
3. The planted-candidate sweeps of tests/test_gpu_prune.py are not vacuous: by the oracle alone at least half of the
   blocks behind the first round are given up against the planted candidate's value."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import prune_cases as PC


def _ulps(x, k):
    return (x.view(np.int64) + k).view(np.float64)


def test_margin_covers_the_tails_monotonicity_in_the_variance():
    z = np.concatenate([np.linspace(-38.0, 8.0, 1841), [-37.5, -30.0, -20.0, -1e-3, 0.0, 1e-3]])
    var = np.geomspace(O.VAR_FLOOR, 1.0, 97)
    Z, V = np.meshgrid(z, var, indexing="ij")
    diff = Z * np.sqrt(V)                         # eta - mean: z at the smaller variance
    lo = PC.ei_tail(diff, V)
    checked = 0
    steps = [_ulps(V, k) for k in (1, 2, 3, 16, 1 << 10, 1 << 20, 1 << 30, 1 << 40)]
    steps += [V * f for f in (1.0 + 1e-6, 1.0 + 1e-3, 1.01, 1.1, 1.5, 2.0)]
    for V2 in steps:
        assert np.all(V2 > V) and np.all(V2 <= 2.0 * V)
        ub = PC.ei_tail(diff, V2)
        live = lo > PC.MIN_BEST
        checked += int(live.sum())
        bad = live & (ub * PC.MARGIN < lo)       # the rule would give up a candidate whose value is `lo`
        assert not bad.any(), (Z[bad][:5], V[bad][:5], V2[bad][:5], lo[bad][:5], ub[bad][:5])
    assert checked > 1_000_000                    # not vacuous: most of the grid lies above MIN_BEST


def test_tail_restatement_matches_the_oracle():
    rng = np.random.default_rng(3)
    mean, var = rng.normal(size=2000), rng.uniform(1e-6, 1.0, size=2000)
    ref = O.expected_improvement(mean, var, -0.3)
    np.testing.assert_allclose(PC.ei_tail(-0.3 - mean, var), ref, rtol=1e-9, atol=1e-300)


@pytest.fixture(scope="module")
def small_sweep():
    """A 512-point model (two row blocks) swept over 96 candidate blocks, the last one ragged."""
    st, eta = PC.oracle_state("m52_N512_d8")
    Xq = PC.candidates("m52_N512_d8")[: 95 * PC.CAND_BLOCK + 77].copy()
    mean, ub = PC.partial_bounds(st, eta, Xq)
    return Xq, mean, ub


@pytest.mark.parametrize("lag", [1, 7, 1000], ids=["lag1", "lag7", "never"])
def test_block_stop_rule_keeps_the_argmax(small_sweep, lag):
    Xq, mean, ub = small_sweep
    want = int(O.argmax_first(ub[-1]))
    val, idx, given = PC.sweep_with_rule(mean, ub, lag)
    assert (val, idx) == (float(ub[-1, want]), want)
    if lag < 1000:
        assert given.any()                        # the rule acts on this model
    else:
        assert not given.any()                    # nothing known, nothing given up


@pytest.mark.parametrize("first", ["low", "high"])
def test_block_stop_rule_keeps_ties(small_sweep, first):
    """The winner's bounds duplicated in two blocks: neither copy is given up and the lower index wins, whichever of the two
    the sweep meets first."""
    Xq, mean, ub = small_sweep
    w = int(O.argmax_first(ub[-1]))
    a, b = 3 * PC.CAND_BLOCK + 5, 80 * PC.CAND_BLOCK + 9
    mean, ub = mean.copy(), ub.copy()
    for i in (a, b):
        mean[i], ub[:, i] = mean[w], ub[:, w]
    if first == "high":                           # sweep the blocks in reverse: the higher index finishes first
        m = ub.shape[1]
        nblk = -(-m // PC.CAND_BLOCK)
        order = np.concatenate([np.arange(k * PC.CAND_BLOCK, min(m, (k + 1) * PC.CAND_BLOCK)) for k in range(nblk - 2, -1, -1)])
        val, idx, given = PC.sweep_with_rule(mean[order], ub[:, order], 1)
        vals = np.full(m, -np.inf)
        vals[order] = np.where(np.repeat(given, PC.CAND_BLOCK)[: order.size], -np.inf, ub[-1, order])
    else:
        val, idx, given = PC.sweep_with_rule(mean, ub, 1)
        vals = np.where(np.repeat(given, PC.CAND_BLOCK)[: ub.shape[1]], -np.inf, ub[-1])
    keep = set(np.flatnonzero(vals == ub[-1].max()))
    assert keep >= {a, b} and int(O.argmax_first(vals)) == min(keep | {a, b})


@pytest.mark.parametrize("name", PC.SHARE_IDS)
def test_planted_candidate_lets_the_oracle_give_up_half_the_blocks(name):
    """The share tests/test_gpu_prune.py asks of the engine, by the oracle: against the planted candidate's value alone
    (what every block behind the first round knows at least) half of a 48-block sample of those blocks is given up."""
    st, eta = PC.oracle_state(name)
    p = PC.problem(name)
    first = PC.FIRST_ROUND * PC.CAND_BLOCK
    Xq = np.vstack([p.plant[None, :], PC.candidates(name)[first: first + 48 * PC.CAND_BLOCK]])
    mean, ub = PC.partial_bounds(st, eta, Xq)
    best = ub[-1, 0]
    blocks = ub[:-1, 1:].reshape(ub.shape[0] - 1, 48, PC.CAND_BLOCK)
    given = [any(PC.gives_up(blocks[i, b], best) for i in range(blocks.shape[0])) for b in range(48)]
    print(name, "planted EI", best, "sample max EI", ub[-1, 1:].max(), "given up", sum(given), "of 48")
    assert sum(given) >= 24
