"""CPU: the seed and the mean screen of the pruned EI arg-max (tests/prune_screen_cases.py states them) against the oracle.

1. eta - mean bounds the tail from below at every variance: on a grid of diff in (0, 10] and var in [1e-12, 1],
   ei_tail(diff, var) >= diff (1 - 1e-5).  (What lets a seed stand where a finished maximum stood.)
2. On every model of tests/prune_cases.py, at the model's eta, eta + 0.5, eta + 3 and -1e6, with the blocks taken as dealt,
   reversed and shuffled, and with each block knowing the others' seeds and maxima at once (lag 1) or never (lag 256 on 96
   blocks): the surviving winner is the arg-max of the full values, value and index; the block that supplies the largest
   seed is never screened; every seed is <= (1 + 1e-5) x its candidate's final value.
3. The table the GPU test takes its shares from (RECORDED) is what the functions give on the whole plain set."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import prune_cases as PC
from tests import prune_screen_cases as S


def test_eta_minus_mean_bounds_the_tail_from_below():
    diff = np.concatenate([np.geomspace(1e-12, 10.0, 1201), np.linspace(1e-3, 10.0, 1000)])
    var = np.geomspace(1e-12, 1.0, 241)
    D, V = np.meshgrid(diff, var, indexing="ij")
    ei = PC.ei_tail(D, V)
    bad = ~(ei >= D * (1.0 - S.SEED_RTOL))
    assert not bad.any(), (D[bad][:5], V[bad][:5], ei[bad][:5])


def test_moments_are_those_of_partial_bounds():
    name = "m52_N700_d8"
    st, eta = PC.oracle_state(name)
    mean, var = S.sample_moments(name)
    pmean, pub = PC.partial_bounds(st, eta, PC.candidates(name)[: S.SAMPLE])
    assert np.array_equal(mean, pmean) and np.array_equal(PC.ei_tail((eta - mean)[None, :], var), pub)


@pytest.mark.parametrize("lag", [1, 256])
@pytest.mark.parametrize("order", ["identity", "reversed", "shuffled"])
@pytest.mark.parametrize("label", S.THRESHOLDS)
@pytest.mark.parametrize("name", PC.IDS)
def test_screen_keeps_the_argmax(name, label, order, lag):
    st, _ = PC.oracle_state(name)
    eta = S.threshold(name, label)
    mean, var = S.sample_moments(name)
    nblk = -(-S.SAMPLE // PC.CAND_BLOCK)
    val, idx, given, screened, seed = S.sweep_with_screen(mean, var, eta, st.variance, S.orders(nblk)[order], lag)
    full = PC.ei_tail(eta - mean, var[-1])
    want = int(O.argmax_first(full))
    assert (val, idx) == (float(full[want]), want)
    assert not (screened & ~given).any()
    if seed.max() > 0.0:
        assert not screened[int(np.argmax(seed))]
    pos = eta - mean > 0.0
    assert np.all((eta - mean)[pos] <= (1.0 + S.SEED_RTOL) * full[pos])
    if st.N <= PC.ROW_BLOCK or label == "-1e6":
        assert not given.any()                    # one row block: no screen, no checkpoint; every EI 0: nothing to compare with
    if lag >= nblk:
        assert not screened.any()                 # a block's own seed never screens the block itself
    elif label == "eta+3" and st.N > PC.ROW_BLOCK:
        assert screened.any()                     # not vacuous: with the others' seeds known the screen acts


def test_recorded_table_is_what_the_oracle_gives():
    """Slow for a CPU test (the means of 131 149 candidates per model); the GPU test reads the table instead."""
    for name in PC.IDS:
        rec = S.RECORDED[name]
        got = {label: S.oracle_screened(name, label) for label in S.THRESHOLDS}
        print(name, got)
        assert got == rec["screened"]
        assert S.top_seed_candidate(name, "eta+3") == rec["top_seed"]
        b = S.blocks_screened_against_top_seed(name, "eta+3")
        assert (int(b[b >= S.DUP_FLOOR][0]), int(b[-1])) == rec["dup_blocks"]
        assert rec["top_seed"] // PC.CAND_BLOCK not in set(b.tolist())
    # the shares the GPU test asserts clear the cap of one half by the oracle's own figures, at every N >= 512
    assert S.SHARE_CASES and {n for n, _ in S.SHARE_CASES} == set(PC.SHARE_IDS)
    assert all(2 * S.RECORDED[n]["screened"][t] >= S.NBLK for n, t in S.SHARE_CASES)
    assert all(v == 0 for v in S.RECORDED["m52_N256_d8"]["screened"].values())
    assert all(S.RECORDED[n]["screened"]["-1e6"] == 0 for n in PC.IDS)
