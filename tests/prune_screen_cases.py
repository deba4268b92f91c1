"""The numpy side of the seed and the mean screen of the pruned EI arg-max (TEST INFRASTRUCTURE; tests/test_prune_screen_bound.py
on the CPU, tests/test_gpu_prune_screen.py on the GPU).  Built on tests/prune_cases.py: its models, candidate sets, tail
restatement ``ei_tail`` and rule ``gives_up``.

Once a 128-candidate block's posterior means are known, the block

* posts its SEED, the largest ``eta - mean`` over its candidates if that is positive, to the launch's best word:
  EI(mean, var) >= eta - mean for every var > 0, so the seed bounds the block's final maximum from below;
* is SCREENED -- given up before its first row block -- when the rule of tests/prune_cases.py holds for every candidate
  with ``ub`` the EI tail at the PRIOR variance (the checkpoint's bound with an empty partial norm).  Models of one row
  block (N <= 256) screen nothing.

The best word a block sees is the largest of its own seed and of the seeds and finished maxima of the blocks that came
``lag`` or more places before it in the order the blocks are taken."""
import functools
import math

import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import gp_oracle as O
from tests import prune_cases as PC

SEED_RTOL = 1e-5                  # the engine's tails hold RTOL = 1e-5 (tests/acq_regimes.py): value >= seed (1 - SEED_RTOL)
THRESHOLDS = ("eta", "eta+0.5", "eta+3", "-1e6")
SAMPLE = 95 * PC.CAND_BLOCK + 77  # the CPU sweeps: 96 blocks of the plain set, the last one ragged
NBLK = -(-PC.M // PC.CAND_BLOCK)


def threshold(name, label):
    """The EI threshold of a case: the model's eta, eta shifted up (more and larger seeds) by 0.5 and 3 prior standard
    deviations, or so low that every EI is 0."""
    return thresholds(PC.problem(name), PC.oracle_state(name)[1])[label]


def thresholds(p, eta):
    """The four thresholds of a model p (variance, mean_const) around `eta`; at variance 1 and mean 0: eta, eta + 0.5,
    eta + 3 and -1e6 bit for bit."""
    sd = math.sqrt(p.variance)
    return {"eta": eta, "eta+0.5": eta + 0.5 * sd, "eta+3": eta + 3.0 * sd, "-1e6": -1e6 * sd + p.mean_const}


@functools.lru_cache(maxsize=None)
def sample_moments(name, bound_variance=None):
    """-> (mean [SAMPLE], var [nrb][SAMPLE]) of the first SAMPLE plain candidates: var[i] the variance bound after row
    blocks 0 .. i (var[-1]: the variance), as tests/prune_cases.partial_bounds forms them.  Read-only.
    ``bound_variance`` plants a defect: the checkpoints' bounds var[:-1] taken from it in place of the model's variance."""
    st, _ = PC.oracle_state(name)
    Xq = PC.candidates(name)[:SAMPLE]
    with PC.form(name):
        K = O.kernel_matrix(st.kind, st.variance, st.lengthscales, st.X, Xq)
    A = solve_triangular(st.L, K, lower=True)
    mean = solve_triangular(st.L.T, A, lower=False).T @ st.err + st.mean_const
    nrb = -(-st.N // PC.ROW_BLOCK)
    sq = np.zeros((nrb * PC.ROW_BLOCK, Xq.shape[0]))
    sq[: st.N] = A * A
    cum = np.cumsum(sq.reshape(nrb, PC.ROW_BLOCK, -1).sum(1), 0)
    var = np.maximum(st.variance - cum, O.VAR_FLOOR)
    if bound_variance is not None:
        var[:-1] = np.maximum(bound_variance - cum[:-1], O.VAR_FLOOR)
    mean.setflags(write=False)
    var.setflags(write=False)
    return mean, var


@functools.lru_cache(maxsize=None)
def full_means(name):
    """The posterior means of the whole plain candidate set (PC.M points), in chunks.  Read-only."""
    st, _ = PC.oracle_state(name)
    alpha = cho_solve((st.L, True), st.err)
    Xq = PC.candidates(name)
    out = np.empty(Xq.shape[0])
    with PC.form(name):
        for lo in range(0, Xq.shape[0], 8192):
            out[lo: lo + 8192] = O.kernel_matrix(st.kind, st.variance, st.lengthscales, Xq[lo: lo + 8192], st.X) @ alpha
    out += st.mean_const
    out.setflags(write=False)
    return out


def screen_bound(eta, mean, variance):
    """The screen's bound: the EI tail at the prior variance."""
    return PC.ei_tail(eta - mean, np.full_like(mean, max(variance, O.VAR_FLOOR)))


def block_seeds(eta, mean):
    """-> seed [blocks]: the block's largest eta - mean where that is positive (a NaN mean supplies nothing), else 0."""
    m = mean.shape[0]
    nblk = -(-m // PC.CAND_BLOCK)
    diff = np.full(nblk * PC.CAND_BLOCK, 0.0)
    diff[:m] = np.where(eta - mean > 0.0, eta - mean, 0.0)   # (NaN > 0 is False)
    return diff.reshape(nblk, PC.CAND_BLOCK).max(1)


def sweep_with_screen(mean, var, eta, variance, order, lag, bound_mean=None):
    """Seed, mean screen and block-stop rule over var [nrb][M], the blocks taken in `order` (a permutation of the block
    numbers).  -> (winner value, winner index, given_up [blocks] bool, screened [blocks] bool, seed [blocks]).
    ``bound_mean`` plants a defect: seeds, screen and checkpoint bounds taken at it, the values at the mean."""
    nrb, m = var.shape
    nblk = -(-m // PC.CAND_BLOCK)
    ub = PC.ei_tail((eta - mean)[None, :], var)
    if bound_mean is not None:
        ub[:-1] = PC.ei_tail((eta - bound_mean)[None, :], var[:-1])
    bmean = mean if bound_mean is None else bound_mean
    ub0 = screen_bound(eta, bmean, variance)
    seed = block_seeds(eta, bmean)
    known_at = np.full(nblk, -np.inf)     # by position: what the block there contributed to the best word
    given = np.zeros(nblk, dtype=bool)
    screened = np.zeros(nblk, dtype=bool)
    for p, b in enumerate(order):
        cols = slice(b * PC.CAND_BLOCK, min(m, (b + 1) * PC.CAND_BLOCK))
        known = known_at[: max(0, p - lag + 1)]
        best = max(0.0, seed[b], known.max() if known.size else 0.0)
        if nrb > 1 and PC.gives_up(ub0[cols], best):
            screened[b] = given[b] = True
        else:
            given[b] = any(PC.gives_up(ub[i, cols], best) for i in range(nrb - 1))
        known_at[p] = seed[b]
        if not given[b]:
            v = ub[-1, cols]
            v = v[~np.isnan(v)]
            known_at[p] = max(seed[b], v.max() if v.size else -np.inf)
    vals = np.where(np.repeat(given, PC.CAND_BLOCK)[:m], -np.inf, ub[-1])
    i = int(O.argmax_first(vals))
    return float(vals[i]), i, given, screened, seed


def orders(nblk):
    """The block orders of the CPU cases: as dealt, reversed, one seeded shuffle."""
    ident = np.arange(nblk)
    return {"identity": ident, "reversed": ident[::-1], "shuffled": np.random.default_rng(4242).permutation(nblk)}


@functools.lru_cache(maxsize=None)
def oracle_screened(name, label, lag=PC.FIRST_ROUND):
    """How many blocks of the whole plain set the oracle screens by the SEEDS alone, blocks taken as dealt and each
    knowing its own seed and those of the blocks `lag` or more places before it (no finished maximum: that needs the
    variances; the engine knows those too and can only screen more).  The GPU test takes its share from here."""
    st, _ = PC.oracle_state(name)
    if st.N <= PC.ROW_BLOCK:
        return 0
    eta = threshold(name, label)
    mean = full_means(name)
    seed = block_seeds(eta, mean)
    run = np.maximum.accumulate(seed)
    ub0 = screen_bound(eta, mean, st.variance)
    count = 0
    for b in range(seed.shape[0]):
        best = max(seed[b], run[b - lag] if b >= lag else 0.0)
        count += PC.gives_up(ub0[b * PC.CAND_BLOCK: (b + 1) * PC.CAND_BLOCK], best)
    return int(count)


def top_seed_candidate(name, label):
    """The plain set's candidate with the largest eta - mean: the one whose block supplies the launch's largest seed."""
    return int(np.argmax(threshold(name, label) - full_means(name)))


def blocks_screened_against_top_seed(name, label):
    """The FULL blocks of the plain set that the oracle screens once the largest seed is known, ascending."""
    st, _ = PC.oracle_state(name)
    eta = threshold(name, label)
    mean = full_means(name)
    best = float(block_seeds(eta, mean).max())
    ub0 = screen_bound(eta, mean, st.variance)
    full = PC.M // PC.CAND_BLOCK
    return np.array([b for b in range(full) if PC.gives_up(ub0[b * PC.CAND_BLOCK: (b + 1) * PC.CAND_BLOCK], best)], dtype=np.int64)


DUP_FLOOR = 300   # the duplicated-winner cases take their lower block behind the first round: one that the engine can screen

# What the functions above give on the whole plain set, recorded so that the GPU test need not form 131 149 means per model
# on the CPU (tests/test_prune_screen_bound.py recomputes every entry):
#   screened    oracle_screened(name, label) per threshold
#   top_seed    top_seed_candidate(name, "eta+3")
#   dup_blocks  the first block >= DUP_FLOOR and the last one of blocks_screened_against_top_seed(name, "eta+3")
RECORDED = {
    "m52_N256_d8": dict(screened={"eta": 0, "eta+0.5": 0, "eta+3": 0, "-1e6": 0}, top_seed=116184, dup_blocks=(300, 1023)),
    "m52_N512_d8": dict(screened={"eta": 754, "eta+0.5": 760, "eta+3": 761, "-1e6": 0}, top_seed=78583, dup_blocks=(300, 1023)),
    "rbf_N512_d8": dict(screened={"eta": 760, "eta+0.5": 760, "eta+3": 762, "-1e6": 0}, top_seed=116184, dup_blocks=(300, 1023)),
    "m12_N512_d8": dict(screened={"eta": 153, "eta+0.5": 718, "eta+3": 763, "-1e6": 0}, top_seed=80918, dup_blocks=(300, 1023)),
    "m32_N512_d8": dict(screened={"eta": 740, "eta+0.5": 757, "eta+3": 761, "-1e6": 0}, top_seed=78583, dup_blocks=(300, 1023)),
    "m52_N512_d2": dict(screened={"eta": 283, "eta+0.5": 573, "eta+3": 756, "-1e6": 0}, top_seed=62285, dup_blocks=(300, 1023)),
    "m52_N700_d8": dict(screened={"eta": 754, "eta+0.5": 762, "eta+3": 763, "-1e6": 0}, top_seed=116184, dup_blocks=(300, 1023)),
    "m52_N700_d16_lownoise": dict(screened={"eta": 0, "eta+0.5": 0, "eta+3": 760, "-1e6": 0}, top_seed=114309, dup_blocks=(300, 1023)),
    "m52_N768_d8": dict(screened={"eta": 754, "eta+0.5": 760, "eta+3": 763, "-1e6": 0}, top_seed=116184, dup_blocks=(300, 1023)),
    "m52_N768_d8_lownoise": dict(screened={"eta": 753, "eta+0.5": 761, "eta+3": 763, "-1e6": 0}, top_seed=116184, dup_blocks=(300, 1023)),
    "m32_N768_d16": dict(screened={"eta": 0, "eta+0.5": 0, "eta+3": 757, "-1e6": 0}, top_seed=114309, dup_blocks=(300, 1023)),
}
# (name, label) for which the oracle screens at least half of the blocks: there the GPU test asks the engine for half of
# the oracle's count
SHARE_CASES = [(n, t) for n in PC.SHARE_IDS for t in THRESHOLDS if 2 * RECORDED[n]["screened"][t] >= NBLK]


def oracle_winner(name, label):
    """-> (index, value): the oracle's EI arg-max over the whole plain set at a threshold (first index on ties)."""
    st, _ = PC.oracle_state(name)
    Xq = PC.candidates(name)
    ei = np.empty(Xq.shape[0])
    with PC.form(name):
        for lo in range(0, Xq.shape[0], 8192):
            ei[lo: lo + 8192] = O.ei_values(st, Xq[lo: lo + 8192], threshold(name, label))
    i = int(O.argmax_first(ei))
    return i, float(ei[i])


# The same for the general models of tests/prune_cases.GENERAL, every oracle call in the difference form
# (tests/test_prune_general_cases.py recomputes every entry), and besides
#   eta         the oracle's eta
#   winner      oracle_winner(name, "eta+0.5"): (index, value), what the GPU test anchors its unpruned launch to
RECORDED_GENERAL = {
    "g_m52_d8_N512_at1024": dict(screened={"eta": 0, "eta+0.5": 584, "eta+3": 761, "-1e6": 0}, top_seed=98678, dup_blocks=(300, 1023),
                                 eta=-33.85038789307664, winner=(98678, 10.24761699070908)),
    "g_rbf_d6_N700_at100": dict(screened={"eta": 756, "eta+0.5": 761, "eta+3": 767, "-1e6": 0}, top_seed=120794, dup_blocks=(300, 1023),
                                eta=34.92427399671836, winner=(120794, 1.0065885234340541)),
    "g_m32_d3_N513_small": dict(screened={"eta": 720, "eta+0.5": 753, "eta+3": 758, "-1e6": 0}, top_seed=5637, dup_blocks=(300, 1023),
                                eta=-1000.0750091284492, winner=(5637, 0.009564162937749643)),
    "g_m12_d5_N600_neg": dict(screened={"eta": 0, "eta+0.5": 0, "eta+3": 750, "-1e6": 0}, top_seed=111006, dup_blocks=(300, 1023),
                              eta=-93.26201392883644, winner=(111006, 0.009862664064817922)),
    "g_m52_d16_N700_lownoise": dict(screened={"eta": 0, "eta+0.5": 0, "eta+3": 666, "-1e6": 0}, top_seed=25629, dup_blocks=(300, 1023),
                                    eta=33.139741719016506, winner=(25629, 0.0004205607549843723)),
    "g_m32_d4_N520_var1e4": dict(screened={"eta": 691, "eta+0.5": 750, "eta+3": 762, "-1e6": 0}, top_seed=9084, dup_blocks=(300, 1023),
                                 eta=-463.5020323334269, winner=(9084, 91.97766486373574)),
}
# A test may ask the engine for a share of the oracle's screened count only where the oracle screens at least half of the
# blocks.  These (name, label) qualify; every general model has one (eta + 3 sd)
SHARE_CASES_GENERAL = [(n, t) for n in PC.GENERAL_IDS for t in THRESHOLDS if 2 * RECORDED_GENERAL[n]["screened"][t] >= NBLK]
