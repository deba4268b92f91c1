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

import numpy as np
from scipy.linalg import cho_solve, solve_triangular

from oracle import gp_oracle as O
from tests import prune_cases as PC

SEED_RTOL = 1e-5                  # the engine's tails hold RTOL = 1e-5 (tests/acq_regimes.py): value >= seed (1 - SEED_RTOL)
THRESHOLDS = ("eta", "eta+0.5", "eta+3", "-1e6")
SAMPLE = 95 * PC.CAND_BLOCK + 77  # the CPU sweeps: 96 blocks of the plain set, the last one ragged
NBLK = -(-PC.M // PC.CAND_BLOCK)


def threshold(name, label):
    """The EI threshold of a case: the model's eta, eta shifted up (more and larger seeds), or so low that every EI is 0."""
    eta = PC.oracle_state(name)[1]
    return {"eta": eta, "eta+0.5": eta + 0.5, "eta+3": eta + 3.0, "-1e6": -1e6}[label]


@functools.lru_cache(maxsize=None)
def sample_moments(name):
    """-> (mean [SAMPLE], var [nrb][SAMPLE]) of the first SAMPLE plain candidates: var[i] the variance bound after row
    blocks 0 .. i (var[-1]: the variance), as tests/prune_cases.partial_bounds forms them.  Read-only."""
    st, _ = PC.oracle_state(name)
    Xq = PC.candidates(name)[:SAMPLE]
    K = O.kernel_matrix(st.kind, st.variance, st.lengthscales, st.X, Xq)
    A = solve_triangular(st.L, K, lower=True)
    mean = solve_triangular(st.L.T, A, lower=False).T @ st.err + st.mean_const
    nrb = -(-st.N // PC.ROW_BLOCK)
    sq = np.zeros((nrb * PC.ROW_BLOCK, Xq.shape[0]))
    sq[: st.N] = A * A
    cum = np.cumsum(sq.reshape(nrb, PC.ROW_BLOCK, -1).sum(1), 0)
    var = np.maximum(st.variance - cum, O.VAR_FLOOR)
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


def sweep_with_screen(mean, var, eta, variance, order, lag):
    """Seed, mean screen and block-stop rule over var [nrb][M], the blocks taken in `order` (a permutation of the block
    numbers).  -> (winner value, winner index, given_up [blocks] bool, screened [blocks] bool, seed [blocks])."""
    nrb, m = var.shape
    nblk = -(-m // PC.CAND_BLOCK)
    ub = PC.ei_tail((eta - mean)[None, :], var)
    ub0 = screen_bound(eta, mean, variance)
    seed = block_seeds(eta, mean)
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
