"""CPU: the float32 pre-screen's bound holds, its planted defects leave it, and its screen drops only what the exact one drops.

tests/prescreen_cases.py restates phase 0 of the pruned EI arg-max in numpy with float32 arithmetic in the
kernel's order.  The reference mean is formed in long double from the raw inputs."""
import math

import numpy as np
import pytest

from tests import prescreen_cases as R
from tests import prune_cases as PC
from tests import prune_screen_cases as S

N, M = 300, 1500
DIMS = (2, 8, 16)
MODELS = ("plain", "ard", "variance", "mean", "shifted", "lownoise")

pytestmark = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63, reason="the reference needs an extended long double")


def _kernel64(kind, variance, ls, A, B):
    r2 = (((A / ls)[:, None, :] - (B / ls)[None, :, :]) ** 2).sum(-1)
    return variance * R.shape_true(kind, R.SCALE[kind] * r2).astype(np.float64)


def _model(kind, d, which):
    """-> (variance, ls, X, alpha, mean_const, Xq): a fitted model (alpha = (K + noise I)^-1 (Y - c)) and candidates."""
    rng = np.random.default_rng(1000 * d + MODELS.index(which))
    lo = 1e3 if which == "shifted" else 0.0
    X, Xq = lo + rng.uniform(size=(N, d)), lo + rng.uniform(size=(M, d))
    Xq[:8] = X[:8] + 1e-9                                   # candidates on top of training rows: r near 0
    ls = np.full(d, 0.4 * math.sqrt(d))
    if which == "ard":
        ls = ls * rng.uniform(0.3, 3.0, size=d)
    variance = 7.5 if which == "variance" else 1.0
    mean_const = -3.25 if which == "mean" else 0.0
    noise = 1e-5 if which == "lownoise" else 1e-2
    Y = np.sin(3.0 * (X - lo).sum(1)) * 2.0 + mean_const + 0.1 * rng.standard_normal(N)
    K = _kernel64(kind, variance, ls, X, X) + noise * np.eye(N)
    alpha = np.linalg.solve(K, Y - mean_const)
    return variance, ls, X, alpha, mean_const, Xq


def _errors(kind, d, which, **defect):
    variance, ls, X, alpha, c, Xq = _model(kind, d, which)
    m32, an = R.restate(kind, variance, ls, X, alpha, c, Xq, **defect)
    mean = R.true_mean(kind, variance, ls, X, alpha, c, Xq)
    xmax, x0 = R.model_extent(kind, ls, X)
    npad = -(-N // PC.ROW_BLOCK) * PC.ROW_BLOCK
    E = R.bound(kind, d, npad, np.abs(alpha).sum(), variance, an, xmax, x0, m32, 0.0)
    return np.abs((m32 - mean).astype(np.float64)), E, np.abs(alpha).sum()


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("d", DIMS)
@pytest.mark.parametrize("which", MODELS)
def test_bound_holds(kind, d, which):
    err, E, l1 = _errors(kind, d, which)
    print(f"{kind} d={d} {which}: |alpha|_1 {l1:.3e}  worst error {err.max():.3e}  E {E.min():.3e} .. {E.max():.3e}  "
          f"worst error / E {(err / E).max():.3e}")
    assert np.all(np.isfinite(E)) and np.all(err <= E)


@pytest.mark.parametrize("kind", R.KINDS)
def test_defect_centring_after_rounding_leaves_the_bound(kind):
    """Rounding the coordinates of a box at 1e3 before centring them costs 1e3 u on every difference."""
    err, E, _ = _errors(kind, 8, "shifted", centre_after_rounding=True)
    assert np.any(err > E), (err / E).max()
    err, E, _ = _errors(kind, 8, "shifted")
    assert np.all(err <= E)


def _far_pair(kind):
    """One row of weight 1 at 50 scaled units from row 0 (weight 0), candidates around it where 2 sqrt(q) |f'| is large: the
    conversion of the two centred operands is all the error there is."""
    rng = np.random.default_rng(5)
    d, m = 2, 4000
    ls = np.ones(d)
    X = np.array([[0.0, 0.0], [30.0, 40.0]]) + 0.123456789
    alpha = np.array([0.0, 1.0])
    phi = rng.uniform(0.0, 2.0 * math.pi, size=m)
    r = {"rbf": 1.0, "matern12": 0.3, "matern32": 0.6, "matern52": 0.75}[kind] * rng.uniform(0.8, 1.2, size=m)
    Xq = X[1] + r[:, None] * np.stack([np.cos(phi), np.sin(phi)], 1)
    return d, ls, X, alpha, Xq


@pytest.mark.parametrize("kind", R.KINDS)
def test_defect_dropped_conversion_term_leaves_the_bound(kind):
    d, ls, X, alpha, Xq = _far_pair(kind)
    m32, an = R.restate(kind, 1.0, ls, X, alpha, 0.0, Xq)
    err = np.abs((m32 - R.true_mean(kind, 1.0, ls, X, alpha, 0.0, Xq)).astype(np.float64))
    xmax, x0 = R.model_extent(kind, ls, X)
    full = R.bound(kind, d, 256, 1.0, 1.0, an, xmax, x0, m32, 0.0)
    dropped = R.bound(kind, d, 256, 1.0, 1.0, an, xmax, x0, m32, 0.0, drop="conversion")
    print(f"{kind}: worst error {err.max():.3e}  E {full.max():.3e}  without the conversion term {dropped.max():.3e}")
    assert np.all(err <= full)
    assert np.any(err > dropped)


@pytest.mark.parametrize("kind", R.KINDS)
def test_defect_dropped_chain_and_direct_terms_leave_the_bound(kind):
    """Against roundings the floating-point model allows, all pushing one way: every product of the chain and the two
    transcendentals off by their full u / 2 ulp.  q (1 + (2 dp + 10) u) moves f by q |f'| (2 dp + 10) u, and the value's
    own roundings by 10 u f: with either term left out the bound is passed where the other two are small."""
    d, dp = 16, 16
    ld = np.longdouble
    q = ld(np.linspace(0.05, 40.0, 4000))
    f = R.shape_true(kind, q)
    pushed = R.shape_true(kind, q * (1 + ld((2 * dp + 10) * R.U))) * (1 - ld(10 * R.U))
    err = np.abs((pushed - f).astype(np.float64))            # one row of weight 1 at S = 0
    zero = np.zeros(q.shape[0])
    args = (kind, d, 256, 1.0, 1.0, zero, 0.0, 0.0, zero, 0.0)
    assert np.all(err <= R.bound(*args))
    assert np.any(err > R.bound(*args, drop="chain"))
    assert np.any(err > R.bound(*args, drop="direct"))


def test_shape_constants_bound_the_shape():
    ld = np.longdouble
    q = ld(np.geomspace(1e-8, 400.0, 200001))
    h = q * ld(1e-6)
    for kind in R.KINDS:
        df = np.abs(((R.shape_true(kind, q + h) - R.shape_true(kind, q - h)) / (2 * h)).astype(np.float64))
        q64 = q.astype(np.float64)
        g1, g2 = (2.0 * np.sqrt(q64) * df).max(), (q64 * df).max()
        print(f"{kind}: sup 2 sqrt(q) |f'| = {g1:.4f} (G1 {R.G1[kind]})  sup q |f'| = {g2:.4f} (G2 {R.G2[kind]})")
        assert g1 <= R.G1[kind] <= 1.1 * g1 and g2 <= R.G2[kind] <= 1.1 * g2


def test_lower_seed_is_rounded_down_and_the_defect_is_not():
    """With the mean as far from mean32 as the model part of the bound allows, mean = mean32 + E_model, the lower seed -- taken
    with the bound's allowance 2^-50 (|mean32| + |eta|) for its own two roundings and pushed down -- stays at or below
    eta - mean taken exactly; the same expression without the allowance, rounded up, passes it."""
    rng = np.random.default_rng(11)
    n = 200000
    eta = rng.uniform(-10.0, 10.0, size=n)
    m32 = eta - np.exp(rng.uniform(-12.0, 3.0, size=n))
    e_model = np.exp(rng.uniform(-30.0, 0.0, size=n)) * (eta - m32)
    E = e_model + 2.0 ** -50 * (np.abs(m32) + np.abs(eta))
    ld = np.longdouble
    exact = ld(eta) - (ld(m32) + ld(e_model))
    assert np.all(ld(R.lower_seed(eta, m32, E)) <= exact)
    assert np.any(ld(R.lower_seed(eta, m32, e_model, round_up=True)) > exact)


@pytest.mark.parametrize("name", ["m52_N512_d8", "rbf_N512_d8", "m12_N512_d8", "m52_N700_d16_lownoise", "m52_N768_d8_lownoise"])
@pytest.mark.parametrize("label", S.THRESHOLDS)
def test_restated_screen_drops_only_what_the_exact_screen_drops(name, label):
    st, _ = PC.oracle_state(name)
    eta = S.threshold(name, label)
    Xq = PC.candidates(name)[: S.SAMPLE]
    mean, _ = S.sample_moments(name)
    ub32, prebest, m32, E = R.restated_blocks(name, label, Xq)
    assert np.all(np.abs(m32 - mean) <= E)
    ub = S.screen_bound(eta, mean, st.variance)
    nblk = ub32.shape[0]
    ub = np.concatenate([ub, np.full(nblk * PC.CAND_BLOCK - ub.shape[0], -np.inf)]).reshape(nblk, PC.CAND_BLOCK).max(1)
    best = float(S.block_seeds(eta, mean).max())
    assert np.all(ub32 >= ub) and prebest <= best
    exact = np.array([best > PC.MIN_BEST and u * PC.MARGIN < best for u in ub])
    pre = R.dismissed(ub32, prebest)
    print(f"{name} {label}: exact screen drops {exact.sum()} of {nblk}, pre-screen {pre.sum()}; prebest {prebest:.6g} best {best:.6g}")
    assert not np.any(pre & ~exact)
    if label == "-1e6":
        assert not pre.any()


def test_recorded_share_case():
    """The GPU test's count condition: on the whole plain set of the recorded case the restatement dismisses at least half
    of the blocks the oracle screens."""
    name, label = R.SHARE_CASE
    ub32, prebest, _, _ = R.restated_blocks(name, label, PC.candidates(name))
    n = int(R.dismissed(ub32, prebest).sum())
    assert n == R.SHARE_DISMISSED
    assert 2 * n >= S.RECORDED[name]["screened"][label] > 0
