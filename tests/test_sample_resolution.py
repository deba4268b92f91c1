"""tests/sample_resolution.py on the CPU: the residual bound holds for the reference alone with a stated margin, the residual and
draw checks pass on a float64 restatement of tgp_sample_joint (same padding), every planted fault is caught where it can occur,
and the comparison of samples at rtol 1e-5, atol 3e-8 (tests/test_gpu_parity.py) does not see a 2^-36 error of a tile of L.

Worst residual / bound, printed per case (pytest -s):
  numpy's Cholesky of the rounded A_ref (term (b) = its rounding): below 0.03 over the four models, n = 1 .. 577, jitter 1e-6 and
    1e-10, and the wide model -- the stated margin is REFERENCE_MARGIN = 0.25;
  the restatement from the float64 reference's W, alpha under the full bound: residual at most 0.026, draws at most 0.45;
  the 2^-36 tile fault: 1.9 (n = 1, 2) and 4.2 (n >= 63) of the bound; every other planted fault above 1e6 of its bound."""
import functools

import numpy as np
import pytest

from tests import factor_resolution as F
from tests import sample_resolution as R

LD = F.LD


@functools.lru_cache(maxsize=None)
def _tol_cov(name, jitter):
    ref = R.reference(name)
    tol = R.covariance_tolerance(ref, R.measured(name, *R.reference_arrays(name)), jitter)
    tol.setflags(write=False)
    return tol


@pytest.mark.parametrize("name", R.MODELS)
def test_term_b_is_finer_than_the_floor_it_replaces(name):
    """The data-dependent covariance tolerance against cancellation_floor (diagonal) and ten times it (off the diagonal)."""
    on, off = R.assert_finer_than_the_floor(name, _tol_cov(name, R.JITTER))
    print(f"{name}: covariance tolerance / floor {on:.3g} on the diagonal, {off:.3g} off it")


def _sizes(name):
    return (70,) if name == R.WIDE else R.SIZES


@pytest.mark.parametrize("name", R.MODELS)
def test_the_reference_alone_stays_inside_the_bound(name):
    """numpy's float64 Cholesky of the float64-rounded A_ref on every query set, jitter 1e-6 and 1e-10: residual / bound below
    REFERENCE_MARGIN, term (b) reduced to the rounding of A_ref."""
    ref = R.reference(name)
    worst = 0.0
    for jitter in (R.JITTER, R.LOW_JITTER):
        for n in _sizes(name):
            A = ref.A(n, jitter)
            L = np.linalg.cholesky(np.asarray(A, dtype=np.float64))
            r = R.factor_checks(f"reference {name} jitter {jitter:g} n={n}", L, A, R.rounding_tolerance(A))
            print(f"reference {name} jitter {jitter:g} n={n}: residual / bound {r:.3g}")
            worst = max(worst, r)
    assert worst < R.REFERENCE_MARGIN, worst


@pytest.mark.parametrize("name", R.MODELS)
def test_the_restatement_passes_both_checks(name):
    """The float64 restatement from the reference's W and alpha, identity in the padding of A, zero-padded draws: the residual under
    the full bound (a) + (b) + (c) and the draws against the factor just formed."""
    ref = R.reference(name)
    _, W, alpha = R.reference_arrays(name)
    bad = []
    pairs = ((70, 65),) if name == R.WIDE else R.DRAW_PAIRS
    for jitter in (R.JITTER, R.LOW_JITTER):
        tol = _tol_cov(name, jitter)
        for n, S in pairs:
            eps = R.draws(n, S)
            Lp, mean, out = R.restate(ref, W, alpha, n, jitter, eps)
            assert np.array_equal(Lp[n:, :n], np.zeros((Lp.shape[0] - n, n))) and np.array_equal(Lp[n:, n:], np.eye(Lp.shape[0] - n))
            r = R.factor_checks(f"restated {name} jitter {jitter:g} n={n}", Lp[:n, :n], ref.A(n, jitter), tol, bad)
            q = R.draw_checks(f"restated {name} jitter {jitter:g} n={n} S={S}", out, Lp[:n, :n], eps, mean, bad)
            print(f"restated {name} jitter {jitter:g} n={n} S={S}: residual / bound {r:.3g}, draws / tolerance {q:.3g}")
    assert not bad, "\n".join(bad)


FAULT_MODEL = "matern52@1e-05"


def _tile(n):
    """The planted tile: the first diagonal 64 x 64 tile, which every n has (clipped to n).  The LAST diagonal tile of n = 257 is the
    single entry L[256, 256], the conditional deviation of one point given 256 others: 2^-36 of it moves the residual by 0.22 of
    the bound -- an error of that size in that entry is below what term (b) grants the covariance itself."""
    return slice(0, min(n, 64))


@pytest.mark.parametrize("n", R.SIZES)
def test_planted_faults_of_the_factor_are_caught(n):
    """At every n: a relative error of 2^-36 in one 64 x 64 tile of L; the last row of L taken from the padded row (n no multiple of
    64); the jitter added to every entry instead of the diagonal (n >= 2).  The clean restatement passes, each fault misses the
    bound."""
    ref = R.reference(FAULT_MODEL)
    _, W, alpha = R.reference_arrays(FAULT_MODEL)
    tol, A = _tol_cov(FAULT_MODEL, R.JITTER), ref.A(n, R.JITTER)
    Lp, _, _ = R.restate(ref, W, alpha, n, R.JITTER)
    clean = R.factor_checks(f"clean n={n}", Lp[:n, :n], A, tol)
    assert clean < 1.0
    faults = {}
    L = Lp[:n, :n].copy()
    L[_tile(n), _tile(n)] *= 1.0 + 2.0 ** -36
    faults["tile of L scaled by 1 + 2^-36"] = L
    if n % 64:
        L = Lp[:n, :n].copy()
        L[n - 1] = Lp[n, :n]
        faults["last row from the padded row"] = L
    if n >= 2:
        faults["jitter on every entry"] = R.restate(ref, W, alpha, n, R.JITTER, jitter_everywhere=True)[0][:n, :n]
    for fault, L in faults.items():
        bad = []
        r = R.factor_checks(f"{fault} n={n}", L, A, tol, bad)
        print(f"n={n}: clean {clean:.3g}; {fault}: {r:.3g} of the bound")
        assert bad and r > 1.0, (fault, n, r)


@pytest.mark.parametrize("n,S", R.DRAW_PAIRS)
def test_planted_faults_of_the_draws_are_caught(n, S):
    """At every pair: draw column 64 zeroed (S >= 65: the padding boundary of the draws); `out` written as [n, S] instead of
    [S, n] (n, S >= 2, where the two layouts differ)."""
    ref = R.reference(FAULT_MODEL)
    _, W, alpha = R.reference_arrays(FAULT_MODEL)
    eps = R.draws(n, S)
    Lp, mean, out = R.restate(ref, W, alpha, n, R.JITTER, eps)
    L = Lp[:n, :n]
    clean = R.draw_checks(f"clean n={n} S={S}", out, L, eps, mean)
    assert clean < 1.0
    faults = {}
    if S >= 65:
        lost = eps.copy()
        lost[:, 64] = 0.0
        faults["draw column 64 zeroed"] = R.restate(ref, W, alpha, n, R.JITTER, lost)[2]
    if n >= 2 and S >= 2:
        faults["out written as [n, S]"] = np.ascontiguousarray(out.T).reshape(S, n)
        faults["out returned as [n, S]"] = np.ascontiguousarray(out.T)
    for fault, got in faults.items():
        bad = []
        r = R.draw_checks(f"{fault} n={n} S={S}", got, L, eps, mean, bad)
        print(f"n={n} S={S}: clean {clean:.3g}; {fault}: {r:.3g} of the tolerance")
        assert bad and r > 1.0, (fault, n, S, r)


@pytest.mark.parametrize("n,S", [(65, 63), (320, 64), (577, 1)])
def test_the_old_comparison_is_blind_to_the_tile_fault(n, S):
    """rtol 1e-5, atol 3e-8 -- tests/test_gpu_parity.py's tolerance for samples at noise 1e-2 -- accepts the draws of a factor with a
    2^-36 error in a tile, which the residual check rejects: why this file exists."""
    ref = R.reference(FAULT_MODEL)
    _, W, alpha = R.reference_arrays(FAULT_MODEL)
    eps = R.draws(n, S)
    Lp, mean, out = R.restate(ref, W, alpha, n, R.JITTER, eps)
    L = Lp[:n, :n].copy()
    L[_tile(n), _tile(n)] *= 1.0 + 2.0 ** -36
    faulty = (mean[:, None] + L @ eps).T
    err = np.abs(faulty - out)
    assert err.max() > 0.0
    assert np.all(err <= 1e-5 * np.abs(out) + 3e-8), "the old tolerance would have caught it"
    bad = []
    r = R.factor_checks(f"tile fault n={n}", L, ref.A(n, R.JITTER), _tol_cov(FAULT_MODEL, R.JITTER), bad)
    print(f"n={n} S={S}: tile fault moves the draws by {err.max():.3g} (old tolerance >= 3e-8); residual / bound {r:.3g}")
    assert bad and r > 1.0


@pytest.mark.parametrize("n,a,b", R.BREAKDOWN_PAIRS)
def test_breakdown_sets_are_positive_definite_up_to_the_duplicate(n, a, b):
    """jitter 0, one exact duplicate pair a < b, everything else separated: the leading b x b block of A_ref is positive
    definite with every pivot (Schur complement) above 1e-6; row b repeats row a."""
    ref = R.Reference("matern52@0.01", R.duplicate_pair_set(n, a, b))
    A = ref.A(n, 0.0)
    piv = np.diag(F.chol_ld(A[:b, :b])) ** 2
    print(f"n={n} a={a} b={b}: smallest pivot of the leading block {float(piv.min()):.3g}")
    assert piv.min() > 1e-6
    assert np.array_equal(A[b], A[a])
