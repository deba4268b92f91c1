"""tests/factor_resolution.py on the CPU: K_exact against mpmath, the float64 reference (the oracle's factor, scipy's triangular
inverse and cho_solve alpha) inside every bound, planted errors outside the bound they are aimed at -- and inside the
tolerances tests/test_gpu_dag.py has compared L, W and alpha with so far (restated here): the gap these bounds close."""
import functools

import numpy as np
import pytest

from tests import factor_resolution as F
from tests.util import record_margin

LD = F.LD
SIZES_FULL = (1, 17, 128, 129, 256, 257, 384, 513, 640)
CASES = [(k, s, N) for k, s in F.HYPERS for N in SIZES_FULL + (1100,)] + [F.LOW_NOISE + (N,) for N in (128, 640)]


def _mp_kernel(kind, variance, ls, x, X):
    """tests/make_kernel_resolution_goldens.py's mpmath kernels with general lengthscales and variance."""
    from mpmath import mp, mpf

    mp.dps = 50
    t = [(mpf(float(a)) - mpf(float(b))) / mpf(float(l)) for a, b, l in zip(x, X, ls)]
    r2 = max(sum(v * v for v in t), mpf(1e-36))
    if kind == "rbf":
        return mpf(variance) * mp.exp(-r2 / 2)
    s = mp.sqrt(5) * mp.sqrt(r2)
    return mpf(variance) * (1 + s + s * s / 3) * mp.exp(-s)


@pytest.mark.parametrize("kind", ["rbf", "matern52"])
def test_K_exact_against_mpmath(kind):
    """64 sampled entries (the diagonal and near-coincident pairs among them) to 4 * 2^-63 relative."""
    from mpmath import mpf

    X, _, ls = F.problem(257)
    X = X.copy()
    X[1] = X[0] + 1e-9 * ls                                    # a near-coincident pair
    noise = 1e-5
    K = F.K_exact(kind, F.VARIANCE, ls, noise, X)
    rng = np.random.default_rng(5)
    pairs = [(0, 0), (1, 0), (256, 256), (256, 0)] + [tuple(rng.integers(0, 257, size=2)) for _ in range(60)]
    worst = 0.0
    for i, j in pairs:
        ref = _mp_kernel(kind, F.VARIANCE, ls, X[i], X[j]) + (mpf(noise) if i == j else 0)
        got = mpf(float(K[i, j])) + mpf(float(K[i, j] - LD(float(K[i, j]))))     # the long double as two doubles, exactly
        worst = max(worst, float(abs(got - ref) / ref))
    record_margin(f"{kind} K_exact vs mpmath", worst, 4 * 2.0 ** -63)
    assert worst <= 4 * 2.0 ** -63, worst


@pytest.mark.parametrize("kind,noise,N", CASES)
def test_reference_is_within_every_bound(kind, noise, N):
    """A correct float64 implementation stays inside the bounds on these inputs -- under the substitution form's bounds (its own)
    and, a fortiori, under every device form's."""
    L, W, alpha = F.reference_factor(kind, noise, N)
    K, E, err = F.k_parts(kind, noise, N)
    evaluate = F.full_ratios if N <= F.FULL_MAX else F.probe_ratios
    bad = []
    r = evaluate(L, W, alpha, K, E, err, [], f"reference {kind} {noise:g} N={N}", bad)
    for form in ("dag", "recursion"):
        if N <= 257 or form == "dag":                          # (the wider forms' bounds contain the narrower: a sample is enough)
            bd = F.Bounds(L, W, E, F.form_levels(form, N), alpha_form="solve")
            x = np.ones((N, 1))
            assert np.all(bd.right(x) >= F.Bounds(L, W, E, []).right(x))
    assert not bad, bad
    assert all(v < 0.5 for v in r.values()), r                 # the bounds are worst-case counts: a correct factor sits well inside


@functools.lru_cache(maxsize=None)
def _planted(N, noise=1e-5, kind="matern52"):
    """The four planted errors of the reference arrays at (matern52, noise 1e-5, N): name -> (L, W, alpha, aimed check)."""
    import scipy.linalg as sl

    L, W, alpha = F.reference_factor(kind, noise, N)
    K, E, err = F.k_parts(kind, noise, N)
    out = {}
    Lt = L.copy()
    Lt[256:384, 128:256] *= 1.0 + 2.0 ** -36                   # one 128 x 128 tile of L
    out["L tile scaled by 1 + 2^-36"] = (Lt, W, alpha, "R_K")
    Wt = W.copy()
    Wt[300, 300] *= 1.0 + 2.0 ** -30                            # (a diagonal entry: the reciprocal of a pivot)
    out["one entry of W moved by 2^-30"] = (L, Wt, alpha, "R_right")
    at = alpha.copy()
    at[int(np.argmax(np.abs(alpha)))] *= 1.0 + 2.0 ** -30
    out["one alpha entry moved by 2^-30"] = (L, W, at, "r_alpha")
    Kp = np.asarray(K, dtype=np.float64)
    Kp = np.tril(Kp) + np.tril(Kp, -1).T
    P = np.random.default_rng(40).choice([-1.0, 1.0], size=Kp.shape)
    Kp = Kp * (1.0 + 2.0 ** -40 * np.tril(P) + 2.0 ** -40 * np.tril(P, -1).T)
    Lp = L.copy()
    Lp[:, 256:384] = np.linalg.cholesky(Kp)[:, 256:384]         # one column block from the factor of a perturbed K
    out["column block of L from K (1 + 2^-40)"] = (np.tril(Lp), W, alpha, "R_K")
    return (L, W, alpha), out, (K, E, err)


def _old_tolerances_accept(N, noise, ref, got):
    """tests/test_gpu_dag.py's comparisons of (L, W, alpha) with numpy's, restated: do they accept ``got``?"""
    (L0, W0, a0), (L, W, a) = ref, got
    tol = 64 * np.finfo(float).eps * (1.0 + N / noise)
    close = lambda x, y, rtol, atol: bool(np.all(np.abs(x - y) <= rtol * np.abs(y) + atol))
    return (close(L, L0, 1e-9, tol * np.abs(L0).max()) and close(W, W0, 1e-7, tol * np.abs(W0).max() * 64)
            and np.abs(np.tril(W) @ np.tril(L) - np.eye(N)).max() < 1e-7 and close(a, a0, 1e-6, 1e-6 * np.abs(a0).max()))


LEVELS_640 = dict(substitution=[], dag=F.form_levels("dag", 640), recursion=F.form_levels("recursion", 640),
                  append=F.form_levels("append", 640, keep=576))

# Stated, not hidden (tests/test_gpu_factor_resolution.py _residuals): under the recursion's and the append's levels the TILE PROBES do not see the two planted
# errors of L in |L (L^T v) - K v| (the recursion's: the tile; the append's: both) -- a probe's bound sums the explicit-inverse term of blocks of up to 576 rows over the 128 columns
# of |v| (planted / bound 0.003 where the full evaluation has 2.8 - 230).  The GPU tests therefore use the probes only under the
# persistent kernel's tile levels (N = 1100, where they do see them: 4.5 and 10.7); the recursion at N = 1100 and the k = 40 append at
# N = 1070 get the full evaluation.
PROBES_MISS = {("L tile scaled by 1 + 2^-36", "recursion"), ("L tile scaled by 1 + 2^-36", "append"),
               ("column block of L from K (1 + 2^-40)", "append")}


@pytest.mark.parametrize("form", sorted(LEVELS_640))
@pytest.mark.parametrize("which", range(4))
def test_planted_errors_fail_their_check_and_pass_the_old_tolerances(which, form):
    """N = 640, noise 1e-5, under the bounds of EVERY form the GPU tests apply (and the reference's own): each planted error misses
    the bound it is aimed at in the full AND in the tile-probe evaluation (the unplanted arrays pass both), and passes
    tests/test_gpu_dag.py's tolerances."""
    N, noise = 640, 1e-5
    ref, planted, (K, E, err) = _planted(N)
    name = sorted(planted)[which]
    L, W, alpha, aimed = planted[name]
    levels = LEVELS_640[form]
    assert _old_tolerances_accept(N, noise, ref, (L, W, alpha)), f"{name}: the old tolerances would have caught it"
    for evaluate in (F.full_ratios, F.probe_ratios):
        bad = []
        clean = evaluate(*ref, K, E, err, levels, "clean", bad)
        assert not bad and clean[aimed] < 1.0
        r = evaluate(L, W, alpha, K, E, err, levels, name, bad)
        print(f"{name} [{form}]: {evaluate.__name__}: clean {clean[aimed]:.3g}, planted {r[aimed]:.3g} of the bound on {aimed}; "
              f"worst of all {max(r.values()):.3g}")
        missed = evaluate is F.probe_ratios and (name, form) in PROBES_MISS
        assert (r[aimed] > 1.0) != missed, (name, form, evaluate.__name__, r)


@pytest.mark.parametrize("kind,noise", F.HYPERS + (F.LOW_NOISE,))
def test_derived_tolerances_are_finer_than_what_they_check(kind, noise):
    """N = 640, the reference arrays: every variance tolerance at a training input is below tests/util.py's cancellation_floor (the
    floor this replaces) and below 1e-6 of the prior variance everywhere; every mean tolerance below 1e-5 of the standardised
    targets' unit scale (1e-3 at noise 1e-8, where |alpha| reaches 2e7 and the mean is a sum cancelling over seven digits: the final
    product's own rounding is 2e-5 there and the long-double reference's worst-case error, carried at 64 times its bound, 7e-4);
    the NLML tolerances (full and factor-only) below 1e-5 of the value (5e-6 at noise 1e-8, 6e-8 at rbf 1e-5)."""
    from tests.util import cancellation_floor

    N = 640
    L, W, alpha = F.reference_factor(kind, noise, N)
    post = F.posterior(kind, noise, N)
    ms = F.Measured(L, W, alpha, post.K, post.err)
    tol_mean, tol_var = F.posterior_tolerances(ms, post, post.predict(F.query_points(N)))
    floor = cancellation_floor(N, F.VARIANCE, noise)
    print(f"{kind} {noise:g}: tol_var at training inputs {tol_var[:16].max():.3g} (old floor {floor:.3g}), anywhere {tol_var.max():.3g}; "
          f"tol_mean {tol_mean.max():.3g}; nlml {float(post.nlml):.6g} tol {F.nlml_tolerance(ms, post, False):.3g} / "
          f"{F.nlml_tolerance(ms, post, True):.3g}")
    assert np.all(tol_var[:16] < floor) and np.all(tol_var < 1e-6 * F.VARIANCE)
    assert np.all(tol_mean < (1e-5 if noise >= 1e-5 else 1e-3))
    assert F.nlml_tolerance(ms, post, True) < 1e-5 * abs(float(post.nlml)) and F.nlml_tolerance(ms, post, False) < 1e-5 * abs(float(post.nlml))


@pytest.mark.parametrize("which", ["tile task's alpha", "leaf pivot's reciprocal"])
def test_emulated_engine_mutations_fail_the_factor_bound(which):
    """Two mutations of the engine, emulated in float64 on the CPU under the persistent kernel's bound: the trailing update of
    tile (4, 2) at N = 640 applied with 1 + 2^-30 (a tile task's alpha), and pivot 37's reciprocal of a 128-leaf rounded through
    float32.  Both pass tests/test_gpu_dag.py's tolerances and miss |L L^T - K| by four orders of magnitude."""
    import scipy.linalg as sl

    kind, noise = "matern52", 1e-5
    N = 640 if which.startswith("tile") else 128
    K, E, err = F.k_parts(kind, noise, N)
    ref = F.reference_factor(kind, noise, N)
    A = np.asarray(K, dtype=np.float64).copy()
    if N == 640:
        L0 = ref[0]
        A[512:640, 256:384] -= 2.0 ** -30 * (L0[512:640, :256] @ L0[256:384, :256].T)
        A[256:384, 512:640] = A[512:640, 256:384].T
        L = np.linalg.cholesky(A)
    else:
        L = np.zeros((N, N))
        for j in range(N):
            rs = 1.0 / np.sqrt(A[j, j])
            if j == 37:
                rs = float(np.float32(rs))
            L[j:, j] = A[j:, j] * rs                            # (L_jj = p rs, as the leaf forms it)
            A[j + 1:, j + 1:] -= np.outer(L[j + 1:, j], L[j + 1:, j])
    W = np.tril(sl.solve_triangular(L, np.eye(N), lower=True))
    alpha = W.T @ (W @ np.asarray(err, dtype=np.float64))
    assert _old_tolerances_accept(N, noise, ref, (L, W, alpha))
    bad = []
    r = F.full_ratios(L, W, alpha, K, E, err, F.form_levels("dag", N), which, bad)
    assert r["R_K"] > 1e3 and bad, r
