"""tests/grad_resolution.py on the CPU: (1) the three long-double references agree with central differences of the long-double
NLML, mean, variance and joint covariance; (2) plain float64 restatements of the kernels' summations meet every tolerance of the
GPU cases with a quarter of it at most, so the bounds are attainable before a device sees them; (3) the defects a parity
tolerance of 1e-5 cannot see are each rejected; (4) the beta = 2 comparison leaves out the near-training points only.

The finite-difference bound.  D(h) = (f(x + h) - f(x - h)) / 2h with h = 2^-20 of the parameter's own scale (the parameter
itself for a hyper-parameter, the lengthscale for a coordinate) has the truncation error h^2 f''' / 6 + O(h^4), and
D(2h) - D(h) = 3 h^2 f''' / 6 + O(h^4) MEASURES the third-derivative scale; the rounding error rho of f (N 2^-63 times the
weights of its sums, the references' own condition) enters as rho / h:
    |D(h) - reference| <= 2/3 |D(2h) - D(h)| + 4 rho / h
(2/3 = twice the measured truncation; 4 rho / h: rho / h from D(h) and up to 3/2 rho / h hidden in the measured difference,
rounded up).  With f of order one, h^2 = 10^-12: agreement of about 10^-12 of the derivative's scale."""
import numpy as np
import pytest

from tests import factor_resolution as F
from tests import grad_resolution as R

LD = F.LD
STEP = LD(2.0) ** -20
EPS_LD = F.EPS_LD


def _steps(x0, scale):
    """(x0 + h, x0 - h, x0 + 2h, x0 - 2h) as doubles and the two EXACT spans in long double."""
    h = float(STEP * LD(scale))
    p = [float(x0 + h), float(x0 - h), float(x0 + 2 * h), float(x0 - 2 * h)]
    return p, LD(p[0]) - LD(p[1]), LD(p[2]) - LD(p[3])


def _fd_check(what, f, span1, span2, ref, rho, bad):
    d1, d2 = (f[0] - f[1]) / span1, (f[2] - f[3]) / span2
    bound = LD(2) / 3 * np.abs(d2 - d1) + 4 * rho / (span1 / 2)
    err = np.abs(d1 - ref)
    if not np.all(err <= bound):
        i = int(np.argmax(np.asarray(err - bound, dtype=np.float64)))
        bad.append(f"{what}: |D(h) - ref| = {float(np.ravel(err)[i]):.3g} > {float(np.ravel(bound)[i]):.3g} "
                   f"(derivative {float(np.ravel(np.asarray(ref))[i]):.3g})")
    scale = np.maximum(np.abs(np.asarray(ref, dtype=np.float64)), 1e-300)
    return float(np.max(np.asarray(err, dtype=np.float64) / scale))


def _ld_factor(kind, noise, N, d=F.D):
    X, Y, ls, Xq = R.design(N, d)
    post = F.Posterior(kind, F.VARIANCE, ls, noise, F.MEAN, X, Y)
    W = F.solve_lower(post.L, np.eye(N, dtype=LD))
    return X, Y, ls, Xq, post, W


FD_CASES = [(k, s, 17, F.D) for k, s in F.HYPERS] + [("matern52", 1e-2, 24, 13)]


@pytest.mark.parametrize("kind,noise,N,d", FD_CASES)
def test_nlml_gradient_is_the_derivative_of_the_long_double_nlml(kind, noise, N, d):
    X, Y, ls, _, post, W = _ld_factor(kind, noise, N, d)
    ref, _, _ = R.nlml_gradient(kind, F.VARIANCE, ls, noise, X, W, post.alpha)
    # rho: the factor's backward error N 2^-64 |L||L|^T (three times: the two substitutions) moves the NLML by 1/2 tr(G dK)
    G = np.abs(W.T @ W - np.outer(post.alpha, post.alpha))
    aL = np.abs(post.L)
    rho = LD(1.5) * N * EPS_LD / 2 * np.sum(G * (aL @ aL.T))
    nlml = lambda var, l, s, c: F.Posterior(kind, var, l, s, c, X, Y).nlml
    bad = []
    for c in range(d):
        p, s1, s2 = _steps(ls[c], ls[c])
        f = [nlml(F.VARIANCE, np.concatenate([ls[:c], [v], ls[c + 1:]]), noise, F.MEAN) for v in p]
        _fd_check(f"d / d lengthscale {c}", f, s1, s2, ref[c], rho, bad)
    for slot, name, x0, call in ((d, "variance", F.VARIANCE, lambda v: nlml(v, ls, noise, F.MEAN)),
                                 (d + 1, "noise", noise, lambda v: nlml(F.VARIANCE, ls, v, F.MEAN)),
                                 (d + 2, "mean", F.MEAN, lambda v: nlml(F.VARIANCE, ls, noise, v))):
        p, s1, s2 = _steps(x0, x0)
        _fd_check(f"d / d {name}", [call(v) for v in p], s1, s2, ref[slot], rho, bad)
    assert not bad, "\n".join(bad)


FD_POINTS = (0, 8, 16, 17, 40)     # a training input, a point 1e-9 lengthscales from one, three uniform points


@pytest.mark.parametrize("kind,noise,N,d", FD_CASES)
def test_value_gradient_is_the_derivative_of_the_long_double_posterior(kind, noise, N, d):
    """mean, variance and v = -(mean - 2 sd) along every coordinate, W and alpha of the long-double factor held fixed."""
    X, _, ls, Xq, post, W = _ld_factor(kind, noise, N, d)
    Xq = Xq[list(FD_POINTS)]
    at = lambda x, beta: R.value_gradient(kind, F.VARIANCE, ls, F.MEAN, X, W, post.alpha, x, beta)
    r0, r2 = at(Xq, 0.0), at(Xq, 2.0)
    ok = r2["ok"]
    assert ok[2:].all()
    bad = []
    for c in range(d):
        ev0, ev2, spans = [], [], None
        cols = [_steps(x[c], ls[c]) for x in Xq]
        for k in range(4):
            x = Xq.copy()
            x[:, c] = [p[0][k] for p in cols]
            ev0.append(at(x, 0.0))
            ev2.append(at(x, 2.0))
        s1, s2 = np.array([p[1] for p in cols]), np.array([p[2] for p in cols])
        n63 = N * EPS_LD
        _fd_check(f"d mean / d x_{c}", [e["mean"] for e in ev0], s1, s2, r0["dmean"][:, c], n63 * r0["w_mean"], bad)
        _fd_check(f"d var / d x_{c}", [e["var"] for e in ev0], s1, s2, r0["dvar"][:, c], n63 * r0["w_var"], bad)
        _fd_check(f"d v(beta = 2) / d x_{c}", [e["v"][ok] for e in ev2], s1[ok], s2[ok], r2["g"][ok, c], n63 * r2["w_v"][ok], bad)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind,noise,N,d", FD_CASES)
@pytest.mark.parametrize("q,G", [(1, 2), (3, 2)])
def test_joint_vjp_is_the_derivative_of_the_long_double_joint_posterior(kind, noise, N, d, q, G):
    """phi = sum gmean mean + sum gcov cov over the groups, along every coordinate of every point."""
    X, _, ls, Xq, post, W = _ld_factor(kind, noise, N, d)
    gm, gc = R.adjoints(q, G)
    Xg = np.array(Xq[[0, 8, 16, 17, 40, 41][:q * G]].reshape(G, q, d))
    at = lambda x: R.joint(kind, F.VARIANCE, ls, F.MEAN, X, W, post.alpha, x, gm, gc)
    J = at(Xg)
    phi = lambda j: np.sum(gm * j["mean"]) + np.sum(gc * j["cov"])
    rho = N * EPS_LD * (np.sum(np.abs(gm) * J["w_mean"]) + np.sum(np.abs(gc) * J["w_cov"]))
    bad = []
    for g in range(G):
        for i in range(q):
            for c in range(d):
                p, s1, s2 = _steps(Xg[g, i, c], ls[c])
                f = []
                for v in p:
                    x = Xg.copy()
                    x[g, i, c] = v
                    f.append(phi(at(x)))
                _fd_check(f"d phi / d x[{g},{i},{c}]", f, s1, s2, J["vjp"][g, i, c], rho, bad)
    assert not bad, "\n".join(bad)


def test_K_exact_with_gradients_is_the_same_K():
    X, _, ls, Xq = R.design(17, F.D)
    for kind in ("rbf", "matern52"):
        K, dk, T, s = F.K_exact(kind, F.VARIANCE, ls, 0.0, X, Xq, grads=True)
        assert np.array_equal(K, F.K_exact(kind, F.VARIANCE, ls, 0.0, X, Xq))
        assert np.all(dk < 0) and T.shape == K.shape + (F.D,)
        assert np.all(T[:8][np.arange(8), np.arange(8)] == 0), "a query point that is a training input"


@pytest.mark.parametrize("d,N", [(13, 130), (40, 130)])
def test_wide_designs_are_neither_diagonal_nor_flat(d, N):
    X, _, ls, _ = R.design(N, d)
    for kind in ("rbf", "matern52"):
        K = np.asarray(F.K_exact(kind, 1.0, ls, 0.0, X, X), dtype=np.float64)
        med = np.median(K[~np.eye(N, dtype=bool)])
        assert 0.05 <= med <= 0.5, (kind, d, med)


# ---- the float64 restatement under every tolerance of the GPU cases ---------------------------------------------------------------------
def all_comparisons(kind, noise, N, d, W, alpha, bad, defect=None, which=("nlml", "value", "joint"), groups=R.GROUPS):
    """Every comparison of a case for the float64 restatement (with ``defect`` planted) -> {what: worst error / tolerance}."""
    X, _, ls, Xq = R.design(N, d)
    out, tag = {}, f"{kind} {noise:g} N={N} d={d}"
    if "nlml" in which:
        ref, tol, wgt = R.nlml_gradient(kind, F.VARIANCE, ls, noise, X, W, alpha)
        got = R.restate_nlml_gradient(kind, F.VARIANCE, ls, noise, X, W, alpha, defect)
        out["nlml gradient"] = R.compare(f"{tag} restated nlml gradient", got, ref, tol, wgt, N, bad)
    if "value" in which:
        for beta in (0.0, 2.0):
            vg = R.value_gradient(kind, F.VARIANCE, ls, F.MEAN, X, W, alpha, Xq[:64], beta)
            v, g, _, var, _, dvar = R.restate_value_gradient(kind, F.VARIANCE, ls, F.MEAN, X, W, alpha, Xq[:64], beta, defect)
            for what, got, key in (("value", v, "v"), ("gradient", g, "g")):
                out[f"{what} beta={beta:g}"] = R.compare(f"{tag} restated {what} beta={beta:g}", got, vg[key], vg["tol_" + key],
                                                        vg["w_" + key], N, bad, vg["ok"])
            if beta == 0.0:
                out["variance"] = R.compare(f"{tag} restated variance", var, vg["var"], vg["tol_var"], vg["w_var"], N, bad)
                out["variance gradient"] = R.compare(f"{tag} restated variance gradient", dvar, vg["dvar"], vg["tol_dvar"],
                                                     vg["w_dvar"], N, bad)
    if "joint" in which:
        for q, G in groups:
            for upper in (False, True):
                gm, gc = R.adjoints(q, G, upper)
                Xg = Xq[:q * G].reshape(G, q, d)
                J = R.joint(kind, F.VARIANCE, ls, F.MEAN, X, W, alpha, Xg, gm, gc)
                m, cv, vj = R.restate_joint(kind, F.VARIANCE, ls, F.MEAN, X, W, alpha, Xg, gm, gc, defect)
                for what, got in (("mean", m), ("cov", cv), ("vjp", vj)):
                    key = f"joint {what}"
                    r = R.compare(f"{tag} restated joint {what} q={q} G={G}" + (" upper" if upper else ""), got, J[what],
                                  J["tol_" + what], J["w_" + what], N, bad)
                    out[key] = max(out.get(key, 0.0), r)
    return out


@pytest.mark.parametrize("kind,noise,N,d", R.CASES)
def test_float64_restatement_uses_a_quarter_of_every_tolerance(kind, noise, N, d):
    _, W, alpha = R.reference_factor(kind, noise, N, d)
    bad = []
    worst = all_comparisons(kind, noise, N, d, W, alpha, bad)
    assert not bad, "\n".join(bad)
    assert max(worst.values()) <= 0.25, worst


# ---- planted defects -----------------------------------------------------------------------------------------------------------------------
DEFECT_HYPERS = (("matern52", 1e-2), ("rbf", 1e-5))      # (the tightest and the widest tolerances)


def _rejected(kind, noise, N, d, defect, which, key, groups=R.GROUPS):
    _, W, alpha = R.reference_factor(kind, noise, N, d)
    clean, planted = [], []
    all_comparisons(kind, noise, N, d, W, alpha, clean, None, (which,), groups)
    worst = all_comparisons(kind, noise, N, d, W, alpha, planted, defect, (which,), groups)
    assert not clean, clean
    assert worst[key] > 1.0 and planted, (defect, key, worst)


@pytest.mark.parametrize("kind,noise", DEFECT_HYPERS)
def test_a_dropped_slice_partial_is_rejected(kind, noise):
    """N = 257: slice 8 of the 16 holds row 256 alone."""
    for key in ("gradient beta=0", "gradient beta=2", "variance gradient", "variance"):
        _rejected(kind, noise, 257, F.D, "drop_slice", "value", key)


@pytest.mark.parametrize("kind,noise", DEFECT_HYPERS)
@pytest.mark.parametrize("N", [130, 386])
def test_a_pair_tile_weighted_once_is_rejected(kind, noise, N):
    _rejected(kind, noise, N, F.D, "tile_once", "nlml", "nlml gradient")


@pytest.mark.parametrize("kind,noise", DEFECT_HYPERS)
@pytest.mark.parametrize("N", [17, 257, 386])
def test_a_skipped_last_row_is_rejected(kind, noise, N):
    _rejected(kind, noise, N, F.D, "skip_last_row", "nlml", "nlml gradient")
    for key in ("gradient beta=0", "variance gradient"):
        _rejected(kind, noise, N, F.D, "skip_last_row", "value", key)


@pytest.mark.parametrize("kind,noise", DEFECT_HYPERS)
@pytest.mark.parametrize("N", [17, 386])
def test_a_one_triangle_Gs_is_rejected(kind, noise, N):
    _rejected(kind, noise, N, F.D, "gs_one_triangle", "joint", "joint vjp", ((5, 14),))


@pytest.mark.parametrize("kind,noise", DEFECT_HYPERS)
@pytest.mark.parametrize("N", [17, 386])
def test_a_skipped_cross_term_is_rejected(kind, noise, N):
    _rejected(kind, noise, N, F.D, "skip_cross_last", "joint", "joint vjp", ((5, 14), (2, 8)))


@pytest.mark.parametrize("kind,noise", DEFECT_HYPERS)
@pytest.mark.parametrize("N", [17, 386])
def test_a_float32_r2_in_one_row_is_rejected(kind, noise, N):
    _rejected(kind, noise, N, F.D, "f32_r2", "value", "gradient beta=0")
    _rejected(kind, noise, N, F.D, "f32_r2", "joint", "joint vjp", ((5, 14),))


def test_a_lengthscale_term_of_the_wrong_chunk_is_rejected():
    kind, noise, N, d = R.CASES[-1]
    assert d > R.MAX_D
    _rejected(kind, noise, N, d, "wide_chunk", "nlml", "nlml gradient")


# ---- the beta = 2 condition ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,noise,N,d", R.CASES)
def test_the_beta_2_condition_leaves_out_near_training_points_only(kind, noise, N, d):
    X, _, ls, Xq = R.design(N, d)
    _, W, alpha = R.reference_factor(kind, noise, N, d)
    ok2 = R.value_gradient(kind, F.VARIANCE, ls, F.MEAN, X, W, alpha, Xq[:64], 2.0)["ok"]
    ok0 = R.value_gradient(kind, F.VARIANCE, ls, F.MEAN, X, W, alpha, Xq[:64], 0.0)["ok"]
    assert ok0.all()
    assert ok2[16:].all(), "a uniform point is left out"
    if noise >= 1e-2:
        assert ok2.all()
