"""`update`'s three device arrays -- L, W = L^-1, alpha (GPEngine.get_factor) -- and what is derived from them (predict through the
small product and through the sweep, nlml, nlml_trial, nlml_trial_batch, append_data, clone_from) at their OWN resolution:
residuals accumulated in long double against K_exact and the long-double posterior, judged by the data-dependent bounds
derived in tests/factor_resolution.py.  Every form of `update` (tgp_set_variant, as in tests/test_gpu_dag.py) is judged against
that reference bound; no form is judged against another.

The forward comparisons of tests/test_gpu_dag.py allow 64 eps (1 + N / noise) max|L| -- 1.4e-6 at N = 1000, noise 1e-5 -- where a
backward-stable factor's residual is of order N eps |L||L|^T whatever the conditioning; tests/test_factor_resolution.py pins that gap.

With TGP_FACTOR_RESIDUALS=<file> in the environment the session also writes the worst residual / bound per form, size and noise
beside the same ratio of the float64 reference (scipy) -- profiles/r12_factor_residuals.txt is one such table."""
import os

import numpy as np
import pytest

from tests import factor_resolution as F
from tests.util import record_margin

pytestmark = pytest.mark.gpu

NO_DAG, DAG_SMALL, DAG_WHOLE_TILES, DAG_ONE_CHAIN = 16, 32, 256, 512
FORMS = dict(default=0, one_chain=DAG_SMALL | DAG_ONE_CHAIN, whole_tiles=DAG_SMALL | DAG_WHOLE_TILES, recursion=NO_DAG)
SIZES = (1, 17, 128, 129, 256, 257, 384, 513, 640, 1100)
# Npad = 256 is two block rows: no split plan, the whole-tile plan IS the one-workgroup chain's there
CASES = [(k, s, N, f) for k, s in F.HYPERS for N in SIZES for f in FORMS if not (f == "whole_tiles" and N <= 256)]
CASES += [F.LOW_NOISE + (N, f) for N in (128, 640) for f in FORMS if not (f == "whole_tiles" and N <= 256)]
_REFERENCE = {}
REPORT = []      # (form, kind, noise, N, what, engine's ratio, reference's ratio or None)


@pytest.fixture(scope="module", autouse=True)
def _write_report():
    yield
    path = os.environ.get("TGP_FACTOR_RESIDUALS")
    if path and REPORT:
        with open(path, "w") as f:
            f.write("worst residual / bound (tests/factor_resolution.py) of the device arrays, beside the float64 reference's (the\n"
                    "oracle's factor, scipy's triangular inverse, cho_solve alpha) under the SAME bound\n")
            f.write(f"{'form':<24}{'kind':<10}{'noise':>7}{'N':>6}  {'quantity':<12}{'engine':>11}{'reference':>11}\n")
            for form, kind, noise, N, what, r, ref in REPORT:
                f.write(f"{form:<24}{kind:<10}{noise:>7g}{N:>6}  {what:<12}{r:>11.3g}" + (f"{ref:>11.3g}\n" if ref is not None else f"{'-':>11}\n"))


def _engine(kind, noise, X, Y, ls, variant):
    from trieste_amd.engine import GPEngine

    eng = GPEngine(F.D, kind)
    eng.set_variant(variant)
    eng.set_hyper(F.VARIANCE, ls, noise, F.MEAN)
    eng.set_data(np.ascontiguousarray(X), np.ascontiguousarray(Y))
    return eng


def _residuals(tag, form_name, kind, noise, N, levels, L, W, alpha, bad, probes_see_tiles=True):
    """L, W exactly lower triangular; the four residuals by the full evaluation (N <= 640) or tile probes.  The probes are used
    only under the persistent kernel's tile levels: under the recursion's and the append's levels (blocks of hundreds of rows)
    they do not see a 2^-36 error of one tile of L (tests/test_factor_resolution.py PROBES_MISS), so those two forms get the full
    evaluation above N = 640 as well."""
    if not (np.array_equal(np.triu(L, 1), np.zeros_like(L)) and np.array_equal(np.triu(W, 1), np.zeros_like(W))):
        bad.append(f"{tag}: L or W is not exactly lower triangular")
    K, E, err = F.k_parts(kind, noise, N)
    evaluate = F.full_ratios if N <= F.FULL_MAX or not probes_see_tiles else F.probe_ratios
    r = evaluate(L, W, alpha, K, E, err, levels, tag, bad)
    ref = {}
    if os.environ.get("TGP_FACTOR_RESIDUALS"):
        key = (kind, noise, N, repr(levels))
        if key not in _REFERENCE:
            _REFERENCE[key] = evaluate(*F.reference_factor(kind, noise, N), K, E, err, levels, tag + " (reference)", [])
        ref = _REFERENCE[key]
    for what, v in r.items():
        REPORT.append((form_name, kind, noise, N, what, v, ref.get(what)))
    return r


def _compare(tag, what, got, ref, tol, bad, row):
    err = np.abs(np.asarray(got, dtype=F.LD) - ref).astype(np.float64)
    worst = record_margin(f"{tag} {what}", err, tol)
    REPORT.append(row + (what, worst, None))
    if not np.all(err <= tol):
        bad.append(f"{tag} {what}: error / tolerance = {worst:.3g}")


def _posterior_checks(tag, row, eng, post, ms, Xq, bad, sweep=True):
    """Mean and variance at ``Xq`` through the small product and (at 4096 points, the same ones first) through the sweep; ``ms`` the
    measured residuals of the arrays the engine predicts from."""
    pred = post.predict(Xq)
    tol_mean, tol_var = F.posterior_tolerances(ms, post, pred)
    ref_var = np.maximum(pred[1], F.LD(1e-12))                  # (the engine clips at the reference's 1e-12)
    m, v = eng.predict(Xq)
    _compare(tag, "mean", m, pred[0], tol_mean, bad, row)
    _compare(tag, "variance", v, ref_var, tol_var, bad, row)
    if sweep:
        big = np.concatenate([Xq, np.random.default_rng(4096).uniform(size=(4096 - len(Xq), F.D))])
        m, v = eng.predict(big)
        _compare(tag, "mean(sweep)", m[:len(Xq)], pred[0], tol_mean, bad, row)
        _compare(tag, "var(sweep)", v[:len(Xq)], ref_var, tol_var, bad, row)


@pytest.mark.parametrize("kind,noise,N,form", CASES)
def test_update_arrays_and_posterior(kind, noise, N, form):
    X, Y, ls = F.problem(N)
    eng = _engine(kind, noise, X, Y, ls, FORMS[form])
    persistent = eng.update_is_persistent(N)
    levels = F.form_levels("dag" if persistent else "recursion", N)
    tag, row = f"{form} {kind} {noise:g} N={N}", (form, kind, noise, N)
    bad = []
    L, W, alpha = eng.get_factor()
    _residuals(tag, form, kind, noise, N, levels, L, W, alpha, bad, probes_see_tiles=persistent)
    if N <= F.FULL_MAX:
        post = F.posterior(kind, noise, N)
        ms = F.Measured(L, W, alpha, post.K, post.err)
        _posterior_checks(tag, row, eng, post, ms, F.query_points(N), bad)
        tol_full, tol_trial = F.nlml_tolerance(ms, post, False), F.nlml_tolerance(ms, post, persistent)
        _compare(tag, "nlml", eng.nlml(False)[0], post.nlml, tol_full, bad, row)
        _compare(tag, "nlml_trial", eng.nlml_trial(), post.nlml, tol_trial, bad, row)    # (leaves no posterior: last)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("kind", ["matern52", "rbf"])
@pytest.mark.parametrize("N,variant", [(17, 0), (257, DAG_SMALL), (513, 0)])
def test_trial_batch_against_the_long_double_nlml(kind, N, variant):
    """Three members in one call -- noise 1e-2, noise 1e-5, noise 1e-2 with another mean: the factor-only plan has no factor to read
    back, its value is its only witness; its budget is 8 times the one measured on the full update's arrays at the member's
    hyper-parameters (tests/factor_resolution.py nlml_tolerance)."""
    X, Y, ls = F.problem(N)
    eng = _engine(kind, 1e-2, X, Y, ls, variant)
    persistent = eng.update_is_persistent(N)
    members = [(1e-2, F.MEAN), (1e-5, F.MEAN), (1e-2, 0.7)]
    hy = np.array([np.concatenate([[F.VARIANCE], ls, [s, c]]) for s, c in members])
    values, ok = eng.nlml_trial_batch(hy)
    assert ok.all()
    bad, tag = [], f"trial batch {kind} N={N}"
    for b, (s, c) in enumerate(members):
        post = F.posterior(kind, s, N)
        post = post if c == F.MEAN else post.with_mean(c)
        eng.set_hyper(F.VARIANCE, ls, s, c)
        eng.set_data(np.ascontiguousarray(X), np.ascontiguousarray(Y))
        tol = F.nlml_tolerance(F.Measured(*eng.get_factor(), post.K, post.err), post, persistent)
        _compare(tag, f"member {b}", values[b], post.nlml, tol, bad, ("trial_batch", kind, s, N))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("N0,k,variant,clone", [(250, 1, NO_DAG, False), (250, 7, NO_DAG, False), (1030, 40, 0, False), (250, 1, NO_DAG, True)])
@pytest.mark.parametrize("kind,noise", [("matern52", 1e-5), ("rbf", 1e-2)])
def test_append_data(kind, noise, N0, k, variant, clone):
    """append_data onto N0 points: the node step at keep = floor(N0 / 64) 64 while the padded size stays (k = 1 onto 250 through the
    recursion's products, k = 40 onto 1030 through the split-k strips), a full update when it grows (k = 7 onto 250, crossing 256);
    after clone_from, the fantasised posterior.  The same residual bounds at the final N, the posterior at the appended points."""
    N = N0 + k
    X, Y, ls = F.problem(N)
    eng = _engine(kind, noise, X[:N0], Y[:N0], ls, variant)
    if clone:
        from trieste_amd.engine import GPEngine

        src, eng = eng, GPEngine(F.D, kind)
        eng.set_variant(variant)
        eng.clone_from(src)
    eng.append_data(np.ascontiguousarray(X[N0:]), np.ascontiguousarray(Y[N0:]))
    same_pad = -(-N // 256) == -(-N0 // 256)
    if same_pad:
        levels = F.form_levels("append", N, keep=(N0 // 64) * 64)
    else:
        levels = F.form_levels("dag" if eng.update_is_persistent(N) else "recursion", N)
    form = ("clone+" if clone else "") + f"append {k} onto {N0}"
    tag, bad = f"{form} {kind} {noise:g}", []
    L, W, alpha = eng.get_factor()
    _residuals(tag, form, kind, noise, N, levels, L, W, alpha, bad, probes_see_tiles=not same_pad and eng.update_is_persistent(N))
    post = F.posterior(kind, noise, N)                          # (N = 1070 too: one long-double factor per hyper-parameter pair)
    Xq = np.concatenate([X[N0:], X[N0:] + 1e-9 * ls, F.query_points(N)[-8:]])
    _posterior_checks(tag, (form, kind, noise, N), eng, post, F.Measured(L, W, alpha, post.K, post.err), Xq, bad, sweep=False)
    assert not bad, "\n".join(bad)
