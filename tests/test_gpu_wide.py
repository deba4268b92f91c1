"""GPU tests of wide inputs (d > 32): the engine's wide kernel forms against the numpy oracle, at the tolerances of
test_gpu_parity.py (1e-5 relative plus the cancellation floor of tests/util.py; no tolerance is loosened for high d).

Wide inputs pad the dimension to a multiple of 32 and run new instantiations of the d-dependent kernels (the sweep with its
candidate tile in device scratch, K assembly, the NLML gradient, the gradient tails, the posterior mean); everything
downstream of K* is the narrow code.  What stays narrow-only is refused cleanly: the int8 sweep rungs and trajectories."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.util import assert_close, cancellation_floor, reparam_sample_atol

pytestmark = pytest.mark.gpu

CONFIGS = [
    # (name, objective, d, kind, N, noise)
    ("ackley33_m52_N300", O.ackley, 33, "matern52", 300, 1e-3),
    ("ackley64_rbf_N1000", O.ackley, 64, "rbf", 1000, 1e-2),
    ("ackley64_rbf_N1000_lownoise", O.ackley, 64, "rbf", 1000, 1e-5),
    ("ackley100_m32_N513", O.ackley, 100, "matern32", 513, 1e-3),
    ("ackley64_m12_N257", O.ackley, 64, "matern12", 257, 1e-3),
]
VARIANT_FUSED, VARIANT_SPLIT, VARIANT_SWEEP_SMALL = 1, 2, 1024


@pytest.fixture(autouse=True)
def _matern12_oracle_in_difference_form(request, monkeypatch):
    """For Matern-1/2 the oracle's squared distances are taken in the difference form.

    The oracle follows gpflow's dot-product form r^2 = |a|^2 + |b|^2 - 2 a.b, whose rounding error at a = b is about
    2 eps |a|^2 instead of 0.  A kernel smooth in r^2 turns that into a relative error of the same size in k.  Matern-1/2,
    k = s^2 exp(-sqrt(r^2)), turns it into s^2 sqrt(2 eps |a|^2), and |a|^2 grows with d.  At d = 64 that is ~1e-7 of
    s^2 at every training input, which propagates to the variance there and to the NLML (measured: variance 6.0e-8 off
    at a training input with noise 1e-3, against a tolerance of 1.4e-8).  The engine computes the exact 0.  So the
    reference is the oracle's own arithmetic with r^2 = sum_c (a_c - b_c)^2, at the unchanged tolerances."""
    callspec = getattr(request.node, "callspec", None)
    cfg = callspec.params.get("cfg") if callspec is not None else None
    if cfg is not None and cfg[3] == "matern12":
        monkeypatch.setattr(O, "scaled_square_dist", O.difference_form_sq_dist)


def _engine(kind, d, variance, ls, noise, c, X, Y, variant=0):
    from trieste_amd.engine import GPEngine

    eng = GPEngine(d, kind)
    eng.set_variant(variant)
    eng.set_hyper(variance, ls, noise, c)
    eng.set_data(X, Y)
    return eng


def _problem(obj, d, kind, N, noise, M=3000, seed=5678):
    X, Y = O.synthetic_problem(obj, d, N)
    ls = O.default_lengthscales(d)
    c = float(np.mean(Y))
    st = O.gpr_update(kind, 1.0, ls, noise, c, X, Y)
    rng = np.random.default_rng(seed)
    Xq = rng.uniform(size=(M, d))
    Xq[:5] = X[:5]                 # exactly at training inputs (variance cancellation)
    Xq[5] = Xq[6]                  # duplicated candidate (ties -> first index)
    Xq[-3:] = 4.0 + rng.uniform(size=(3, d))  # far field: var -> variance, EI underflow
    return X, Y, ls, c, st, Xq


def _argmax_agrees(idx, oracle_vals, tol):
    oi = int(np.argmax(oracle_vals))
    return idx == oi or abs(oracle_vals[oi] - oracle_vals[idx]) <= tol


# ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, VARIANT_FUSED, VARIANT_SPLIT], ids=["default-policy", "fused", "rowsplit"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_wide_sweep_matches_oracle(cfg, variant):
    """Predict (3000 candidates: the sweep, not the small path), eta, EI values, the fused arg-max and top-k under every launch
    policy of the wide sweep: the default (3000 candidates are 24 blocks: the row-group SPLIT form and its combine kernel), the
    one-workgroup-per-block form forced, the split forced."""
    _, obj, d, kind, N, noise = cfg
    X, Y, ls, c, st, Xq = _problem(obj, d, kind, N, noise)
    floor = cancellation_floor(N, 1.0, noise)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y, variant)
    mean, var = eng.predict(Xq)
    om, ov = O.predict(st, Xq)
    assert_close(mean, om, atol=floor * 10, what="mean")
    assert_close(var, ov, atol=floor, what="var")
    assert_close(eng.predict_mean(Xq), om, atol=floor * 10, what="predict_mean")
    eta = eng.eta()
    assert_close(eta, O.eta_min_mean(st), atol=floor, what="eta")
    ei = eng.acq_values("ei", eta, Xq)
    oei = O.expected_improvement(om, ov, eta)
    assert_close(ei, oei, atol=floor, what="ei")
    val, idx, x = eng.acq_argmax("ei", eta, Xq)
    assert idx == int(np.argmax(ei)) and val == ei[idx]
    assert_close(val, np.max(oei), atol=floor, what="max ei")
    assert _argmax_agrees(idx, oei, 1e-5 * np.max(oei) + floor), (idx, int(np.argmax(oei)))
    np.testing.assert_array_equal(x, Xq[idx])
    tv, ti = eng.acq_topk("ei", eta, Xq, 17)
    ov_, oi_ = O.top_k(ei, 17)
    np.testing.assert_array_equal(ti, oi_)
    np.testing.assert_array_equal(tv, ov_)
    for acq, par, fn in (("pi", eta, O.probability_of_improvement), ("nlcb", 1.96, O.negative_lower_confidence_bound)):
        assert_close(eng.acq_values(acq, par, Xq), fn(om, ov, par), atol=floor, what=acq)


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[2], CONFIGS[3]], ids=lambda c: c[0])
def test_wide_ego_sized_and_large_sweeps_pick_the_oracle_argmax(cfg):
    """EGO's 8000-candidate sweep (the SPLIT form) and a large sweep of 10^5 candidates (one workgroup per block): arg-max value
    and first index, top-k against the engine's own values."""
    _, obj, d, kind, N, noise = cfg
    X, Y, ls, c, st, _ = _problem(obj, d, kind, N, noise, M=8)
    floor = cancellation_floor(N, 1.0, noise)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    eta = eng.eta()
    rng = np.random.default_rng(99)
    for M in (8000, 100_000):
        Xq = rng.uniform(size=(M, d))
        Xq[17] = X[3]
        val, idx, _ = eng.acq_argmax("ei", eta, Xq)
        oei = np.concatenate([O.ei_values(st, Xq[s:s + 10000], eta) for s in range(0, M, 10000)])
        assert_close(val, np.max(oei), atol=floor, what=f"max ei M={M}")
        assert _argmax_agrees(idx, oei, 1e-5 * np.max(oei) + floor), (M, idx, int(np.argmax(oei)))
        ei = eng.acq_values("ei", eta, Xq)
        assert idx == int(np.argmax(ei)) and val == ei[idx]
        tv, ti = eng.acq_topk("ei", eta, Xq, 9)
        ov_, oi_ = O.top_k(ei, 9)
        np.testing.assert_array_equal(ti, oi_)
        np.testing.assert_array_equal(tv, ov_)


@pytest.mark.parametrize("M", [1, 65, 2048])
@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_wide_predict_at_a_handful_of_points_matches_the_oracle_and_the_sweep(cfg, M):
    """<= 2048 points take the small path (K*^T, skinny product, two-pass tail); the same points through the wide sweep
    (tgp_set_variant bit 10) agree with it and with the oracle."""
    _, obj, d, kind, N, noise = cfg
    X, Y, ls, c, st, Xq_all = _problem(obj, d, kind, N, noise, M=2100)
    Xq = np.ascontiguousarray(np.concatenate([Xq_all[:M - 3], Xq_all[-3:]]) if M >= 7 else Xq_all[:M])
    floor = cancellation_floor(N, 1.0, noise)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y, 0)
    sweep = _engine(kind, d, 1.0, ls, noise, c, X, Y, VARIANT_SWEEP_SMALL)
    mean, var = eng.predict(Xq)
    om, ov = O.predict(st, Xq)
    assert_close(mean, om, atol=floor * 10, what="mean (small path)")
    assert_close(var, ov, atol=floor, what="var (small path)")
    ms, vs = sweep.predict(Xq)
    assert_close(ms, om, atol=floor * 10, what="mean (sweep)")
    assert_close(vs, ov, atol=floor, what="var (sweep)")


@pytest.mark.parametrize("variant", [0, VARIANT_SWEEP_SMALL], ids=["skinny-product", "joint-sweep"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_wide_joint_qei_and_samples_match_oracle(cfg, variant):
    """predict_joint, qEI and the reparametrised samples at q = 1, 5, 50, 64 through the small path and the JOINT sweep (the
    register-staged joint instantiation: the packed DMA kernel is dp <= 16 only); a group starts at a training input."""
    _, obj, d, kind, N, noise = cfg
    X, Y, ls, c, st, _ = _problem(obj, d, kind, N, noise, M=8)
    floor = cancellation_floor(N, 1.0, noise)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y, variant)
    rng = np.random.default_rng(7)
    for q, G, S in ((1, 9, 8), (1, 300, 4), (5, 11, 32), (5, 60, 8), (50, 5, 16), (64, 3, 8)):
        Xg = rng.uniform(size=(G, q, d))
        Xg[0, 0] = X[0]
        jm, jc = eng.predict_joint(Xg)
        om, oc = O.predict_joint(st, Xg)
        assert_close(jm, om, atol=floor, what=f"joint mean q={q}")
        assert_close(jc, oc, atol=floor, what=f"joint cov q={q}")
        eps = rng.normal(size=(q, S))
        eta = float(np.median(om))
        want = O.batch_mc_ei(st, Xg, eps, eta, 1e-6)
        assert np.count_nonzero(want) >= want.size // 2, f"vacuous qEI comparison at q={q}"
        assert_close(eng.qei(Xg, eps, eta, 1e-6), want, atol=floor, what=f"qei q={q}")
        smp = eng.reparam_samples(Xg, eps, 1e-6)
        want_s = O.batch_reparam_samples(st, Xg, eps, 1e-6)
        assert_close(smp, want_s, atol=reparam_sample_atol(oc, floor, eps), what=f"reparam samples q={q}")


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_wide_acq_value_and_gradient_match_oracle(cfg):
    """tgp_acq_value_grad (the wide gradient tail: the coordinate chunk on a grid axis) vs the oracle's analytic gradient
    (finite-difference checked in tests/test_oracle_gradient.py), training inputs and the far field among the points."""
    _, obj, d, kind, N, noise = cfg
    X, Y, ls, c, st, Xq = _problem(obj, d, kind, N, noise, M=70)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    floor = cancellation_floor(N, 1.0, noise)
    eta = eng.eta()
    for acq, par in (("ei", eta), ("pi", eta), ("nlcb", 1.96), ("aei", eta)):
        val, grad = eng.acq_value_grad(acq, par, Xq)
        oval, ograd = O.acq_value_and_grad(st, acq, par, Xq)
        assert_close(val, oval, atol=floor, what=f"{acq} value")
        gscale = np.abs(ograd).max() + 1e-300
        assert_close(grad, ograd, rtol=1e-5, atol=max(floor * 1e3, 1e-9 * gscale), what=f"{acq} gradient")
        assert_close(val, eng.acq_values(acq, par, Xq), rtol=1e-9, atol=floor, what=f"{acq} value == sweep value")


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_wide_qei_value_and_gradient_match_the_oracle(cfg, monkeypatch):
    """The qEI gradient for the L-BFGS-B refinement of a joint batch: tgp_qei_value_grad, and tgp_joint_forward + the host's
    adjoint + tgp_joint_vjp (the wide partial layout), against the oracle's forward-mode derivative."""
    from trieste_amd.acquisition.function import batch_monte_carlo_expected_improvement

    _, obj, d, kind, N, noise = cfg
    X, Y, ls, c, st, _ = _problem(obj, d, kind, N, noise, M=8)
    floor = cancellation_floor(N, 1.0, noise)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    rng = np.random.default_rng(23)
    for q, G, S in ((1, 6, 32), (3, 5, 64), (9, 4, 70), (64, 2, 33)):
        Xg = rng.uniform(size=(G, q, d))
        eps = rng.normal(size=(q, S))
        eta = float(np.median(O.predict_joint(st, Xg)[0]))

        class _Sampler:
            def eps(self, qq):
                assert qq == q
                return eps

        fn = batch_monte_carlo_expected_improvement.__new__(batch_monte_carlo_expected_improvement)
        fn._engine, fn._sampler, fn._eta, fn._jitter, fn._sample_size = eng, _Sampler(), eta, 1e-6, S
        oval, ograd = O.batch_mc_ei_value_and_grad(st, Xg, eps, eta, 1e-6)
        gtol = max(floor * 1e3 * q, 1e-7 * (np.abs(ograd).max() + 1e-300))
        val, grad = fn.value_and_gradient(Xg)
        assert_close(val, oval, atol=floor, what=f"qEI value q={q}")
        assert_close(grad, ograd, rtol=1e-5, atol=gtol, what=f"qEI gradient q={q}")
        monkeypatch.setattr(type(eng), "qei_value_grad_fits", staticmethod(lambda q_, S_: False))
        hval, hgrad = fn.value_and_gradient(Xg)
        monkeypatch.undo()
        assert_close(hval, oval, atol=floor, what=f"qEI value (host adjoint) q={q}")
        assert_close(hgrad, ograd, rtol=1e-5, atol=gtol, what=f"qEI gradient (host adjoint) q={q}")


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_wide_nlml_gradient_and_trials_match_oracle(cfg):
    """tgp_nlml with its gradient (the wide pair reduction: one workgroup per coordinate chunk) vs the oracle; the value-only
    path; a batch of trials equal bit for bit to one-by-one trials at the same hyper-parameters."""
    _, obj, d, kind, N, noise = cfg
    X, Y, ls, c, st, _ = _problem(obj, d, kind, N, noise, M=8)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    val, grad = eng.nlml()
    oval, ograd = O.nlml_and_grad(st)
    assert grad.shape == (d + 3,)
    assert_close(val, oval, rtol=1e-9, atol=1e-7, what="nlml")
    vonly, gnone = eng.nlml(with_gradient=False)
    assert gnone is None and vonly == val
    assert_close(grad, ograd, rtol=1e-5, atol=1e-7 * np.abs(ograd).max() + 1e-6 / noise * 1e-6, what="nlml gradient")
    rng = np.random.default_rng(3)
    B = 5
    hy = np.empty((B, d + 3))
    hy[:, 0] = rng.uniform(0.5, 2.0, B)
    hy[:, 1:1 + d] = ls * rng.uniform(0.7, 1.4, size=(B, d))
    hy[:, 1 + d] = noise * rng.uniform(1.0, 3.0, B)
    hy[:, 2 + d] = c + rng.normal(size=B) * 0.1
    values, ok = eng.nlml_trial_batch(hy)
    assert ok.all() and np.isfinite(values).all()
    single = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    for b in range(B):
        single.set_hyper(hy[b, 0], hy[b, 1:1 + d], hy[b, 1 + d], hy[b, 2 + d])
        assert single.nlml_trial() == values[b], (b, single.nlml_trial(), values[b])
        sb = O.gpr_update(kind, hy[b, 0], hy[b, 1:1 + d], hy[b, 1 + d], hy[b, 2 + d], X, Y)
        assert_close(values[b], O.nlml_and_grad(sb)[0], rtol=1e-9, atol=1e-7, what="trial value")


def test_wide_trial_batch_at_the_persistent_kernels_sizes():
    """N = 2048, d = 64: the batched trials through one persistent launch (the members' lengthscales behind the fixed
    variance / noise / mean slots of the wide layout) equal one-by-one trials bit for bit, and the oracle's values."""
    d, N, noise, kind = 64, 2048, 1e-2, "matern52"
    X, Y = O.synthetic_problem(O.ackley, d, N)
    ls = O.default_lengthscales(d)
    c = float(np.mean(Y))
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    rng = np.random.default_rng(4)
    B = 4
    hy = np.empty((B, d + 3))
    hy[:, 0] = rng.uniform(0.5, 2.0, B)
    hy[:, 1:1 + d] = ls * rng.uniform(0.7, 1.4, size=(B, d))
    hy[:, 1 + d] = noise * rng.uniform(1.0, 3.0, B)
    hy[:, 2 + d] = c
    values, ok = eng.nlml_trial_batch(hy)
    assert ok.all()
    for b in range(B):
        eng.set_hyper(hy[b, 0], hy[b, 1:1 + d], hy[b, 1 + d], hy[b, 2 + d])
        assert eng.nlml_trial() == values[b], b
        sb = O.gpr_update(kind, hy[b, 0], hy[b, 1:1 + d], hy[b, 1 + d], hy[b, 2 + d], X, Y)
        assert_close(values[b], O.nlml_and_grad(sb)[0], rtol=1e-9, atol=1e-7, what="trial value")


@pytest.mark.parametrize("cfg", CONFIGS, ids=[c[0] for c in CONFIGS])
def test_wide_cov_between_clone_and_append(cfg):
    """tgp_cov_between vs the oracle; a clone conditioned on new rows by tgp_append_data vs a refit on the concatenated data."""
    _, obj, d, kind, N, noise = cfg
    X, Y, ls, c, st, Xq = _problem(obj, d, kind, N, noise, M=200)
    floor = cancellation_floor(N + 80, 1.0, noise)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    for p1, p2 in ((1, 1), (63, 65), (5, 200)):
        X1, X2 = Xq[:p1], Xq[200 - p2:]
        assert_close(eng.cov_between(X1, X2), O.covariance_between_points(st, X1, X2), atol=floor * 10, what=f"cov {p1}x{p2}")
    rng = np.random.default_rng(23)
    cl = eng.clone()
    Xall, Yall = X, Y
    for k in (1, 70):
        Xn = rng.uniform(size=(k, d))
        Yn = rng.standard_normal(k) * 0.3 + c
        cl.append_data(Xn, Yn)
        Xall, Yall = np.concatenate([Xall, Xn]), np.concatenate([Yall, Yn])
        full = _engine(kind, d, 1.0, ls, noise, c, Xall, Yall)
        sto = O.gpr_update(kind, 1.0, ls, noise, c, Xall, Yall)
        assert_close(cl.get_factor()[0], full.get_factor()[0], rtol=1e-9, atol=floor, what="L append == refit")
        ma, va = cl.predict(Xq)
        mo, vo = O.predict(sto, Xq)
        assert_close(ma, mo, atol=floor * 10, what="mean after append")
        assert_close(va, vo, atol=floor, what="var after append")
        assert_close(cl.eta(), O.eta_min_mean(sto), atol=floor, what="eta after append")
    m0, v0 = eng.predict(Xq)   # the original is untouched
    om, ov = O.predict(st, Xq)
    assert_close(m0, om, atol=floor * 10, what="original mean")


def test_wide_gibbon_with_a_repulsion_twin_of_a_few_appended_rows_sweeps_the_twin():
    """A twin that is this model + m <= 16 rows takes the rank-m form (kernel sums of the trajectory kernel) at d <= 32.  That
    kernel has no wide instantiation: at d = 33 the twin is swept, and GIBBON equals the oracle's block-determinant form at
    the tolerances of test_gpu_parity.py's rank-m test.  (Before the launchers refused a padded dimension they are not compiled
    for, this case ran the dp = 32 instantiation over rows of 64 coordinates and returned numbers.)"""
    _, obj, d, kind, N, noise = CONFIGS[0]
    X, Y, ls, c, st, Xq = _problem(obj, d, kind, N, noise, M=1200)
    floor = cancellation_floor(N, 1.0, noise)
    rng = np.random.default_rng(17)
    samples = O.eta_min_mean(st) - np.array([0.02, 0.1, 0.3])
    om, ov = O.predict(st, Xq)
    gmax = np.max((samples[None, :] - om[:, None]) / np.sqrt(ov)[:, None], axis=1)
    ok = gmax <= 30.0
    m = 3
    pending = rng.uniform(size=(m, d))
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    eng.set_min_value_samples(samples)
    twin = eng.clone()
    twin.append_data(pending, rng.standard_normal(m))  # observations do not matter
    eng.set_repulsion(twin, 1.0 / m ** 2)
    vals = eng.acq_values("gibbon", 0.0, Xq)
    ref = O.gibbon_quality_term(om, ov, samples, noise) + O.gibbon_repulsion_term(st, Xq, pending, True)
    sens = floor * 10 * (1.0 + np.abs(gmax)) / np.sqrt(ov) + floor / noise + 1e-13
    assert_close(vals[ok], ref[ok], rtol=1e-6, atol=sens[ok], what="wide GIBBON with a rank-3 twin == reference form")


@pytest.mark.parametrize("kind", ["soft", "hard"])
def test_wide_penalized_values_and_gradient_match_oracle(kind):
    """Local penalization at d = 64 (the penalty kernels loop over the coordinates: no MAX_D-sized locals)."""
    _, obj, d, kname, N, noise = CONFIGS[1]
    X, Y, ls, c, st, Xq = _problem(obj, d, kname, N, noise, M=3000)
    floor = cancellation_floor(N, 1.0, noise)
    eng = _engine(kname, d, 1.0, ls, noise, c, X, Y)
    rng = np.random.default_rng(11)
    pending = np.concatenate([rng.uniform(size=(4, d)), Xq[7:8]])
    lip, eta = O.lipschitz_estimate(st, np.concatenate([X, rng.uniform(size=(100, d))]))
    radius, scale = O.local_penalizer_parameters(st, pending, lip, eta)
    base = eng.acq_values("ei", eta, Xq)
    open_ = O.PENALIZERS[kind](Xq, pending, radius, scale)
    with eng.penalized(kind, pending, radius, scale):
        assert_close(eng.penalization_values(Xq), open_, rtol=1e-11, atol=1e-300, what="penalization")
        vals = eng.acq_values("ei", eta, Xq)
        val, idx, _ = eng.acq_argmax("ei", eta, Xq)
        gv, gg = eng.acq_value_grad("ei", eta, Xq[:64])
    assert_close(vals, base * open_, rtol=1e-11, atol=1e-300, what="penalized = base * phi")
    assert idx == int(np.argmax(vals)) and val == vals[idx]
    oval, ograd = O.penalized_value_and_grad(st, "ei", eta, kind, pending, radius, scale, Xq[:64])
    assert_close(gv, oval, atol=floor, what="penalized value")
    gscale = np.abs(ograd).max() + 1e-300
    assert_close(gg, ograd, rtol=1e-5, atol=max(floor * 1e3, 1e-9 * gscale), what="penalized gradient")


def test_wide_every_ei_value_at_n4096():
    """d = 64, N = 4096, 2^15 candidates: every EI value of the sweep against the oracle, and the arg-max."""
    d, N, noise, kind = 64, 4096, 1e-2, "matern52"
    X, Y, ls, c, st, Xq = _problem(O.ackley, d, kind, N, noise, M=1 << 15)
    floor = cancellation_floor(N, 1.0, noise)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    eta = eng.eta()
    assert_close(eta, O.eta_min_mean(st), atol=floor, what="eta")
    ei = eng.acq_values("ei", eta, Xq)
    oei = np.concatenate([O.ei_values(st, Xq[s:s + 4096], eta) for s in range(0, Xq.shape[0], 4096)])
    assert_close(ei, oei, atol=floor, what="ei")
    val, idx, _ = eng.acq_argmax("ei", eta, Xq)
    assert idx == int(np.argmax(ei)) and val == ei[idx]
    assert _argmax_agrees(idx, oei, 1e-5 * np.max(oei) + floor)


def test_wide_d256_update_predict_and_argmax():
    """d = 256 (eight coordinate chunks), RBF, N = 200: the factor, the posterior through the sweep, the EI arg-max."""
    d, N, noise, kind = 256, 200, 1e-3, "rbf"
    X, Y, ls, c, st, Xq = _problem(O.ackley, d, kind, N, noise, M=4000)
    floor = cancellation_floor(N, 1.0, noise)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    assert_close(eng.get_factor()[0], st.L, atol=floor, what="L")
    mean, var = eng.predict(Xq)
    om, ov = O.predict(st, Xq)
    assert_close(mean, om, atol=floor * 10, what="mean")
    assert_close(var, ov, atol=floor, what="var")
    eta = eng.eta()
    val, idx, _ = eng.acq_argmax("ei", eta, Xq)
    oei = O.expected_improvement(om, ov, eta)
    assert_close(val, np.max(oei), atol=floor, what="max ei")
    assert _argmax_agrees(idx, oei, 1e-5 * np.max(oei) + floor)


def test_wide_precision_trajectories_and_limits():
    """At d = 64: "auto" resolves to float64 at once (results bit for bit the float64 ones), "i8x4" / "i8x5" are refused,
    trajectories are refused before anything is launched; d above the engine's limit is a shape error."""
    import trieste_amd.models as M
    from trieste_amd import _lib
    from trieste_amd.acquisition.rule import DiscreteThompsonSampling
    from trieste_amd.acquisition.sampler import ThompsonSamplerFromTrajectory
    from trieste_amd.data import Dataset
    from trieste_amd.engine import GPEngine
    from trieste_amd.space import Box

    _, obj, d, kind, N, noise = CONFIGS[1]
    X, Y, ls, c, st, Xq = _problem(obj, d, kind, N, noise, M=20000)
    f64 = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    auto = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    auto.set_precision("auto")
    eta = f64.eta()
    for a, b in zip(auto.predict(Xq), f64.predict(Xq)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(auto.acq_values("ei", eta, Xq), f64.acq_values("ei", eta, Xq))
    assert auto.acq_argmax("ei", eta, Xq)[:2] == f64.acq_argmax("ei", eta, Xq)[:2]
    for p in ("i8x4", "i8x5"):
        with pytest.raises(ValueError):
            f64.set_precision(p)
    rng = np.random.default_rng(0)
    F = 16
    with pytest.raises(ValueError, match="up to 32"):
        f64.trajectory(rng.normal(size=(F, d)), rng.uniform(size=F), rng.normal(size=(F, 2)), rng.normal(size=(N, 2)))
    with pytest.raises(ValueError, match="up to 32"):
        f64.trajectory_rff(rng.normal(size=(F, d)), rng.uniform(size=F), rng.normal(size=(F, 2)))
    space = Box([0.0] * d, [1.0] * d)
    data = Dataset(X[:40], Y[:40, None])
    model = M.GaussianProcessRegression(M.build_gpr(data, space, likelihood_variance=noise))
    with pytest.raises(ValueError, match="up to 32"):
        model.trajectory_sampler()
    rule = DiscreteThompsonSampling(1000, 2, thompson_sampler=ThompsonSamplerFromTrajectory())
    with pytest.raises(ValueError, match="up to 32"):
        rule.acquire(space, {"OBJECTIVE": model}, {"OBJECTIVE": data})
    GPEngine(_lib.MAX_D, kind)   # the limit itself is accepted
    with pytest.raises(ValueError, match="d must be in"):
        GPEngine(_lib.MAX_D + 1, kind)


def test_wide_group_of_one_returns_the_engines_argmax_and_topk():
    from trieste_amd.group import GPEngineGroup

    _, obj, d, kind, N, noise = CONFIGS[1]
    X, Y, ls, c, st, Xq = _problem(obj, d, kind, N, noise, M=20000)
    eng = _engine(kind, d, 1.0, ls, noise, c, X, Y)
    eta = eng.eta()
    grp = GPEngineGroup(d, kind, devices=[0])
    try:
        grp.set_hyper(1.0, ls, noise, c)
        grp.set_data(X, Y)
        grp.set_candidates(Xq)
        gval, gidx, _ = grp.acq_argmax("ei", eta)
        val, idx, _ = eng.acq_argmax("ei", eta, Xq)
        assert (gval, gidx) == (val, idx)
        gv, gi = grp.acq_topk("ei", eta, 9)
        tv, ti = eng.acq_topk("ei", eta, Xq, 9)
        np.testing.assert_array_equal(gi, ti)
        np.testing.assert_array_equal(gv, tv)
    finally:
        grp.close()


def test_wide_ask_tell_ego_on_a_50d_ackley():
    """End to end at d = 50: EGO with ExpectedImprovement over a fixed candidate set picks the oracle's arg-max; five Ask-Tell
    steps of the default EGO (sweep + L-BFGS-B refinement) with a fit every step stay inside the box; one batch of
    BatchMonteCarloExpectedImprovement (q = 3) is refined by L-BFGS-B on the engine's qEI gradient."""
    import trieste_amd.models as M
    from trieste_amd.acquisition import BatchMonteCarloExpectedImprovement, EfficientGlobalOptimization, ExpectedImprovement
    from trieste_amd.ask_tell_optimization import AskTellOptimizer
    from trieste_amd.data import Dataset
    from trieste_amd.space import Box, DiscreteSearchSpace

    d = 50
    space = Box([0.0] * d, [1.0] * d)
    x = space.sample(60, seed=0)
    data = Dataset(x, O.ackley(x)[:, None])
    model = M.GaussianProcessRegression(M.build_gpr(data, space, likelihood_variance=1e-3))
    g = model.model
    st = O.gpr_update("matern52", g.kernel.variance, g.kernel.lengthscales, g.likelihood_variance, g.mean_function.c,
                      x, data.observations[:, 0])
    cands = np.random.default_rng(1).uniform(size=(8000, d))
    pt = EfficientGlobalOptimization(ExpectedImprovement()).acquire_single(DiscreteSearchSpace(cands), model, dataset=data)
    oei = O.ei_values(st, cands, O.eta_min_mean(st))
    floor = cancellation_floor(60, g.kernel.variance, g.likelihood_variance)
    hit = int(np.where((cands == pt[0]).all(axis=1))[0][0])
    assert _argmax_agrees(hit, oei, 1e-5 * np.max(oei) + floor), (hit, int(np.argmax(oei)))
    opt = AskTellOptimizer(space, data, model, EfficientGlobalOptimization(ExpectedImprovement()))
    for _ in range(5):
        q = opt.ask()
        assert q.shape == (1, d) and np.all((q >= 0.0) & (q <= 1.0))
        opt.tell(Dataset(q, O.ackley(q)[:, None]))
    assert opt.dataset.query_points.shape == (65, d)
    builder = BatchMonteCarloExpectedImprovement(256)
    batch = EfficientGlobalOptimization(builder, num_query_points=3).acquire_single(space, model, dataset=opt.dataset)
    assert batch.shape == (3, d) and np.all((batch >= 0.0) & (batch <= 1.0))
    val = float(np.asarray(builder.prepare_acquisition_function(model, dataset=opt.dataset)(batch[None]))[0, 0])
    assert np.isfinite(val) and val >= 0.0


def test_wide_default_ego_beyond_the_top_k_limit():
    """d = 110: the default optimizer starts 10 d = 1100 L-BFGS-B runs, more than tgp_acq_topk's k <= 1024; the best starts are
    then ranked from the swept values on the host.  The pick is inside the box with a positive EI."""
    import trieste_amd.models as M
    from trieste_amd.acquisition import EfficientGlobalOptimization, ExpectedImprovement
    from trieste_amd.data import Dataset
    from trieste_amd.space import Box

    d = 110
    space = Box([0.0] * d, [1.0] * d)
    x = space.sample(40, seed=2)
    data = Dataset(x, O.ackley(x)[:, None])
    model = M.GaussianProcessRegression(M.build_gpr(data, space, likelihood_variance=1e-3))
    rule = EfficientGlobalOptimization(ExpectedImprovement())
    pt = rule.acquire_single(space, model, dataset=data)
    assert pt.shape == (1, d) and np.all((pt >= 0.0) & (pt <= 1.0))
    val = float(np.asarray(rule.acquisition_function(pt[None]))[0, 0])
    assert np.isfinite(val) and val > 0.0
