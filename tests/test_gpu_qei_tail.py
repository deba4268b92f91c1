"""GPU: the Monte-Carlo qEI tail and its adjoint (``qei_tail_kernel``, ``qei_grad_tail_kernel``) on GIVEN moments, at their own
resolution: against 50-digit goldens and the numpy restatement for every q = 1 ... 64 in every regime of output scale and
threshold, at the sample counts around the wave width and at the largest count the gradient tail's LDS holds, on degenerate
batches (a duplicate point, cov = 0, a diagonal at the clip and next to it, an exact tie, an improvement of exactly 0, an
exactly singular group), and bit for bit against the model entries that run the same kernels.

Tolerances (tests/test_qei_reference.py measures the constants and checks, on the CPU, the conditions they rely on):
  value, samples   100 x QEI_RESTATEMENT_WORST x the scale of the entry
  gcov             100 x QEI_GRAD_RESTATEMENT_WORST x its scale, entrywise; symmetric within the two entries' tolerances
  gmean            2 ulp of count / S: away from a kink it is an integer count times 1 / S
  + lip x sample_atol on value, samples and gcov of the near-duplicate and jitter-dominated inputs (``conditioned_tolerances``).
No group is left out: every input keeps its kinks further away than ``sample_atol`` (asserted on the CPU).

What each test would catch: a dropped eps column of a ragged block moves samples, values and counts of the draws 64 ... S - 1
(the goldens at S = 65, the sweep at S = 65, the edges at 63 / 65 / 129); ``<=`` in the tie rule sends the count of the exact
tie to index 1; a missing clip leaves gcov_ii != 0 at cov = 0 and at the diagonal of exactly 1e-12; an adjoint scaled by
1 + 1e-9 is 260 x the gcov tolerance wherever an entry is as large as its scale (q = 1: |gcov| / scale is 0.2 ... 1)."""
import numpy as np
import pytest

from tests import qei_reference as QR
from tests import test_qei_reference as T
from tests.make_qei_tail_goldens import SCALES, SHIFTS
from tests.util import record_margin

pytestmark = pytest.mark.gpu

VAL_TOL = 100.0 * T.QEI_RESTATEMENT_WORST
GRAD_TOL = 100.0 * T.QEI_GRAD_RESTATEMENT_WORST
JITTER = T.JITTER


def _E():
    from trieste_amd import engine as E

    return E


def _bare_engine(d=2):
    return _E().GPEngine(d, "matern52", device=0)


def _check(what, got, want, tol):
    got, want, tol = (np.asarray(a, np.float64) for a in (got, want, tol))
    tol = np.broadcast_to(tol, want.shape)
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    err = np.abs(got - want)
    worst = record_margin(what, err, tol)
    print(f"{what}: worst {worst:.3f} of the tolerance")
    assert np.all(err <= tol), (what, float(np.max(err / np.where(tol > 0, tol, 1.0))), float(np.max(err[tol == 0.0], initial=0.0)))


def _check_gmean(what, gm, counts, S):
    want = -counts / float(S)
    _check(f"{what} gmean", gm, want, 2.0 * np.spacing(np.abs(want)) * (counts > 0))


def _call(E, eng, mean, cov, eps, eta, jitter):
    """(value, samples, gmean, gcov) of the two entries; the gradient entry's value IS the value entry's."""
    val, sam = E.qei_moments(eng, mean, cov, eps, eta, jitter, samples=True)
    gval, gm, gc = E.qei_moments_grad(eng, mean, cov, eps, eta, jitter)
    np.testing.assert_array_equal(gval, val)
    np.testing.assert_array_equal(E.qei_moments(eng, mean, cov, eps, eta, jitter), val)    # with and without the samples
    return val, sam, gm, gc


def _check_against(what, got, r, want, cond_terms=None, parts=("value", "samples", "gmean", "gcov")):
    """The device's (value, samples, gmean, gcov) against ``want`` (a dict of value, samples, counts, gcov: the restatement ``r``
    itself or a golden case in its layout) with ``r``'s scales, by the rule of the module docstring."""
    val, sam, gm, gc = got
    cv, cs, cg = cond_terms if cond_terms is not None else (0.0, 0.0, 0.0)
    S = r["samples"].shape[1]
    if "value" in parts:
        _check(f"{what} value", val, want["value"], VAL_TOL * r["value_scale"] + cv)
    if "samples" in parts:
        _check(f"{what} samples", sam, want["samples"], VAL_TOL * r["samples_scale"] + cs)
    if "gmean" in parts:
        _check_gmean(what, gm, want["counts"], S)
    if "gcov" in parts:
        tol = GRAD_TOL * r["gcov_scale"] + cg
        _check(f"{what} gcov", gc, want["gcov"], tol)
        _check(f"{what} gcov symmetry", gc, np.swapaxes(gc, -1, -2), tol + np.swapaxes(tol, -1, -2))


# ---- a. goldens ---------------------------------------------------------------------------------------------------------
def test_both_entries_match_the_mpmath_goldens():
    E = _E()
    eng = _bare_engine()
    contracted = 0
    for c in T.load_tail_goldens():
        mean, cov = c["mean"][None], c["cov"][None]
        r = T.restate(c)
        cond = T.conditioned_tolerances(r, mean, cov, c["eps"], c["jitter"]) if T.conditioned(c) else None
        got = _call(E, eng, mean, cov, c["eps"], c["eta"], c["jitter"])
        want = dict(value=np.array([c["value"]]), samples=c["samples"][None], counts=c["counts"][None], gcov=c["gcov"][None])
        kind = "golden " + ("near-duplicate pair" if c["base"].endswith("pair") else "cov = 0" if c["base"].endswith("zero") else
                            f"q={c['q']} S={c['S']}")
        _check_against(kind, got, r, want, cond)
        assert got[0][0] > 0.0 and np.any(got[3] != 0.0), c["note"]
        gc = got[3][0]
        for (i, j), diff in c["diffs"].items():     # q <= 4: the 50-digit central differences in every coordinate of cov
            fold = 1.0 if i == j else 2.0
            clipped = i == j and c["cov"][i, i] <= QR.VAR_FLOOR
            tol = fold * (GRAD_TOL * r["gcov_scale"][0, i, j] + (cond[2][0, i, j] if cond else 0.0))
            _check(f"{kind} central differences", gc[i, j] + (gc[j, i] if i != j else 0.0), 0.0 if clipped else diff,
                   0.0 if clipped else tol)
            contracted += 1
    assert contracted == 9 * (1 + 3 + 6) + 3 + 6 + 6


# ---- b. every q in every regime -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", range(1, 65))
def test_every_q_in_every_regime(q):
    E = _E()
    eng = _bare_engine()
    for s in SCALES:
        for t in SHIFTS:
            mean, cov, eps, eta = T.sweep_inputs(q, s, t)
            r = QR.moment_adjoints(mean, cov, eps, eta, JITTER)
            cond = T.conditioned_tolerances(r, mean, cov, eps, JITTER) if s == 1e-4 else None
            got = _call(E, eng, mean, cov, eps, eta, JITTER)
            assert got[0].shape == (T.SWEEP_G,) and got[1].shape == (T.SWEEP_G, T.SWEEP_S, q) and got[3].shape == (T.SWEEP_G, q, q)
            _check_against(f"s={s:g} t={t:+g}", got, r, r, cond)
            assert np.all(got[0] > 0.0)


# ---- c. sample counts -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", T.EDGE_Q)
def test_sample_counts_around_the_wave_width(q):
    E = _E()
    eng = _bare_engine()
    for S in T.EDGE_S:
        mean, cov, eps, eta, jitter = T.edge_inputs(q, S)
        r = QR.moment_adjoints(mean, cov, eps, eta, jitter)
        _check_against(f"S={S}", _call(E, eng, mean, cov, eps, eta, jitter), r, r)


def test_the_largest_sample_count_the_gradient_tail_holds():
    """q = 64 at the largest S of ``qei_value_grad_fits`` (the int per sample fills the LDS to its last word): value and gmean
    against the restatement; S + 2 is refused by both gradient entries with the shape error."""
    E = _E()
    q = 64
    S = T.largest_fitting_draws(q)
    assert E.GPEngine.qei_value_grad_fits(q, S) and not E.GPEngine.qei_value_grad_fits(q, S + 2) and S > 20000
    rng = np.random.default_rng(64)
    mean, cov = T.random_moments(rng, 2, q, 1.0)
    mean, eta = T.same_threshold(mean, cov, 0.0)
    eps = rng.standard_normal((q, S + 2))
    ok, r = T.kinks_are_out_of_reach(mean, cov, eps[:, :S], eta, JITTER)
    assert ok and np.all(r["improving"] > S // 4)
    eng = _bare_engine()
    val, gm, _ = E.qei_moments_grad(eng, mean, cov, np.ascontiguousarray(eps[:, :S]), eta, JITTER)
    np.testing.assert_array_equal(val, E.qei_moments(eng, mean, cov, np.ascontiguousarray(eps[:, :S]), eta, JITTER))
    _check(f"S={S} value", val, r["value"], VAL_TOL * r["value_scale"])
    _check_gmean(f"S={S}", gm, r["counts"], S)
    with pytest.raises(ValueError, match="LDS"):
        E.qei_moments_grad(eng, mean, cov, eps, eta, JITTER)
    model = _small_model()
    with pytest.raises(ValueError, match="LDS"):
        model.qei_value_grad(rng.uniform(size=(2, q, 2)), eps, eta, JITTER)
    assert E.qei_moments(eng, mean, cov, eps, eta, JITTER).shape == (2,)      # the value entry takes any S


# ---- d. degenerate batches ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", T.DEGENERATE_Q)
def test_duplicate_point(q):
    E = _E()
    mean, cov, eps, eta, jitter = T.duplicate_inputs(q)
    r = QR.moment_adjoints(mean, cov, eps, eta, jitter)
    got = _call(E, _bare_engine(), mean, cov, eps, eta, jitter)
    _check_against("duplicate point", got, r, r, T.conditioned_tolerances(r, mean, cov, eps, jitter))
    assert np.any(got[3][:, 1, 1] != 0.0)


@pytest.mark.parametrize("q", T.DEGENERATE_Q)
def test_zero_covariance(q):
    E = _E()
    mean, cov, eps, eta, jitter = T.zero_cov_inputs(q)
    r = QR.moment_adjoints(mean, cov, eps, eta, jitter)
    got = _call(E, _bare_engine(), mean, cov, eps, eta, jitter)
    want = mean[:, None, :] + np.sqrt(jitter) * eps.T[None]
    _check("cov = 0 samples", got[1], want, 2.0 * np.spacing(np.abs(want)))
    d = np.arange(q)
    assert np.all(got[3][:, d, d] == 0.0) and np.any(r["gcov"] != 0.0) == (q > 1)
    unclipped = QR.moment_adjoints(mean, cov, eps, eta, jitter, clip=False)["gcov"]
    assert np.count_nonzero(unclipped[:, d, d]) >= min(q, 8)        # (the clip is what makes them zero)
    _check_against("cov = 0", got, r, r, T.conditioned_tolerances(r, mean, cov, eps, jitter))


@pytest.mark.parametrize("q", T.DEGENERATE_Q)
def test_diagonal_at_the_clip_and_next_to_it(q):
    E = _E()
    mean, cov, eps, eta, jitter = T.mixed_clip_inputs(q)
    assert np.all(cov[:, 0, 0] == 1e-12) and np.all(cov[:, 1, 1] == np.nextafter(1e-12, 1.0))
    r = QR.moment_adjoints(mean, cov, eps, eta, jitter)
    got = _call(E, _bare_engine(), mean, cov, eps, eta, jitter)
    assert np.all(got[3][:, 0, 0] == 0.0) and np.all(got[3][:, 1, 1] != 0.0)
    _check_against("mixed clip", got, r, r, T.conditioned_tolerances(r, mean, cov, eps, jitter))


class _GivenMoments:
    """Stands in for the engine behind ``batch_monte_carlo_expected_improvement.value_and_gradient``'s HOST adjoint path
    (``qei_value_grad_fits`` False): hands out given moments and keeps the adjoints the host computed."""
    JOINT_SMALL_POINTS = 2048
    qei_value_grad_fits = staticmethod(lambda q, S: False)

    def __init__(self, mean, cov):
        self.mean, self.cov = mean, cov

    def qei_value_grad(self, *a):
        raise AssertionError("the device path")

    def joint_forward(self, xs):
        return self.mean, self.cov

    def joint_vjp(self, xs, gmean, gcov):
        self.gmean, self.gcov = np.array(gmean), np.array(gcov)
        return np.zeros(xs.shape)


def _host_adjoints(mean, cov, eps, eta, jitter):
    from trieste_amd.acquisition.function import batch_monte_carlo_expected_improvement

    class _Sampler:
        def eps(self, q):
            return eps

    stub = _GivenMoments(mean, cov)
    fn = batch_monte_carlo_expected_improvement.__new__(batch_monte_carlo_expected_improvement)
    fn._engine, fn._sampler, fn._eta, fn._jitter, fn._sample_size = stub, _Sampler(), eta, jitter, eps.shape[1]
    val, _ = fn.value_and_gradient(np.zeros(mean.shape + (2,)))
    return val, stub.gmean, stub.gcov


@pytest.mark.parametrize("q", T.DEGENERATE_Q)
def test_exact_tie_goes_to_the_first_index(q):
    """cov = 0, mean_0 = mean_1 the smallest, eps[0] = eps[1]: the samples of points 0 and 1 are the same bits in every draw;
    the whole count goes to index 0 -- on the device and in the host adjoint path of the acquisition function alike."""
    E = _E()
    rng = np.random.default_rng(600 + q)
    S, G = 33, 3
    eps = rng.standard_normal((q, S))
    eps[1] = eps[0]
    mean = 5.0 + rng.uniform(1.0, 2.0, size=(G, q))       # the others are 1000 sqrt(jitter) above: points 0 / 1 always win
    mean[:, 0] = mean[:, 1] = 5.0
    cov = np.zeros((G, q, q))
    eta = 5.0 + 1e-4
    val, sam, gm, gc = _call(E, _bare_engine(), mean, cov, eps, eta, JITTER)
    np.testing.assert_array_equal(sam[:, :, 0], sam[:, :, 1])
    r = QR.moment_adjoints(mean, cov, eps, eta, JITTER)
    n = r["improving"]
    assert np.all(n >= S // 4) and np.all(r["counts"][:, 0] == n) and not np.any(r["counts"][:, 1:])
    assert np.abs(eta - r["samples"].min(axis=2)).min() > T._sample_atol(mean, cov, eps, JITTER)   # (the tie is the only kink in reach)
    _check_gmean("tie", gm, r["counts"], S)
    assert np.all(gm[:, 0] < 0.0) and not np.any(gm[:, 1:])
    hval, hgm, hgc = _host_adjoints(mean, cov, eps, eta, JITTER)
    _check_gmean("tie (host adjoint path)", hgm, r["counts"], S)
    _check("tie value (host adjoint path)", hval, val, VAL_TOL * r["value_scale"])
    cond = T.conditioned_tolerances(r, mean, cov, eps, JITTER)
    _check("tie gcov (host adjoint path)", hgc, gc, 2.0 * GRAD_TOL * r["gcov_scale"] + cond[2])


@pytest.mark.parametrize("q", T.DEGENERATE_Q)
def test_improvement_of_exactly_zero_does_not_count(q):
    E = _E()
    rng = np.random.default_rng(700 + q)
    S, G = 33, 3
    mean = 5.0 + 1e-3 * rng.standard_normal((G, q))
    eta = float(mean.min() - 1e-4)
    mean[:, q - 1] = eta                                    # the last point holds the smallest mean, eta, in every group
    cov = np.zeros((G, q, q))
    # every draw zero or upwards: no draw improves, draw 7 sits at eta exactly
    eps = np.abs(rng.standard_normal((q, S)))
    eps[:, 7] = 0.0
    val, sam, gm, gc = _call(E, _bare_engine(), mean, cov, eps, eta, JITTER)
    np.testing.assert_array_equal(sam[:, 7, :], mean)
    assert not np.any(val) and not np.any(gm) and not np.any(gc)
    # ordinary draws around it: draw 7 still counts nowhere
    eps = rng.standard_normal((q, S))
    eps[:, 7] = 0.0
    keep = np.arange(S) != 7
    ok, r = T.kinks_are_out_of_reach(mean, cov, np.ascontiguousarray(eps[:, keep]), eta, JITTER)
    assert ok and np.all(r["improving"] >= 4)
    got = _call(E, _bare_engine(), mean, cov, eps, eta, JITTER)
    full = QR.moment_adjoints(mean, cov, eps, eta, JITTER)
    np.testing.assert_array_equal(full["counts"], r["counts"])
    np.testing.assert_array_equal(got[1][:, 7, :], mean)
    _check_against("zero improvement", got, full, full, T.conditioned_tolerances(full, mean, cov, eps, JITTER))


@pytest.mark.parametrize("q", T.DEGENERATE_Q)
def test_an_exactly_singular_group_is_reported_and_leaves_no_trace(q):
    """jitter = 0, group 5 of 9 with a duplicate row of powers of two (the second pivot is 0.25 - 0.5^2 = 0.0 exactly): both
    entries return TGP_ERR_NOT_PD naming group 5 -- the documented error return, the kernel goes on with pivot 1 -- and the next
    call on the same handle returns the bits of a fresh handle."""
    E = _E()
    from trieste_amd._lib import NotPositiveDefiniteError

    rng = np.random.default_rng(800 + q)
    G, S = 9, 40
    eps = rng.standard_normal((q, S))
    mean, cov = T.random_moments(rng, G, q, 1.0)
    mean, eta = T.same_threshold(mean, cov, 0.0)
    bad = cov.copy()
    bad[5] = 0.5 * np.eye(q)
    bad[5, :2, :2] = 0.25
    eng = _bare_engine()
    with pytest.raises(NotPositiveDefiniteError, match="group 5"):
        E.qei_moments(eng, mean, bad, eps, eta, 0.0)
    with pytest.raises(NotPositiveDefiniteError, match="group 5"):
        E.qei_moments_grad(eng, mean, bad, eps, eta, 0.0)
    after = _call(E, eng, mean, cov, eps, eta, 0.0)
    fresh = _call(E, _bare_engine(), mean, cov, eps, eta, 0.0)
    for a, b in zip(after, fresh):
        np.testing.assert_array_equal(a, b)
    r = QR.moment_adjoints(mean, cov, eps, eta, 0.0)
    assert np.all(r["kink_distance"] > T._sample_atol(mean, cov, eps, 0.0))
    _check_against("jitter = 0", after, r, r)


# ---- e. the model entries are the same kernels ----------------------------------------------------------------------------
def _small_model(N=64, d=2):
    from oracle import gp_oracle as O

    X, Y = O.synthetic_problem(O.branin, d, N)
    eng = _bare_engine(d)
    eng.set_hyper(1.0, O.default_lengthscales(d), 1e-3, 0.0)
    eng.set_data(X, Y)
    return eng


@pytest.mark.parametrize("q", [1, 9, 64])
def test_model_entries_run_the_same_kernels(q):
    """``qei`` / ``reparam_samples`` are ``qei_moments`` on ``predict_joint``'s arrays, ``qei_value_grad`` is ``qei_moments_grad``
    on ``joint_forward``'s arrays with ``joint_vjp`` behind it: BIT FOR BIT (the composed call runs the same kernels in the same
    order on the same arrays; no summation order differs).  Host- and device-resident inputs and a repeated call likewise."""
    import torch

    E = _E()
    eng = _small_model()
    rng = np.random.default_rng(900 + q)
    G, S, d = 4, 70, 2
    Xq = rng.uniform(size=(G, q, d))
    eps = rng.standard_normal((q, S))
    pm, pc = eng.predict_joint(Xq)
    eta = float(np.median(pm.min(axis=1)))
    val, sam = E.qei_moments(eng, pm, pc, eps, eta, JITTER, samples=True)
    assert np.count_nonzero(val) >= G // 2
    np.testing.assert_array_equal(val, eng.qei(Xq, eps, eta, JITTER))
    np.testing.assert_array_equal(sam, eng.reparam_samples(Xq, eps, JITTER))
    fm, fc = eng.joint_forward(Xq)
    gval, gm, gc = E.qei_moments_grad(eng, fm, fc, eps, eta, JITTER)
    mval, mgrad = eng.qei_value_grad(Xq, eps, eta, JITTER)
    np.testing.assert_array_equal(gval, mval)
    np.testing.assert_array_equal(eng.joint_vjp(Xq, gm, gc), mgrad)
    assert np.any(mgrad != 0.0)
    # residency and repetition
    dev = [torch.as_tensor(a).to("cuda:0") for a in (fm, fc, eps)]
    dval, dsam = E.qei_moments(eng, *dev, eta, JITTER, samples=True)
    hval, hsam = E.qei_moments(eng, fm, fc, eps, eta, JITTER, samples=True)
    np.testing.assert_array_equal(dval.cpu().numpy(), hval)
    np.testing.assert_array_equal(dsam.cpu().numpy(), hsam)
    for a, b in zip(E.qei_moments_grad(eng, *dev, eta, JITTER), (gval, gm, gc)):
        np.testing.assert_array_equal(a.cpu().numpy(), b)
    for a, b in zip(E.qei_moments_grad(eng, fm, fc, eps, eta, JITTER), (gval, gm, gc)):
        np.testing.assert_array_equal(a, b)


def test_argument_checks_of_the_two_entries():
    E = _E()
    L = E._lib
    lib = L.load()
    eng = _bare_engine()
    rng = np.random.default_rng(5)
    G, q, S = 3, 4, 10
    mean, cov = T.random_moments(rng, G, q, 1.0)
    eps = rng.standard_normal((q, S))
    out, gm, gc = np.empty(G), np.empty((G, q)), np.empty((G, q, q))
    p = lambda a: a.ctypes.data  # noqa: E731

    def value_rc(q_=q, S_=S, jitter=1e-6, G_=G, out_=out):
        return lib.tgp_qei_moments(eng._h, p(mean), p(cov), G_, q_, p(eps), S_, 0.0, jitter, None if out_ is None else p(out_),
                                   None, L.HOST)

    def grad_rc(q_=q, S_=S, jitter=1e-6, G_=G, out_=out):
        return lib.tgp_qei_moments_grad(eng._h, p(mean), p(cov), G_, q_, p(eps), S_, 0.0, jitter, None if out_ is None else p(out_),
                                        p(gm), p(gc), L.HOST)

    for call in (value_rc, grad_rc):
        for kwargs, code in ((dict(q_=0), L.TGP_ERR_SHAPE), (dict(q_=65), L.TGP_ERR_SHAPE), (dict(S_=0), L.TGP_ERR_ARG),
                             (dict(jitter=-1e-9), L.TGP_ERR_ARG), (dict(out_=None), L.TGP_ERR_ARG), (dict(G_=-1), L.TGP_ERR_ARG)):
            assert call(**kwargs) == code and lib.tgp_last_error(eng._h).decode().strip(), kwargs
        assert call(G_=0) == L.TGP_OK and call() == L.TGP_OK
    with pytest.raises(ValueError):
        E.qei_moments(eng, mean, cov[:, :, :2], eps, 0.0)
    with pytest.raises(ValueError):
        E.qei_moments_grad(eng, mean, cov, eps[:2], 0.0)
