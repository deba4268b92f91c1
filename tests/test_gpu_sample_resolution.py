"""tgp_sample_joint (GPEngine.sample_joint) at its own resolution: the factor of cov + jitter I READ from the entry (a model with
Y = 0 and mean 0, eps = I_n), its residual L L^T - A_ref in long double under the bound of tests/sample_resolution.py, the draws
against the factor just read, the breakdown report at jitter 0 and the refusals.  The factorisation runs chol_inv at the padded sizes
64, 128, 192, 320, 640, which `update` (padded to 256) never factorises.

Worst ratios on the MI355X (printed per case; the margin table has every one):
  residual / bound: 0.014 (matern52, noise 1e-2), 0.024 (matern52, 1e-5), 0.006 (rbf, 1e-2), 0.026 (rbf, 1e-5) over n = 1 .. 577 at
    jitter 1e-6; 0.024 at jitter 1e-10 (n = 129); 0.052 at d = 40 (n = 70);
  draws / tolerance: at most 0.48 (matern52, 1e-5, n = 320, S = 64); 0.22 at d = 40.
  The three duplicate-pair sets at jitter 0 factorised (pivot 4e-9 .. 8e-9 at the duplicate; leading block 0.003 .. 0.005 of the
  bound); of the open sets the triplicate across the 64 boundary was reported not positive definite at point 64."""
import numpy as np
import pytest

from tests import factor_resolution as F
from tests import sample_resolution as R

pytestmark = pytest.mark.gpu

_ENGINES, _TOL, _FACTORS = {}, {}, {}


def _engine(name, zero=False, data=True):
    from trieste_amd.engine import GPEngine

    m = R.model(name)
    eng = GPEngine(m.d, m.kind)
    eng.set_hyper(m.variance, m.ls, m.noise, 0.0 if zero else m.mean)
    if data:
        eng.set_data(np.ascontiguousarray(m.X), np.zeros(m.N) if zero else np.ascontiguousarray(m.Y))
    return eng


def _engines(name):
    """(the model's engine, the same X and hyper-parameters with Y = 0 and mean 0)."""
    if name not in _ENGINES:
        _ENGINES[name] = (_engine(name), _engine(name, zero=True))
    return _ENGINES[name]


def _tol_cov(name, jitter):
    """Term (b) from the residuals of THIS engine's `update` arrays."""
    if (name, jitter) not in _TOL:
        eng, eng0 = _engines(name)
        L, W, alpha = eng.get_factor()
        L0, W0, alpha0 = eng0.get_factor()
        assert np.array_equal(L, L0) and np.array_equal(W, W0) and not alpha0.any(), "the Y = 0 model has another factor, or alpha != 0"
        _TOL[name, jitter] = R.covariance_tolerance(R.reference(name), R.measured(name, L, W, alpha), jitter)
        R.assert_finer_than_the_floor(name, _TOL[name, jitter])
    return _TOL[name, jitter]


def _read_factor(name, n, jitter):
    """L of cov(Xq[:n]) + jitter I: out[s, j] = L[j, s] for eps = I_n on the Y = 0 model."""
    if (name, n, jitter) not in _FACTORS:
        eng0 = _engines(name)[1]
        Xq = R.query_points(name)[:n]
        assert not eng0.predict_mean(Xq).any(), "the posterior mean of the Y = 0 model is not exactly 0"
        out = eng0.sample_joint(Xq, np.eye(n), jitter)
        assert out.shape == (n, n)
        _FACTORS[name, n, jitter] = np.ascontiguousarray(out.T)
    return _FACTORS[name, n, jitter]


FACTOR_CASES = [(name, n, R.JITTER) for name in R.MODELS[:4] for n in R.SIZES]
FACTOR_CASES += [("matern52@1e-05", 129, R.LOW_JITTER), (R.WIDE, 70, R.JITTER)]


@pytest.mark.parametrize("name,n,jitter", FACTOR_CASES)
def test_factor_read_from_the_entry(name, n, jitter):
    """Exactly lower triangular with a positive diagonal; zero draws return predict_mean bit for bit; the residual under the bound."""
    eng = _engines(name)[0]
    Xq = R.query_points(name)[:n]
    L = _read_factor(name, n, jitter)
    assert np.array_equal(eng.sample_joint(Xq, np.zeros((n, 1)), jitter), eng.predict_mean(Xq)[None, :])
    r = R.factor_checks(f"{name} jitter {jitter:g} n={n}", L, R.reference(name).A(n, jitter), _tol_cov(name, jitter))
    print(f"{name} jitter {jitter:g} n={n}: residual / bound {r:.3g}")


DRAW_CASES = [(name, n, S) for name in R.MODELS[:4] for n, S in R.DRAW_PAIRS] + [(R.WIDE, 70, 65)]


@pytest.mark.parametrize("name,n,S", DRAW_CASES)
def test_draws_against_the_factor_just_read(name, n, S):
    """out [S, n] = predict_mean + L eps in long double, ragged n against ragged S."""
    eng = _engines(name)[0]
    Xq, eps = R.query_points(name)[:n], R.draws(n, S)
    out = eng.sample_joint(Xq, eps, R.JITTER)
    r = R.draw_checks(f"{name} n={n} S={S}", out, _read_factor(name, n, R.JITTER), eps, eng.predict_mean(Xq))
    print(f"{name} n={n} S={S}: draws / tolerance {r:.3g}")


def test_device_resident_inputs_return_the_same_bits():
    """n = 129, S = 65 (no multiple of 64): CUDA tensors in, a CUDA tensor out, equal to the host call bit for bit."""
    import torch

    name, n, S = "matern52@0.01", 129, 65
    eng = _engines(name)[0]
    Xq, eps = R.query_points(name)[:n], R.draws(n, S)
    dev = eng.sample_joint(torch.from_numpy(np.array(Xq)).cuda(), torch.from_numpy(eps).cuda(), R.JITTER)
    assert isinstance(dev, torch.Tensor) and dev.is_cuda and tuple(dev.shape) == (S, n)
    assert np.array_equal(dev.cpu().numpy(), eng.sample_joint(Xq, eps, R.JITTER))


# ---- breakdown ------------------------------------------------------------------------------------------------------------------
def _attempt(eng, Xq, n):
    """sample_joint(Xq, I, jitter 0): (out, None) or (None, the index the error names, checked to be a point of the set)."""
    from trieste_amd._lib import NotPositiveDefiniteError

    try:
        return eng.sample_joint(Xq, np.eye(n), 0.0), None
    except NotPositiveDefiniteError as e:
        assert str(e)
        i = R.pd_index(str(e))
        assert 0 <= i < n, str(e)
        return None, i


@pytest.mark.parametrize("n,a,b", R.BREAKDOWN_PAIRS)
def test_breakdown_at_an_exact_duplicate(n, a, b):
    """jitter 0, rows a < b of A identical, the leading b x b block positive definite with pivots above 1e-6
    (tests/test_sample_resolution.py): the exact pivot b is 0 and rounding decides.  Either the error names a point in [b, n), or the
    call succeeds and the leading b x b block of the factor obeys the residual bound."""
    name = "matern52@0.01"
    Xq = R.duplicate_pair_set(n, a, b)
    ref = R.Reference(name, Xq)
    assert (np.diag(F.chol_ld(ref.A(n, 0.0)[:b, :b])) ** 2).min() > 1e-6
    eng, eng0 = _engines(name)
    out, i = _attempt(eng0, Xq, n)
    if out is None:
        print(f"n={n} a={a} b={b}: not positive definite at point {i}")
        assert b <= i < n, i
    else:
        tol = R.covariance_tolerance(ref, R.measured(name, *eng.get_factor()), 0.0)
        r = R.factor_checks(f"duplicate pair n={n} b={b}", np.ascontiguousarray(out.T[:b, :b]), ref.A(b, 0.0), tol)
        print(f"n={n} a={a} b={b}: factorised (pivot {out[b, b]:.3g} at the duplicate); leading block residual / bound {r:.3g}")


@pytest.mark.parametrize("which", range(3))
def test_a_handle_answers_as_a_fresh_one_after_a_breakdown(which):
    """Triplicated points and copies of training inputs at jitter 0 -- the outcome is rounding's; an error names a point of the set,
    and the next jitter-1e-6 call on the same handle returns the bits of a fresh handle."""
    name, Xq = R.open_breakdown_set(which)
    n = Xq.shape[0]
    eng = _engine(name)
    out, i = _attempt(eng, Xq, n)
    print(f"open set {which}: " + ("factorised" if out is not None else f"not positive definite at point {i}"))
    Xn, eps = R.query_points(name)[:129], R.draws(129, 65)
    assert np.array_equal(eng.sample_joint(Xn, eps, R.JITTER), _engine(name).sample_joint(Xn, eps, R.JITTER))


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_next_call_unaffected():
    import torch

    name = "rbf@0.01"
    eng = _engine(name)
    m = R.model(name)
    Xq, eps = R.query_points(name)[:65], R.draws(65, 63)
    want = eng.sample_joint(Xq, eps, R.JITTER)
    refused = {
        "negative jitter": lambda: eng.sample_joint(Xq, eps, -1e-6),
        "NaN jitter": lambda: eng.sample_joint(Xq, eps, float("nan")),
        "S = 0": lambda: eng.sample_joint(Xq, np.zeros((65, 0)), R.JITTER),
        "n = 0": lambda: eng.sample_joint(np.zeros((0, m.d)), np.zeros((0, 3)), R.JITTER),
        "eps of another leading size": lambda: eng.sample_joint(Xq, eps[:64], R.JITTER),
        "host Xq, device eps": lambda: eng.sample_joint(Xq, torch.from_numpy(eps).cuda(), R.JITTER),
        "no data": lambda: _engine(name, data=False).sample_joint(Xq, eps, R.JITTER),
    }
    for what, call in refused.items():
        with pytest.raises((ValueError, RuntimeError)) as info:
            call()
        assert str(info.value), what
        assert np.array_equal(eng.sample_joint(Xq, eps, R.JITTER), want), f"after {what}"
