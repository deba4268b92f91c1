"""The gradient kernels at their OWN resolution: tgp_nlml's gradient (Kinv = W^T W, nlml_grad_kernel / nlml_grad_wide_kernel,
nlml_final*_kernel), tgp_acq_value_grad (grad_partial_kernel / grad_partial_wide_kernel, grad_finish_kernel) and
tgp_joint_forward / tgp_joint_vjp (joint_mix_kernel, the tall products, joint_vjp_finish_kernel, joint_pick_kernel) against
long-double references built FROM THE ENGINE'S OWN W and alpha (get_factor), judged by the counted bounds of
tests/grad_resolution.py.  tests/test_gpu_factor_resolution.py judges W and alpha themselves; the parity suites compare these
paths at rtol 1e-5 plus a cancellation floor, which a dropped slice partial, a pair tile weighted once or a one-triangle Gs passes
(tests/test_grad_resolution.py plants them).

Cases: the four (kind, noise) pairs x N in {17, 130, 256, 257, 386} at d = 4 (both paddings, slices of 16 and 32 rows, a slice
holding one row, empty slices, one to seven pair tiles per side), one d = 13 design (the DP = 16 instantiation) and one d = 40
design (the wide kernels, two chunks).  Every miss of a test is collected before it fails; every margin is recorded
(tests/util.py record_margin) under "<form> <path>", so the parity-margins table of a run holds one summary line per path and form.

Observed worst error / tolerance on an MI355X (the parity-margins table of the run that added this file), beside the float64
restatement's ratio under the same bound (tests/test_grad_resolution.py: the reference factor's W and alpha):
    path                                     narrow (d = 4)     DP = 16 (d = 13)   wide (d = 40)      device / restatement
    nlml gradient                            0.024  / 0.028     0.015  / 0.010     0.0081 / 0.0053
    mean value (beta = 0)                    0.035  / 0.044     0.0088 / 0.011     0.0067 / 0.0068
    mean gradient (beta = 0)                 0.061  / 0.063     0.018  / 0.021     0.014  / 0.014
    nlcb value (beta = 2: variance)          0.053  / 0.035     0.024  / 0.015     0.043  / 0.081
    nlcb gradient (beta = 2: variance chain) 0.022  / 0.028     0.0023 / 0.0029    0.0025 / 0.0024
    joint mean                               0.035  / 0.044     0.0088 / 0.011     0.0067 / 0.0068
    joint cov                                0.093  / 0.087     0.027  / 0.047     0.042  / 0.054
    joint vjp                                0.035  / 0.045     0.0042 / 0.017     0.0085 / 0.0098
    joint vjp (strictly upper gcov)          0.052  / 0.045     0.015  / 0.017     0.011  / 0.0098
The variance gradient -2 sum_k Z_k dk_k/dx is no output of its own: it is judged through the beta = 2 gradient, whose tolerance
is tol_dmean + tol_dvar / sd (the restatement's variance gradient alone uses 0.029 / 0.0022 / 0.0008 of tol_dvar).  The device
stays within a tenth of every bound, at the restatement's level: the first run found nothing to fix."""
import functools

import numpy as np
import pytest

from tests import factor_resolution as F
from tests import grad_resolution as R

pytestmark = pytest.mark.gpu

CASE_IDS = [f"{k}-{s:g}-N{N}-d{d}" for k, s, N, d in R.CASES]


def _form(d):
    return "narrow" if d == F.D else "dp16" if d <= 16 else "wide"


@functools.lru_cache(maxsize=None)
def _case(kind, noise, N, d):
    """(engine, X, lengthscales, query points, W, alpha) of a case: one engine and one read of the factor per case."""
    from trieste_amd.engine import GPEngine

    X, Y, ls, Xq = R.design(N, d)
    eng = GPEngine(d, kind)
    eng.set_hyper(F.VARIANCE, ls, noise, F.MEAN)
    eng.set_data(np.ascontiguousarray(X), np.ascontiguousarray(Y))
    _, W, alpha = eng.get_factor()
    assert np.array_equal(np.triu(W, 1), np.zeros_like(W)), "W is not exactly lower triangular"
    return eng, X, ls, Xq, W, alpha


@functools.lru_cache(maxsize=4)
def _value_reference(kind, noise, N, d, beta):
    _, X, ls, Xq, W, alpha = _case(kind, noise, N, d)
    return R.value_gradient(kind, F.VARIANCE, ls, F.MEAN, X, W, alpha, Xq[:64], beta)


class Misses:
    def __init__(self, tag, form, N):
        self.tag, self.form, self.N, self.bad = tag, form, N, []

    def compare(self, path, got, ref, tol, weight, mask=None, detail=""):
        bad = []
        R.compare(f"{self.form} {path}", got, ref, tol, weight, self.N, bad, mask)
        self.bad += [f"{self.tag} {detail}: {b}" for b in bad]

    def require(self, cond, msg):
        if not cond:
            self.bad.append(f"{self.tag}: {msg}")

    def done(self):
        assert not self.bad, "\n".join(self.bad)


@pytest.mark.parametrize("kind,noise,N,d", R.CASES, ids=CASE_IDS)
def test_nlml_gradient(kind, noise, N, d):
    eng, X, ls, _, W, alpha = _case(kind, noise, N, d)
    m = Misses(f"{kind} {noise:g} N={N} d={d}", _form(d), N)
    value, grad = eng.nlml()
    m.require(value == eng.nlml(False)[0], "the value-only call returns other bits")
    ref, tol, wgt = R.nlml_gradient(kind, F.VARIANCE, ls, noise, X, W, alpha)
    m.compare("nlml gradient", grad, ref, tol, wgt)
    m.done()


@pytest.mark.parametrize("beta", [0.0, 2.0])
@pytest.mark.parametrize("kind,noise,N,d", R.CASES, ids=CASE_IDS)
def test_acq_value_grad(kind, noise, N, d, beta):
    eng, _, _, Xq, _, _ = _case(kind, noise, N, d)
    m = Misses(f"{kind} {noise:g} N={N} d={d} beta={beta:g}", _form(d), N)
    vg = _value_reference(kind, noise, N, d, beta)
    m.require(beta != 0.0 or vg["ok"].all(), "the beta = 0 comparison leaves a point out")
    full = None
    for P in reversed(R.P_SIZES):
        v, g = (np.array(a) for a in eng.acq_value_grad("nlcb", beta, np.ascontiguousarray(Xq[:P])))
        if full is None:
            full = (v, g)
        m.require(np.array_equal(v, full[0][:P]) and np.array_equal(g, full[1][:P]),
                  f"P={P}: other bits than the first {P} results of the call with {R.P_SIZES[-1]} points")
        ok = vg["ok"][:P]
        name = "mean" if beta == 0.0 else "nlcb"
        m.compare(f"{name} value", v, vg["v"][:P], vg["tol_v"][:P], vg["w_v"][:P], ok, f"P={P}")
        m.compare(f"{name} gradient", g, vg["g"][:P], vg["tol_g"][:P], vg["w_g"][:P], ok, f"P={P}")
    m.done()


@pytest.mark.parametrize("q,G", R.GROUPS)
@pytest.mark.parametrize("kind,noise,N,d", R.CASES, ids=CASE_IDS)
def test_joint_forward_and_vjp(kind, noise, N, d, q, G):
    eng, X, ls, Xq, W, alpha = _case(kind, noise, N, d)
    m = Misses(f"{kind} {noise:g} N={N} d={d} q={q} G={G}", _form(d), N)
    Xg = np.ascontiguousarray(Xq[:q * G].reshape(G, q, d))
    mean, cov = (np.array(a) for a in eng.joint_forward(Xg))
    m.require(np.array_equal(cov, np.swapaxes(cov, 1, 2)), "cov is not exactly symmetric")
    for upper in (False, True):
        gm, gc = R.adjoints(q, G, upper)
        J = R.joint(kind, F.VARIANCE, ls, F.MEAN, X, W, alpha, Xg, gm, gc)
        if not upper:
            m.compare("joint mean", mean, J["mean"], J["tol_mean"], J["w_mean"])
            m.compare("joint cov", cov, J["cov"], J["tol_cov"], J["w_cov"])
        vjp = np.array(eng.joint_vjp(Xg, np.ascontiguousarray(gm), np.ascontiguousarray(gc)))
        m.compare("joint vjp" + (" (upper gcov)" if upper else ""), vjp, J["vjp"], J["tol_vjp"], J["w_vjp"])
    m.done()
