"""The engine's own scalar math -- fast_sqrt_pos, fast_exp_nonpos, traj_sqrt, traj_exp2, traj_shape, kernel_from_r2,
kernel_rt, kernel_dr2 (csrc/tgp_dev.hpp) -- at ulp resolution, read through the public C-ABI.

The parity suites compare at 1e-5 relative plus an absolute floor; a wrong low-order coefficient, a lost Goldschmidt step
or a kernel value wrong by 1e-7 anywhere passes them.  Here the inputs are chosen so that the posterior mean IS one kernel
value (or a short positive sum of them) with no rounding in between, and the reference is mpmath on the exact doubles of
the probes (tests/golden/kernel_resolution_goldens.json, written by tests/make_kernel_resolution_goldens.py).

The exact design: N = 1, d = 3, lengthscales [0.5, 0.25, 2.0], variance 1, noise 3, mean 0, X0 = [0.25, 0.5, 0.75],
Y = 4.  K + noise = 4, L = 2, W = 1/2, alpha = 1 without rounding, so mean(x) = k(x, X0) and the gradient of
acq("nlcb", 0) is -dk/dx.  The lengthscales are powers of two: x / ls is exact.

Tolerance: |got - ref| <= eps (A + B s) |ref| with A and B per kind and path counted from the code path in
tests/kernel_resolution.py; the dense sum adds 17 eps for the summation.

Underflow probes (s = 760, 1e4, 1e8) assert only 0 <= value <= 1e-300 and finite.  The int8 precisions quantise K* by
design and are out of scope (tests/test_gpu_i8.py)."""
import functools
import json
import os

import numpy as np
import pytest

from tests.kernel_resolution import A_COEF, A_GRAD, B_DIFF, B_TRAJ, KINDS, nlcb2_tolerances
from tests.util import EPS, record_margin

pytestmark = pytest.mark.gpu

M_SMALL, M_LARGE = 288, 2100


@functools.lru_cache(maxsize=None)
def _goldens():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_resolution_goldens.json")) as f:
        return json.load(f)


class Probes:
    """Probe points tiled to M rows with their references; ``under`` marks the underflow probes."""

    def __init__(self, block, under_x, M):
        x = np.array(block["x"] + list(under_x))
        n, nu = len(block["x"]), len(under_x)
        idx = np.resize(np.arange(n + nu), M)
        self.x = np.ascontiguousarray(x[idx])
        self.under = idx >= n
        pad = lambda a, fill: np.concatenate([np.asarray(a, dtype=np.float64), fill])[idx]
        self.k = pad(block["k"], np.zeros(nu))
        self.s = pad(block["s"], np.zeros(nu))
        self.dk = pad(block["dk"], np.zeros((nu, 3)))


class Checker:
    """Collects every comparison of one test, so that one run shows every path that misses its bound."""

    def __init__(self, kind, B):
        self.kind, self.base, self.B, self.bad = kind, kind, B, []

    def values(self, what, got, p, extra=0.0, tol=None):
        got = np.asarray(got, dtype=np.float64).reshape(-1)
        assert got.shape == p.k.shape, (what, got.shape)
        if not np.all(np.isfinite(got)):
            self.bad.append(f"{what}: non-finite values")
            return
        u = p.under
        if np.any(u) and not np.all((got[u] >= 0.0) & (got[u] <= 1e-300)):
            self.bad.append(f"{what}: underflow probes give {got[u][:3]}")
        n = ~u
        tol = EPS * (A_COEF[self.base] + extra + self.B * p.s[n]) * np.abs(p.k[n]) if tol is None else tol[n]
        err = np.abs(got[n] - p.k[n])
        worst = record_margin(f"{self.kind} {what}", err, tol)
        if not np.all(err <= tol):
            i = int(np.argmax(err / tol))
            self.bad.append(f"{what}: worst/tol {worst:.3g} at s={p.s[n][i]:.4g}: got {got[n][i]!r} ref {p.k[n][i]!r}")

    def gradients(self, what, got, p, sign=1.0):
        got = sign * np.asarray(got, dtype=np.float64).reshape(-1, p.dk.shape[1])
        n = ~p.under
        if not np.all(np.isfinite(got)):
            self.bad.append(f"{what}: non-finite gradients")
            return
        if not np.all(np.abs(got[p.under]) <= 1e-290):
            self.bad.append(f"{what}: gradient at the underflow probes {got[p.under][:2]}")
        ref = p.dk[n]
        tol = (EPS * (A_GRAD[self.base] + self.B * p.s[n]) * np.abs(ref).max(axis=1))[:, None] * np.ones_like(ref)
        err = np.abs(got[n] - ref)
        worst = record_margin(f"{self.kind} {what}", err, tol)
        if not np.all(err <= tol):
            i = int(np.argmax((err / np.where(tol > 0, tol, 1e-320)).max(axis=1)))
            self.bad.append(f"{what}: worst/tol {worst:.3g} at s={p.s[n][i]:.4g}: got {got[n][i]} ref {ref[i]}")

    def nlcb2(self, what, val, grad, p):
        """The variance chain: value and gradient of -LCB at beta = 2 against the closed form of the exact one-point design
        (tests/kernel_resolution.py nlcb2_tolerances); at the underflow probes k = dk = 0: v = 2 sd = 2, g = 0."""
        val, grad = np.asarray(val, dtype=np.float64).reshape(-1), np.asarray(grad, dtype=np.float64).reshape(len(p.k), -1)
        if not (np.all(np.isfinite(val)) and np.all(np.isfinite(grad))):
            self.bad.append(f"{what}: non-finite values")
            return
        if not np.all(grad[:, 3:] == 0.0):
            self.bad.append(f"{what}: gradient along coordinates that do not differ")
        if not np.all(np.abs(grad[p.under]) <= 1e-290):
            self.bad.append(f"{what}: gradient at the underflow probes {grad[p.under][:2]}")
        v, g, tol_v, tol_g = nlcb2_tolerances(self.base, self.B, p.k, p.s, p.dk)
        for name, got, ref, tol, rows in (("value", val, v, tol_v, np.ones_like(p.under)), ("gradient", grad[:, :3], g, tol_g, ~p.under)):
            got, ref, tol, s = got[rows], ref[rows], tol[rows], p.s[rows]
            err = np.abs(np.asarray(got - ref, dtype=np.float64))
            worst = record_margin(f"{self.kind} {what} {name}", err, tol)
            if not np.all(err <= tol):
                i = int(np.argmax((err / np.where(tol > 0, tol, 1e-320)).reshape(len(s), -1).max(axis=1)))
                self.bad.append(f"{what} {name}: worst/tol {worst:.3g} at s={s[i]:.4g}: got {got[i]} ref {np.asarray(ref[i], dtype=np.float64)}")

    def done(self):
        assert not self.bad, f"{self.kind}: {len(self.bad)} path(s) outside eps (A + B s):\n" + "\n".join(self.bad)


def _engine(kind, ls, noise, X, Y, variant=0, variance=1.0, c=0.0):
    from trieste_amd.engine import GPEngine

    eng = GPEngine(len(ls), kind)
    eng.set_variant(variant)
    eng.set_hyper(variance, ls, noise, c)
    eng.set_data(np.ascontiguousarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64))
    return eng


def _widen(x, d):
    """The d-dimensional copy of 3-dimensional points: the extra coordinates are the same for every point."""
    if d == 3:
        return np.ascontiguousarray(x)
    extra = 0.1 + 0.05 * (np.arange(d - 3) % 7)
    return np.ascontiguousarray(np.concatenate([x, np.broadcast_to(extra, (x.shape[0], d - 3))], axis=1))


def _ls(g, d):
    return np.concatenate([np.array(g["lengthscales"]), 0.3 + 0.1 * (np.arange(d - 3) % 5)])


VARIANTS = ((0, "default"), (1, "fused"), (2, "rowsplit"), (9, "regstage"))


def _difference_form_paths(chk, make, p, d, joint=True):
    """Every difference-form path that forms k(x, X): ``make(variant)`` -> engine, ``p`` the probes."""
    x = _widen(p.x, d)
    M = x.shape[0]
    eng = make(0)
    chk.values(f"d={d} M={M} predict_mean", eng.predict_mean(x), p)
    chk.values(f"d={d} M={M} predict (default path)", eng.predict(x)[0], p)
    if M == M_SMALL:
        val, grad = eng.acq_value_grad("nlcb", 0.0, x)
        chk.values(f"d={d} acq_value_grad value", -np.asarray(val), p)
        chk.gradients(f"d={d} acq_value_grad gradient", np.asarray(grad)[:, :3], p, sign=-1.0)
        if d > 3:
            assert np.all(np.asarray(grad)[:, 3:] == 0.0), "gradient along coordinates that do not differ"
        chk.nlcb2(f"d={d} acq_value_grad nlcb(2)", *eng.acq_value_grad("nlcb", 2.0, x), p)
    chk.values(f"d={d} M={M} predict (sweep)", make(1024).predict(x)[0], p)
    for v, name in VARIANTS:
        chk.values(f"d={d} M={M} nlcb values ({name})", -np.asarray(make(v).acq_values("nlcb", 0.0, x)), p)
    if joint and M == M_SMALL:
        xg = x.reshape(-1, 4, d)
        for v, name in ((0, "skinny"), (1024, "joint kernel"), (4, "slots")):
            e = make(v)
            chk.values(f"d={d} predict_joint mean ({name})", e.predict_joint(xg)[0], p)
        chk.values(f"d={d} joint_forward mean", eng.joint_forward(xg)[0], p)


@pytest.mark.parametrize("d", [3, 40])
@pytest.mark.parametrize("kind", KINDS)
def test_single_point_design_every_path(kind, d):
    """mean(x) = k(x, X0) from predict_mean, predict (skinny product, sweep), the -LCB epilogue of the DMA, split and
    register-staged sweeps, both joint paths and the gradient kernel; at d = 40 the wide forms."""
    g = _goldens()
    chk = Checker(kind, B_DIFF[kind])
    X0, ls = _widen(np.array([g["X0"]]), d), _ls(g, d)
    make = functools.lru_cache(maxsize=None)(lambda v: _engine(kind, ls, g["noise"], X0, [4.0], v))
    L, W, alpha = make(0).get_factor()
    assert (L[0, 0], W[0, 0], alpha[0]) == (2.0, 0.5, 1.0), "the exact design is not exact"
    for M in (M_SMALL, M_LARGE):
        _difference_form_paths(chk, make, Probes(g["single"][kind], g["underflow"][kind]["x"], M), d)
    chk.done()


@pytest.mark.parametrize("kind", KINDS)
def test_single_point_design_trajectory(kind):
    """A trajectory with one feature of weight 0 and no noise draw is the canonical sum k(x, X0) v with v = alpha = 1:
    traj_shape / traj_sqrt / traj_exp2 through Trajectory.__call__ (shared and per-trajectory inputs), kernel_rt and
    kernel_dr2 through value_and_gradient."""
    g = _goldens()
    p = Probes(g["single"][kind], g["underflow"][kind]["x"], M_SMALL)
    eng = _engine(kind, np.array(g["lengthscales"]), g["noise"], [g["X0"]], [4.0])
    traj = eng.trajectory(np.array([[0.3, -0.7, 1.1]]), np.array([0.4]), np.zeros((1, 1)), np.zeros((1, 1)))
    assert traj.v()[0, 0] == 1.0, "the exact design is not exact"
    short, full = Checker(kind, B_TRAJ[kind]), Checker(kind, B_DIFF[kind])
    short.values("trajectory (shared inputs)", traj(p.x), p)
    short.values("trajectory (per-trajectory inputs)", traj(p.x[:, None, :]), p)
    val, grad = traj.value_and_gradient(p.x[:, None, :])
    full.values("trajectory value_and_gradient value", val, p)
    full.gradients("trajectory value_and_gradient gradient", grad, p)
    short.bad += full.bad
    short.done()


@pytest.mark.parametrize("kind", KINDS)
def test_row_positions(kind):
    """N = 257 training points 4096 lengthscales apart: K + noise I = 4 I exactly, and with Y = 4 e_i the mean around X_i is
    k(x, X_i) read from row i -- rows 0, 15, 16, 255, 256 sit in other fragments, k-steps and row blocks."""
    g = _goldens()
    R = g["rows"]
    N, ls = R["N"], np.array(g["lengthscales"])
    X = np.tile(np.array(g["X0"]), (N, 1))
    X[:, 0] += R["spacing"] * np.arange(N)
    chk = Checker(kind, B_DIFF[kind])
    for i in R["rows"]:
        Y = np.zeros(N)
        Y[i] = 4.0
        make = functools.lru_cache(maxsize=None)(lambda v: _engine(kind, ls, g["noise"], X, Y, v))
        _, _, alpha = make(0).get_factor()
        assert np.array_equal(alpha, np.eye(N)[i]), f"alpha is not one-hot at row {i}: the design is wrong"
        chk.kind = f"{kind} row {i}"
        _difference_form_paths(chk, make, Probes(R[kind][str(i)], [], M_SMALL), 3, joint=False)
    chk.kind = kind
    chk.done()


@pytest.mark.parametrize("kind", KINDS)
def test_dense_positive_sum(kind):
    """N = 17 with noise = 32 variance and Y > 0: mean = sum_k k(x, X_k) alpha_k, every term positive (condition 1); alpha
    is the engine's own (get_factor), the kernel values are the goldens'."""
    g = _goldens()
    D = g["dense"]
    X, Y, x = np.array(D["X"]), np.array(D["Y"]), np.array(D["x"])
    K, S = np.array(D[kind]["K"]), np.array(D[kind]["s"])
    ls = np.array(g["lengthscales"])
    make = functools.lru_cache(maxsize=None)(lambda v: _engine(kind, ls, 32.0, X, Y, v))
    _, _, alpha = make(0).get_factor()
    assert np.all(alpha > 0.0), "the dense design needs positive weights"
    terms = K * alpha
    p = Probes(dict(x=x.tolist(), k=[float(np.sum(np.sort(t))) for t in terms], s=np.zeros(len(x)).tolist(),
                    dk=np.zeros((len(x), 3)).tolist()), [], len(x))
    tol = EPS * (np.sum((A_COEF[kind] + B_DIFF[kind] * S) * terms, axis=1) + 17.0 * p.k)
    chk = Checker(kind, B_DIFF[kind])
    eng = make(0)
    chk.values("dense predict_mean", eng.predict_mean(p.x), p, tol=tol)
    chk.values("dense predict (default path)", eng.predict(p.x)[0], p, tol=tol)
    chk.values("dense predict (sweep)", make(1024).predict(p.x)[0], p, tol=tol)
    chk.values("dense acq_value_grad value", -np.asarray(eng.acq_value_grad("nlcb", 0.0, p.x)[0]), p, tol=tol)
    for v, name in VARIANTS:
        chk.values(f"dense nlcb values ({name})", -np.asarray(make(v).acq_values("nlcb", 0.0, p.x)), p, tol=tol)
    chk.done()
