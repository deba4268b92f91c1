"""GPU tests of general models through every large-shape kernel.

The other parity suites build one kind of model: equal lengthscales, kernel variance 1, a constant mean of about 0 and
inputs on the unit cube.  There sigma^2, sigma^4, sigma and 1 are the same number, a dropped mean changes nothing, ls[0]
reads the same value as ls[c], and |x|^2 + |X|^2 - 2 x.X is as good as sum_c (x_c - X_c)^2.  Every configuration here
departs from that model in all four ways at once:

* ARD lengthscales over about a decade, shuffled so that the shortest is not at index 0;
* a kernel variance far from 1 (0.37 or 250; Branin's empirical variance), the noise scaled with it;
* observations Y = a f + b with the constant mean far from 0;
* boxes of unequal sides, far from the origin ([1024, 1025]^d among them).

The reference is the numpy oracle in the difference form (oracle/gp_oracle.py ``difference_form``) on the engine's own
inputs; the dot-product form the oracle uses by default is no reference on a box far from the origin
(tests/test_oracle_difference_form.py).  Tolerances are those of tests/util.py with each configuration's own sigma^2:
1e-5 relative plus ``cancellation_floor(N, sigma^2, noise)`` (ten floors on mean-like quantities, the gradient tolerances
of tests/test_gpu_parity.py).  The metamorphic tests at the end need no tolerance: power-of-two scalings of inputs and
lengthscales, or of outputs and kernel variance, commute exactly with every operation of the engine."""
import functools

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.util import assert_close, cancellation_floor, i8x4_variance_bound

pytestmark = pytest.mark.gpu

MEAN_C = 37.5


def _cfg(name, d, kind, N, rel_noise, variance, lo, width, objective="ackley"):
    return dict(name=name, d=d, kind=kind, N=N, rel_noise=rel_noise, variance=variance,
                lo=np.array(np.broadcast_to(np.asarray(lo, dtype=np.float64), (d,))),
                width=np.array(np.broadcast_to(np.asarray(width, dtype=np.float64), (d,))), objective=objective)


def _unequal(d, seed):
    return np.round(np.random.default_rng(seed).uniform(0.5, 4.0, size=d), 2)


CONFIGS = [
    # DMA sweep and the int8 sweep's matrix-core generation on a box far from the origin
    _cfg("m52_d8_N1000_at1024", 8, "matern52", 1000, 1e-2, 250.0, 1024.0, 1.0),
    _cfg("m52_d8_N1000_at1024_lownoise", 8, "matern52", 1000, 1e-5, 0.37, 1024.0, 1.0),
    _cfg("rbf_d6_N700_at100", 6, "rbf", 700, 1e-2, 0.37, 100.0, 1.0),
    _cfg("rbf_d6_N700_at1024", 6, "rbf", 700, 1e-2, 250.0, 1024.0, 1.0),
    # Branin in its native box, observations not normalised (variance = their empirical variance)
    _cfg("branin_m52_d2_N300", 2, "matern52", 300, 1e-3, None, [-5.0, 0.0], [15.0, 15.0], objective="branin"),
    # dp = 32: the register-staged sweep, joint_kernel<32>, the gradient tails
    _cfg("rbf_d24_N600_at100", 24, "rbf", 600, 1e-2, 0.37, 100.0, _unequal(24, 1)),
    _cfg("m32_d17_N513_unequal", 17, "matern32", 513, 1e-3, 250.0, -40.0 + 7.0 * np.arange(17), _unequal(17, 2)),
    # wide form: coordinates in chunks of 32, lengthscales differing between the chunks
    _cfg("m52_d40_N700_at100", 40, "matern52", 700, 1e-2, 2.5, 100.0, _unequal(40, 3)),
    # the difference-form kernel family
    _cfg("m12_d3_N130_at300", 3, "matern12", 130, 1e-3, 0.37, [300.0, 0.5, -20.0], [10.0, 1.5, 3.0]),
]
IDS = [c["name"] for c in CONFIGS]
NARROW = [c for c in CONFIGS if c["d"] <= 32]
I8 = [c for c in CONFIGS if c["d"] <= 32]


@pytest.fixture(autouse=True)
def _difference_form_oracle():
    with O.difference_form():
        yield


class P:
    """One configuration's problem: data, hyper-parameters, candidates, the oracle's state."""


@functools.lru_cache(maxsize=None)
def _problem(name, M=2100, seed=5678):
    cfg = next(c for c in CONFIGS if c["name"] == name)
    return _build(cfg, M, seed)


def _build(cfg, M=2100, seed=5678):
    d, N, lo, w = cfg["d"], cfg["N"], cfg["lo"], cfg["width"]
    rng = np.random.default_rng(seed)
    U = rng.uniform(size=(N, d))
    X = lo + w * U
    if cfg["objective"] == "branin":
        Y = O.branin(U)                                   # the native function values (U is the unit-cube image)
        variance = float(np.var(Y))
    else:
        f = O.ackley(U)
        variance = cfg["variance"]
        Y = np.sqrt(variance) * (f - f.mean()) / f.std() + MEAN_C
    p = P()
    p.cfg, p.d, p.N, p.kind, p.lo, p.w = cfg, d, N, cfg["kind"], lo, w
    p.variance, p.noise = variance, cfg["rel_noise"] * variance
    p.ls = w * 0.2 * np.sqrt(d) * rng.permutation(np.geomspace(0.35, 3.5, d))
    assert d < 3 or int(np.argmin(p.ls)) != 0
    p.c = float(np.mean(Y))
    p.X, p.Y = X, Y
    Xq = lo + w * rng.uniform(size=(M, d))
    Xq[:5] = X[:5]                                         # exactly at training inputs (variance cancellation)
    Xq[5:10] = X[5:10] + 1e-6 * w                          # next to them
    Xq[10] = Xq[11]                                        # a duplicate (ties -> first index)
    Xq[-3:] = lo + 4.0 * w + w * rng.uniform(size=(3, d))  # far field at box + 4 width
    p.Xq = np.ascontiguousarray(Xq)
    p.st = O.gpr_update(p.kind, variance, p.ls, p.noise, p.c, X, Y)
    p.floor = cancellation_floor(N, variance, p.noise)
    p.om, p.ov = O.predict(p.st, p.Xq)
    p.eta = O.eta_min_mean(p.st)
    p.box = lambda n, s: lo + w * np.random.default_rng(s).uniform(size=n + (d,))
    return p


def _engine(p, variant=0, variance=None, ls=None, noise=None, c=None, X=None, Y=None):
    from trieste_amd.engine import GPEngine

    eng = GPEngine(p.d, p.kind)
    eng.set_variant(variant)
    eng.set_hyper(p.variance if variance is None else variance, p.ls if ls is None else ls,
                  p.noise if noise is None else noise, p.c if c is None else c)
    eng.set_data(p.X if X is None else X, p.Y if Y is None else Y)
    return eng


def _argmax_agrees(idx, oracle_vals, tol):
    oi = int(np.argmax(oracle_vals))
    return idx == oi or abs(oracle_vals[oi] - oracle_vals[idx]) <= tol


def _tails(p, mean, var, eta):
    return dict(ei=O.expected_improvement(mean, var, eta), pi=O.probability_of_improvement(mean, var, eta),
                nlcb=O.negative_lower_confidence_bound(mean, var, 1.96),
                aei=O.augmented_expected_improvement(mean, var, eta, p.noise))


def _acq_param(acq, eta):
    return 1.96 if acq == "nlcb" else eta


# ---- update ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_update_factor_matches_oracle(cfg):
    p = _problem(cfg["name"])
    eng = _engine(p)
    if p.N >= 512:
        assert eng.update_is_persistent(p.N)   # the persistent DAG update with a ragged tail (N is not a multiple of 128)
    L, W, alpha = eng.get_factor()
    assert_close(L, p.st.L, atol=p.floor, what="L")
    oalpha = O._solve_triangular(p.st.L.T, O._solve_triangular(p.st.L, p.st.err, lower=True), lower=False)
    ascale = max(1.0, np.abs(oalpha).max())
    assert_close(alpha, oalpha, atol=p.floor * ascale / min(p.noise, 1.0), what="alpha")
    assert_close(eng.eta(), p.eta, atol=p.floor * 10, what="eta")


# ---- sweeps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1, 2, 9], ids=["default-policy", "fused", "rowsplit", "fused-regstage"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_sweep_matches_oracle(cfg, variant):
    """predict, predict_mean, eta, the EI / PI / -LCB / AEI values, the fused arg-max and top-k under every launch policy
    (at d = 40 the wide forms: variant 9 runs the wide fused form as variant 1 does)."""
    p = _problem(cfg["name"])
    eng = _engine(p, variant)
    mean, var = eng.predict(p.Xq)
    assert_close(mean, p.om, atol=p.floor * 10, what="mean")
    assert_close(var, p.ov, atol=p.floor, what="var")
    assert_close(eng.predict_mean(p.Xq), p.om, atol=p.floor * 10, what="predict_mean")
    eta = eng.eta()
    assert_close(eta, p.eta, atol=p.floor * 10, what="eta")
    for acq, want in _tails(p, p.om, p.ov, eta).items():
        got = eng.acq_values(acq, _acq_param(acq, eta), p.Xq)
        atol = p.floor * (1e3 if acq == "pi" else 1)
        assert_close(got, want, atol=atol, what=f"{acq} values")
        val, idx, x = eng.acq_argmax(acq, _acq_param(acq, eta), p.Xq)
        assert idx == int(np.argmax(got)) and val == got[idx], (acq, idx, int(np.argmax(got)))
        assert _argmax_agrees(idx, want, 1e-5 * abs(np.max(want)) + atol), (acq, idx, int(np.argmax(want)))
        np.testing.assert_array_equal(x, p.Xq[idx])
        tv, ti = eng.acq_topk(acq, _acq_param(acq, eta), p.Xq, 17)
        ov_, oi_ = O.top_k(np.asarray(got), 17)
        np.testing.assert_array_equal(ti, oi_)
        np.testing.assert_array_equal(tv, ov_)


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_small_calls_match_oracle(cfg):
    """predict at M = 1, 65 and 2048 points (the skinny-product path) against the oracle and against the sweep."""
    p = _problem(cfg["name"])
    eng = _engine(p)
    sweep = _engine(p, 1024)
    for M in (1, 65, 2048):
        Xq = np.ascontiguousarray(np.concatenate([p.Xq[:M - 3], p.Xq[-3:]]) if M >= 7 else p.Xq[:M])
        om, ov = O.predict(p.st, Xq)
        mean, var = eng.predict(Xq)
        assert_close(mean, om, atol=p.floor * 10, what=f"mean M={M}")
        assert_close(var, ov, atol=p.floor, what=f"var M={M}")
        ms, vs = sweep.predict(Xq)
        assert_close(mean, ms, atol=p.floor * 10, what=f"mean: skinny product vs sweep M={M}")
        assert_close(var, vs, atol=p.floor, what=f"var: skinny product vs sweep M={M}")


# ---- joint and batch -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1024, 4], ids=["skinny-product", "joint-kernel", "slots"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_joint_and_qei_match_oracle(cfg, variant):
    p = _problem(cfg["name"])
    eng = _engine(p, variant)
    rng = np.random.default_rng(7)
    for q, G, S in ((1, 9, 8), (9, 4, 16), (33, 5, 8), (64, 3, 8)):
        Xg = p.box((G, q), 100 + q)
        Xg[0, 0] = p.X[0]
        jm, jc = eng.predict_joint(Xg)
        om, oc = O.predict_joint(p.st, Xg)
        assert_close(jm, om, atol=p.floor * 10, what=f"joint mean q={q}")
        assert_close(jc, oc, atol=p.floor, what=f"joint cov q={q}")
        eps = rng.normal(size=(q, S))
        eta = float(np.median(om))
        want = O.batch_mc_ei(p.st, Xg, eps, eta, 1e-6)
        assert np.count_nonzero(want) >= want.size // 2, f"vacuous qEI comparison at q={q}: {want}"
        assert_close(eng.qei(Xg, eps, eta, 1e-6), want, atol=p.floor, what=f"qei q={q}")


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_joint_forward_vjp_and_qei_gradient_match_oracle(cfg):
    from tests.test_gpu_parity import _dense_joint_vjp

    p = _problem(cfg["name"])
    eng = _engine(p)
    rng = np.random.default_rng(17)
    for q, G, S in ((1, 5, 32), (9, 3, 48), (33, 2, 64), (64, 2, 33)):
        Xg = p.box((G, q), 200 + q)
        Xg[0, 0] = p.X[0]
        jm, jc = eng.joint_forward(Xg)
        om, oc = O.predict_joint(p.st, Xg)
        assert_close(jm, om, atol=p.floor * 10, what=f"joint_forward mean q={q}")
        assert_close(jc, oc, atol=p.floor * 10, what=f"joint_forward cov q={q}")
        gm, gc = rng.normal(size=(G, q)), rng.normal(size=(G, q, q))
        want = _dense_joint_vjp(p.st, Xg, gm, gc)
        gscale = np.abs(want).max() + 1e-300
        assert_close(eng.joint_vjp(Xg, gm, gc), want, rtol=1e-5, atol=max(p.floor * 1e3 * q, 1e-9 * gscale),
                     what=f"joint_vjp q={q}")
        eps = rng.normal(size=(q, S))
        eta = float(np.median(om))
        val, grad = eng.qei_value_grad(Xg, eps, eta, 1e-6)
        oval, ograd = O.batch_mc_ei_value_and_grad(p.st, Xg, eps, eta, 1e-6)
        assert_close(val, oval, atol=p.floor, what=f"qEI value q={q}")
        gscale = np.abs(ograd).max() + 1e-300
        assert_close(grad, ograd, rtol=1e-5, atol=max(p.floor * 1e3 * q, 1e-7 * gscale), what=f"qEI gradient q={q}")


# ---- gradients -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_acq_value_and_gradient_match_oracle(cfg):
    p = _problem(cfg["name"])
    eng = _engine(p)
    Xq = np.ascontiguousarray(np.concatenate([p.Xq[:70], p.Xq[-3:]]))
    eta = eng.eta()
    for acq in ("ei", "pi", "nlcb", "aei"):
        par = _acq_param(acq, eta)
        val, grad = eng.acq_value_grad(acq, par, Xq)
        oval, ograd = O.acq_value_and_grad(p.st, acq, par, Xq)
        assert_close(val, oval, atol=p.floor * (1e3 if acq == "pi" else 1), what=f"{acq} value")
        gscale = np.abs(ograd).max() + 1e-300
        assert_close(grad, ograd, rtol=1e-5, atol=max(p.floor * 1e3, 1e-9 * gscale), what=f"{acq} gradient")


@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_nlml_and_its_gradient_match_oracle(cfg):
    """The value and the derivative w.r.t. EACH lengthscale, the variance, the noise and the mean; the trial paths."""
    p = _problem(cfg["name"])
    eng = _engine(p)
    val, grad = eng.nlml()
    oval, ograd = O.nlml_and_grad(p.st)
    assert_close(val, oval, rtol=1e-9, atol=1e-7, what="nlml")
    assert_close(grad, ograd, rtol=1e-5, atol=1e-7 * np.abs(ograd).max() + 1e-6 / p.noise * 1e-6, what="nlml gradient")
    d = p.d
    # every entry on its own scale too: a lengthscale read from the wrong coordinate moves one entry, maybe a small one
    for k in range(d + 3):
        assert_close(grad[k], ograd[k], rtol=1e-5, atol=1e-7 * np.abs(ograd).max(), what=f"nlml gradient[{k}]")
    eng.set_hyper(p.variance, p.ls, p.noise, p.c)
    eng.set_data(p.X, p.Y)
    assert_close(eng.nlml_trial(), oval, rtol=1e-9, atol=1e-7, what="nlml_trial")
    eng = _engine(p)
    rng = np.random.default_rng(3)
    hy, want = [], []
    for b in range(3):
        v, ls, nz, c = p.variance * (0.5 + b), p.ls * rng.uniform(0.7, 1.4, size=d), p.noise * (1 + b), p.c + 0.25 * b
        hy.append(np.concatenate([[v], ls, [nz, c]]))
        want.append(O.nlml_and_grad(O.gpr_update(p.kind, v, ls, nz, c, p.X, p.Y))[0])
    values, ok = eng.nlml_trial_batch(np.array(hy))
    assert np.all(ok)
    assert_close(values, np.array(want), rtol=1e-9, atol=1e-7, what="nlml_trial_batch")


# ---- cross-covariance and fantasising --------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_cov_between_and_fantasised_model_match_oracle(cfg):
    p = _problem(cfg["name"])
    eng = _engine(p)
    for p1, p2 in ((1, 1), (63, 65), (64, 130)):
        X1, X2 = p.Xq[:p1], p.Xq[200:200 + p2]
        assert_close(eng.cov_between(X1, X2), O.covariance_between_points(p.st, X1, X2), atol=p.floor * 10,
                     what=f"cov {p1}x{p2}")
    twin = eng.clone()
    pend = p.box((6,), 31)
    kb = eng.predict_mean(pend)
    twin.append_data(pend[:1], kb[:1])
    twin.append_data(pend[1:], kb[1:])
    floor = cancellation_floor(p.N + 6, p.variance, p.noise)
    sto = O.fantasized_state(p.st, pend, np.asarray(kb))
    fm, fv = twin.predict(p.Xq[:300])
    om, ov = O.predict(sto, p.Xq[:300])
    assert_close(fm, om, atol=floor * 10, what="fantasised mean")
    assert_close(fv, ov, atol=floor, what="fantasised var")
    refit = _engine(p, X=np.concatenate([p.X, pend]), Y=np.concatenate([p.Y, kb]))
    rm, rv = refit.predict(p.Xq[:300])
    assert_close(fm, rm, atol=floor * 10, what="append == refit mean")
    assert_close(fv, rv, atol=floor, what="append == refit var")


@pytest.mark.parametrize("kind", ["soft", "hard"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=IDS)
def test_penalized_sweeps_match_oracle(cfg, kind):
    p = _problem(cfg["name"])
    eng = _engine(p)
    pending = np.concatenate([p.box((4,), 11), p.Xq[7:8]])
    lip, eta = O.lipschitz_estimate(p.st, np.concatenate([p.X, p.box((100,), 12)]))
    radius, scale = O.local_penalizer_parameters(p.st, pending, lip, eta)
    base = eng.acq_values("ei", eta, p.Xq)
    phi = O.PENALIZERS[kind](p.Xq, pending, radius, scale)
    with eng.penalized(kind, pending, radius, scale):
        assert_close(eng.penalization_values(p.Xq), phi, rtol=1e-11, atol=1e-300, what="penalization")
        vals = eng.acq_values("ei", eta, p.Xq)
        val, idx, _ = eng.acq_argmax("ei", eta, p.Xq)
        gv, gg = eng.acq_value_grad("ei", eta, p.Xq[:64])
    assert_close(vals, base * phi, rtol=1e-11, atol=1e-300, what="penalized = base * phi")
    assert idx == int(np.argmax(vals)) and val == vals[idx]
    oval, ograd = O.penalized_value_and_grad(p.st, "ei", eta, kind, pending, radius, scale, p.Xq[:64])
    assert_close(gv, oval, atol=p.floor, what="penalized value")
    gscale = np.abs(ograd).max() + 1e-300
    assert_close(gg, ograd, rtol=1e-5, atol=max(p.floor * 1e3, 1e-9 * gscale), what="penalized gradient")


# ---- trajectories ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", NARROW, ids=[c["name"] for c in NARROW])
def test_trajectories_match_oracle(cfg):
    """Decoupled trajectories on the shifted inputs themselves (the RFF phase is not translation invariant)."""
    from trieste_amd.sampler import sample_rff_basis

    p = _problem(cfg["name"])
    eng = _engine(p)
    rng = np.random.default_rng(99)
    F, B = 300, 4
    W, b = sample_rff_basis(p.kind, F, p.d, rng)
    w, xi = rng.standard_normal((F, B)), rng.standard_normal((p.N, B))
    traj = eng.trajectory(W, b, w, xi)
    v = traj.v()
    ov = O.decoupled_weights(p.st, W, b, w, xi)
    scale = max(1.0, np.abs(ov).max())
    assert_close(v, ov, atol=p.floor * scale / min(p.noise, 1.0), what="trajectory weights v")
    ref = O.trajectory_eval(p.st, W, b, w, v, p.Xq)
    tscale = np.sqrt(p.variance) * max(1.0, np.abs(v).max())
    got = traj(p.Xq)
    assert_close(got, ref, rtol=1e-7, atol=1e-8 * tscale, what="trajectory values")
    vals, idx = traj.argmin(p.Xq)
    for bb in range(B):
        oi = int(np.argmin(ref[:, bb]))
        assert idx[bb] == oi or abs(ref[idx[bb], bb] - ref[oi, bb]) <= 1e-7 * abs(ref[oi, bb]) + 1e-8 * tscale
    Xp = p.box((37, B), 5)
    Xp[0, 0] = p.X[3]
    val, grad = traj.value_and_gradient(Xp)
    oval, ograd = O.trajectory_value_and_grad(p.st, W, b, w, v, Xp)
    assert_close(val, oval, rtol=1e-7, atol=1e-8 * tscale, what="trajectory value")
    sl = slice(1, None) if p.kind == "matern12" else slice(None)
    assert_close(grad[sl], ograd[sl], rtol=1e-6, atol=1e-8 * np.abs(ograd).max(), what="trajectory gradient")
    for n, S in ((1, 3), (65, 7), (300, 5)):
        eps = rng.standard_normal((n, S))
        want = O.joint_samples(p.st, p.Xq[:n], eps, 1e-6)
        assert_close(eng.sample_joint(p.Xq[:n], eps, 1e-6), want, rtol=1e-5,
                     atol=max(p.floor * 1e3, 1e-9 * p.variance) * 30, what=f"joint samples n={n}")


# ---- int8 rungs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["i8x4", "i8x5"])
@pytest.mark.parametrize("cfg", I8, ids=[c["name"] for c in I8])
def test_i8_sweeps_match_oracle(cfg, precision):
    """i8x4 within its variance budget, i8x5 within the plain tolerance; the mean never leaves float64 (it is accumulated
    from the same float64 kernel values the variance's digits are cut from)."""
    p = _problem(cfg["name"])
    eng = _engine(p)
    if precision == "i8x5" and p.d > 16:
        with pytest.raises(ValueError):
            eng.set_precision("i8x5")
        return
    budget = 0.0 if precision == "i8x5" else i8x4_variance_bound(p.N, p.variance, np.abs(eng.get_factor()[1]).max())
    fm, fv = eng.predict(p.Xq)
    eng.set_precision(precision)
    mean, var = eng.predict(p.Xq)
    assert_close(mean, p.om, atol=p.floor * 10, what=f"{precision} mean")
    assert_close(var, p.ov, atol=p.floor + budget, what=f"{precision} var")
    assert_close(mean, fm, rtol=1e-12, atol=1e-12 * max(1.0, abs(p.c)), what=f"{precision} mean == float64 mean")
    eta = eng.eta()
    oei = O.expected_improvement(p.om, p.ov, eta)
    ei = eng.acq_values("ei", eta, p.Xq)
    assert_close(ei, oei, atol=p.floor * 10 + budget, what=f"{precision} ei")
    val, idx, _ = eng.acq_argmax("ei", eta, p.Xq)
    assert idx == int(np.argmax(ei)) and val == ei[idx]
    assert _argmax_agrees(idx, oei, 1e-5 * np.max(oei) + p.floor * 10 + budget), (idx, int(np.argmax(oei)))


@pytest.mark.parametrize("cfg", I8, ids=[c["name"] for c in I8])
def test_auto_precision_matches_oracle_on_every_rung(cfg):
    p = _problem(cfg["name"])
    eng = _engine(p)
    eta = eng.eta()
    eta_mid = float(np.median(p.om))
    f64 = {e: eng.acq_argmax("ei", e, p.Xq)[:2] for e in (eta, eta_mid)}
    fm, _ = eng.predict(p.Xq)
    eng.set_precision("auto")
    rungs = []
    for _ in range(4):
        eff = eng.get_precision()[1]
        rungs.append(eff)
        mean, var = eng.predict(p.Xq)
        assert_close(var, p.ov, atol=p.floor, what=f"var under auto ({eff})")
        assert_close(mean, p.om, atol=p.floor * 10, what=f"mean under auto ({eff})")
        assert_close(mean, fm, rtol=1e-12, atol=1e-12 * max(1.0, abs(p.c)), what=f"auto mean == float64 mean ({eff})")
        for e in (eta, eta_mid):
            assert_close(eng.acq_values("ei", e, p.Xq), O.expected_improvement(p.om, p.ov, e), atol=p.floor,
                         what=f"ei under auto ({eff})")
            val, idx, _ = eng.acq_argmax("ei", e, p.Xq)
            assert idx == f64[e][1] and abs(val - f64[e][0]) <= 1e-12 * abs(f64[e][0]), (eff, e, val, idx, f64[e])
    print(f"[auto] {cfg['name']}: rungs {rungs}")


@pytest.mark.parametrize("rel_noise", [1e-2, 1e-5])
def test_headline_shaped_model_under_auto(rel_noise):
    """N = 4096, d = 8, Matern-5/2 on [1024, 1025]^8 with a general model, 20 000 candidates: f64, i8x4, i8x5 and auto
    against the oracle (in row chunks), and auto's arg-max is the float64 sweep's."""
    cfg = _cfg("m52_d8_N4096_at1024", 8, "matern52", 4096, rel_noise, 250.0, 1024.0, 1.0)
    p = _build(cfg, M=20000, seed=4321)
    eng = _engine(p)
    om = np.empty(p.Xq.shape[0])
    ov = np.empty(p.Xq.shape[0])
    for s in range(0, p.Xq.shape[0], 4000):
        om[s:s + 4000], ov[s:s + 4000] = O.predict(p.st, p.Xq[s:s + 4000])
    eta = eng.eta()
    oei = O.expected_improvement(om, ov, eta)
    f64 = eng.acq_argmax("ei", eta, p.Xq)[:2]
    fm, _ = eng.predict(p.Xq)
    for precision in ("f64", "i8x4", "i8x5", "auto"):
        eng.set_precision(precision)
        for _ in range(2 if precision == "auto" else 1):
            eff = eng.get_precision()[1]
            m, v = eng.predict(p.Xq)
            assert_close(v, ov, atol=p.floor, what=f"{precision} ({eff}) var")
            assert_close(m, om, atol=p.floor * 10, what=f"{precision} ({eff}) mean")
            assert_close(m, fm, rtol=1e-12, atol=1e-12 * abs(p.c), what=f"{precision} ({eff}) mean == float64 mean")
            assert_close(eng.acq_values("ei", eta, p.Xq), oei, atol=p.floor, what=f"{precision} ({eff}) ei")
            val, idx, _ = eng.acq_argmax("ei", eta, p.Xq)
            assert _argmax_agrees(idx, oei, 1e-5 * np.max(oei) + p.floor), (precision, idx, int(np.argmax(oei)))
            if precision == "auto":
                assert idx == f64[1], (eff, idx, f64)


# ---- host layer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("problem", ["branin_native", "hartmann6_shifted"])
def test_host_model_and_ego_on_unnormalised_boxes(problem):
    """GaussianProcessRegression(build_gpr(...)) in the problem's own box: the model's predictions against the oracle at the
    model's own hyper-parameters, an EGO step's point against the oracle's arg-max (tolerance band), the same point under
    sweep_precision="auto", and a device group of one returning the engine's winner."""
    import trieste_amd.models as M
    from trieste_amd.acquisition import EfficientGlobalOptimization
    from trieste_amd.data import Dataset
    from trieste_amd.group import GPEngineGroup
    from trieste_amd.space import Box, DiscreteSearchSpace

    if problem == "branin_native":
        lo, hi = np.array([-5.0, 0.0]), np.array([10.0, 15.0])
        fn = lambda x: O.branin((x - lo) / (hi - lo))   # noqa: E731
    else:
        lo = np.array([300.0, 0.5, -20.0, 1024.0, 7.0, 50.0])
        hi = lo + np.array([10.0, 1.5, 3.0, 1.0, 0.25, 40.0])
        fn = lambda x: 3.0 * O.hartmann_6((x - lo) / (hi - lo)) + 12.0   # noqa: E731
    d = lo.size
    space = Box(lo, hi)
    x = space.sample(80, seed=3)
    data = Dataset(x, fn(x)[:, None])
    gpr = M.build_gpr(data, space, likelihood_variance=1e-3 * float(np.var(data.observations)))
    model = M.GaussianProcessRegression(gpr)
    k = gpr.kernel
    st = O.gpr_update("matern52", k.variance, k.lengthscales, gpr.likelihood_variance, gpr.mean_function.c,
                      x, data.observations[:, 0])
    floor = cancellation_floor(80, k.variance, gpr.likelihood_variance)
    cands = space.sample(5000, seed=5678)
    cands[:3] = x[:3]
    m, v = model.predict(cands)
    om, ov = O.predict(st, cands)
    assert_close(m[:, 0], om, atol=floor * 10, what="model mean")
    assert_close(v[:, 0], ov, atol=floor, what="model var")
    eta = O.eta_min_mean(st)
    oei = O.expected_improvement(om, ov, eta)
    band = 1e-5 * np.max(oei) + floor
    pt = EfficientGlobalOptimization().acquire_single(DiscreteSearchSpace(cands), model, dataset=data)
    idx = int(np.flatnonzero(np.all(cands == pt[0], axis=1))[0])
    assert _argmax_agrees(idx, oei, band), (idx, int(np.argmax(oei)))
    auto = M.GaussianProcessRegression(model.model, sweep_precision="auto")
    pt_auto = EfficientGlobalOptimization().acquire_single(DiscreteSearchSpace(cands), auto, dataset=data)
    np.testing.assert_array_equal(pt_auto, pt)
    from trieste_amd.engine import GPEngine

    eng = GPEngine(d, "matern52")
    eng.set_hyper(k.variance, k.lengthscales, gpr.likelihood_variance, gpr.mean_function.c)
    eng.set_data(x, data.observations[:, 0])
    e = eng.eta()
    val, i, _ = eng.acq_argmax("ei", e, cands)
    grp = GPEngineGroup(d, "matern52", devices=[0])
    try:
        grp.set_hyper(k.variance, k.lengthscales, gpr.likelihood_variance, gpr.mean_function.c)
        grp.set_data(x, data.observations[:, 0])
        grp.set_candidates(cands)
        gval, gidx, _ = grp.acq_argmax("ei", e)
    finally:
        grp.close()
    assert (gval, gidx) == (val, i)


# ---- metamorphic: no tolerance ---------------------------------------------------------------------------------------
def _assert_scaled(got, want, s, what=""):
    """got == want bit for bit where the value is a normal number both before and after the scaling by s (a power of two).
    Below tiny * max(s, 1 / s) the unscaled value (or a term of its sum) was subnormal, and the rounding of a subnormal is
    not undone by the scaling: there the two may differ by at most that bound, a rounding far below any tolerance."""
    got, want = np.asarray(got), np.asarray(want)
    band = np.finfo(np.float64).tiny * max(s, 1.0 / s)
    normal = np.abs(want) >= band
    np.testing.assert_array_equal(got[normal], want[normal], err_msg=what)
    assert np.all(np.abs(got[~normal] - want[~normal]) <= band), what


def _sweep_outputs(eng, Xq, eta):
    mean, var = eng.predict(Xq)
    out = dict(mean=np.asarray(mean), var=np.asarray(var), ei=np.asarray(eng.acq_values("ei", eta, Xq)))
    out["argmax"] = eng.acq_argmax("ei", eta, Xq)[:2]
    out["topk"] = eng.acq_topk("ei", eta, Xq, 9)
    return out


SCALING = [c for c in CONFIGS if c["name"] in ("m52_d8_N1000_at1024", "rbf_d6_N700_at100", "m52_d40_N700_at100",
                                               "m12_d3_N130_at300", "rbf_d24_N600_at100")]


@pytest.mark.parametrize("k", [-2, 3])
@pytest.mark.parametrize("cfg", SCALING, ids=[c["name"] for c in SCALING])
def test_input_scaling_by_a_power_of_two_is_exact(cfg, k):
    """X, Xq and the lengthscales times 2^k: x / ls is bit-identical, so every output is; gradients w.r.t. x are exactly 2^-k
    times the unscaled ones (the f64 sweeps, the wide form, i8x4 and i8x5, joint, trajectories)."""
    p = _problem(cfg["name"])
    s = 2.0 ** k
    a, b = _engine(p), _engine(p, ls=p.ls * s, X=p.X * s)
    Xq, Xs = p.Xq, p.Xq * s
    eta = a.eta()
    assert b.eta() == eta
    precisions = ["f64"] + (["i8x4"] if p.d <= 32 else []) + (["i8x5"] if p.d <= 16 else [])
    for prec in precisions:
        a.set_precision(prec)
        b.set_precision(prec)
        oa, ob = _sweep_outputs(a, Xq, eta), _sweep_outputs(b, Xs, eta)
        for key in ("mean", "var", "ei"):
            np.testing.assert_array_equal(ob[key], oa[key], err_msg=f"{prec} {key}")   # (x / ls is bit-identical)
        assert ob["argmax"] == oa["argmax"], prec
        np.testing.assert_array_equal(ob["topk"][1], oa["topk"][1])
        np.testing.assert_array_equal(ob["topk"][0], oa["topk"][0])
    a.set_precision("f64")
    b.set_precision("f64")
    va, ga = a.acq_value_grad("ei", eta, Xq[:64])
    vb, gb = b.acq_value_grad("ei", eta, Xs[:64])
    np.testing.assert_array_equal(vb, va)
    _assert_scaled(gb, ga / s, s, "acquisition gradient")
    Xg = p.box((5, 9), 41)
    for x, y in zip(b.predict_joint(Xg * s), a.predict_joint(Xg)):
        np.testing.assert_array_equal(x, y)
    na, nga = a.nlml()
    nb, ngb = b.nlml()
    assert na == nb
    _assert_scaled(ngb[:p.d], nga[:p.d] / s, s, "nlml lengthscale gradient")
    np.testing.assert_array_equal(ngb[p.d:], nga[p.d:])
    if p.d <= 32:
        from trieste_amd.sampler import sample_rff_basis

        rng = np.random.default_rng(5)
        W, bb = sample_rff_basis(p.kind, 64, p.d, rng)
        w, xi = rng.standard_normal((64, 2)), rng.standard_normal((p.N, 2))
        ta, tb = a.trajectory(W, bb, w, xi), b.trajectory(W, bb, w, xi)
        np.testing.assert_array_equal(tb(Xs[:500]), ta(Xq[:500]))
        np.testing.assert_array_equal(tb.argmin(Xs[:500])[1], ta.argmin(Xq[:500])[1])


@pytest.mark.parametrize("k", [-1, 2])
@pytest.mark.parametrize("cfg", SCALING, ids=[c["name"] for c in SCALING])
def test_output_scaling_by_a_power_of_two_is_exact(cfg, k):
    """Y, c and eta times 2^k, variance and noise times 4^k: K + noise I scales by 4^k exactly, L by 2^k, alpha by 2^-k;
    mean and EI scale by 2^k exactly, the variance by 4^k, and the arg-max does not move.  (The variance clip VAR_FLOOR is an
    absolute constant: no candidate here reaches it.)"""
    p = _problem(cfg["name"])
    s = 2.0 ** k
    a = _engine(p)
    b = _engine(p, variance=p.variance * s * s, noise=p.noise * s * s, c=p.c * s, Y=p.Y * s)
    eta = a.eta()
    assert b.eta() == eta * s
    La, _, aa = a.get_factor()
    Lb, _, ab = b.get_factor()
    np.testing.assert_array_equal(Lb, La * s)
    np.testing.assert_array_equal(ab, aa / s)
    precisions = ["f64"] + (["i8x4"] if p.d <= 32 else []) + (["i8x5"] if p.d <= 16 else [])
    for prec in precisions:
        a.set_precision(prec)
        b.set_precision(prec)
        oa, ob = _sweep_outputs(a, p.Xq, eta), _sweep_outputs(b, p.Xq, eta * s)
        assert np.all(oa["var"] > 1e-12)
        np.testing.assert_array_equal(ob["mean"], oa["mean"] * s, err_msg=prec)
        np.testing.assert_array_equal(ob["var"], oa["var"] * s * s, err_msg=prec)
        _assert_scaled(ob["ei"], oa["ei"] * s, s, prec)
        assert ob["argmax"][1] == oa["argmax"][1], prec
        np.testing.assert_array_equal(ob["topk"][1], oa["topk"][1])
    a.set_precision("f64")
    b.set_precision("f64")
    Xg = p.box((5, 9), 43)
    (ma, ca), (mb, cb) = a.predict_joint(Xg), b.predict_joint(Xg)
    np.testing.assert_array_equal(mb, ma * s)
    np.testing.assert_array_equal(cb, ca * s * s)
    va, ga = a.acq_value_grad("ei", eta, p.Xq[:64])
    vb, gb = b.acq_value_grad("ei", eta * s, p.Xq[:64])
    _assert_scaled(vb, va * s, s, "ei value")
    _assert_scaled(gb, ga * s, s, "ei gradient")


@pytest.mark.parametrize("cfg", [c for c in CONFIGS if c["name"] in ("rbf_d6_N700_at1024", "m52_d8_N1000_at1024",
                                                                       "rbf_d6_N700_at100", "rbf_d24_N600_at100")],
                         ids=lambda c: c["name"])
def test_translation_changes_nothing_beyond_the_tolerance(cfg):
    """The engine on (X + t, Xq + t) against the engine on the exact centred copies (X + t) - t, within the parity
    tolerance: the rounding of the scaled coordinates differs, so this cannot be bit-exact.  Also on the int8 rungs.  (Boxes
    [t, t + w] with w <= t: X - t is exact.)"""
    p = _problem(cfg["name"])
    X0, Xq0 = p.X - p.lo, p.Xq - p.lo
    assert np.array_equal(X0 + p.lo, p.X) and np.array_equal(Xq0 + p.lo, p.Xq)
    a, b = _engine(p), _engine(p, X=X0)
    eta = a.eta()
    assert_close(b.eta(), eta, atol=p.floor * 10, what="translated eta")
    for prec in ["f64", "i8x4"] + (["i8x5"] if p.d <= 16 else []):
        a.set_precision(prec)
        b.set_precision(prec)
        ma, va = a.predict(p.Xq)
        mb, vb = b.predict(Xq0)
        budget = 0.0 if prec != "i8x4" else 2 * i8x4_variance_bound(p.N, p.variance, np.abs(a.get_factor()[1]).max())
        assert_close(ma, mb, atol=p.floor * 10, what=f"{prec} translated mean")
        assert_close(va, vb, atol=p.floor + budget, what=f"{prec} translated var")
