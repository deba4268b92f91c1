"""GPU tests: results do not depend on a handle's history or on stale memory.

The other GPU suites build a handle, give it one model and query it once.  The engine keeps state from one call to the
next -- factor matrices wiped once per (allocation, Npad) and not per update, a process-wide scratch for the batched trial
evaluations with the same rule, grow-only scratch buffers, int8 digit planes / task plans / the low-rank twin check cached
per factorisation -- and every transition below aims at one of those mechanisms.  The assertion needs no tolerance: the
kernels use no floating-point atomics and every summation order is fixed by (model, inputs), so after any sequence of calls

    battery(handle with a history) == battery(fresh handle given the final model directly)      bit for bit,

under the default launch policy and with ``update`` forced through the recursion (tgp_set_variant bit 4).  Once per state
the fresh handle is anchored against the numpy oracle at the suite's usual tolerances, which keeps "both wrong alike" out.
States, battery and the tour of the poisoned run live in tests/history_tour.py.

Trajectories are the one object that legitimately depends on history: a trajectory belongs to the factorisation it was
drawn from, and every tgp_traj_* call refuses (TGP_ERR_STATE -> RuntimeError) once the handle's model has moved on.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import gp_oracle as O
from tests import history_tour as T
from tests.util import assert_close, cancellation_floor, i8x4_variance_bound

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = pytest.mark.parametrize("variant", [0, T.NO_DAG], ids=["default", "no-dag"])
M4 = "m52_d4"


def _same(got: dict, want: dict, what: str) -> None:
    assert sorted(got) == sorted(want), what
    for k in want:
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"{what}: {k}")


@functools.lru_cache(maxsize=None)
def _fresh(model: str, name: str, variant: int) -> dict:
    """The battery of a fresh handle given the state directly -- computed once, shared, anchored against the oracle."""
    s = T.state(model, name)
    eng = T.engine(s, variant)
    out = T.battery(eng, s)
    eng.close()
    st = T.oracle_state(s)
    floor = cancellation_floor(s.N, s.variance, s.noise)
    om, ov = O.predict(st, s.Xq)
    assert_close(out["mean"], om, atol=floor * 10, what=f"{name}: mean vs oracle")
    assert_close(out["var"], ov, atol=floor, what=f"{name}: var vs oracle")
    eta = float(out["eta"])
    assert_close(eta, O.eta_min_mean(st), atol=floor, what=f"{name}: eta vs oracle")
    assert_close(out["acq.ei"], O.expected_improvement(om, ov, eta), atol=floor, what=f"{name}: ei vs oracle")
    jm, jc = O.predict_joint(st, T.inputs(s).Xg)
    assert_close(out["joint.mean"], jm, atol=floor * 10, what=f"{name}: joint mean vs oracle")
    assert_close(out["joint.cov"], jc, atol=floor, what=f"{name}: joint cov vs oracle")
    oval, ograd = O.nlml_and_grad(st)
    assert_close(out["nlml"], oval, rtol=1e-9, atol=1e-7, what=f"{name}: nlml vs oracle")
    assert_close(out["nlml.g"], ograd, rtol=1e-5, atol=1e-7 * np.abs(ograd).max() + 1e-6 / s.noise * 1e-6,
                 what=f"{name}: nlml gradient vs oracle")
    assert np.count_nonzero(out["qei"]) >= out["qei"].size // 2 and np.all(np.isfinite(out["bei"]))  # not vacuous
    return out


@functools.lru_cache(maxsize=None)
def _single_trials(model: str, name: str, variant: int) -> np.ndarray:
    """tgp_nlml_trial of one fresh handle at every member of T.trial_hypers -- computed once, anchored against the oracle."""
    s = T.state(model, name)
    vals = T.single_trials(s, variant)
    want = [O.nlml_and_grad(O.gpr_update(s.kind, r[0], r[1:-2], r[-2], r[-1], s.X, s.Y))[0] for r in T.trial_hypers(s)]
    assert_close(vals, np.array(want), rtol=1e-9, atol=1e-7, what=f"{name}: nlml_trial vs oracle")
    return vals


# ---- 1 ---------------------------------------------------------------------------------------------------------------
@VARIANTS
@pytest.mark.parametrize("model", list(T.MODELS))
def test_set_data_chain_on_one_handle(model, variant):
    """A -> B -> C -> D -> A -> B on ONE handle.  Aims at d_L / d_W being wiped once per (allocation, Npad): A -> B shrinks
    inside Npad = 512 with no fresh wipe, so A's rows 300 .. 499 become padding rows of buffers the sweeps, the skinny
    products and Wt read in full; C and D change Npad (a wipe each, grow-only buffers keep their capacity); the second
    A -> B repeats the in-place shrink in buffers that by then held D."""
    eng = T.engine(T.state(model, "A"), variant, data=False)
    for i, n in enumerate(T.CHAIN):
        s = T.state(model, n)
        T.put(eng, s)
        _same(T.battery(eng, s), _fresh(model, n, variant), f"step {i}: {n}")


# ---- 2 ---------------------------------------------------------------------------------------------------------------
@VARIANTS
def test_failed_update_then_a_good_one_at_the_same_size(variant):
    """A breakdown half way through the factorisation at N = 300 inside A's buffers (duplicated inputs, no noise: the
    NOT_PD recipe of test_edge_cases_and_errors) leaves L / W partly written -- possibly with NaNs -- and no wipe follows,
    because the (allocation, Npad) key is unchanged: the next good update must still give a fresh handle's bits."""
    from trieste_amd._lib import NotPositiveDefiniteError

    a, b = T.state(M4, "A"), T.state(M4, "B")
    eng = T.engine(a, variant)
    X2 = b.X.copy()
    X2[150:] = X2[:150]
    eng.set_hyper(b.variance, b.ls, 1e-30, 0.0)
    with pytest.raises(NotPositiveDefiniteError):
        eng.set_data(X2, b.Y)
    with pytest.raises(RuntimeError):
        eng.predict(b.Xq)  # a failed update leaves the model unusable until the next good one
    T.put(eng, b)
    _same(T.battery(eng, b), _fresh(M4, "B", variant), "B after a failed update")


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@VARIANTS
def test_trial_evaluations_in_between(variant):
    """Two tgp_nlml_trial evaluations at far-away hyper-parameters on a handle holding A: from Npad = 512 on the trial
    builds the factor only, so d_W and Wt (d_A, overwritten by K) stay from another model than d_L.  The values match the
    oracle; the handle has no posterior until the next set_data, which must leave nothing of the trials behind."""
    a = T.state(M4, "A")
    eng = T.engine(a, variant)
    for scale, noise in ((5.0, 0.3), (0.2, 1e-5)):
        eng.set_hyper(a.variance * scale, a.ls * scale, noise, a.c - 1.0)
        val = eng.nlml_trial()
        want = O.nlml_and_grad(O.gpr_update(a.kind, a.variance * scale, a.ls * scale, noise, a.c - 1.0, a.X, a.Y))[0]
        assert_close(val, want, rtol=1e-9, atol=1e-7, what="nlml_trial vs oracle")
        with pytest.raises(RuntimeError):
            eng.predict(a.Xq)
    T.put(eng, a)
    _same(T.battery(eng, a), _fresh(M4, "A", variant), "A after trial evaluations")


# ---- 4 ---------------------------------------------------------------------------------------------------------------
@VARIANTS
def test_batched_trials_on_the_shared_scratch(variant):
    """tgp_nlml_trial_batch keeps its members' K / L / W in a PROCESS-WIDE scratch wiped once per (pointer, Npad, member
    count): three members at N = 500, three at N = 300 from another handle (same Npad, no wipe: A's rows are padding now),
    five (a larger scratch), three at N = 500 again.  Every value is tgp_nlml_trial's of a single fresh handle bit for bit
    (the contract of include/tgp.h) and the calling handle's own posterior is untouched.  C (Npad = 256) takes the
    sequential fallback on the handle itself, which restores the posterior by refactorising."""
    st = {n: T.state(M4, n) for n in "ABC"}
    h = {n: T.engine(st[n], variant) for n in "ABC"}
    for n, B in (("A", 3), ("B", 3), ("B", 5), ("A", 5), ("A", 3), ("C", 3), ("C", 5), ("B", 3)):
        vals, ok = h[n].nlml_trial_batch(T.trial_hypers(st[n])[:B])
        assert np.all(ok)
        np.testing.assert_array_equal(vals, _single_trials(M4, n, variant)[:B], err_msg=f"{B} members on {n}")
    for n in "ABC":
        _same(T.battery(h[n], st[n]), _fresh(M4, n, variant), f"{n} after batched trials")


# ---- 5 ---------------------------------------------------------------------------------------------------------------
@VARIANTS
def test_append_then_replace(variant):
    """B + 1 + 7 + 70 appended rows (stays in Npad = 512, crosses the 64-row blocks at 320 and 384): the rank-k path
    rewrites only the trailing strip of L / W.  An appended factor is NOT bit-equal to a refit, so after each append it is
    held to the tolerances of test_append_data_equals_full_refactorisation against the oracle and a full refit; the two
    set_data that follow (C: a new Npad; B: back into buffers that held 378 rows) must give a fresh handle's bits."""
    b, c = T.state(M4, "B"), T.state(M4, "C")
    eng = T.engine(b, variant)
    rng = np.random.default_rng(23)
    floor = cancellation_floor(b.N + 80, b.variance, b.noise)
    Xall, Yall = b.X, b.Y
    for k in (1, 7, 70):
        Xn, Yn = rng.uniform(size=(k, b.d)), rng.standard_normal(k) * 0.3 + b.c
        eng.append_data(Xn, Yn)
        Xall, Yall = np.concatenate([Xall, Xn]), np.concatenate([Yall, Yn])
        assert eng.N == Xall.shape[0]
        full = T.engine(b, variant, data=False)
        full.set_data(Xall, Yall)
        sto = O.gpr_update(b.kind, b.variance, b.ls, b.noise, b.c, Xall, Yall)
        (La, _, aa), (Lf, _, af) = eng.get_factor(), full.get_factor()
        assert_close(La, sto.L, atol=floor, what=f"L after append k={k}")
        assert_close(La, Lf, rtol=1e-9, atol=floor, what="L append == full")
        ascale = max(1.0, np.abs(af).max())
        assert_close(aa, af, rtol=1e-7, atol=floor * ascale / min(b.noise, 1.0), what="alpha append == full")
        ma, va = eng.predict(b.Xq)
        mo, vo = O.predict(sto, b.Xq)
        assert_close(ma, mo, atol=floor, what="mean after append")
        assert_close(va, vo, atol=floor, what="var after append")
        assert_close(eng.eta(), O.eta_min_mean(sto), atol=floor, what="eta after append")
        full.close()
    T.put(eng, c)
    _same(T.battery(eng, c), _fresh(M4, "C", variant), "C after appends")
    T.put(eng, b)
    _same(T.battery(eng, b), _fresh(M4, "B", variant), "B after appends and C")


# ---- 6 ---------------------------------------------------------------------------------------------------------------
@VARIANTS
def test_clone_into_used_handles(variant):
    """tgp_clone_from into a handle that held D (larger buffers: the copy lands in the front of them) and into one that
    held C (smaller: reallocated), with the wipe-once bookkeeping carried along.  The clone answers with the source's
    bits; afterwards the two are independent: set_data(B) on the source leaves the clone alone, an append to the clone
    leaves the source alone."""
    a, b = T.state(M4, "A"), T.state(M4, "B")
    src = T.engine(a, variant)
    clones = [T.engine(T.state(M4, n), variant) for n in "DC"]
    for cl in clones:
        T.battery(cl, T.state(M4, "D" if cl is clones[0] else "C"))  # their scratch has been used at their own size
        cl.clone_from(src)
        _same(T.battery(cl, a), _fresh(M4, "A", variant), "clone of A")
    _same(T.battery(src, a), _fresh(M4, "A", variant), "the source after being cloned")
    T.put(src, b)
    for cl in clones:
        _same(T.battery(cl, a), _fresh(M4, "A", variant), "clone of A after the source moved to B")
    rng = np.random.default_rng(5)
    for cl in clones:
        cl.append_data(rng.uniform(size=(5, a.d)), rng.standard_normal(5))
    _same(T.battery(src, b), _fresh(M4, "B", variant), "the source after its clones were appended to")
    # and a clone of the smaller model into a handle whose buffers hold the larger one's rows
    clones[0].clone_from(src)
    _same(T.battery(clones[0], b), _fresh(M4, "B", variant), "clone of B into buffers that held A + 5 rows")


# ---- 7 ---------------------------------------------------------------------------------------------------------------
def _scratch_calls(s, large: bool):
    from trieste_amd import engine as E

    rng = np.random.default_rng(1234 + large)
    d = s.d
    M, q, S, G, qb = (5000, 50, 512, 8, 16) if large else (65, 3, 8, 8, 2)
    Xp = rng.uniform(size=(M, d))
    Xg, eps = rng.uniform(size=(G, q, d)), rng.standard_normal((q, S))
    Xb, w1, w2 = rng.uniform(size=(G, qb, d)), rng.uniform(size=(64, qb)), rng.uniform(size=(64, qb - 1))
    eta = float(np.median(s.Y))
    return [("predict", lambda e: np.stack(e.predict(Xp))), ("qei", lambda e: e.qei(Xg, eps, eta)),
            ("batch_ei", lambda e: E.batch_ei(e, Xb, w1, w2, eta))]


@VARIANTS
def test_scratch_order_large_then_small_and_back(variant):
    """Every s_* scratch buffer only grows.  Large calls (M = 5000; qEI at q = 50, S = 512; batch EI at q = 16) and then
    small ones (M = 65; q = 3, S = 8; q = 2) on one handle: each small call must equal the same call as the FIRST call of
    a fresh handle -- a launch geometry or a reduction that looked at capacity instead of size would show here -- and the
    reverse order must reproduce the large ones."""
    a = T.state(M4, "A")
    big, small = _scratch_calls(a, True), _scratch_calls(a, False)
    first = {}
    for name, call in small + [("L" + n, c) for n, c in big]:
        eng = T.engine(a, variant)
        first[name] = np.array(call(eng))
        eng.close()
    eng = T.engine(a, variant)
    for name, call in big:
        np.testing.assert_array_equal(call(eng), first["L" + name], err_msg=f"large {name}")
    for name, call in small:
        np.testing.assert_array_equal(call(eng), first[name], err_msg=f"small {name} after large")
    _same(T.battery(eng, a), _fresh(M4, "A", variant), "battery after large and small calls")
    rev = T.engine(a, variant)
    for name, call in small:
        np.testing.assert_array_equal(call(rev), first[name], err_msg=f"small {name} first")
    for name, call in big:
        np.testing.assert_array_equal(call(rev), first["L" + name], err_msg=f"large {name} after small")
    _same(T.battery(rev, a), _fresh(M4, "A", variant), "battery after small and large calls")


# ---- 8 ---------------------------------------------------------------------------------------------------------------
def _sweep(eng, s):
    m, v = eng.predict(s.Xq)
    eta = eng.eta()
    val, idx, x = eng.acq_argmax("ei", eta, s.Xq)
    return dict(mean=np.array(m), var=np.array(v), ei=np.array(eng.acq_values("ei", eta, s.Xq)),
                argmax=np.concatenate([[val, float(idx)], x]))


@pytest.mark.parametrize("precision", ["i8x4", "i8x5"])
def test_int8_planes_follow_the_model(precision):
    """The int8 digit planes of W are built lazily and cached per (data_version, plane count).  A handle that has swept A
    at this precision -- planes cached -- is given B (set_data), five more rows (append) and, as the TARGET of a clone,
    another handle's model: each time the sweep must run on planes of the current factor.  After set_data: the bits of a
    fresh handle at this precision.  After the append: the bits of a clone of the appended handle (the clone copies the
    factor exactly; a refit would not) made INTO a handle with cached planes of its own, and inside the int8 parity
    tolerance of tests/test_gpu_i8.py against the same handle's float64 sweep."""
    a, b = T.state(M4, "A"), T.state(M4, "B")
    eng = T.engine(a, precision=precision)
    fresh_a = _sweep(eng, a)
    T.put(eng, b)
    fresh = T.engine(b, precision=precision)
    _same(_sweep(eng, b), _sweep(fresh, b), f"{precision}: B after A")
    rng = np.random.default_rng(8)
    eng.append_data(rng.uniform(size=(5, b.d)), rng.standard_normal(5) * 0.3 + b.c)
    got = _sweep(eng, b)
    used = T.engine(a, precision=precision)
    _same(_sweep(used, a), fresh_a, f"{precision}: a second handle at A")  # (its planes of A are cached now)
    used.clone_from(eng)
    _same(_sweep(used, b), got, f"{precision}: clone of the appended handle into a handle with cached planes")
    floor = cancellation_floor(eng.N, b.variance, b.noise)
    budget = i8x4_variance_bound(eng.N, b.variance, np.abs(eng.get_factor()[1]).max()) if precision == "i8x4" else 0.0
    eng.set_precision("f64")
    f64 = _sweep(eng, b)
    assert_close(got["var"], f64["var"], atol=floor + budget, what=f"{precision} var vs float64 after append")
    np.testing.assert_allclose(got["mean"], f64["mean"], rtol=1e-12, atol=1e-12)   # the mean never leaves float64
    assert_close(got["ei"], f64["ei"], atol=floor * 10 + budget, what=f"{precision} ei vs float64 after append")
    eng.set_precision(precision)
    _same(_sweep(eng, b), got, f"{precision}: back from float64")
    # shrinking set_data on the clone target, whose planes were built for 305 rows
    T.put(used, T.state(M4, "C"))
    fresh_c = T.engine(T.state(M4, "C"), precision=precision)
    _same(_sweep(used, T.state(M4, "C")), _sweep(fresh_c, T.state(M4, "C")), f"{precision}: C after the clone")


def test_auto_precision_holds_the_plain_tolerance_across_transitions():
    """TGP_PREC_AUTO is history-dependent by design (the ladder keeps its rung), so there is no bitwise claim: after every
    transition mean, variance and EI hold the PLAIN parity tolerance against the oracle, as
    test_auto_precision_stays_inside_the_plain_tolerance asserts for a handle without a history."""
    a, b = T.state(M4, "A"), T.state(M4, "B")

    def check(eng, X, Y, Xq, what):
        st = O.gpr_update(a.kind, a.variance, a.ls, a.noise, a.c, X, Y)
        floor = cancellation_floor(X.shape[0], a.variance, a.noise)
        om, ov = O.predict(st, Xq)
        mean, var = eng.predict(Xq)
        assert_close(var, ov, atol=floor, what=f"var under auto, {what}")
        assert_close(mean, om, atol=floor * 10, what=f"mean under auto, {what}")
        eta = eng.eta()
        assert_close(eng.acq_values("ei", eta, Xq), O.expected_improvement(om, ov, eta), atol=floor,
                     what=f"ei under auto, {what}")

    eng = T.engine(a, precision="auto")
    check(eng, a.X, a.Y, a.Xq, "A")
    T.put(eng, b)
    check(eng, b.X, b.Y, b.Xq, "B after A")
    rng = np.random.default_rng(8)
    Xn, Yn = rng.uniform(size=(5, b.d)), rng.standard_normal(5) * 0.3 + b.c
    eng.append_data(Xn, Yn)
    Xall, Yall = np.concatenate([b.X, Xn]), np.concatenate([b.Y, Yn])
    check(eng, Xall, Yall, b.Xq, "B + 5 rows")
    used = T.engine(a, precision="auto")
    check(used, a.X, a.Y, a.Xq, "a second handle at A")
    used.clone_from(eng)
    check(used, Xall, Yall, b.Xq, "clone of B + 5 rows into a used handle")
    T.put(used, T.state(M4, "C"))
    check(used, T.state(M4, "C").X, T.state(M4, "C").Y, T.state(M4, "C").Xq, "C after the clone")


# ---- 9 ---------------------------------------------------------------------------------------------------------------
def _traj_calls(t, s, decoupled):
    import torch

    Xb = np.random.default_rng(2).uniform(size=(6, t.B, s.d))
    dev = torch.as_tensor(s.Xq).cuda()
    return [lambda: t(s.Xq), lambda: t(Xb), lambda: t.value_and_gradient(Xb), lambda: t.argmin(s.Xq),
            lambda: t.argmin_pairs(dev), (lambda: t.v()) if decoupled else (lambda: t.theta())]


STALE_OPS = ["append", "set_data_larger", "set_data_smaller", "set_hyper_same_data", "nlml_trial", "clone_from"]


@pytest.mark.parametrize("op", STALE_OPS)
def test_stale_trajectories_are_refused(op):
    """A trajectory's weights are solved for -- and sized by -- the model at its creation, while its kernels walk the
    handle's CURRENT N, inputs and lengthscales: after the model is replaced every tgp_traj_* call must refuse (with more
    rows it would read past the weights, with fewer or other hyper-parameters return neither posterior's draw).  The
    refusal leaves no sticky error, and a trajectory drawn afterwards matches the oracle at the tolerances of
    test_trajectories_match_oracle_and_argmin."""
    a, b, c = (T.state(M4, n) for n in "ABC")
    eng = T.engine(b)
    W, bb, w, xi, eps = T.traj_draws(b)
    td, tr = eng.trajectory(W, bb, w, xi), eng.trajectory_rff(W, bb, eps)
    for call in _traj_calls(td, b, True) + _traj_calls(tr, b, False):
        call()  # every entry answers while the model stands
    rng = np.random.default_rng(9)
    X, Y, hyper = b.X, b.Y, (b.variance, b.ls, b.noise, b.c)
    if op == "append":
        Xn, Yn = rng.uniform(size=(1, b.d)), np.array([b.c])
        eng.append_data(Xn, Yn)
        X, Y = np.concatenate([X, Xn]), np.concatenate([Y, Yn])
    elif op == "set_data_larger":
        eng.set_data(a.X, a.Y)
        X, Y = a.X, a.Y
    elif op == "set_data_smaller":
        eng.set_data(c.X, c.Y)
        X, Y = c.X, c.Y
    elif op == "set_hyper_same_data":
        eng.set_hyper(*hyper)
        for call in _traj_calls(td, b, True) + _traj_calls(tr, b, False):
            with pytest.raises(RuntimeError, match="stale trajectory"):
                call()  # no posterior at all in between
        eng.set_data(b.X, b.Y)
    elif op == "nlml_trial":
        eng.nlml_trial()
    else:
        other = T.engine(a)
        eng.clone_from(other)
        X, Y = a.X, a.Y
    for call in _traj_calls(td, b, True) + _traj_calls(tr, b, False):
        with pytest.raises(RuntimeError, match="stale trajectory"):
            call()
    if op == "nlml_trial":
        eng.set_data(b.X, b.Y)  # (a trial leaves no posterior: the next ordinary call is the update)
    mean, var = eng.predict(b.Xq)  # no sticky error
    st = O.gpr_update(b.kind, *hyper, X, Y)
    floor = cancellation_floor(X.shape[0], b.variance, b.noise)
    assert_close(mean, O.predict(st, b.Xq)[0], atol=floor * 10, what="mean after the refusals")
    W, bb, w, xi, eps = T.traj_draws(b, N=X.shape[0])
    t2 = eng.trajectory(W, bb, w, xi)
    ov = O.decoupled_weights(st, W, bb, w, xi)
    vs = np.abs(ov).max()
    assert_close(t2.v(), ov, rtol=1e-5, atol=1e-7 * vs, what="v of a trajectory drawn afterwards")
    assert_close(t2(b.Xq), O.trajectory_eval(st, W, bb, w, t2.v(), b.Xq), rtol=1e-5, atol=1e-8 * max(1.0, vs),
                 what="a trajectory drawn afterwards")
    for call in _traj_calls(td, b, True)[:1] + _traj_calls(tr, b, False)[:1]:
        with pytest.raises(RuntimeError, match="stale trajectory"):
            call()  # the old ones stay refused


@pytest.mark.parametrize("name", ["B", "C"])
def test_trajectories_live_across_batched_trials(name):
    """tgp_nlml_trial_batch promises an untouched posterior: at N = 300 the members live in scratch, at N = 130 the handle
    itself evaluates them and then reproduces its factor -- bit for bit, so the factorisation keeps its stamp and a
    trajectory drawn before the call answers with the same bits after it."""
    s = T.state(M4, name)
    eng = T.engine(s)
    W, b, w, xi, eps = T.traj_draws(s)
    trajs = [(eng.trajectory(W, b, w, xi), True), (eng.trajectory_rff(W, b, eps), False)]

    def answers():  # eval (shared and per-trajectory inputs), value-and-gradient, arg-min, the weights
        return [np.array(x.cpu().numpy() if hasattr(x, "cpu") else x) for t, dec in trajs for call in _traj_calls(t, s, dec)
                for r in [call()] for x in (r if isinstance(r, tuple) else (r,))]

    before = answers()
    assert len(before) == 2 * 8
    vals, ok = eng.nlml_trial_batch(T.trial_hypers(s)[:3])
    assert np.all(ok)
    np.testing.assert_array_equal(vals, _single_trials(M4, name, 0)[:3])
    for got, want in zip(answers(), before):
        np.testing.assert_array_equal(got, want)
    _same(T.battery(eng, s), _fresh(M4, name, 0), f"{name} after batched trials with live trajectories")


def test_stale_trajectories_are_refused_through_a_group_of_one():
    """tgp_group_traj_argmin inherits the rule through its members and reports the member's refusal."""
    from trieste_amd.group import GPEngineGroup

    a, b = T.state(M4, "A"), T.state(M4, "B")
    grp = GPEngineGroup(b.d, b.kind, devices=[0])
    try:
        grp.set_hyper(b.variance, b.ls, b.noise, b.c)
        grp.set_data(b.X, b.Y)
        grp.set_candidates(b.Xq)
        W, bb, w, xi, _ = T.traj_draws(b)
        gt = grp.trajectory(W, bb, w, xi)
        vals, idx = gt.argmin()
        eng = T.engine(b)
        ev, ei = eng.trajectory(W, bb, w, xi).argmin(b.Xq)
        np.testing.assert_array_equal(idx, ei)
        np.testing.assert_array_equal(vals, ev)
        grp.append_data(np.full((1, b.d), 0.5), np.array([b.c]))
        with pytest.raises(RuntimeError, match="stale trajectory"):
            gt.argmin()
        grp.set_data(a.X, a.Y)
        with pytest.raises(RuntimeError, match="stale trajectory"):
            gt.argmin()
        val, gidx, _ = grp.acq_argmax("ei", grp.eta())  # the group's next ordinary call succeeds
        assert (val, gidx) == T.engine(a).acq_argmax("ei", grp.eta(), b.Xq)[:2]
        W, bb, w, xi, _ = T.traj_draws(a)
        v2, i2 = grp.trajectory(W, bb, w, xi).argmin()
        e2, j2 = T.engine(a).trajectory(W, bb, w, xi).argmin(b.Xq)
        np.testing.assert_array_equal(i2, j2)
        np.testing.assert_array_equal(v2, e2)
    finally:
        grp.close()


# ---- 10 --------------------------------------------------------------------------------------------------------------
def test_settings_persist_across_set_data_and_clear_completely():
    """Penalisation, min-value samples and the repulsion twin are settings of the HANDLE, not of the model: set on A, they
    still apply after set_data(B) -- with the bits of a fresh B handle given the same settings -- and the low-rank twin
    check, cached per (data version, twin version) and true for A (the twin is A + 4 rows), must be taken again for B.
    After clearing them plain EI has the bits of a handle that never had them."""
    a, b = T.state(M4, "A"), T.state(M4, "B")
    rng = np.random.default_rng(13)
    pending, r, sc = rng.uniform(size=(4, a.d)), rng.uniform(0.1, 0.3, 4), rng.uniform(0.05, 0.2, 4)
    eng = T.engine(a)
    twin = eng.clone()
    twin.append_data(pending, np.full(4, a.c))
    samples = float(np.min(b.Y)) - np.array([0.01, 0.05, 0.2, 0.35, 0.6])

    def settings(e):
        e.set_penalization("soft", pending, r, sc)
        e.set_min_value_samples(samples)
        e.set_repulsion(twin, 1.0 / 16.0)

    def queries(e, s):
        eta = e.eta()
        return {acq: np.array(e.acq_values(acq, 0.0 if acq != "ei" else eta, s.Xq)) for acq in ("ei", "mes", "gibbon")}

    settings(eng)
    on_a = queries(eng, a)  # (takes the low-rank path for the twin: it IS A + 4 rows)
    plain_a = _fresh(M4, "A", 0)
    assert not np.array_equal(on_a["ei"], plain_a["acq.ei"])
    T.put(eng, b)
    fresh = T.engine(b)
    settings(fresh)
    _same(queries(eng, b), queries(fresh, b), "settings made on A, queried on B")
    pen = O.soft_local_penalizer(b.Xq, pending, r, sc)
    assert_close(queries(eng, b)["ei"], _fresh(M4, "B", 0)["acq.ei"] * pen, rtol=1e-11, atol=1e-300, what="penalised ei")
    eng.set_penalization("none")
    eng.set_min_value_samples([])
    eng.set_repulsion(None)
    np.testing.assert_array_equal(eng.acq_values("ei", eng.eta(), b.Xq), _fresh(M4, "B", 0)["acq.ei"])
    with pytest.raises(RuntimeError):
        eng.acq_values("mes", 0.0, b.Xq)  # no min-value samples any more
    _same(T.battery(eng, b), _fresh(M4, "B", 0), "B after the settings were cleared")


# ---- poisoned allocations --------------------------------------------------------------------------------------------
def test_tour_under_poisoned_allocations():
    """TGP_POISON=1 fills every fresh device allocation of the library with NaNs, so a read of memory the engine did not
    write cannot hide behind whatever the allocator recycled.  The variable is read once per process: the tour of
    tests/history_tour.py runs in a fresh child process under it and here, unpoisoned; every array must be finite where
    the unpoisoned one is, and bit-equal.  The child's timeout is a safety cap (the tour takes a few seconds); a child
    that hangs or dies on a signal ends the whole session, so that nothing else is started on a GPU that has just faulted."""
    import tempfile

    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "tour.npz")
        env = dict(os.environ, TGP_POISON="1")
        try:
            child = subprocess.run([sys.executable, "-m", "tests.history_tour", out], env=env, cwd=ROOT, timeout=120,
                                   capture_output=True, text=True)
        except subprocess.TimeoutExpired as e:  # a hang on the GPU: nothing else is started on it in this session
            pytest.exit(f"the poisoned tour hung (120 s cap); stderr:\n{(e.stderr or b'')[-4000:]}", returncode=1)
        if child.returncode < 0 or child.returncode in (134, 139):  # killed by a signal: a GPU fault or an abort
            pytest.exit(f"the poisoned tour died with {child.returncode}; stderr:\n{child.stderr[-4000:]}", returncode=1)
        assert child.returncode == 0, f"poisoned tour exited with {child.returncode}:\n{child.stderr[-4000:]}"
        print(child.stdout.strip())
        with np.load(out) as z:
            poisoned = {k: z[k] for k in z.files}
    plain = T.tour()
    assert sorted(poisoned) == sorted(plain)
    for k, want in plain.items():
        got = poisoned[k]
        if want.dtype.kind == "f":
            assert np.all(np.isfinite(got) | ~np.isfinite(want)), f"{k}: not finite under poisoned allocations"
        np.testing.assert_array_equal(got, want, err_msg=k)
    # and the tour itself: every chain step / every handle after the batched trials has its fresh handle's bits
    for k, want in plain.items():
        head, where, query = k.split(".", 2) if k.count(".") >= 2 else (k, "", "")
        name = where[-1:] if head == "chain" else where
        if head in ("chain", "after_trials") and f"fresh.{name}.{query}" in plain:  # (the tour has no fresh D)
            np.testing.assert_array_equal(want, plain[f"fresh.{name}.{query}"], err_msg=k)
