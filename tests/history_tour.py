"""TEST INFRASTRUCTURE of tests/test_gpu_history.py: the states, the battery of queries and a fixed tour through them.

The property under test is the README's: an answer is a pure function of (model, inputs).  So after ANY sequence of calls a
handle must answer every query with exactly the bits of a fresh handle that was given the final model directly -- whatever
its grow-only buffers, its wiped-once factor matrices, the process-wide scratch of the batched trial evaluations or its
cached derived state held before.  ``battery`` is the fixed set of queries; its inputs come from a seed and the state's
data, never from the handle.

Run as a module (``python -m tests.history_tour OUT.npz``) it walks a fixed tour -- fresh handles at A, B, C, the chain
A -> B -> C -> D -> A -> B on one handle, batched trial evaluations on the shared scratch -- and writes every array to
OUT.npz.  tests/test_gpu_history.py runs it in a child process under TGP_POISON=1 (fresh device allocations filled with
NaNs; the variable is read once per process) and compares with an unpoisoned run bit for bit.
"""
from __future__ import annotations

import functools
import sys
import time

import numpy as np

from oracle import gp_oracle as O

# Sizes by the engine's own constants (NPAD_MULT = 256, LEAF = 64, the persistent update from Npad = 512):
#   A 500 -> Npad 512 (persistent); B 300 -> 512 (persistent: shrinks IN PLACE inside A's buffers, no fresh wipe);
#   C 130 -> 256 (the recursion); D 700 -> 768 (grows: new buffers)
SIZES = dict(A=500, B=300, C=130, D=700)
SEEDS = dict(A=11, B=22, C=33, D=44)
MODELS = dict(m52_d4=(4, "matern52"), rbf_d6=(6, "rbf"))
VARIANCE, NOISE, MEAN_C = 1.3, 1e-3, 0.2
NO_DAG = 16  # tgp_set_variant bit 4: `update` through the recursion of dependent launches at every size
ACQS = ("ei", "pi", "nlcb", "aei", "mes", "gibbon")
CHAIN = "ABCDAB"


class State:
    """One model state: data, hyper-parameters, candidates."""


@functools.lru_cache(maxsize=None)
def state(model: str, name: str) -> State:
    d, kind = MODELS[model]
    N = SIZES[name]
    rng = np.random.default_rng(SEEDS[name] + 1000 * d)
    s = State()
    s.model, s.name, s.d, s.kind, s.N = model, name, d, kind, N
    s.X = rng.uniform(size=(N, d))
    f = O.ackley(s.X)
    s.Y = np.sqrt(VARIANCE) * (f - f.mean()) / f.std() + MEAN_C
    s.variance, s.noise, s.c = VARIANCE, NOISE, MEAN_C
    # ARD lengthscales over a decade, the shortest not at index 0 (tests/test_gpu_general.py); the same for every state
    s.ls = 0.2 * np.sqrt(d) * np.random.default_rng(7 + d).permutation(np.geomspace(0.35, 3.5, d))
    if int(np.argmin(s.ls)) == 0:
        s.ls = s.ls[::-1].copy()
    q = np.random.default_rng(5678)
    Xq = q.uniform(size=(1500, d))
    Xq[:5] = s.X[:5]                          # exactly at training inputs (variance cancellation)
    Xq[5] = Xq[6]                             # a duplicate (ties -> first index)
    Xq[-3:] = 4.0 + q.uniform(size=(3, d))    # far field
    s.Xq = np.ascontiguousarray(Xq)
    return s


def oracle_state(s: State):
    if not hasattr(s, "st"):
        s.st = O.gpr_update(s.kind, s.variance, s.ls, s.noise, s.c, s.X, s.Y)
    return s.st


def engine(s: State, variant: int = 0, precision: str = "f64", data: bool = True):
    from trieste_amd.engine import GPEngine

    eng = GPEngine(s.d, s.kind)
    eng.set_variant(variant)
    if precision != "f64":
        eng.set_precision(precision)
    eng.set_hyper(s.variance, s.ls, s.noise, s.c)
    if data:
        eng.set_data(s.X, s.Y)
    return eng


def put(eng, s: State) -> None:
    """The state on a handle that may hold anything."""
    eng.set_hyper(s.variance, s.ls, s.noise, s.c)
    eng.set_data(s.X, s.Y)


def traj_draws(s: State, N: int = None, F: int = 64, B: int = 3):
    """The draws of the battery's trajectories: RFF basis, prior weights, noise draws, RFF-posterior draws."""
    from trieste_amd.sampler import sample_rff_basis

    rng = np.random.default_rng(64)
    W, b = sample_rff_basis(s.kind, F, s.d, rng)
    return W, b, rng.standard_normal((F, B)), rng.standard_normal((s.N if N is None else N, B)), rng.standard_normal((F, B))


def inputs(s: State):
    """The battery's inputs: a function of a seed and the state's data, never of the handle."""
    if hasattr(s, "inp"):
        return s.inp
    rng = np.random.default_rng(99)
    d = s.d
    i = State()
    i.near = np.clip(s.X[np.argsort(s.Y)[:9]] + 0.03 * rng.standard_normal((9, d)), 0.0, 1.0)  # P = 9 gradient points
    i.near[0] = s.X[np.argmin(s.Y)]
    i.Xg = rng.uniform(size=(40, 5, d))                    # G = 40 batches of q = 5
    i.Xg[0, 0] = s.X[0]
    i.eps = rng.standard_normal((5, 64))                   # S = 64
    i.X4 = np.ascontiguousarray(i.Xg[:, :4])               # batch EI: q = 4
    i.w1, i.w2 = rng.uniform(size=(64, 4)), rng.uniform(size=(64, 3))
    i.eps_joint = rng.standard_normal((33, 4))             # sample_joint: n = 33, S = 4
    i.pending, i.radius, i.scale = rng.uniform(size=(3, d)), rng.uniform(0.1, 0.3, 3), rng.uniform(0.05, 0.2, 3)
    i.Xb = rng.uniform(size=(11, 3, d))                    # per-trajectory points
    i.eta_mid = float(np.median(s.Y))                      # an incumbent that leaves most batches an improvement
    s.inp = i
    return i


def battery(eng, s: State) -> dict:
    """Every query kind once, with fixed inputs -> {name: array}.  Leaves no setting behind on the handle."""
    from trieste_amd import engine as E

    out = {}
    i = inputs(s)
    Xq, X7 = s.Xq, np.ascontiguousarray(s.Xq[:7])
    out["L"], out["W"], out["alpha"] = eng.get_factor()
    for tag, x in (("", Xq), ("7", X7)):
        out["mean" + tag], out["var" + tag] = eng.predict(x)
        out["predict_mean" + tag] = eng.predict_mean(x)
    eta = eng.eta()
    out["eta"] = np.array(eta)
    eng.set_min_value_samples(eta - np.array([0.01, 0.05, 0.2, 0.35, 0.6]))
    param = lambda acq: 1.96 if acq == "nlcb" else (0.0 if acq in ("mes", "gibbon") else eta)
    for acq in ACQS:
        out["acq." + acq] = eng.acq_values(acq, param(acq), Xq)
        out["acq7." + acq] = eng.acq_values(acq, param(acq), X7)
    for acq in ("ei", "mes", "gibbon"):
        val, idx, x = eng.acq_argmax(acq, param(acq), Xq)
        out["argmax." + acq] = np.concatenate([[val, float(idx)], x])
        out["topk.v." + acq], out["topk.i." + acq] = eng.acq_topk(acq, param(acq), Xq, 17)
        out["grad.v." + acq], out["grad.g." + acq] = eng.acq_value_grad(acq, param(acq), i.near)
    eng.set_min_value_samples([])
    out["joint.mean"], out["joint.cov"] = eng.predict_joint(i.Xg)
    out["qei"] = eng.qei(i.Xg, i.eps, i.eta_mid)
    out["qei.v"], out["qei.g"] = eng.qei_value_grad(i.Xg, i.eps, i.eta_mid)
    out["reparam"] = eng.reparam_samples(i.Xg, i.eps)
    out["bei"] = E.batch_ei(eng, i.X4, i.w1, i.w2, i.eta_mid)
    out["bei.v"], out["bei.g"] = E.batch_ei_value_grad(eng, i.X4, i.w1, i.w2, i.eta_mid)
    out["cov"] = eng.cov_between(Xq[:9], Xq[9:20])
    out["sample_joint"] = eng.sample_joint(Xq[20:53], i.eps_joint)
    val, grad = eng.nlml()
    out["nlml"], out["nlml.g"] = np.array(val), grad
    for kind in ("soft", "hard"):
        eng.set_penalization(kind, i.pending, i.radius, i.scale)
        out["pen." + kind] = eng.acq_values("ei", eta, Xq)
        eng.set_penalization("none")
    out["pen.cleared"] = eng.acq_values("ei", eta, Xq)
    W, b, w, xi, eps_t = traj_draws(s)
    for tag, t in (("traj", eng.trajectory(W, b, w, xi)), ("rff", eng.trajectory_rff(W, b, eps_t))):
        out[tag + ".w"] = t.v() if tag == "traj" else t.theta()
        out[tag + ".eval"] = t(Xq)
        out[tag + ".eval_b"] = t(i.Xb)
        out[tag + ".argmin.v"], out[tag + ".argmin.i"] = t.argmin(Xq)
        out[tag + ".vg.v"], out[tag + ".vg.g"] = t.value_and_gradient(i.Xb)
        t.close()
    return {k: np.array(v) for k, v in out.items()}


def trial_hypers(s: State, B: int = 5) -> np.ndarray:
    """B members (variance, lengthscales, noise, mean) around the state's own hyper-parameters."""
    rng = np.random.default_rng(3)
    rows = []
    for b in range(B):
        rows.append(np.concatenate([[s.variance * (0.5 + 0.4 * b)], s.ls * rng.uniform(0.7, 1.4, size=s.d),
                                    [s.noise * (1 + b), s.c + 0.25 * b]]))
    return np.array(rows)


def single_trials(s: State, variant: int = 0) -> np.ndarray:
    """tgp_nlml_trial of ONE fresh handle at every member of ``trial_hypers``: what tgp_nlml_trial_batch must return."""
    eng = engine(s, variant)
    vals = []
    for row in trial_hypers(s):
        eng.set_hyper(row[0], row[1:1 + s.d], row[1 + s.d], row[2 + s.d])
        vals.append(eng.nlml_trial())
    eng.close()
    return np.array(vals)


def tour(model: str = "m52_d4") -> dict:
    """Fresh handles at A, B, C; the set_data chain on one handle; batched trials on the shared scratch -> flat dict."""
    res = {}
    st = {n: state(model, n) for n in SIZES}
    for n in "ABC":
        eng = engine(st[n])
        res.update({f"fresh.{n}.{k}": v for k, v in battery(eng, st[n]).items()})
        eng.close()
    eng = engine(st["A"], data=False)
    for i, n in enumerate(CHAIN):
        put(eng, st[n])
        res.update({f"chain.{i}{n}.{k}": v for k, v in battery(eng, st[n]).items()})
    hA = engine(st["A"])
    for tag, n, B, h in (("a3", "A", 3, hA), ("b3", "B", 3, eng), ("b5", "B", 5, eng), ("a3again", "A", 3, hA)):
        vals, ok = h.nlml_trial_batch(trial_hypers(st[n])[:B])
        res[f"trials.{tag}"], res[f"trials.{tag}.ok"] = vals, ok
    res.update({f"after_trials.A.{k}": v for k, v in battery(hA, st["A"]).items()})
    hC = engine(st["C"])
    res["trials.c3"], res["trials.c3.ok"] = hC.nlml_trial_batch(trial_hypers(st["C"])[:3])
    res.update({f"after_trials.C.{k}": v for k, v in battery(hC, st["C"]).items()})
    for h in (eng, hA, hC):
        h.close()
    return res


if __name__ == "__main__":
    t0 = time.perf_counter()
    arrays = tour()
    np.savez(sys.argv[1], **arrays)
    print(f"history tour: {len(arrays)} arrays in {time.perf_counter() - t0:.2f} s")
