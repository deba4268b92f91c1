"""A short tour of the integrated-variance-reduction entry points whose arrays must not depend on a handle's history or on what
device memory held before (TEST INFRASTRUCTURE): tests/test_gpu_ivr.py runs it in process and, as
``python -m tests.ivr_tour out.npz``, in a child process under TGP_POISON=1, and compares the arrays bit for bit.

Per model: a handle that had integration points and a call BEFORE its data changed (append_data; set_hyper + set_data) against
a fresh handle given the final model and the same points."""
import sys

import numpy as np


def problem(seed, N, d):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N, d))
    Y = np.sin(3.0 * X @ rng.uniform(0.5, 1.5, d)) + 0.05 * rng.standard_normal(N)
    return rng, X, Y


def tour():
    from trieste_amd import engine as E

    out = {}
    for name, kernel, N, d, P, q in (("small", "matern52", 40, 2, 70, 3), ("two-tiles", "rbf", 300, 5, 130, 16), ("q1", "matern32", 257, 3, 1, 1)):
        rng, X, Y = problem(31 + N, N + 7, d)
        Z, w = rng.uniform(size=(P, d)), rng.uniform(size=P)
        if P > 1:
            w[-1] = 0.0   # an exact zero in the last partial tile
        Xq =rng.uniform(size=(2048 // q + 3, q, d))   # two chunks, the second partial
        ls = rng.uniform(0.3, 0.8, d)
        eng = E.GPEngine(d, kernel, device=0)
        eng.set_hyper(1.0, ls, 1e-3, 0.1)
        eng.set_data(X[:N], Y[:N])
        E.set_integration_points(eng, Z, w)
        v0, r0 = E.ivr_values(eng, Xq, with_reduction=True)
        out[f"{name} first value"], out[f"{name} first reduction"] = v0, r0
        out[f"{name} again"] = np.stack(E.ivr_values(eng, Xq, with_reduction=True))
        # append_data: against a fresh handle holding a copy of the final factor
        eng.append_data(X[N:], Y[N:])
        out[f"{name} appended"] = np.stack(E.ivr_values(eng, Xq, with_reduction=True))
        fresh = E.GPEngine(d, kernel, device=0)
        fresh.clone_from(eng)
        E.set_integration_points(fresh, Z, w)
        out[f"{name} appended fresh"] = np.stack(E.ivr_values(fresh, Xq, with_reduction=True))
        # set_hyper + set_data: against a fresh handle given the same
        eng.set_hyper(1.3, 1.5 * ls, 1e-2, -0.2)
        eng.set_data(X, Y)
        out[f"{name} refit"] = np.stack(E.ivr_values(eng, Xq, with_reduction=True))
        fresh2 = E.GPEngine(d, kernel, device=0)
        fresh2.set_hyper(1.3, 1.5 * ls, 1e-2, -0.2)
        fresh2.set_data(X, Y)
        E.set_integration_points(fresh2, Z, w)
        out[f"{name} refit fresh"] = np.stack(E.ivr_values(fresh2, Xq, with_reduction=True))
        # the tail alone, both residencies of the weights' absence
        cov = np.stack([np.eye(q) * (1.0 + g) for g in range(5)])
        cross = rng.standard_normal((5, q, P))
        out[f"{name} moments"] = E.ivr_moments(eng, cov, cross, w, 1e-3)
        out[f"{name} moments unweighted"] = E.ivr_moments(eng, cov, cross, None, 1e-3)
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **tour())
    print("ivr tour written")
