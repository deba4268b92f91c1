"""A short tour of the batch Monte-Carlo EHVI's gradient entry points whose arrays must not depend on what device memory held
before (TEST INFRASTRUCTURE): tests/test_gpu_qehvi_grad.py runs it in process and, as ``python -m tests.qehvi_grad_tour
out.npz``, in a child process under TGP_POISON=1, and compares the arrays bit for bit.  Also the mixed-kernel stack WITH the
oracle's states that the composition tests need."""
import sys

import numpy as np

from tests.ehvi_tour import table_partition
from tests.qehvi_tour import random_moments


def mixed_problem(kernels, N, d, seed):
    """``qehvi_tour.mixed_stack``'s models as (X, [(kernel, variance, lengthscales, noise, mean constant, Y)])."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N, d))
    members = []
    for j, kernel in enumerate(kernels):
        Y = np.sin(3.0 * X @ rng.uniform(0.5, 1.5, d) + j) + 0.1 * rng.standard_normal(N)
        members.append((kernel, 0.8 + 0.3 * j, rng.uniform(0.3, 0.8, d), 1e-3 * (1 + j), 0.1 * j, Y))
    return X, members


def problem_engines(X, members):
    from trieste_amd.engine import GPEngine

    engines = []
    for kernel, variance, ls, noise, c, Y in members:
        eng = GPEngine(X.shape[1], kernel, device=0)
        eng.set_hyper(variance, ls, noise, c)
        eng.set_data(X, Y)
        engines.append(eng)
    return engines


def tour():
    from trieste_amd import engine as E

    out = {}
    rng = np.random.default_rng(13)
    for P, q, S, K in ((2, 1, 5, 3), (3, 4, 130, 9), (4, 8, 70, 6)):
        eng = E.GPEngine(2, "matern52", device=0)
        E.ehvi_set_partition_tables(eng, *table_partition(rng, P, 6, K))
        eps = rng.standard_normal((P, q, S))
        for G in (1, 65, 300):
            mean, cov = random_moments(rng, P, G, q)
            for name, a in zip(("val", "gmean", "gcov"), E.qehvi_moments_grad(eng, mean, cov, eps)):
                out[f"moments {name} P={P} q={q} S={S} K={K} G={G}"] = a
    engines = problem_engines(*mixed_problem(("matern52", "rbf", "matern32"), 60, 3, seed=6))
    E.ehvi_set_partition_tables(engines[0], *table_partition(rng, 3, 8, 20))
    for G, q in ((40, 3), (682, 3)):
        val, grad = E.qehvi_value_grad(engines, rng.uniform(size=(G, q, 3)), rng.standard_normal((3, q, 33)))
        out[f"value_grad val G={G} q={q}"], out[f"value_grad grad G={G} q={q}"] = val, grad
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **tour())
    print("qehvi gradient tour written")
