"""A short tour of the EHVI entry points whose arrays must not depend on what device memory held before (TEST
INFRASTRUCTURE): tests/test_gpu_ehvi.py runs it in process and, as ``python -m tests.ehvi_tour out.npz``, in a child
process under TGP_POISON=1, and compares the arrays bit for bit."""
import sys

import numpy as np


def table_partition(rng, P, V, K):
    """Random bound tables: bounds [P, V] ascending, K cells with lower index < upper index."""
    bounds = np.sort(rng.uniform(0.0, 1.0, size=(P, V)), axis=1)
    bounds[:, 0] = -1e10
    lo = rng.integers(0, V - 1, size=(K, P))
    hi = lo + 1 + (rng.integers(0, V, size=(K, P)) % (V - 1 - lo))
    return bounds, np.full(P, V, np.int32), lo.astype(np.int32), hi.astype(np.int32)


def stack_engines(P, N, d, kernel, seed):
    from trieste_amd.engine import GPEngine

    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N, d))
    engines = []
    for j in range(P):
        Y = np.sin(3.0 * X @ rng.uniform(0.5, 1.5, d) + j) + 0.1 * rng.standard_normal(N)
        eng = GPEngine(d, kernel, device=0)
        eng.set_hyper(0.8 + 0.3 * j, rng.uniform(0.3, 0.8, d), 1e-3 * (1 + j), 0.1 * j)
        eng.set_data(X, Y)
        engines.append(eng)
    return engines


def tour():
    from trieste_amd import engine as E

    out = {}
    rng = np.random.default_rng(11)
    for P, V, K in ((2, 5, 3), (3, 40, 200), (4, 512, 130)):
        eng = E.GPEngine(2, "matern52", device=0)
        E.ehvi_set_partition_tables(eng, *table_partition(rng, P, V, K))
        for M in (1, 65, 700):
            mean, var = rng.uniform(0.0, 1.0, (P, M)), 10.0 ** rng.uniform(-4, 0, (P, M))
            out[f"moments P={P} V={V} K={K} M={M}"] = E.ehvi_moments(eng, mean, var)
    for M in (100, 2500):
        engines = stack_engines(3, 60, 3, "matern52", seed=5)
        E.ehvi_set_partition_tables(engines[0], *table_partition(rng, 3, 20, 77))
        Xq = rng.uniform(size=(M, 3))
        out[f"values M={M}"] = E.ehvi_values(engines, Xq)
        v, i, x = E.ehvi_argmax(engines, Xq, index_base=5)
        out[f"argmax M={M}"] = np.concatenate([[v, float(i)], x])
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **tour())
    print("ehvi tour written")
