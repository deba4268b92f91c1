"""A short tour of the batch Monte-Carlo EHVI entry points whose arrays must not depend on what device memory held before
(TEST INFRASTRUCTURE): tests/test_gpu_qehvi.py runs it in process and, as ``python -m tests.qehvi_tour out.npz``, in a child
process under TGP_POISON=1, and compares the arrays bit for bit."""
import sys

import numpy as np

from tests.ehvi_tour import table_partition


def random_moments(rng, P, G, q, scale=0.05):
    """mean [P, G, q] in [0, 1], full covariances cov [P, G, q, q] with eigenvalues of about ``scale``."""
    a = rng.standard_normal((P, G, q, q))
    cov = scale * (a @ np.swapaxes(a, -1, -2) / q + 0.05 * np.eye(q))
    return rng.uniform(0.0, 1.0, (P, G, q)), cov


def mixed_stack(kernels, N, d, seed):
    """One engine per kernel kind on the same inputs, each with its own hyper-parameters and observations."""
    from trieste_amd.engine import GPEngine

    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(N, d))
    engines = []
    for j, kernel in enumerate(kernels):
        Y = np.sin(3.0 * X @ rng.uniform(0.5, 1.5, d) + j) + 0.1 * rng.standard_normal(N)
        eng = GPEngine(d, kernel, device=0)
        eng.set_hyper(0.8 + 0.3 * j, rng.uniform(0.3, 0.8, d), 1e-3 * (1 + j), 0.1 * j)
        eng.set_data(X, Y)
        engines.append(eng)
    return engines


def tour():
    from trieste_amd import engine as E

    out = {}
    rng = np.random.default_rng(12)
    for P, q, S, K in ((2, 1, 5, 3), (3, 4, 130, 9), (4, 8, 129, 6)):
        eng = E.GPEngine(2, "matern52", device=0)
        E.ehvi_set_partition_tables(eng, *table_partition(rng, P, 6, K))
        eps = rng.standard_normal((P, q, S))
        for G in (1, 65, 300):
            mean, cov = random_moments(rng, P, G, q)
            out[f"moments P={P} q={q} S={S} K={K} G={G}"] = E.qehvi_moments(eng, mean, cov, eps)
    engines = mixed_stack(("matern52", "rbf", "matern32"), 60, 3, seed=6)
    E.ehvi_set_partition_tables(engines[0], *table_partition(rng, 3, 8, 20))
    for G, q in ((40, 3), (700, 3)):   # both posterior paths (G q <= 2048 and above)
        out[f"values G={G} q={q}"] = E.qehvi_values(engines, rng.uniform(size=(G, q, 3)), rng.standard_normal((3, q, 33)))
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **tour())
    print("qehvi tour written")
