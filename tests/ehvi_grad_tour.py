"""A short tour of the EHVI value-and-gradient entry points whose arrays must not depend on what device memory held before
(TEST INFRASTRUCTURE): tests/test_gpu_ehvi_grad.py runs it in process and, as ``python -m tests.ehvi_grad_tour out.npz``, in
a fresh child process under TGP_POISON=1, and compares the arrays bit for bit."""
import sys

import numpy as np

from tests.ehvi_tour import stack_engines, table_partition


def tour():
    from trieste_amd import engine as E

    out = {}
    rng = np.random.default_rng(13)
    for P, V, K in ((2, 5, 3), (3, 40, 200), (4, 512, 130)):
        eng = E.GPEngine(2, "matern52", device=0)
        E.ehvi_set_partition_tables(eng, *table_partition(rng, P, V, K))
        for M in (1, 65, 300):
            mean, var = rng.uniform(0.0, 1.0, (P, M)), 10.0 ** rng.uniform(-4, 0, (P, M))
            val, gm, gv = E.ehvi_moments_grad(eng, mean, var)
            out[f"moments P={P} V={V} K={K} M={M} val"], out[f"moments P={P} V={V} K={K} M={M} gmean"] = val, gm
            out[f"moments P={P} V={V} K={K} M={M} gvar"] = gv
    for P, d, M in ((3, 3, 100), (2, 40, 70), (4, 2, 2048)):
        engines = stack_engines(P, 60, d, "matern52", seed=5)
        E.ehvi_set_partition_tables(engines[0], *table_partition(rng, P, 20, 77))
        val, grad = E.ehvi_value_grad(engines, rng.uniform(size=(M, d)))
        out[f"value_grad P={P} d={d} M={M} val"], out[f"value_grad P={P} d={d} M={M} grad"] = val, grad
    return out


if __name__ == "__main__":
    np.savez(sys.argv[1], **tour())
    print("ehvi gradient tour written")
