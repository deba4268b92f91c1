"""Generator of tests/golden/qehvi_goldens.json: 50-digit mpmath values of the batch Monte-Carlo expected hypervolume
improvement from given joint moments,

    L_j      = chol(cov_j + jitter I),   y[s,i,j] = mean[j,i] + sum_m L_j[i,m] eps[j,m,s],
    value    = (1/S) sum_s sum_cells sum_{J != {}} (-1)^(|J|+1) prod_j max(ub_j - max(lb_j, max_{i in J} y[s,i,j]), 0),

(the Cholesky factor, the samples and the inclusion-exclusion all at 50 digits, from the float64 inputs taken exactly), and of
``abs_terms``, the same sum with every sign positive, that every comparison is made relative to.  mean [P, q], cov [P, q, q]
full, eps [P, q, S].  Run ``python -m tests.make_qehvi_goldens`` from the repository root to regenerate (deterministic)."""
import json
import os
from itertools import combinations

import mpmath as mp
import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qehvi_goldens.json")


def exact(mean, cov, eps, jitter, lb, ub):
    """(value, abs_terms) at 50 digits."""
    mp.mp.dps = 50
    mean, cov, eps = np.asarray(mean), np.asarray(cov), np.asarray(eps)
    P, q = mean.shape
    S = eps.shape[2]
    y = [[[None] * P for _ in range(q)] for _ in range(S)]
    for j in range(P):
        A = mp.matrix(q, q)
        for a in range(q):
            for b in range(q):
                A[a, b] = mp.mpf(float(cov[j, a, b])) + (mp.mpf(float(jitter)) if a == b else 0)
        L = mp.cholesky(A)
        for s in range(S):
            for i in range(q):
                v = mp.mpf(float(mean[j, i]))
                for m in range(i + 1):
                    v += L[i, m] * mp.mpf(float(eps[j, m, s]))
                y[s][i][j] = v
    subsets = [J for n in range(1, q + 1) for J in combinations(range(q), n)]
    value = scale = mp.mpf(0)
    for s in range(S):
        for lo_row, up_row in zip(lb, ub):
            lo = [max(mp.mpf(float(v)), mp.mpf(-1e10)) for v in lo_row]
            up = [mp.mpf(float(v)) for v in up_row]
            for J in subsets:
                t = mp.mpf(1)
                for j in range(P):
                    t *= max(up[j] - max(lo[j], max(y[s][i][j] for i in J)), mp.mpf(0))
                scale += t
                value += t if len(J) % 2 else -t
    return value / S, scale / S


def _partition(front, ref):
    from trieste_amd.acquisition.multi_objective import prepare_default_non_dominated_partition_bounds

    front = np.asarray(front, np.float64)
    return prepare_default_non_dominated_partition_bounds(np.asarray(ref, np.float64), front if front.size else None)


FRONT_2D = np.stack([np.linspace(0.1, 0.9, 4), np.linspace(0.9, 0.1, 4) ** 1.5], axis=1)
FRONT_3D = np.array([[0.2, 0.7, 0.5], [0.6, 0.3, 0.4]])
FRONT_4D = np.array([[0.4, 0.5, 0.3, 0.6]])
SETUPS = {2: (FRONT_2D, [1.1, 1.1]), 3: (FRONT_3D, [1.0, 1.0, 1.0]), 4: (FRONT_4D, [1.0, 1.0, 1.0, 1.0])}


def _cov(rng, P, q, scale):
    a = rng.standard_normal((P, q, q))
    return scale * (a @ np.swapaxes(a, -1, -2) / q + 0.05 * np.eye(q))


def cases():
    rng = np.random.default_rng(20250311)
    out = []

    def add(note, P, mean, cov, eps, jitter=1e-6):
        front, ref = SETUPS[P]
        lb, ub = _partition(front, ref)
        out.append(dict(note=note, jitter=float(jitter), mean=np.asarray(mean, np.float64).tolist(),
                        cov=np.asarray(cov, np.float64).tolist(), eps=np.asarray(eps, np.float64).tolist(),
                        lb=np.asarray(lb, np.float64).tolist(), ub=np.asarray(ub, np.float64).tolist()))

    # the grid: every P with every q; S <= 16 (q = 8 with few samples: 255 subsets each)
    for P in (2, 3, 4):
        for q, S in ((1, 16), (2, 16), (3, 11), (8, 3)):
            add(f"P={P} q={q} S={S}", P, rng.uniform(0.0, 0.9, (P, q)), _cov(rng, P, q, 0.05), rng.standard_normal((P, q, S)))
    # wide marginals, and jitter 0
    add("P=2 q=3 wide marginals", 2, rng.uniform(-0.5, 1.5, (2, 3)), _cov(rng, 2, 3, 1.0), rng.standard_normal((2, 3, 8)))
    add("P=3 q=2 jitter 0", 3, rng.uniform(0.0, 0.9, (3, 2)), _cov(rng, 3, 2, 0.05), rng.standard_normal((3, 2, 8)), jitter=0.0)
    # two nearly coincident batch points: rows 0 and 1 of the moments almost equal, correlation 1 - 1e-9
    for P in (2, 3):
        q = 3
        mean = rng.uniform(0.1, 0.6, (P, q))
        mean[:, 1] = mean[:, 0] + 1e-9
        cov = _cov(rng, P, q, 0.02)
        for j in range(P):
            cov[j, 1, :] = cov[j, 0, :]
            cov[j, :, 1] = cov[j, :, 0]
            cov[j, 1, 1] = cov[j, 0, 0] * (1.0 + 2e-9)
        add(f"P={P} q=3 two nearly coincident points", P, mean, cov, rng.standard_normal((P, q, 8)))
    # every sample dominated by the front (means far above the reference point, tiny covariance): exactly 0
    add("P=2 q=3 every sample dominated", 2, rng.uniform(1.5, 2.0, (2, 3)), _cov(rng, 2, 3, 1e-4), rng.standard_normal((2, 3, 8)))
    add("P=3 q=2 every sample dominated", 3, np.tile(FRONT_3D[0][:, None] + 0.05, (1, 2)), _cov(rng, 3, 2, 1e-8),
        rng.standard_normal((3, 2, 8)))
    # a sample below every front point in every objective
    mean = rng.uniform(0.2, 0.8, (2, 2))
    mean[:, 0] = [-0.5, -0.5]
    add("P=2 q=2 a point below every front point", 2, mean, _cov(rng, 2, 2, 1e-3), rng.standard_normal((2, 2, 8)))
    mean = rng.uniform(0.2, 0.8, (4, 3))
    mean[:, 2] = -0.3
    add("P=4 q=3 a point below every front point", 4, mean, _cov(rng, 4, 3, 1e-3), rng.standard_normal((4, 3, 5)))
    return out


def main():
    out = cases()
    for c in out:
        value, scale = exact(c["mean"], c["cov"], c["eps"], c["jitter"], c["lb"], c["ub"])
        c["value"], c["abs_terms"] = mp.nstr(value, 25), mp.nstr(scale, 25)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"cases": out}, f, indent=0)
    print(f"{len(out)} cases -> {OUT} ({os.path.getsize(OUT)} bytes)")
    for c in out:
        print(f"{c['note']:45s} K={len(c['lb'])} value {c['value'][:14]} abs_terms {c['abs_terms'][:14]}")


if __name__ == "__main__":
    main()
