"""Generator of tests/golden/batch_ei_goldens.json (not collected by pytest; run by hand:
``python -m tests.make_batch_ei_goldens``): the analytic multi-point expected improvement of the reference
(trieste/acquisition/function/function.py:1651-1805, function/utils.py:109-199) in 50-digit mpmath, written from the
formulas with scalar loops and independently of tests/batch_ei_reference.py (``mp.cholesky``, ``mp.ncdf``,
``sqrt(2) erfinv(2 u - 1)``), on moments of small GPR problems (the numpy oracle's ``predict_joint``).

Stored per case: mean [q], cov [q, q], eta, w1 [S, q], w2 [S, q - 1] (the inputs, float64), value, p [q], Phi [q, q] and
abs_terms = the sum of the absolute summands of the value (the scale its float64 evaluations are accurate to)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "batch_ei_goldens.json")


def mp_mvn_cdf(mp, x, cov, w):
    """utils.py:142-197, mean 0: x [n], cov n x n (mp matrix), w [S][>= n - 1] -> mp number."""
    n = len(x)
    A = cov.copy()
    for i in range(n):
        A[i, i] += mp.mpf(1e-6)
    C = mp.cholesky(A)
    tiny, lo, span = mp.mpf(1e-12), mp.mpf(1e-6), mp.mpf(1) - mp.mpf(2e-6)
    e0 = mp.ncdf(x[0] / (C[0, 0] + tiny))
    if n == 1:
        return e0
    total = mp.mpf(0)
    for ws in w:
        e, f, y = e0, e0, []
        for i in range(1, n):
            u = lo + span * mp.mpf(float(ws[i - 1])) * e
            y.append(mp.sqrt(2) * mp.erfinv(2 * u - 1))
            acc = mp.mpf(0)
            for j in range(i):
                acc += C[i, j] * y[j]
            e = mp.ncdf((x[i] - acc) / (C[i, i] + tiny))
            f = e * f
        total += f
    return total / len(w)


def mp_batch_ei(mp, mean, cov, eta, w1, w2):
    q = len(mean)
    mu = [-mp.mpf(float(v)) for v in mean]                                   # function.py:1798
    T = -mp.mpf(float(eta))                                                  # :1800
    cv = mp.matrix(q, q)
    for i in range(q):
        for j in range(q):
            cv[i, j] = mp.mpf(float(cov[i][j])) + (mp.mpf(1e-6) if i == j else 0)   # :1776-1783

    def sig(i, j, k):                                                        # :1413-1424
        a = cv[j, k] if (j != i and k != i) else 0
        b = cv[j, i] if j != i else 0
        c = cv[i, k] if k != i else 0
        return a - b - c + cv[i, i]

    def dif(i, j):                                                           # :1343-1352, :1480
        b = -T if j == i else 0
        m = mu[j] - mu[i] - (mu[i] if j == i else 0)
        return b - m

    p, Phi = [], [[None] * q for _ in range(q)]
    value, abs_terms = mp.mpf(0), mp.mpf(0)
    for i in range(q):
        S_i = mp.matrix(q, q)
        for j in range(q):
            for k in range(q):
                S_i[j, k] = sig(i, j, k)
        d = [dif(i, j) for j in range(q)]
        p.append(mp_mvn_cdf(mp, d, S_i, w1))                                 # :1476-1488
        t = (mu[i] - T) * p[i]                                               # :1734
        value += t
        abs_terms += abs(t)
        for k in range(q):
            keep = [j for j in range(q) if j != k]
            c = [d[j] - d[k] * S_i[k, j] / S_i[k, k] for j in keep]          # :1524-1525
            R = mp.matrix(q - 1, q - 1)
            for a, u in enumerate(keep):
                for b_, v in enumerate(keep):
                    R[a, b_] = S_i[u, v] - S_i[k, u] * S_i[k, v] / S_i[k, k]   # :1559
            Phi[i][k] = mp_mvn_cdf(mp, c, R, w2)                             # :1642-1647
            sc = mp.sqrt(S_i[k, k])
            pdf = mp.npdf(d[k] / sc) / sc                                    # :1725-1727 (b_ik - m_ik = d_k)
            t = S_i[k, i] * pdf * Phi[i][k]                                  # :1729-1730, :1738
            value += t
            abs_terms += abs(t)
    return value, p, Phi, abs_terms


def make_cases():
    from oracle import gp_oracle as O
    from scipy.stats import qmc

    cases = []
    plan = [(2, 64, 4), (3, 48, 4), (4, 40, 4), (6, 32, 3), (8, 32, 3)]   # (q, S, q-batches)
    for q, S, nb in plan:
        d, N = 3, 40
        X, Y = O.synthetic_problem(lambda x: np.sum((x - 0.4) ** 2, axis=-1, keepdims=True), d, N, seed=100 + q)
        noise = 1e-3 if q % 2 == 0 else 1e-5
        st = O.gpr_update("matern52", 1.3, np.array([0.3, 0.5, 0.8]), noise, 0.1, X, Y)
        rng = np.random.default_rng(q)
        Xq = rng.uniform(size=(nb, q, d))
        Xq[0, 1] = Xq[0, 0] + 1e-3 / np.sqrt(d)        # two nearly coincident points
        Xq[1, 0] = X[3] + 1e-4 / np.sqrt(d)            # a point next to a training input
        mean, cov = O.predict_joint(st, Xq)
        eta = float(np.median(mean.min(axis=1)))
        w = []
        for dim in (q, q - 1):
            gen = qmc.Sobol(d=dim, scramble=False)
            gen.fast_forward(1 + 7 * q)
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                w.append(gen.random(S))
        for g in range(nb):
            cases.append({"q": q, "S": S, "mean": mean[g].tolist(), "cov": cov[g].tolist(), "eta": eta,
                          "w1": w[0].tolist(), "w2": w[1].tolist(),
                          "note": {0: "near-duplicate pair", 1: "next to a training input"}.get(g, "random")})
    return cases


def main():
    import mpmath as mp

    mp.mp.dps = 50
    cases = make_cases()
    for n, c in enumerate(cases):
        v, p, Phi, at = mp_batch_ei(mp, c["mean"], c["cov"], c["eta"], c["w1"], c["w2"])
        c["value"] = float(v)
        c["p"] = [float(t) for t in p]
        c["Phi"] = [[float(t) for t in row] for row in Phi]
        c["abs_terms"] = float(at)
        print(f"case {n}: q={c['q']} S={c['S']} value={c['value']:.6e} abs_terms={c['abs_terms']:.3e}", file=sys.stderr, flush=True)
    doc = {"what": "analytic batch EI (reference function.py:1651-1805, utils.py:109-199) in 50-digit mpmath; "
                   "tests/make_batch_ei_goldens.py", "dps": 50, "cases": cases}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(f"wrote {OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
