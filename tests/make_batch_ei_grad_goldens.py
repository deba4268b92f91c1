"""Generator of tests/golden/batch_ei_grad_goldens.json (not collected by pytest; run by hand:
``python -m tests.make_batch_ei_grad_goldens``): 50-digit directional derivatives of the analytic multi-point expected
improvement on the cases of tests/golden/batch_ei_goldens.json, by central differences with h = 1e-18 in mpmath.

tests/make_batch_ei_goldens.py casts its inputs through ``float``, which swallows a 1e-18 step, so this file carries its
own copy of that file's two functions on *mpf* inputs (the Sobol points stay float64 numbers: they are data).  At 50
digits a central difference with h = 1e-18 is exact to about 1e-32 (truncation h^2, round-off 1e-50 / h).

Directions (dm [q], dC [q, q] symmetric; derivative = d/dt value(mean + t dm, cov + t dC) at t = 0):
  (a) q <= 4: every coordinate of mean (dm = e_i) and every symmetric pair of cov (dC = E_ij + E_ji for i < j, E_ii);
  (b) q = 6, 8: three seeded random symmetric directions per case (standard normal entries; stored in the file).
One (case, direction) per worker process; about 0.3 s (q = 2) to 30 s (q = 8) each."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "golden", "batch_ei_goldens.json")
OUT = os.path.join(HERE, "golden", "batch_ei_grad_goldens.json")
STEP = "1e-18"


def mp_mvn_cdf(mp, x, cov, w):
    """utils.py:142-197, mean 0: x [n] (mpf), cov n x n (mp matrix), w [S][>= n - 1] -> mp number."""
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
    """The value alone on mpf mean [q] and cov [q][q] (no cast through float)."""
    q = len(mean)
    mu = [-v for v in mean]                                                  # function.py:1798
    T = -mp.mpf(float(eta))                                                  # :1800
    cv = mp.matrix(q, q)
    for i in range(q):
        for j in range(q):
            cv[i, j] = cov[i][j] + (mp.mpf(1e-6) if i == j else 0)           # :1776-1783

    def sig(i, j, k):                                                        # :1413-1424
        a = cv[j, k] if (j != i and k != i) else 0
        b = cv[j, i] if j != i else 0
        c = cv[i, k] if k != i else 0
        return a - b - c + cv[i, i]

    def dif(i, j):                                                           # :1343-1352, :1480
        b = -T if j == i else 0
        m = mu[j] - mu[i] - (mu[i] if j == i else 0)
        return b - m

    value = mp.mpf(0)
    for i in range(q):
        S_i = mp.matrix(q, q)
        for j in range(q):
            for k in range(q):
                S_i[j, k] = sig(i, j, k)
        d = [dif(i, j) for j in range(q)]
        value += (mu[i] - T) * mp_mvn_cdf(mp, d, S_i, w1)                    # :1476-1488, :1734
        for k in range(q):
            keep = [j for j in range(q) if j != k]
            c = [d[j] - d[k] * S_i[k, j] / S_i[k, k] for j in keep]          # :1524-1525
            R = mp.matrix(q - 1, q - 1)
            for a, u in enumerate(keep):
                for b_, v in enumerate(keep):
                    R[a, b_] = S_i[u, v] - S_i[k, u] * S_i[k, v] / S_i[k, k]   # :1559
            sc = mp.sqrt(S_i[k, k])
            pdf = mp.npdf(d[k] / sc) / sc                                    # :1725-1727
            value += S_i[k, i] * pdf * mp_mvn_cdf(mp, c, R, w2)              # :1729-1730, :1738, :1642-1647
    return value


def direction_arrays(q, d):
    """(dm [q], dC [q, q]) of a stored direction."""
    dm, dC = np.zeros(q), np.zeros((q, q))
    if d["kind"] == "mean":
        dm[d["i"]] = 1.0
    elif d["kind"] == "cov":
        dC[d["i"], d["j"]] = 1.0
        dC[d["j"], d["i"]] = 1.0
    else:
        dm, dC = np.asarray(d["dm"], dtype=np.float64), np.asarray(d["dC"], dtype=np.float64)
    return dm, dC


def _derivative(task):
    import mpmath as mp

    mp.mp.dps = 50
    c, d = task
    q = c["q"]
    dm, dC = direction_arrays(q, d)
    h = mp.mpf(STEP)
    vals = []
    for sgn in (1, -1):
        mean = [mp.mpf(float(c["mean"][i])) + sgn * h * mp.mpf(float(dm[i])) for i in range(q)]
        cov = [[mp.mpf(float(c["cov"][i][j])) + sgn * h * mp.mpf(float(dC[i, j])) for j in range(q)] for i in range(q)]
        vals.append(mp_batch_ei(mp, mean, cov, c["eta"], c["w1"], c["w2"]))
    return float((vals[0] - vals[1]) / (2 * h))


def make_directions(cases):
    out = []
    for n, c in enumerate(cases):
        q = c["q"]
        if q <= 4:
            for i in range(q):
                out.append({"case": n, "kind": "mean", "i": i})
            for i in range(q):
                for j in range(i, q):
                    out.append({"case": n, "kind": "cov", "i": i, "j": j})
        else:
            for r in range(3):
                rng = np.random.default_rng(1000 * n + r)
                dm = rng.standard_normal(q)
                A = rng.standard_normal((q, q))
                dC = 0.5 * (A + A.T)
                out.append({"case": n, "kind": "random", "seed": 1000 * n + r, "dm": dm.tolist(), "dC": dC.tolist()})
    return out


def main():
    from multiprocessing import Pool

    with open(SRC) as f:
        cases = json.load(f)["cases"]
    dirs = make_directions(cases)
    order = sorted(range(len(dirs)), key=lambda t: -cases[dirs[t]["case"]]["q"])   # the long ones first
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_derivative, [(cases[dirs[t]["case"]], dirs[t]) for t in order], chunksize=1)
    for t, v in zip(order, res):
        dirs[t]["deriv"] = v
    doc = {"what": "directional derivatives of the analytic batch EI on the cases of batch_ei_goldens.json: central "
                   "differences, h = 1e-18, 50-digit mpmath; tests/make_batch_ei_grad_goldens.py",
           "dps": 50, "step": STEP, "directions": dirs}
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(f"wrote {OUT}: {len(dirs)} directions, {os.path.getsize(OUT)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
