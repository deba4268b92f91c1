"""Generator of tests/golden/ivr_goldens.json (not collected by pytest; run by hand: ``python -m tests.make_ivr_goldens``): the
integrated variance reduction in 50-digit mpmath, by the reference's route -- the posterior of the exact GP, the conditioned
variance at every integration point as a Schur complement over the q query points, the weights, the mean.

Full cases (model, integration points, batch): N in {2, 5, 8}, P in {1, 3, 7}, q in {1, 2, 3}, RBF and Matern-5/2 with ARD
lengthscales, noise 1e-7 ... 1e-1, no / one / two thresholds; one case with a query point AT a training input, one with two
query points 1e-7 apart.  Stored: the inputs as float64, and out = -mean(w v_new), reduction = mean(w (v_old - v_new)),
c0 = mean(w v_old) with v_old clipped at 1e-12 as the posterior's variance is, and the weights.

Moments cases (the tail alone: cov [G, q, q], cross [G, q, P], weights, noise -> reduction [G]): q in {1, 2, 5, 16}; cov + s^2 I
with condition numbers up to 1e7; weights spanning 1e-300 ... 1 with exact zeros among them; cross entries of mixed sign; a
group whose reduction is below 1e-200.  Inputs are float64 values with few decimal digits where that keeps the file small."""
from __future__ import annotations

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "ivr_goldens.json")
VAR_FLOOR = "1e-12"
DIGITS = 30   # digits stored of every 50-digit result


def _mp():
    import mpmath

    mpmath.mp.dps = 50
    return mpmath


def kernel(mp, kind, variance, ls, x, y):
    r2 = sum(((mp.mpf(a) - mp.mpf(b)) / mp.mpf(l)) ** 2 for a, b, l in zip(x, y, ls))
    if kind == "rbf":
        return mp.mpf(variance) * mp.exp(-r2 / 2)
    r = mp.sqrt(r2)
    s5 = mp.sqrt(5)
    return mp.mpf(variance) * (1 + s5 * r + mp.mpf(5) * r2 / 3) * mp.exp(-s5 * r)


def chol(mp, A):
    n = len(A)
    L = [[mp.mpf(0)] * n for _ in range(n)]
    for i in range(n):
        for j in range(i + 1):
            s = A[i][j] - sum(L[i][k] * L[j][k] for k in range(j))
            L[i][j] = mp.sqrt(s) if i == j else s / L[j][j]
    return L


def solve_lower(mp, L, b):
    a = []
    for i in range(len(L)):
        a.append((b[i] - sum(L[i][k] * a[k] for k in range(i))) / L[i][i])
    return a


def reduction_of(mp, cov, cross, weights, noise):
    """cov q x q, cross q x P (mpf) -> mean_z w_z |L^-1 c_z|^2."""
    q, P = len(cov), len(cross[0])
    A = [[cov[i][j] + (mp.mpf(noise) if i == j else 0) for j in range(q)] for i in range(q)]
    L = chol(mp, A)
    total = mp.mpf(0)
    for z in range(P):
        a = solve_lower(mp, L, [cross[i][z] for i in range(q)])
        total += (mp.mpf(1) if weights is None else mp.mpf(weights[z])) * sum(v * v for v in a)
    return total / P


def full_case(mp, name, kind, variance, ls, noise, mean_const, X, Y, Z, Xq, threshold):
    N, P, q = len(X), len(Z), len(Xq)
    K = [[kernel(mp, kind, variance, ls, X[i], X[j]) + (mp.mpf(noise) if i == j else 0) for j in range(N)] for i in range(N)]
    L = chol(mp, K)
    err = solve_lower(mp, L, [mp.mpf(y) - mp.mpf(mean_const) for y in Y])

    def col(x):   # L^-1 k(X, x)
        return solve_lower(mp, L, [kernel(mp, kind, variance, ls, X[i], x) for i in range(N)])

    cz, cx = [col(z) for z in Z], [col(x) for x in Xq]
    dot = lambda a, b: sum(u * v for u, v in zip(a, b))
    floor = mp.mpf(VAR_FLOOR)
    var_old = [max(mp.mpf(variance) - dot(c, c), floor) for c in cz]
    mean_old = [dot(c, err) + mp.mpf(mean_const) for c in cz]
    cov = [[kernel(mp, kind, variance, ls, Xq[i], Xq[j]) - dot(cx[i], cx[j]) for j in range(q)] for i in range(q)]
    for i in range(q):
        cov[i][i] = max(cov[i][i], floor)
    cross = [[kernel(mp, kind, variance, ls, Xq[i], Z[z]) - dot(cx[i], cz[z]) for z in range(P)] for i in range(q)]
    if threshold is None:
        w = None
    else:
        cdf = lambda t, m, s: mp.erfc(-(mp.mpf(t) - m) / (s * mp.sqrt(2))) / 2
        pdf = lambda t, m, s: mp.exp(-((mp.mpf(t) - m) / s) ** 2 / 2) / (s * mp.sqrt(2 * mp.pi))
        sd = [mp.sqrt(v) for v in var_old]
        if len(threshold) == 1:
            w = [pdf(threshold[0], m, s) for m, s in zip(mean_old, sd)]
        else:
            w = [cdf(threshold[1], m, s) - cdf(threshold[0], m, s) for m, s in zip(mean_old, sd)]
    red = reduction_of(mp, cov, cross, w, noise)
    c0 = sum((mp.mpf(1) if w is None else w[z]) * var_old[z] for z in range(P)) / P
    s = lambda v: mp.nstr(v, DIGITS)
    return dict(name=name, kind=kind, variance=variance, lengthscales=list(ls), noise=noise, mean_const=mean_const,
                X=[list(map(float, r)) for r in X], Y=list(map(float, Y)), Z=[list(map(float, r)) for r in Z],
                Xq=[list(map(float, r)) for r in Xq], threshold=threshold, weights=None if w is None else [s(v) for v in w],
                reduction=s(red), c0=s(c0), out=s(red - c0))


def full_cases(mp):
    rng = np.random.default_rng(20261)
    r3 = lambda *shape: np.round(rng.uniform(size=shape), 3)
    table = [  # (N, P, q, kind, noise, threshold): every value of every list appears
        (2, 1, 1, "rbf", 1e-1, None), (5, 3, 2, "matern52", 1e-3, [0.4]), (8, 7, 3, "rbf", 1e-5, [0.2, 0.9]),
        (2, 7, 2, "matern52", 1e-7, None), (5, 1, 3, "rbf", 1e-2, [0.1, 0.5]), (8, 3, 1, "matern52", 1e-4, [0.7]),
        (8, 7, 3, "matern52", 1e-7, None), (5, 7, 1, "rbf", 1e-7, [0.3]), (2, 3, 3, "rbf", 1e-3, [0.0, 1.0]),
        (8, 1, 2, "matern52", 1e-1, [0.6]), (5, 3, 2, "rbf", 1e-6, None), (8, 3, 3, "matern52", 1e-2, [0.25, 0.75]),
    ]
    cases = []
    for n, (N, P, q, kind, noise, th) in enumerate(table):
        d = 2 + n % 2
        X, Z, Xq = r3(N, d), r3(P, d), r3(q, d)
        Y = np.round(np.sin(3.0 * X.sum(axis=1)) * 0.5 + 0.5, 3)
        ls = [0.3, 0.7, 0.45][:d]
        cases.append(full_case(mp, f"full-{n}", kind, [1.0, 1.7][n % 2], ls, noise, [0.0, 0.25][n % 2], X, Y, Z, Xq, th))
    # a query point AT a training input; two query points 1e-7 apart
    X, Z = r3(5, 2), r3(7, 2)
    Y = np.round(np.cos(2.0 * X.sum(axis=1)), 3)
    Xq = np.array([X[2], [0.61, 0.13]])
    cases.append(full_case(mp, "at-training-input", "matern52", 1.3, [0.4, 0.6], 1e-6, 0.1, X, Y, Z, Xq, [0.2]))
    Xq = np.array([[0.37, 0.52], [0.37 + 1e-7, 0.52], [0.9, 0.1]])
    cases.append(full_case(mp, "near-duplicate-pair", "rbf", 1.0, [0.5, 0.5], 1e-7, 0.0, X, Y, Z, Xq, None))
    return cases


def moments_case(mp, name, cov, cross, weights, noise):
    cov, cross = np.asarray(cov, dtype=np.float64), np.asarray(cross, dtype=np.float64)
    red = []
    for g in range(len(cov)):
        mc = [[mp.mpf(float(v)) for v in row] for row in cov[g]]
        mx = [[mp.mpf(float(v)) for v in row] for row in cross[g]]
        red.append(mp.nstr(reduction_of(mp, mc, mx, None if weights is None else [float(v) for v in weights], noise), DIGITS))
    return dict(name=name, cov=cov.tolist(), cross=cross.tolist(), weights=None if weights is None else [float(v) for v in weights],
                noise=noise, reduction=red)


def spd(rng, G, q, floor):
    """B B^T / q + floor I with B of two-digit entries: condition number at most about q / floor."""
    B = np.round(rng.standard_normal((G, q, q)), 2)
    return B @ np.swapaxes(B, -1, -2) / q + floor * np.eye(q)


def moments_cases(mp):
    rng = np.random.default_rng(20262)
    x2 = lambda *shape: np.round(rng.standard_normal(shape), 2)   # mixed sign
    cases = []
    for q, P, G in ((1, 3, 3), (2, 7, 3), (5, 65, 2), (16, 66, 1)):
        w = np.round(rng.uniform(size=P), 2)
        w[::3] = 0.0                                               # exact zeros (the last tile's among them at P = 65, 66)
        cases.append(moments_case(mp, f"q{q}", spd(rng, G, q, 0.1), x2(G, q, P), w if q != 2 else None, 1e-3))
    # condition numbers 1e3, 1e5, 1e7 of cov + noise I: v v^T + noise I with |v|^2 about q
    v = np.round(rng.uniform(0.5, 1.5, size=(3, 5)), 2)
    for g, noise in enumerate((5e-3, 5e-5, 5e-7)):
        cov = v[g][:, None] * v[g][None, :]
        cond = (float(v[g] @ v[g]) + noise) / noise
        cases.append(moments_case(mp, f"cond-{cond:.0e}", cov[None], x2(1, 5, 7), None, noise))
    # weights across 300 decades, zeros among them
    w = np.array([1.0, 1e-300, 0.0, 1e-150, 1e-30, 0.0, 0.5, 1e-290, 1e-3])
    cases.append(moments_case(mp, "weights-300-decades", spd(rng, 2, 2, 0.2), x2(2, 2, 9), w, 1e-2))
    # a group whose reduction is below 1e-200 next to an ordinary one
    cross = x2(2, 2, 5)
    cross[0] = cross[0] * 1e-101
    cases.append(moments_case(mp, "reduction-below-1e-200", spd(rng, 2, 2, 0.3), cross, None, 1e-4))
    return cases


def main():
    mp = _mp()
    doc = dict(digits=DIGITS, full=full_cases(mp), moments=moments_cases(mp))
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(OUT, os.path.getsize(OUT), "bytes;", len(doc["full"]), "full and", len(doc["moments"]), "moments cases")


if __name__ == "__main__":
    main()
