"""Writes tests/golden/kernel_resolution_goldens.json: the four stationary kernels and their input gradients in mpmath
(50 digits) on the EXACT doubles of the probes it stores, for tests/test_oracle_tails.py and the
comparison of the engine's kernel functions at ulp resolution.  Needs mpmath; the tests do not.

    python tests/make_kernel_resolution_goldens.py

k(x, X) with r^2 = sum_c ((x_c - X_c) / ls_c)^2 and gpflow's r = sqrt(max(r^2, 1e-36)) (1e-36 the double):
rbf exp(-r^2 / 2); matern12 exp(-r); matern32 (1 + s) exp(-s), s = sqrt(3) r; matern52 (1 + s + s^2 / 3) exp(-s),
s = sqrt(5) r; variance 1.  dk/dx_c = 2 k'(max(r^2, 1e-36)) (x_c - X_c) / ls_c^2 with k' = dk / d(r^2) -- the form of the
oracle's ``acq_value_and_grad`` (exactly 0 at a coincident point).  ``s`` is the argument of the exponential, ``r2`` the
nearest double of max(r^2, 1e-36).

Three designs share the lengthscales [0.5, 0.25, 2.0] (powers of two: the scaled coordinates are exact):
* ``single``: one training point X0 = [0.25, 0.5, 0.75]; probes X0 + r * U * ls along the oblique unit vector U for
  r in {0, 1e-18, 1e-12, 1e-8, 1e-4} and 40 log-spaced radii from 1e-3 to the radius at which s = 680 (700 at most), so
  every value is a normal double; three more probes per kind with s = 760, 1e4, 1e8 (underflow: no reference value).
* ``rows``: 257 training points [0.25 + 2048 i, 0.5, 0.75] (4096 lengthscales apart: every off-diagonal kernel value is
  exactly 0 in float64); probes around rows 0, 15, 16, 255, 256 at 12 radii from 1e-3 to 30.
* ``dense``: 17 training points and 24 probes in the unit cube; the whole [24, 17] matrix of kernel values.
``scalar`` holds exp, 2^x and sqrt as (double, remainder) pairs for the restatement of the device's fast math."""
import json
import os

import numpy as np
from mpmath import mp, mpf

mp.dps = 50
KINDS = ("rbf", "matern12", "matern32", "matern52")
LS = [0.5, 0.25, 2.0]
X0 = [0.25, 0.5, 0.75]
U = [0.6, -0.48, 0.64]          # 0.36 + 0.2304 + 0.4096 = 1
FLOOR = mpf(1e-36)
S_CAP = 680.0
ROWS = (0, 15, 16, 255, 256)


def s_of_r(kind, r):
    return {"rbf": 0.5 * r * r, "matern12": r, "matern32": np.sqrt(3.0) * r, "matern52": np.sqrt(5.0) * r}[kind]


def r_of_s(kind, s):
    return {"rbf": np.sqrt(2.0 * s), "matern12": s, "matern32": s / np.sqrt(3.0), "matern52": s / np.sqrt(5.0)}[kind]


def kernel(kind, x, X):
    """(k, dk/dx [d], s) in mpmath on the exact doubles x, X."""
    t = [(mpf(float(a)) - mpf(float(b))) / mpf(l) for a, b, l in zip(x, X, LS)]
    r2 = max(sum(v * v for v in t), FLOOR)
    if kind == "rbf":
        s = r2 / 2
        k = mp.exp(-s)
        dr2 = -k / 2
    else:
        r = mp.sqrt(r2)
        if kind == "matern12":
            s = r
            k = mp.exp(-r)
            dr2 = -k / (2 * r)
        elif kind == "matern32":
            s = mp.sqrt(3) * r
            k = (1 + s) * mp.exp(-s)
            dr2 = -mpf(3) / 2 * mp.exp(-s)
        else:
            s = mp.sqrt(5) * r
            k = (1 + s + s * s / 3) * mp.exp(-s)
            dr2 = -mpf(5) / 6 * (1 + s) * mp.exp(-s)
    dk = [2 * dr2 * v / mpf(l) for v, l in zip(t, LS)]
    return float(k), [float(v) for v in dk], float(s), float(r2)


def probes(centre, radii):
    return [[float(c + r * u * l) for c, u, l in zip(centre, U, LS)] for r in radii]


def block(kind, xs, X):
    out = dict(x=xs, k=[], dk=[], s=[], r2=[])
    for x in xs:
        k, dk, s, r2 = kernel(kind, x, X)
        out["k"].append(k)
        out["dk"].append(dk)
        out["s"].append(s)
        out["r2"].append(r2)
    return out


def hilo(v):
    """A 50-digit value as the pair (nearest double, nearest double of the remainder): about 32 digits."""
    hi = float(v)
    return [hi, float(v - mpf(hi))]


def scalar():
    """References for the CPU restatement of the device's fast math (tests/test_fast_math_restatement.py): exp(x) and 2^x
    on x <= 0, sqrt(y) on [1e-36, 1e300]."""
    xs = [-float(v) for v in np.concatenate([np.geomspace(1e-6, 680.0, 120), np.linspace(0.01, 40.0, 120)])]
    ys = [float(v) for v in np.geomspace(1e-36, 1e300, 160)]
    return dict(x=xs, exp=[hilo(mp.exp(mpf(x))) for x in xs], exp2=[hilo(mp.power(2, mpf(x))) for x in xs],
                y=ys, sqrt=[hilo(mp.sqrt(mpf(y))) for y in ys])


def main():
    g = dict(lengthscales=LS, X0=X0, direction=U, variance=1.0, noise=3.0, single={}, underflow={}, rows={}, dense={})
    for kind in KINDS:
        rmax = min(700.0, float(r_of_s(kind, S_CAP)))
        radii = [0.0, 1e-18, 1e-12, 1e-8, 1e-4] + [float(r) for r in np.geomspace(1e-3, rmax, 40)]
        b = block(kind, probes(X0, radii), X0)
        assert max(b["s"]) <= S_CAP * (1 + 1e-12) and min(b["k"]) > 1e-300
        g["single"][kind] = b
        us = [760.0, 1e4, 1e8]
        g["underflow"][kind] = dict(x=probes(X0, [float(r_of_s(kind, s)) for s in us]), s=us)
    g["rows"]["rows"] = list(ROWS)
    g["rows"]["N"] = 257
    g["rows"]["spacing"] = 2048.0
    for kind in KINDS:
        g["rows"][kind] = {}
        for i in ROWS:
            Xi = [0.25 + 2048.0 * i, 0.5, 0.75]
            g["rows"][kind][str(i)] = block(kind, probes(Xi, [float(r) for r in np.geomspace(1e-3, 30.0, 12)]), Xi)
    rng = np.random.default_rng(20240917)
    Xd = rng.uniform(size=(17, 3))
    xq = rng.uniform(size=(24, 3))
    xq[0] = Xd[3]                          # at a training input
    xq[1] = Xd[5] + 1e-9                   # next to one
    xq[2] = [3.0, -1.0, 9.0]               # outside the cube
    g["dense"]["X"] = Xd.tolist()
    g["dense"]["Y"] = rng.uniform(1.0, 2.0, size=17).tolist()
    g["dense"]["x"] = xq.tolist()
    for kind in KINDS:
        K, S = [], []
        for x in xq:
            ks = [kernel(kind, x, X) for X in Xd]
            K.append([v[0] for v in ks])
            S.append([v[2] for v in ks])
        g["dense"][kind] = dict(K=K, s=S)
    g["scalar"] = scalar()
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kernel_resolution_goldens.json")
    with open(path, "w") as f:
        json.dump(g, f)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
