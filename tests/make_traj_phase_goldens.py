"""Writes tests/golden/traj_phase_goldens.json: the references of tests/traj_cases.py in mpmath (50 digits), each value as
the pair (nearest double, nearest double of the remainder).  Needs mpmath; the tests do not.

    python tests/make_traj_phase_goldens.py

``halfturn``: sin(pi y) on the exact doubles y for the CPU restatement of traj_cos_halfturns -- 120 points of [-1/2, 1/2],
80 within 0.05 of +-1/2 (where the polynomial is worst), 100 of [-50, 50], and the edges: y = k and y = k + 1/2 (the ties
of rint) for 19 values of k in [-50, 50] with their neighbouring doubles, tiny y down to 1e-300.  The remainders keep five
digits (1e-21 absolute): the file stays small.
``phase``: for every case of tests/traj_cases.py (regime x d x F) the inputs x, ls, W, b as doubles, cos(sum_c (x_c / ls_c)
W_fc + b_f) for every point and feature, and sqrt(2 variance / F).  The feature weights are not here: the tests read them
back from the trajectory under test and take the sum over the features in rational arithmetic."""
import json
import os
import sys

import numpy as np
from mpmath import mp, mpf

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tests import traj_cases as T  # noqa: E402

mp.dps = 50


def hilo(v):
    hi = float(v)
    return [hi, float(f"{float(v - mpf(hi)):.4e}")]


def halfturn():
    rng = np.random.default_rng(20260102)
    ys = list(rng.uniform(-0.5, 0.5, 120)) + list(rng.uniform(0.45, 0.5, 40)) + list(rng.uniform(-0.5, -0.45, 40))
    ys += list(rng.uniform(-50.0, 50.0, 100))
    for k in list(range(-50, 51, 10)) + [-49, -3, -2, -1, 1, 2, 3, 49]:
        for y in (float(k), k + 0.5):
            ys += [y, np.nextafter(y, np.inf), np.nextafter(y, -np.inf)]
    for t in (1e-300, 1e-200, 1e-100, 1e-30, 1e-17, 1e-9, 1e-4):
        ys += [t, -t]
    ys = [float(y) for y in ys]
    return dict(y=ys, sinpi=[hilo(mp.sin(mp.pi * mpf(y))) for y in ys])


def phase_case(regime, d, F):
    x, ls, W, b, lo = T.case_inputs(regime, d, F)
    cos = []
    for xr in x:
        row = []
        for f in range(F):
            arg = mpf(float(b[f]))
            for c in range(d):
                arg += mpf(float(xr[c])) / mpf(float(ls[c])) * mpf(float(W[f, c]))
            row.append(hilo(mp.cos(arg)))
        cos.append(row)
    return dict(regime=regime, d=d, F=F, lo=lo, variance=T.VARIANCE, x=x.tolist(), ls=ls.tolist(), W=W.tolist(),
                b=b.tolist(), cos=cos, scale=hilo(mp.sqrt(2 * mpf(T.VARIANCE) / F)))


def main():
    g = dict(halfturn=halfturn(),
             phase=[phase_case(r, d, F) for r in T.REGIMES for d in T.DIMS for F in T.FEATURES])
    with open(T.GOLDEN, "w") as f:
        json.dump(g, f)
        f.write("\n")
    print(T.GOLDEN, os.path.getsize(T.GOLDEN), "bytes")


if __name__ == "__main__":
    main()
