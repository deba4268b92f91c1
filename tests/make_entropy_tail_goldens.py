"""Writes tests/golden/entropy_tail_goldens.json: the per-sample functions of the entropy-search tails in mpmath, good to 50
digits, for tests/test_entropy_regimes_conditions.py.  Needs mpmath; the tests do not.

    python tests/make_entropy_tail_goldens.py

With Phi, phi the standard normal's, h = phi(gamma) / Phi(-gamma), delta = h - gamma and w = 1 - h delta:
    f_MES(gamma)        = -gamma h / 2 - log Phi(-gamma)                 f_MES'  = h (1 - gamma delta) / 2
    f_GIB(gamma, rho2)  = -1/2 log(1 + rho2 h (gamma - h))               d/dgamma = rho2 h (delta^2 - w) / (2 inner)
                        = -1/2 log(inner), inner = (1 - rho2) + rho2 w   d/drho2  = h delta / (2 inner)
on GAMMAS x RHO2S.  rho2 is the DOUBLE written into the file (1 - 1e-10 is not representable: the functions are those of the
nearest double, and 1 - rho2 is then exact in float64 too).

Fifty digits of working precision do not give fifty digits here: log Phi(-gamma) at gamma = -37.5 is the logarithm of
1 - 1e-308, 1 - gamma delta and w at gamma = 4e7 are 1e-15 apart from two terms of size 1, and phi / Phi(-gamma) at gamma = 4e7
is the ratio of two exponentials whose arguments (8e14) each carry the rounding of gamma^2.  The formulas are therefore
evaluated as they stand with 450 digits (400 guard digits: 308 + 50 for the first, 15 + 16 + 50 for the others) and checked
against a second evaluation with 600; the file holds the nearest doubles."""
import json
import os

GAMMAS = (-37.5, -36.0, -30.0, -20.5, -20.0, -12.0, -8.5, -8.0, -7.5, -7.0, -6.5, -5.0, -1.0, 0.0, 1.0, 3.0, 6.0, 8.0, 8.5,
          12.0, 20.0, 20.5, 25.0, 30.0, 37.0, 100.0, 1e3, 1e4, 1e5, 1e6, 1e7, 4e7)
RHO2S = (0.5, 0.99, 1.0 - 1e-5, 1.0 - 1e-10)


def functions(gamma, rho2, dps):
    from mpmath import mp, mpf

    with mp.workdps(dps):
        u, r2 = mpf(gamma), mpf(rho2)
        Q = mp.ncdf(-u)
        h = mp.npdf(u) / Q
        delta = h - u
        w = 1 - h * delta
        inner = (1 - r2) + r2 * w
        return dict(mes=-u * h / 2 - mp.log(Q), dmes=h * (1 - u * delta) / 2, gib=-mp.log(inner) / 2,
                    dgib=r2 * h * (delta * delta - w) / (2 * inner), dgib_drho2=h * delta / (2 * inner))


def main():
    from mpmath import mp, mpf

    cases = []
    for rho2 in RHO2S:
        for gamma in GAMMAS:
            f, g = functions(gamma, rho2, 450), functions(gamma, rho2, 600)
            with mp.workdps(600):
                for k in f:
                    assert f[k] > 0 and abs(f[k] - g[k]) <= mpf(10) ** -50 * abs(g[k]), (gamma, rho2, k)
            cases.append(dict(gamma=float(gamma), rho2=float(rho2), **{k: float(v) for k, v in f.items()}))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "entropy_tail_goldens.json")
    with open(path, "w") as f:
        json.dump(dict(cases=cases), f, indent=0)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
