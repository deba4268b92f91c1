"""Writes tests/golden/acq_tail_goldens.json: expected improvement, probability of improvement and augmented expected
improvement in mpmath (50 digits) on z in {-37.5 ... 20} x sigma in {1e-6 ... 1e3}, for tests/test_oracle_tails.py.
Needs mpmath; the test does not.

    python tests/make_acq_tail_goldens.py

Each case stores the doubles the oracle is called with (mean, var, eta, noise) and the values of the exact functions of
THOSE doubles: with sd = sqrt(var), z = (eta - mean) / sd,
    EI = (eta - mean) Phi(z) + sd phi(z),  PI = Phi(z),  AEI = EI (1 - sqrt(noise) / sqrt(noise + var))."""
import json
import os

from mpmath import mp, mpf

mp.dps = 50
ZS = (-37.5, -37.0, -36.0, -30.0, -20.0, -10.0, -5.0, -1.0, 0.0, 1.0, 5.0, 8.0, 20.0)
SIGMAS = (1e-6, 1e-3, 0.3, 1.0, 1e3)
MEAN = 0.75
NOISE_REL = 0.01      # noise variance = 0.01 var


def main():
    cases = []
    for sigma in SIGMAS:
        for z in ZS:
            mean, var = MEAN, float(sigma * sigma)
            eta = float(mean + z * sigma)
            noise = float(NOISE_REL * var)
            sd = mp.sqrt(mpf(var))
            diff = mpf(eta) - mpf(mean)
            zz = diff / sd
            ei = diff * mp.ncdf(zz) + sd * mp.npdf(zz)
            pi = mp.ncdf(zz)
            aei = ei * (1 - mp.sqrt(mpf(noise)) / mp.sqrt(mpf(noise) + mpf(var)))
            cases.append(dict(z=z, sigma=sigma, mean=mean, var=var, eta=eta, noise=noise, z_exact=float(zz),
                              ei=float(ei), pi=float(pi), aei=float(aei)))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "acq_tail_goldens.json")
    with open(path, "w") as f:
        json.dump(dict(cases=cases), f, indent=0)
        f.write("\n")
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
