"""Per gamma-bin failure counts and worst relative errors of the value comparison of tests/test_gpu_entropy_regimes.py
(one min-value sample per call, every sample of every model's list, MES and GIBBON on the 2100 candidates; reference and
tolerance of tests/entropy_regimes.py at the engine's own moments), for the library in use.  TGP_LIB selects another build
(a parent commit's): the table of profiles/r24_entropy_tails.txt.

    python tests/entropy_tail_tally.py
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tests import acq_regimes as R  # noqa: E402
from tests import entropy_regimes as E  # noqa: E402
from trieste_amd import _lib  # noqa: E402
from trieste_amd.engine import GPEngine  # noqa: E402


def engine(p, variant=0):
    eng = GPEngine(p.d, p.kind)
    eng.set_variant(variant)
    eng.set_hyper(p.variance, p.ls, p.noise, p.c)
    eng.set_data(p.X, p.Y)
    return eng


def main():
    print("library", _lib.LIB_PATH)
    print("bins", E.G_BIN_NAMES)
    for name in E.IDS:
        p = E.problem(name)
        mean, var = (np.asarray(a) for a in engine(p, 1024).predict(p.Xq))
        eng = engine(p)
        for acq in E.ACQS:
            fails = np.zeros(len(E.G_BINS), dtype=np.int64)
            total = np.zeros_like(fails)
            worst = np.zeros(len(E.G_BINS))
            nonfinite = 0
            for s in p.params:
                eng.set_min_value_samples([s])
                got = np.asarray(eng.acq_values(acq, 0.0, p.Xq))
                ref = E.tails(p, acq, [s], mean, var)
                tol = R.RTOL * np.abs(ref) + E.sensitivity(p, acq, [s], mean, var)
                gb = E.g_bin(E.gammas([s], mean, var)[:, 0])
                ok = (np.abs(ref) >= R.TINY) & (gb >= 0)
                bad = ok & ~((np.abs(got - ref) <= tol) & (got >= 0.0))
                nonfinite += int(np.sum(~np.isfinite(got)))
                np.add.at(fails, gb[bad], 1)
                np.add.at(total, gb[ok], 1)
                with np.errstate(all="ignore"):
                    rel = np.where(ok, np.abs(got - ref) / np.abs(ref), 0.0)
                rel[~np.isfinite(rel)] = np.inf
                np.maximum.at(worst, gb[ok], rel[ok])
            print(f"{name} {acq}: failed {fails.tolist()} of {total.tolist()}; non-finite {nonfinite}; worst rel {['%.1e' % w for w in worst]}", flush=True)


if __name__ == "__main__":
    main()
