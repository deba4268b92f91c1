"""Generator of tests/golden/qehvi_grad_goldens.json: the batch Monte-Carlo expected hypervolume improvement from given joint
moments (the formula of tests/make_qehvi_goldens.py, restated here on mpmath numbers: an mpmath Cholesky factor, the samples
and the inclusion-exclusion at 50 digits) and its derivatives w.r.t. the moments as 50-digit CENTRAL DIFFERENCES of that
value with step 1e-20:

    gmean[j,i]          along mean[j,i]
    gcov[j,a,a]         along E_aa
    gcov[j,a,b], a != b half the derivative along E_ab + E_ba   (the symmetric adjoint)

Within the kink distance (tests/qehvi_grad_reference.py) the value is a polynomial of the samples and the samples are smooth
in the moments, so the differences are exact to about 1e-30 of the value (entries below 1e-26 of it are stored as zero).  The generator asserts that every case's kink distance is at
least 1e-6 (cases are redrawn until it is), and that every case has a non-zero gmean and a non-zero off-diagonal gcov entry
(where q > 1) unless it is marked as a zero case.  Run ``python -m tests.make_qehvi_grad_goldens`` from the repository root to
regenerate (deterministic)."""
import json
import os
from itertools import combinations

import mpmath as mp
import numpy as np

from tests import qehvi_grad_reference as GR
from tests import qehvi_reference as R
from tests.make_qehvi_goldens import SETUPS, _cov, _partition

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "qehvi_grad_goldens.json")
STEP = "1e-20"
DIGITS = 20          # of the stored results (float64 holds 17)
MIN_KINK = 1e-6


def _mp_array(a):
    a = np.asarray(a, np.float64)
    return np.vectorize(lambda v: mp.mpf(float(v)), otypes=[object])(a) if a.size else a.astype(object)


def value(mean, cov, eps, jitter, lo, up, subsets):
    """The value at 50 digits; every argument an object array / list of mpf (mean [P, q], cov [P, q, q], eps [P, q, S])."""
    P, q = mean.shape
    S = eps.shape[2]
    y = [[[None] * P for _ in range(q)] for _ in range(S)]
    for j in range(P):
        A = mp.matrix(q, q)
        for a in range(q):
            for b in range(q):
                A[a, b] = cov[j, a, b] + (jitter if a == b else 0)
        L = mp.cholesky(A)
        for s in range(S):
            for i in range(q):
                v = mean[j, i]
                for m in range(i + 1):
                    v += L[i, m] * eps[j, m, s]
                y[s][i][j] = v
    total = mp.mpf(0)
    for s in range(S):
        # the overlap vertex of every subset once per sample
        vertex = {J: [max(y[s][i][j] for i in J) for j in range(P)] for J in subsets}
        for lo_row, up_row in zip(lo, up):
            for J in subsets:
                t = mp.mpf(1)
                for j in range(P):
                    t *= max(up_row[j] - max(lo_row[j], vertex[J][j]), mp.mpf(0))
                    if t == 0:
                        break
                total += t if len(J) % 2 else -t
    return total / S


def exact(c):
    """(value, gmean [P, q], gcov [P, q, q]) of a case at 50 digits."""
    mp.mp.dps = 50
    mean, cov, eps = _mp_array(c["mean"]), _mp_array(c["cov"]), _mp_array(c["eps"])
    P, q = mean.shape
    jitter, h = mp.mpf(float(c["jitter"])), mp.mpf(STEP)
    lo = [[max(mp.mpf(float(v)), mp.mpf(-1e10)) for v in row] for row in c["lb"]]
    up = [[mp.mpf(float(v)) for v in row] for row in c["ub"]]
    subsets = [J for n in range(1, q + 1) for J in combinations(range(q), n)]

    def f(m, k):
        return value(m, k, eps, jitter, lo, up, subsets)

    def central(perturb):
        plus_m, plus_c, minus_m, minus_c = mean.copy(), cov.copy(), mean.copy(), cov.copy()
        perturb(plus_m, plus_c, h)
        perturb(minus_m, minus_c, -h)
        return (f(plus_m, plus_c) - f(minus_m, minus_c)) / (2 * h)

    gmean, gcov = np.empty((P, q), object), np.empty((P, q, q), object)
    for j in range(P):
        for i in range(q):
            def bump_mean(m, k, step, j=j, i=i):
                m[j, i] = m[j, i] + step

            gmean[j, i] = central(bump_mean)
        for a in range(q):
            for b in range(a + 1):
                def bump_cov(m, k, step, j=j, a=a, b=b):
                    k[j, a, b] = k[j, a, b] + step
                    if a != b:
                        k[j, b, a] = k[j, b, a] + step

                d = central(bump_cov)
                gcov[j, a, b] = gcov[j, b, a] = d if a == b else d / 2
    # A difference resolves 10^-50 |value| / step = 1e-30 |value|: what lies below 1e-26 |value| is the rounding of the two
    # values (a moment the value does not depend on at all gives such an entry), stored as an exact zero
    val = f(mean, cov)
    floor = mp.mpf("1e-26") * abs(val)
    for arr in (gmean, gcov):
        for idx in np.ndindex(arr.shape):
            if abs(arr[idx]) < floor:
                arr[idx] = mp.mpf(0)
    return val, gmean, gcov


def _rho_cov(P, q, rho, scale):
    """Equicorrelated covariances: scale ((1 - rho) I + rho 1 1^T), objective j scaled by 1 + j / 4."""
    base = scale * ((1.0 - rho) * np.eye(q) + rho * np.ones((q, q)))
    return np.stack([(1.0 + 0.25 * j) * base for j in range(P)])


def cases():
    out = []

    def add(note, P, draw, seed, jitter=1e-6, zero=False):
        """``draw(rng) -> (mean, cov, eps)``; redrawn from the next seeds until the kink distance is at least MIN_KINK (and,
        but for a zero case, some sample adds volume)."""
        front, ref = SETUPS[P]
        lb, ub = _partition(front, ref)
        assert len(lb) <= 12
        for attempt in range(50):
            mean, cov, eps = (np.asarray(a, np.float64) for a in draw(np.random.default_rng(seed + 1000 * attempt)))
            cov = np.tril(cov) + np.swapaxes(np.tril(cov, -1), -1, -2)     # (the file keeps the lower triangles)
            samples = R.samples_from_moments(mean[:, None], cov[:, None], eps, jitter)
            kink = float(GR.kink_distance(samples, lb, ub)[0])
            # (a batch that happens to add no volume is redrawn too, unless that is the case's point)
            if kink >= MIN_KINK and (zero or np.any(GR.sample_adjoints(samples, lb, ub) != 0.0)):
                break
        assert kink >= MIN_KINK, (note, kink)
        assert eps.shape[2] <= 8
        out.append(dict(note=note, zero=bool(zero), jitter=float(jitter), kink=kink, mean=mean, cov=cov, eps=eps,
                        lb=np.asarray(lb, np.float64), ub=np.asarray(ub, np.float64)))

    seed = 0
    # the grid: every P with q = 1, 2, 3, 5; q = 8 (255 subsets) at P = 2 and 3 with very few samples
    for P in (2, 3, 4):
        for q, S in ((1, 8), (2, 5), (3, 4), (5, 2)) + (((8, 2),) if P == 2 else ((8, 1),) if P == 3 else ()):
            seed += 1
            add(f"P={P} q={q} S={S}", P, lambda rng, P=P, q=q, S=S: (rng.uniform(0.0, 0.9, (P, q)), _cov(rng, P, q, 0.05),
                                                                     rng.standard_normal((P, q, S))), seed)
    # wide marginals; jitter 0; one draw
    add("P=2 q=3 wide marginals", 2, lambda rng: (rng.uniform(-0.5, 1.5, (2, 3)), _cov(rng, 2, 3, 1.0),
                                                  rng.standard_normal((2, 3, 5))), 101)
    add("P=3 q=2 jitter 0", 3, lambda rng: (rng.uniform(0.0, 0.9, (3, 2)), _cov(rng, 3, 2, 0.05),
                                            rng.standard_normal((3, 2, 5))), 102, jitter=0.0)
    add("P=4 q=3 one draw", 4, lambda rng: (rng.uniform(0.0, 0.7, (4, 3)), _cov(rng, 4, 3, 0.05),
                                            rng.standard_normal((4, 3, 1))), 103)
    # strongly correlated batch points
    for P, q, S, s in ((2, 3, 5, 111), (3, 2, 5, 112), (4, 2, 4, 113), (2, 5, 2, 114)):
        add(f"P={P} q={q} correlation 0.99", P, lambda rng, P=P, q=q, S=S: (rng.uniform(0.0, 0.8, (P, q)), _rho_cov(P, q, 0.99, 0.05),
                                                                            rng.standard_normal((P, q, S))), s)
    # batches inside the dominated region: everything exactly zero
    add("P=2 q=3 every sample dominated", 2, lambda rng: (rng.uniform(1.5, 2.0, (2, 3)), _cov(rng, 2, 3, 1e-4),
                                                          rng.standard_normal((2, 3, 4))), 121, zero=True)
    add("P=3 q=2 every sample dominated", 3, lambda rng: (np.tile(SETUPS[3][0][0][:, None] + 0.05, (1, 2))
                                                          + rng.uniform(0.0, 0.01, (3, 2)), _cov(rng, 3, 2, 1e-8),
                                                          rng.standard_normal((3, 2, 4))), 122, zero=True)

    # a point below every front point, and a point far below every lower bound in one objective (beyond the -1e10 that
    # stands in for an infinite lower bound: its samples sit at that bound, the other objectives' lengths are about 1e10)
    def below(P, q, S, level, objectives):
        def draw(rng):
            mean = rng.uniform(0.2, 0.8, (P, q))
            mean[objectives, q - 1] = level
            return mean, _cov(rng, P, q, 1e-3), rng.standard_normal((P, q, S))
        return draw

    add("P=2 q=2 a point below every front point", 2, below(2, 2, 5, -0.5, [0, 1]), 131)
    add("P=4 q=3 a point below every front point", 4, below(4, 3, 4, -0.3, [0, 1, 2, 3]), 132)
    add("P=2 q=2 a point far below every lower bound", 2, below(2, 2, 5, -1e11, [0]), 133)
    add("P=3 q=3 a point far below every lower bound", 3, below(3, 3, 4, -1e11, [1]), 134)
    return out


def main():
    out = cases()
    for c in out:
        val, gmean, gcov = exact(c)
        q = gmean.shape[1]
        off = [gcov[j, a, b] for j in range(gcov.shape[0]) for a in range(q) for b in range(a)]
        if c["zero"]:
            assert val == 0 and all(v == 0 for v in gmean.ravel()) and all(v == 0 for v in gcov.ravel()), c["note"]
        else:
            assert any(v != 0 for v in gmean.ravel()), c["note"]
            assert q == 1 or any(v != 0 for v in off), c["note"]
        print(f"{c['note']:48s} K={len(c['lb']):2d} kink {c['kink']:.1e} value {mp.nstr(val, 12)}", flush=True)
        # the file: the partition by its objective count, symmetric matrices by their lower triangles (row by row)
        low = np.tril_indices(q)
        c["value"] = mp.nstr(val, DIGITS)
        c["gmean"] = [[mp.nstr(v, DIGITS) for v in row] for row in gmean]
        c["gcov"] = [[mp.nstr(v, DIGITS) for v in mat[low]] for mat in gcov]
        c["cov"] = [mat[low].tolist() for mat in c["cov"]]
        c["mean"], c["eps"], c["kink"] = c["mean"].tolist(), c["eps"].tolist(), float(f"{c['kink']:.3e}")
        del c["lb"], c["ub"]
    partitions = {str(P): dict(zip(("lb", "ub"), (np.asarray(b, np.float64).tolist() for b in _partition(*SETUPS[P]))))
                  for P in SETUPS}
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump({"step": STEP, "partitions": partitions, "cases": out}, f, separators=(",", ":"))
    print(f"{len(out)} cases -> {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
