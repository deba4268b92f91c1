"""Generator of tests/golden/batch_ei_regime_goldens.json (not collected by pytest; run by hand:
``python -m tests.make_batch_ei_regime_goldens``): the analytic multi-point expected improvement and its directional
derivatives in 50-digit mpmath across output scales and thresholds, the regimes tests/golden/batch_ei_goldens.json (unit
scale, eta at the median minimum) does not reach.  The mpmath code is that of the two existing generators: the value, p,
Phi and abs_terms by ``tests.make_batch_ei_goldens.mp_batch_ei``, the derivatives by
``tests.make_batch_ei_grad_goldens._derivative`` (central differences, h = 1e-18, on mpf inputs).

Cases.  Base moments per q as ``_random_moments`` of the GPU tests draws them, the means offset by + 5; then
  mean x s, cov x s^2            for s in 1e-4, 1e-2, 1, 1e3, 1e6 (at 1e-4 the reference's absolute constants, + 1e-6 I twice
                                 and + 1e-12, dominate the covariance; at 1e3 and above they vanish below its rounding);
  eta = min(mean) + t mean(sd)   for t in -12, -6, 0, + 6 (sd = sqrt(diag cov)): EI far below its maximum ... every p_i near 1;
  (q, S) = (3, 16), (5, 8), (9, 4);
  q = 9 at S = 65, s = 1, t = 0 and t = -6 (from q = 9 the device adds per-chunk sums over chunks of 64 samples);
  one near-duplicate pair per q at s = 1e3, t = 0: the factor row of point 1 is that of point 0 moved by 3 % (correlation
  0.996 ... 0.998), so that kappa = max |cov| / lambda_min is several hundred -- the jitter no longer helps at this scale --
  and every Cholesky factor exists in float64 (asserted below through the numpy restatement) as well as in mpmath.
Directions: every coordinate for q <= 4, three seeded random symmetric directions per q above (shared by the cases of one q).

The file is compact (it holds 65 cases): base moments, Sobol points and random directions are stored once and named by
the cases; ``load()`` expands them to the layout of the two existing golden files, and is what the tests read.  mean x s and
cov x s^2 are single float64 roundings, the same here and in the tests.  value, abs_terms, eta and the derivatives are
stored as full float64 numbers, p and Phi rounded to 9 significant digits (diagnostics; the bulk of the file)."""
from __future__ import annotations

import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "batch_ei_regime_goldens.json")
SCALES = (1e-4, 1e-2, 1.0, 1e3, 1e6)
SHIFTS = (-12.0, -6.0, 0.0, 6.0)
SIZES = ((3, 16), (5, 8), (9, 4))
PAIR_STEP = 0.03


def base_moments(q, pair):
    """(mean [q], cov [q, q]): cov = F F^T with three shared factors and one own factor per point (the structure of
    ``_random_moments``), mean = standard normal + 5.  ``pair``: point 1 is point 0 with its factor row and its mean moved
    by PAIR_STEP x standard normal."""
    rng = np.random.default_rng(7000 + q)
    A = rng.standard_normal((q, 3))
    own = rng.uniform(0.02, 0.5, size=q)
    mean = rng.standard_normal(q) + 5.0
    F = np.concatenate([np.sqrt(0.1) * A, np.diag(np.sqrt(own))], axis=1)
    if pair:
        F[1] = F[0] + PAIR_STEP * rng.standard_normal(3 + q)
        mean[1] = mean[0] + PAIR_STEP * rng.standard_normal()
    return mean, F @ F.T


def threshold(mean, cov, t):
    """eta = min(mean) + t x the mean posterior standard deviation of the q-batch."""
    return float(np.min(mean) + t * np.mean(np.sqrt(np.diagonal(cov, axis1=-2, axis2=-1))))


def random_directions(q):
    out = []
    for r in range(3):
        rng = np.random.default_rng(1000 * q + r)
        dm = np.round(rng.standard_normal(q), 3)
        A = rng.standard_normal((q, q))
        out.append({"dm": dm.tolist(), "dC": np.round(0.5 * (A + A.T), 3).tolist()})
    return out


def case_directions(n, q, random_dirs):
    """The directions of case n in the layout of batch_ei_grad_goldens.json, in the order the derivatives are stored."""
    if q <= 4:
        out = [{"case": n, "kind": "mean", "i": i} for i in range(q)]
        return out + [{"case": n, "kind": "cov", "i": i, "j": j} for i in range(q) for j in range(i, q)]
    return [{"case": n, "kind": "random", "dm": d["dm"], "dC": d["dC"]} for d in random_dirs[str(q)]]


def expand(doc):
    """(cases, directions) in the layout of batch_ei_goldens.json and batch_ei_grad_goldens.json."""
    cases, dirs = [], []
    for n, c in enumerate(doc["cases"]):
        q, S, s = c["q"], c["S"], c["s"]
        base, sob = doc["base"][c["base"]], doc["sobol"][f"{q}x{S}"]
        e = dict(c)
        e["note"] = f"{c['note']} s={s:g} t={c['t']:+g}"
        e["mean"] = (np.array(base["mean"]) * s).tolist()
        e["cov"] = (np.array(base["cov"]) * (s * s)).tolist()
        e["w1"] = np.array(sob["w1"]).reshape(S, q).tolist()
        e["w2"] = np.array(sob["w2"]).reshape(S, q - 1).tolist()
        cases.append(e)
        ds = case_directions(n, q, doc["directions"])
        if "derivs" in c:
            assert len(ds) == len(c["derivs"])
            for d, v in zip(ds, c["derivs"]):
                d["deriv"] = v
        dirs.extend(ds)
    return cases, dirs


def load():
    with open(OUT) as f:
        return expand(json.load(f))


def make_doc():
    from tests import batch_ei_reference as R

    doc = {"what": "analytic batch EI and its directional derivatives (central differences, h = 1e-18) in 50-digit mpmath "
                   "across output scales s and thresholds t; tests/make_batch_ei_regime_goldens.py, read through its load()",
           "dps": 50, "step": "1e-18", "base": {}, "sobol": {}, "directions": {}, "cases": []}
    for q, S in SIZES + ((9, 65),):
        w1, w2 = R.sobol_points(S, q, skip=q)
        doc["sobol"][f"{q}x{S}"] = {"w1": w1.ravel().tolist(), "w2": w2.ravel().tolist()}
    for q, _ in SIZES:
        for pair in (False, True):
            mean, cov = base_moments(q, pair)
            doc["base"][f"q{q}" + ("pair" if pair else "")] = {"mean": mean.tolist(), "cov": cov.tolist()}
        if q > 4:
            doc["directions"][str(q)] = random_directions(q)
    plan = [(q, S, f"q{q}", s, t, "random") for q, S in SIZES for s in SCALES for t in SHIFTS]
    plan += [(9, 65, "q9", 1.0, t, "random, S = 65") for t in (0.0, -6.0)]
    plan += [(q, S, f"q{q}pair", 1e3, 0.0, "near-duplicate pair") for q, S in SIZES]
    for q, S, base, s, t, note in plan:
        b = doc["base"][base]
        eta = threshold(np.array(b["mean"]) * s, np.array(b["cov"]) * (s * s), t)
        doc["cases"].append({"q": q, "S": S, "base": base, "s": s, "t": t, "eta": eta, "note": note})
    return doc


def _work(task):
    import mpmath as mp

    from tests.make_batch_ei_goldens import mp_batch_ei
    from tests.make_batch_ei_grad_goldens import _derivative

    c, d = task
    if d is not None:
        return _derivative((c, d))
    mp.mp.dps = 50
    v, p, Phi, at = mp_batch_ei(mp, c["mean"], c["cov"], c["eta"], c["w1"], c["w2"])
    short = lambda x: float(f"{float(x):.8e}")  # noqa: E731
    return {"value": float(v), "abs_terms": float(at), "p": [short(x) for x in p],
            "Phi": [[short(x) for x in row] for row in Phi]}


def main():
    from multiprocessing import Pool

    from tests import batch_ei_reference as R

    doc = make_doc()
    cases, dirs = expand(doc)
    for c in cases:   # every float64 Cholesky factor exists (np.linalg.cholesky raises otherwise) and the value is finite
        q, S = c["q"], c["S"]
        v = R.batch_ei(np.array(c["mean"])[None], np.array(c["cov"])[None], c["eta"], np.array(c["w1"]).reshape(S, q),
                       np.array(c["w2"]).reshape(S, q - 1))
        assert np.all(np.isfinite(v)), c["note"]
    tasks = [(n, None) for n in range(len(cases))] + [(d["case"], d) for d in dirs]
    cost = lambda t: cases[t[0]]["q"] ** 3 * cases[t[0]]["S"] * (1 if t[1] is None else 2)  # noqa: E731
    order = sorted(range(len(tasks)), key=lambda k: -cost(tasks[k]))   # the long ones first
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_work, [(cases[tasks[k][0]], tasks[k][1]) for k in order], chunksize=1)
    derivs = {}
    for k, r in zip(order, res):
        n, d = tasks[k]
        if d is None:
            doc["cases"][n].update(r)
        else:
            derivs[id(d)] = r
    for n in range(len(cases)):
        doc["cases"][n]["derivs"] = [derivs[id(d)] for d in dirs if d["case"] == n]
    with open(OUT, "w") as f:
        json.dump(doc, f, separators=(",", ":"))
    print(f"wrote {OUT}: {len(cases)} cases, {len(dirs)} directions, {os.path.getsize(OUT)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
