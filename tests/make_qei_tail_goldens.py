"""Generator of tests/golden/qei_tail_goldens.json (not collected by pytest; run by hand:
``python -m tests.make_qei_tail_goldens``): the batch Monte-Carlo expected improvement on given moments in 50-digit mpmath --
the value, the samples, the exact integer counts of the improving draws per arg-min point, and the adjoint of the covariance
by the closed form  gcov = L^-T sym(Phi(L^T Lbar)) L^-1  (tests/qei_reference.py states the formulas).  For q <= 4 also the
central differences of the value (h = 1e-18, on mpf inputs) in every coordinate of cov -- the symmetric unit directions
(i, j), i <= j: both cov_ij and cov_ji move -- so that the closed form is not its own witness.

Cases.  Base moments per q by ``tests.make_batch_ei_regime_goldens.base_moments`` (means offset by + 5), then
  (q, S) = (1, 16), (2, 16), (3, 16), (9, 8), (17, 4), (33, 4), (64, 4) and q = 9 at S = 65;
  mean x s, cov x s^2            for s in 1e-4, 1, 1e6, the jitter fixed at 1e-6: at 1e-4 the jitter IS the covariance, at 1e6
                                 it is below the covariance's rounding;
  eta = min(mean) + t mean(sd)   for t in -2, 0, +3, sd = sqrt(diag(cov) + jitter): the standard deviations of what the tail
                                 draws from (at s = 1e-4, where sqrt(diag cov) is a tenth of them, t sqrt(diag cov) would leave
                                 every threshold in the middle of the draws);
  one near-duplicate pair per q >= 2 at s = 1, t = 0: point 1's factor row is point 0's moved by 3 %;
  one case with cov = 0 exactly (q = 3): L = sqrt(jitter) I, every diagonal entry clipped; the means a fraction of sqrt(jitter)
  apart, eta = min(mean) (the rule at t = 0).
The base draws eps [q, S] are standard normal, seeded per (q, S) by ``EPS_SEEDS``: the seeds are the first for which the
conditions of tests/test_qei_reference.py hold (kink distance, improving and non-improving draws in every case).

The file is compact (``compact``): base moments and draws are stored once and named by the cases, the samples once per
(base, s), equal gcov arrays once; every float64 array is packed as base64 of its bytes; gcov is stored as its lower triangle
(the closed form WITHOUT the clip of a diagonal entry at cov_ii <= 1e-12: ``load()`` applies it, as the entry does).
mean x s and cov x s^2 are single float64 roundings, the same here and in the tests."""
from __future__ import annotations

import base64
import json
import os
import sys

import numpy as np

from tests.make_batch_ei_regime_goldens import base_moments

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "golden", "qei_tail_goldens.json")
SCALES = (1e-4, 1.0, 1e6)
SHIFTS = (-2.0, 0.0, 3.0)
SIZES = ((1, 16), (2, 16), (3, 16), (9, 8), (17, 4), (33, 4), (64, 4), (9, 65))
JITTER = 1e-6
VAR_FLOOR = 1e-12
STEP = "1e-18"
# seed of the draws of (q, S): 5000 + 100 q + S unless named here (the first seed counted up from there that meets the conditions)
EPS_SEEDS = {(2, 16): 5221, (9, 8): 5915, (17, 4): 6708, (33, 4): 8316, (64, 4): 11412}


def eps_seed(q, S):
    return EPS_SEEDS.get((q, S), 5000 + 100 * q + S)


def draws(q, S):
    return np.random.default_rng(eps_seed(q, S)).standard_normal((q, S))


def threshold(mean, cov, t, jitter=JITTER):
    """eta = min(mean) + t x the mean standard deviation of cov + jitter I over the q-batch."""
    return float(np.min(mean) + t * np.mean(np.sqrt(np.diagonal(cov, axis1=-2, axis2=-1) + jitter)))


def plan():
    """[(q, S, base name, s, t, note)]"""
    out = [(q, S, f"q{q}", s, t, "random") for q, S in SIZES for s in SCALES for t in SHIFTS]
    out += [(q, S, f"q{q}pair", 1.0, 0.0, "near-duplicate pair") for q, S in SIZES[:-1] if q >= 2]
    out += [(3, 16, "q3zero", 1.0, 0.0, "cov = 0")]
    return out


def bases():
    out = {}
    for q in sorted({q for q, _ in SIZES}):
        for pair in ((False, True) if q >= 2 else (False,)):
            mean, cov = base_moments(q, pair)
            out[f"q{q}" + ("pair" if pair else "")] = {"mean": mean.tolist(), "cov": cov.tolist()}
    # (the means within a fraction of sqrt(jitter) of each other: every point is the arg-min of some draw)
    out["q3zero"] = {"mean": (5.0 + 1e-4 * (np.array(out["q3"]["mean"]) - 5.0)).tolist(), "cov": np.zeros((3, 3)).tolist()}
    return out


def make_doc():
    doc = {"what": "batch Monte-Carlo EI on given moments in 50-digit mpmath: value, samples, counts, the closed-form adjoint of "
                   "cov (lower triangle, unclipped) and, for q <= 4, central differences (h = 1e-18) in every coordinate of cov; "
                   "tests/make_qei_tail_goldens.py, read through its load()",
           "dps": 50, "step": STEP, "jitter": JITTER, "base": bases(), "eps": {}, "cases": []}
    for q, S in SIZES:
        doc["eps"][f"{q}x{S}"] = draws(q, S).ravel().tolist()
    for q, S, base, s, t, note in plan():
        b = doc["base"][base]
        eta = threshold(np.array(b["mean"]) * s, np.array(b["cov"]) * (s * s), t)
        doc["cases"].append({"q": q, "S": S, "base": base, "s": s, "t": t, "eta": eta, "note": note})
    return doc


def directions(q):
    return [(i, j) for i in range(q) for j in range(i, q)]


def expand(doc):
    """The cases with their arrays: mean [q], cov [q, q], eps [q, S], and -- once computed -- samples [S, q], counts [q], gcov
    [q, q] (symmetric, the clip applied), gcov_unclipped, diffs {(i, j): central difference} for q <= 4."""
    cases = []
    for c in doc["cases"]:
        q, S, s = c["q"], c["S"], c["s"]
        base = doc["base"][c["base"]]
        e = dict(c)
        e["note"] = f"q={q} S={S} {c['note']} s={s:g} t={c['t']:+g}"
        e["jitter"] = doc["jitter"]
        e["mean"] = np.array(base["mean"]) * s
        e["cov"] = np.array(base["cov"]) * (s * s)
        e["eps"] = np.array(doc["eps"][f"{q}x{S}"]).reshape(q, S)
        if "gcov" in c:
            e["samples"] = np.array(c["samples"]).reshape(S, q)
            e["counts"] = np.array(c["counts"], np.int64)
            low = np.zeros((q, q))
            low[np.tril_indices(q)] = c["gcov"]
            full = low + np.tril(low, -1).T
            e["gcov_unclipped"] = full
            e["gcov"] = full.copy()
            clipped = np.flatnonzero(np.diagonal(e["cov"]) <= VAR_FLOOR)
            e["gcov"][clipped, clipped] = 0.0
            e["diffs"] = dict(zip(directions(q), c["diffs"])) if "diffs" in c else {}
        cases.append(e)
    return cases


def _pack(a):
    """float64 array -> base64 of its little-endian bytes (10.7 characters per number instead of 24, every bit kept)."""
    return base64.b64encode(np.ascontiguousarray(a, "<f8").tobytes()).decode()


def _unpack(text):
    return np.frombuffer(base64.b64decode(text), "<f8").tolist()


def _padded(low, q):
    return low + [0.0] * (q * (q + 1) // 2 - len(low))


def _tri(q):
    return np.tril_indices(q)


def compact(doc):
    """The document as it is written: every float64 array packed (``_pack``), the base covariances as their lower triangles
    (they are symmetric to the bit: asserted), a pair's base as what it changes in the plain one, the samples once per (base, S, s) -- they do not depend on eta --, equal gcov arrays
    (thresholds between which no draw changes sides) once in a pool that the cases index."""
    out = {k: doc[k] for k in ("what", "dps", "step", "jitter")}
    out["packing"] = "base64 of little-endian float64; cov and gcov: lower triangles, row by row, gcov without its trailing zeros"
    out["base"] = {}
    for name, b in doc["base"].items():
        cov = np.array(b["cov"])
        assert np.array_equal(cov, cov.T)
        if name.endswith("pair"):   # point 1 moved: row and column 1 of the plain base's covariance, and mean 1, are replaced
            plain = doc["base"][name[:-4]]
            back = cov.copy()
            back[1, :], back[:, 1] = np.array(plain["cov"])[1, :], np.array(plain["cov"])[:, 1]
            assert np.array_equal(back, np.array(plain["cov"])) and np.array_equal(np.delete(b["mean"], 1), np.delete(plain["mean"], 1))
            out["base"][name] = {"of": name[:-4], "mean1": b["mean"][1], "row1": _pack(cov[1])}
            continue
        out["base"][name] = {"mean": _pack(b["mean"]), "cov": _pack(cov[_tri(len(cov))])}
    out["eps"] = {k: _pack(v) for k, v in doc["eps"].items()}
    out["samples"], out["gcov"], out["cases"] = {}, [], []
    for c in doc["cases"]:
        e = {k: v for k, v in c.items() if k not in ("samples", "gcov")}
        key, g = f"{c['base']}x{c['S']}@{c['s']:g}", _pack(np.trim_zeros(c["gcov"], "b"))   # (rows below the last arg-min: 0)
        assert out["samples"].setdefault(key, _pack(c["samples"])) == _pack(c["samples"])
        if g not in out["gcov"]:
            out["gcov"].append(g)
        e["gcov"] = out["gcov"].index(g)
        out["cases"].append(e)
    return out


def restore(doc):
    """``compact``'s inverse: the document in the layout ``expand`` reads."""
    out = dict(doc)
    out["base"] = {}
    for name, b in doc["base"].items():
        if "of" in b:
            continue
        mean = _unpack(b["mean"])
        low = np.zeros((len(mean), len(mean)))
        low[_tri(len(mean))] = _unpack(b["cov"])
        out["base"][name] = {"mean": mean, "cov": (low + np.tril(low, -1).T).tolist()}
    for name, b in doc["base"].items():
        if "of" in b:
            mean, cov = list(out["base"][b["of"]]["mean"]), np.array(out["base"][b["of"]]["cov"])
            mean[1] = b["mean1"]
            cov[1, :] = cov[:, 1] = _unpack(b["row1"])
            out["base"][name] = {"mean": mean, "cov": cov.tolist()}
    out["eps"] = {k: _unpack(v) for k, v in doc["eps"].items()}
    out["cases"] = [dict(c, samples=_unpack(doc["samples"][f"{c['base']}x{c['S']}@{c['s']:g}"]), gcov=_padded(_unpack(doc["gcov"][c["gcov"]]), c["q"]))
                    for c in doc["cases"]]
    return out


def load():
    with open(OUT) as f:
        return expand(restore(json.load(f)))


def _mp_value(mp, mean, cov, eps, eta, jitter, full=False):
    q, S = len(mean), len(eps[0])
    A = mp.matrix(q, q)
    for i in range(q):
        for j in range(q):
            A[i, j] = mp.mpf(cov[i][j]) + (mp.mpf(jitter) if i == j else 0)
    L = mp.cholesky(A)
    f = [[mp.mpf(mean[j]) + mp.fsum(L[j, k] * eps[k][s] for k in range(j + 1)) for j in range(q)] for s in range(S)]
    total, hits = mp.mpf(0), []
    for s in range(S):
        jmin = min(range(q), key=lambda j: (f[s][j], j))                   # the first index on ties
        imp = mp.mpf(eta) - f[s][jmin]
        if imp > 0:
            total += imp
            hits.append((s, jmin))
    return (total / S, L, f, hits) if full else total / S


def _work(c):
    import mpmath as mp

    mp.mp.dps = 50
    q, S = c["q"], c["S"]
    mean, cov, eta, jitter = c["mean"].tolist(), c["cov"].tolist(), c["eta"], c["jitter"]
    eps = [[mp.mpf(x) for x in row] for row in c["eps"].tolist()]
    value, L, f, hits = _mp_value(mp, mean, cov, eps, eta, jitter, full=True)
    counts = [sum(1 for _, j in hits if j == i) for i in range(q)]
    # Lbar = tril(sum_s df_s eps_s^T), df_s = -1/S at the arg-min
    Lbar = [[mp.mpf(0)] * q for _ in range(q)]
    for s, i in hits:
        for k in range(i + 1):
            Lbar[i][k] -= eps[k][s] / S
    # R = sym(Phi(L^T Lbar))
    Q = [[mp.fsum(L[k, a] * Lbar[k][c_] for k in range(a, q)) if a >= c_ else mp.mpf(0) for c_ in range(q)] for a in range(q)]
    R = [[(Q[a][b] if a >= b else Q[b][a]) / 2 for b in range(q)] for a in range(q)]
    # Y = L^-T R (back substitution down every column), gcov = Y L^-1 (back substitution along every row)
    Y = [[None] * q for _ in range(q)]
    for col in range(q):
        for a in range(q - 1, -1, -1):
            Y[a][col] = (R[a][col] - mp.fsum(L[k, a] * Y[k][col] for k in range(a + 1, q))) / L[a, a]
    gc = [[None] * q for _ in range(q)]
    for row in range(q):
        for a in range(q - 1, -1, -1):
            gc[row][a] = (Y[row][a] - mp.fsum(L[k, a] * gc[row][k] for k in range(a + 1, q))) / L[a, a]
    sym = max(abs(gc[i][j] - gc[j][i]) for i in range(q) for j in range(q))
    assert sym <= mp.mpf(10) ** -30 * max(1, max(abs(gc[i][j]) for i in range(q) for j in range(q))), c["note"]
    out = {"value": float(value), "samples": [float(f[s][j]) for s in range(S) for j in range(q)], "counts": counts,
           "gcov": [float(gc[i][j]) for i in range(q) for j in range(i + 1)]}
    if q <= 4:
        h = mp.mpf(STEP)
        out["diffs"] = []
        for i, j in directions(q):
            v = []
            for sign in (1, -1):
                moved = [[mp.mpf(x) for x in row] for row in cov]
                moved[i][j] += sign * h
                if i != j:
                    moved[j][i] += sign * h
                v.append(_mp_value(mp, mean, moved, eps, eta, jitter))
            out["diffs"].append(float((v[0] - v[1]) / (2 * h)))
    return out


def main():
    from multiprocessing import Pool

    doc = make_doc()
    cases = expand(doc)
    order = sorted(range(len(cases)), key=lambda n: -cases[n]["q"] ** 3)   # the long ones first
    with Pool(min(8, os.cpu_count() or 1)) as pool:
        res = pool.map(_work, [cases[n] for n in order], chunksize=1)
    for n, r in zip(order, res):
        doc["cases"][n].update(r)
    with open(OUT, "w") as f:
        json.dump(compact(doc), f, separators=(",", ":"))
    print(f"wrote {OUT}: {len(cases)} cases, {os.path.getsize(OUT)} bytes", file=sys.stderr)


if __name__ == "__main__":
    main()
