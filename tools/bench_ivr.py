"""Measurement aid (not bench.py): the integrated variance reduction of 16384 candidate points at N = 4096, d = 8, Matern-5/2,
P = 4096 integration points, as 16384 batches of q = 1 and as 4096 batches of q = 4 --

  ivr       tgp_ivr_values, host clock around the synchronising call, and its device time split by events into the
            posterior part, the cross product and the tail (tgp_ivr_last_ms), summed over the call's chunks;
  composed  the same quantity from calls the engine had before: per chunk of 2048 points cov_between(chunk, Z) and
            predict_joint(chunk), then numpy for the q x q part (factorisation, solve, weighted mean), predict(Z) once for c0.

The two are run alternately, WARMUP rounds unrecorded and then REPEATS recorded; median, minimum and maximum are printed, and
the largest difference of the two results against the reduction's scale (they must agree: faster and different is not faster).

usage: python tools/bench_ivr.py [--N 4096] [--P 4096] [--points 16384] [--repeats 10] [--warmup 3]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from trieste_amd import engine as E  # noqa: E402


def composed(eng, Z, w, Xq, noise, chunk_points=2048):
    G, q, d = Xq.shape
    P = len(Z)
    _, var_old = eng.predict(Z)
    c0 = float(np.mean(w * np.asarray(var_old)))
    red = np.empty(G)
    step = max(1, chunk_points // q)
    for g0 in range(0, G, step):
        x = Xq[g0:g0 + step]
        gc = len(x)
        cross = np.asarray(eng.cov_between(x.reshape(-1, d), Z)).reshape(gc, q, P)
        _, cov = eng.predict_joint(x)
        L = np.linalg.cholesky(np.asarray(cov) + noise * np.eye(q))
        if q == 1:
            A = cross / L
        else:
            A = np.linalg.solve(L, cross)
        red[g0:g0 + gc] = np.einsum("gip,gip,p->g", A, A, w) / P
    return red - c0, red


def summary(xs):
    xs = np.asarray(xs)
    return dict(median=float(np.median(xs)), min=float(xs.min()), max=float(xs.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--P", type=int, default=4096)
    ap.add_argument("--points", type=int, default=16384)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(a.N, a.d))
    Y = np.sin(3.0 * X.sum(axis=1)) + 0.05 * rng.standard_normal(a.N)
    noise = 1e-3
    eng = E.GPEngine(a.d, "matern52")
    eng.set_hyper(1.0, np.full(a.d, 0.2 * np.sqrt(a.d)), noise, 0.0)
    eng.set_data(X, Y)
    Z, w = rng.uniform(size=(a.P, a.d)), rng.uniform(size=a.P)
    E.set_integration_points(eng, Z, w)
    for q in (1, 4):
        Xq = rng.uniform(size=(a.points // q, q, a.d))
        wall, parts, base = [], [], []
        for r in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            out, red = E.ivr_values(eng, Xq, with_reduction=True)
            t1 = time.perf_counter()
            cout, cred = composed(eng, Z, w, Xq, noise)
            t2 = time.perf_counter()
            if r >= a.warmup:
                wall.append((t1 - t0) * 1e3)
                parts.append(E.ivr_last_ms(eng))
                base.append((t2 - t1) * 1e3)
        parts = np.asarray(parts)
        print(json.dumps(dict(
            what="ivr", N=a.N, d=a.d, P=a.P, q=q, groups=len(Xq), repeats=a.repeats, warmup=a.warmup,
            ivr_wall_ms=summary(wall), posterior_ms=summary(parts[:, 0]), cross_product_ms=summary(parts[:, 1]),
            tail_ms=summary(parts[:, 2]), composed_wall_ms=summary(base),
            speedup_median=float(np.median(base) / np.median(wall)),
            max_reduction_difference_over_scale=float(np.abs(red - cred).max() / np.abs(cred).max()),
            max_out_difference_over_scale=float(np.abs(out - cout).max() / np.abs(cout).max()))), flush=True)


if __name__ == "__main__":
    main()
