"""Expected hypervolume improvement (tgp_ehvi_values) at N = 500, d = 6, M = 10^5 candidates: milliseconds of the P posterior
sweeps and of the tail kernel (ehvi_tail_kernel) of the same call, beside the host time of the partition (development aid;
bench.py is the contract).  Partitions: two objectives with a front of 50 points, three with fronts of 25 and of 80.

    python tools/bench_ehvi.py [--M 100000] [--N 500]

Times are HIP-event times as tgp_ehvi_last_ms reports them: one warm-up call, then three timed ones, each printed.  The fronts
are points of the unit sphere's positive orthant (mutually non-dominated) scaled into the range of the models' posterior means.
Prints one line per partition and a JSON line (profiles/r13_ehvi.txt).

    python tools/bench_ehvi.py --grad [--N 500]

times the value-and-gradient call (tgp_ehvi_value_grad) over the same three partitions at 20, 200 and 2048 points -- what an
L-BFGS-B iteration holds -- the same way: the tail (ehvi_grad_tail_kernel) and the whole call, whose remainder is the two
posterior halves of the P models (profiles/r20_ehvi_value_grad.txt; --cmax labels a library built with another tile cap)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trieste_amd import objectives as O  # seeded synthetic problems (product side)
from trieste_amd.acquisition import prepare_default_non_dominated_partition_bounds
from trieste_amd.engine import (GPEngine, ehvi_argmax, ehvi_grad_tile_width, ehvi_last_ms, ehvi_partition_tables,
                                ehvi_set_partition_tables, ehvi_tile_width, ehvi_value_grad, ehvi_values)


def sphere_front(P, n, seed):
    g = np.abs(np.random.default_rng(seed).standard_normal((n, P)))
    return g / np.linalg.norm(g, axis=1, keepdims=True)


def engines_for(P, N, d):
    out = []
    for j, objective in enumerate((O.hartmann_6, O.ackley, lambda x: O.rosenbrock(x, 6))[:P]):
        X, Y = O.synthetic_problem(objective, d, N, seed=1234 + j)
        eng = GPEngine(d, "matern52")
        eng.set_hyper(1.0, O.default_lengthscales(d), 1e-2, 0.0)
        eng.set_data(X, Y)
        eng.use_torch_stream()
        out.append(eng)
    return out


def run(P, n_front, N, d, M, reps=3):
    engines = engines_for(P, N, d)
    front = 2.0 * sphere_front(P, n_front, seed=n_front) - 1.5   # standardised targets: means lie around [-1.5, 1.5]
    ref = np.full(P, 1.0)
    t0 = time.perf_counter()
    lb, ub = prepare_default_non_dominated_partition_bounds(ref, front)
    t_part = time.perf_counter() - t0
    t0 = time.perf_counter()
    tables = ehvi_partition_tables(lb, ub)
    ehvi_set_partition_tables(engines[0], *tables)
    t_tables = time.perf_counter() - t0
    V, K = int(tables[1].max()), len(lb)
    Xq = torch.as_tensor(np.random.default_rng(P * 1000 + n_front).uniform(size=(M, d))).cuda()
    sweeps, tail, wall = [], [], []
    for rep in range(reps + 1):   # (the first one warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vals = ehvi_values(engines, Xq)
        torch.cuda.synchronize()
        w = (time.perf_counter() - t0) * 1e3
        s, t = ehvi_last_ms(engines[0])
        if rep:
            sweeps.append(s), tail.append(t), wall.append(w)
    best = ehvi_argmax(engines, Xq)
    assert best[0] == float(vals.max()) and best[1] == int(vals.argmax())
    r = {"P": P, "front": n_front, "V": V, "K": K, "C": ehvi_tile_width(P, V), "N": N, "d": d, "M": M,
         "partition_host_s": t_part, "tables_and_upload_s": t_tables, "sweeps_ms": sweeps, "tail_ms": tail, "call_wall_ms": wall,
         "positive_fraction": float((vals > 1e-6 * vals.max()).double().mean())}
    print(f"P={P} front={n_front}: V={V} K={K} C={r['C']}; partition on the host {t_part:.3f} s (+ tables and upload "
          f"{t_tables * 1e3:.1f} ms); {P} sweeps " + " / ".join(f"{v:.3f}" for v in sweeps) + " ms, tail "
          + " / ".join(f"{v:.3f}" for v in tail) + " ms, whole call " + " / ".join(f"{v:.2f}" for v in wall)
          + f" ms; {100 * r['positive_fraction']:.0f} % of the values above 1e-6 of the largest", flush=True)
    return r


def run_grad(P, n_front, N, d, points=(20, 200, 2048), reps=3, cmax=8):
    """tgp_ehvi_value_grad at the point counts of an L-BFGS-B iteration: HIP-event times of the tail (tgp_ehvi_last_ms) and of
    the whole call (events on the stream all engines share), and the tail alone on the same moments (tgp_ehvi_moments_grad)."""
    engines = engines_for(P, N, d)
    front = 2.0 * sphere_front(P, n_front, seed=n_front) - 1.5
    lb, ub = prepare_default_non_dominated_partition_bounds(np.full(P, 1.0), front)
    tables = ehvi_partition_tables(lb, ub)
    ehvi_set_partition_tables(engines[0], *tables)
    V, K = int(tables[1].max()), len(lb)
    C = cmax   # (the rule of ehvi_grad_tile_width with the cap the library under test was built with)
    while C > 1 and 24 * P * V * C > 160 * 1024:
        C //= 2
    assert cmax != 8 or C == ehvi_grad_tile_width(P, V)
    out = []
    for M in points:
        Xq = torch.as_tensor(np.random.default_rng(P * 1000 + n_front + M).uniform(size=(M, d))).cuda()
        tail, whole, wall = [], [], []
        for rep in range(reps + 1):   # (the first one warms up)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            e0.record()
            val, grad = ehvi_value_grad(engines, Xq)
            e1.record()
            torch.cuda.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            if rep:
                tail.append(ehvi_last_ms(engines[0])[1]), whole.append(e0.elapsed_time(e1)), wall.append(w)
        assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(grad).all())
        r = {"P": P, "front": n_front, "V": V, "K": K, "C": C, "N": N, "d": d, "M": M, "tail_ms": tail, "call_ms": whole,
             "call_wall_ms": wall, "posterior_halves_ms": [c - t for c, t in zip(whole, tail)]}
        print(f"value_grad P={P} front={n_front}: V={V} K={K} C={C} M={M}: tail " + " / ".join(f"{v:.3f}" for v in tail)
              + " ms, whole call (events) " + " / ".join(f"{v:.3f}" for v in whole) + " ms, (host clock) "
              + " / ".join(f"{v:.3f}" for v in wall) + " ms", flush=True)
        out.append(r)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--M", type=int, default=100_000)
    ap.add_argument("--N", type=int, default=500)
    ap.add_argument("--grad", action="store_true", help="time tgp_ehvi_value_grad at 20, 200 and 2048 points instead")
    ap.add_argument("--cmax", type=int, default=8, help="the tile-width cap the library under test was built with (label only)")
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    partitions = ((2, 50), (3, 25), (3, 80))
    if args.grad:
        res = {"ehvi_value_grad": [r for P, n in partitions for r in run_grad(P, n, args.N, 6, cmax=args.cmax)], "cmax": args.cmax}
    else:
        res = {"ehvi": [run(P, n, args.N, 6, args.M) for P, n in partitions]}
    print(json.dumps(res))
