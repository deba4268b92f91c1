"""Batch Monte-Carlo expected hypervolume improvement (tgp_qehvi_values) at N = 1024, d = 6, G = 10^4 batches, S = 128 samples:
milliseconds of the tail kernel (qehvi_tail_kernel) and of the P tgp_predict_joint calls of the same call, beside the time of
a numpy restatement of the reference's loop (below; the tests keep their own) on a few of the same batches on this box's CPU
(development aid; bench.py is the contract).  Partitions: two objectives with a front of 25 points, three with a front of 16 points whose
partition has 249 cells; q = 2, 4, 8 points per batch.

    python tools/bench_qehvi.py [--G 10000] [--N 1024] [--S 128]
    python tools/bench_qehvi.py --grad [--N 1024] [--S 128]

--grad times the value-and-gradient call (tgp_qehvi_value_grad) over the same partitions at G = 10, 100 and 2048 // q batches --
what an L-BFGS-B iteration holds: the gradient tail (qehvi_grad_tail_kernel, tgp_ehvi_last_ms), the whole call (events on the
stream all engines share; the remainder is the posterior halves of the P models) and, from the same run, the value tail at the
same shape; three warm-up calls, then 21 timed ones, median (min .. max).  Then one ``acquire`` of
EfficientGlobalOptimization(BatchMonteCarloExpectedHypervolumeImprovement(64), num_query_points=3) on VLMOP2 with and without
``differentiable=True`` from the same seeds: the time and the qEHVI reached (profiles/r22_qehvi_grad.txt).

Times are HIP-event times as tgp_ehvi_last_ms reports them: one warm-up call, then three timed ones, each printed.  The fronts
are points of the unit sphere's positive orthant (mutually non-dominated) scaled into the range of the models' posterior means.
Prints one line per shape and a JSON line (profiles/r21_qehvi.txt)."""
import argparse
import itertools
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from tools.bench_ehvi import engines_for, sphere_front
from trieste_amd.acquisition import prepare_default_non_dominated_partition_bounds
from trieste_amd.engine import (ehvi_last_ms, ehvi_partition_tables, ehvi_set_partition_tables, qehvi_grad_sample_chunk,
                                qehvi_sample_chunk, qehvi_value_grad, qehvi_values)


def numpy_value(mean, cov, eps, jitter, lb, ub):
    """The value of one batch as the reference computes it (multi_objective.py:366-410 behind sampler.py:278-287): mean [P, q],
    cov [P, q, q], eps [P, q, S]; per subset size j the C(q, j) subsets gathered from the samples, all cells at once."""
    q = mean.shape[-1]
    samples = np.transpose(mean[..., None] + np.linalg.cholesky(cov + jitter * np.eye(q)) @ eps, (2, 1, 0))   # [S, q, P]
    total = np.zeros(samples.shape[0])
    for j in range(1, q + 1):
        subsets = np.array(list(itertools.combinations(range(q), j)))                # [C, j]
        vertices = np.max(samples[:, subsets, :], axis=-2)                           # [S, C, P]
        vertices = np.maximum(vertices[:, None], lb[None, :, None, :])               # [S, K, C, P]
        lengths = np.maximum(ub[None, :, None, :] - vertices, 0.0)
        total += (-1.0) ** (j + 1) * np.sum(np.prod(lengths, axis=-1), axis=(-1, -2))
    return float(np.mean(total))


def run(P, n_front, q, N, d, G, S, reps=3):
    engines = engines_for(P, N, d)
    front = 2.0 * sphere_front(P, n_front, seed=n_front) - 1.5   # standardised targets: means lie around [-1.5, 1.5]
    lb, ub = prepare_default_non_dominated_partition_bounds(np.full(P, 1.0), front)
    ehvi_set_partition_tables(engines[0], *ehvi_partition_tables(lb, ub))
    rng = np.random.default_rng(P * 1000 + n_front + q)
    X_host, eps_host = rng.uniform(size=(G, q, d)), rng.standard_normal((P, q, S))
    Xq, eps = torch.as_tensor(X_host).cuda(), torch.as_tensor(eps_host).cuda()
    posterior, tail, wall = [], [], []
    for rep in range(reps + 1):   # (the first one warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        vals = qehvi_values(engines, Xq, eps)
        torch.cuda.synchronize()
        w = (time.perf_counter() - t0) * 1e3
        s, t = ehvi_last_ms(engines[0])
        if rep:
            posterior.append(s), tail.append(t), wall.append(w)
    # the numpy restatement on a few of the same batches, one at a time (its [S, K, C(q, j), j, P] tensors are large)
    n_host = 2 if q >= 8 else 8
    moments = [eng.predict_joint(X_host[:n_host]) for eng in engines]
    mean, cov = np.stack([m for m, _ in moments]), np.stack([c for _, c in moments])
    t0 = time.perf_counter()
    host = np.array([numpy_value(mean[:, g], cov[:, g], eps_host, 1e-6, lb, ub) for g in range(n_host)])
    host_ms = (time.perf_counter() - t0) * 1e3 / n_host
    dev = vals[:n_host].cpu().numpy()
    assert np.all(np.abs(dev - host) <= 1e-9 * (1.0 + np.abs(host))), (dev, host)
    r = {"P": P, "front": n_front, "K": len(lb), "q": q, "S": S, "chunk": qehvi_sample_chunk(P, q), "N": N, "d": d, "G": G,
         "posterior_ms": posterior, "tail_ms": tail, "call_wall_ms": wall, "numpy_ms_per_batch": host_ms, "numpy_batches": n_host,
         "positive_fraction": float((vals > 1e-6 * vals.max()).double().mean())}
    print(f"P={P} front={n_front} K={len(lb)} q={q} S={S}: {P} predict_joint " + " / ".join(f"{v:.3f}" for v in posterior)
          + " ms, tail " + " / ".join(f"{v:.3f}" for v in tail) + " ms, whole call " + " / ".join(f"{v:.2f}" for v in wall)
          + f" ms; numpy restatement {host_ms:.1f} ms per batch over {n_host} batches (x G = {host_ms * G / 1e3:.0f} s); "
          f"{100 * r['positive_fraction']:.0f} % of the values above 1e-6 of the largest", flush=True)
    return r


def _stats(values):
    return {"median": float(np.median(values)), "min": float(np.min(values)), "max": float(np.max(values))}


def _fmt(st):
    return f"{st['median']:.3f} ({st['min']:.3f} .. {st['max']:.3f})"


def run_grad(P, n_front, q, N, d, S, warmup=3, reps=21):
    """tgp_qehvi_value_grad at the batch counts of an L-BFGS-B iteration: HIP-event times of the gradient tail and of the whole
    call, and the value tail (tgp_qehvi_values) at the same shape from the same run."""
    engines = engines_for(P, N, d)
    front = 2.0 * sphere_front(P, n_front, seed=n_front) - 1.5
    lb, ub = prepare_default_non_dominated_partition_bounds(np.full(P, 1.0), front)
    ehvi_set_partition_tables(engines[0], *ehvi_partition_tables(lb, ub))
    out = []
    for G in (10, 100, 2048 // q):
        rng = np.random.default_rng(P * 1000 + n_front + q + G)
        Xq = torch.as_tensor(rng.uniform(size=(G, q, d))).cuda()
        eps = torch.as_tensor(rng.standard_normal((P, q, S))).cuda()
        tail, whole, vtail = [], [], []
        for rep in range(warmup + reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            val, grad = qehvi_value_grad(engines, Xq, eps)
            e1.record()
            torch.cuda.synchronize()
            t = ehvi_last_ms(engines[0])[1]
            vals = qehvi_values(engines, Xq, eps)
            torch.cuda.synchronize()
            if rep >= warmup:
                tail.append(t), whole.append(e0.elapsed_time(e1)), vtail.append(ehvi_last_ms(engines[0])[1])
        assert bool(torch.equal(val, vals)) and bool(torch.isfinite(grad).all())
        r = {"P": P, "front": n_front, "K": len(lb), "q": q, "S": S, "grad_chunk": qehvi_grad_sample_chunk(P, q), "N": N, "d": d,
             "G": G, "grad_tail_ms": _stats(tail), "call_ms": _stats(whole), "value_tail_ms": _stats(vtail),
             "posterior_halves_ms": _stats([c - t for c, t in zip(whole, tail)]),
             "positive_fraction": float((vals > 1e-6 * vals.max()).double().mean())}
        print(f"value_grad P={P} K={len(lb)} q={q} S={S} G={G}: gradient tail {_fmt(r['grad_tail_ms'])} ms, whole call (events) "
              f"{_fmt(r['call_ms'])} ms, the rest (posterior halves) {_fmt(r['posterior_halves_ms'])} ms; value tail at the same "
              f"shape {_fmt(r['value_tail_ms'])} ms; {100 * r['positive_fraction']:.0f} % of the values above 1e-6 of the largest",
              flush=True)
        out.append(r)
    return out


def run_acquire(reps=5):
    """One ``acquire`` of the batch rule on VLMOP2 (10 Sobol points, two models) with and without the gradient, same seeds."""
    import trieste_amd
    import trieste_amd.models as M
    from trieste_amd import objectives as OBJ
    from trieste_amd.acquisition import BatchMonteCarloExpectedHypervolumeImprovement, EfficientGlobalOptimization
    from trieste_amd.data import Dataset
    from trieste_amd.space import Box

    space = Box([-2.0, -2.0], [2.0, 2.0])
    x = space.sample_sobol(10, skip=0)
    data = Dataset(x, OBJ.vlmop2(x, 2))
    members = [M.GaussianProcessRegression(M.build_gpr(Dataset(x, data.observations[:, j:j + 1]), space, likelihood_variance=1e-5))
               for j in range(2)]
    stack = M.TrainablePredictJointReparamModelStack(*[(m, 1) for m in members])
    out = {}
    for differentiable in (False, True):
        times, reached = [], []
        for rep in range(reps + 1):   # (the first one warms up)
            trieste_amd.set_seed(100 + rep)
            rule = EfficientGlobalOptimization(BatchMonteCarloExpectedHypervolumeImprovement(64, differentiable=differentiable),
                                               num_query_points=3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            batch = rule.acquire_single(space, stack, dataset=data)
            torch.cuda.synchronize()
            w = (time.perf_counter() - t0) * 1e3
            if rep:
                times.append(w), reached.append(float(np.asarray(rule.acquisition_function(np.asarray(batch)[None]))[0, 0]))
        out["differentiable" if differentiable else "value_only"] = {"acquire_ms": _stats(times), "qehvi_reached": reached}
        print(f"acquire differentiable={differentiable}: {_fmt(_stats(times))} ms (host clock); qEHVI reached "
              + " / ".join(f"{v:.5f}" for v in reached), flush=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--G", type=int, default=10_000)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--S", type=int, default=128)
    ap.add_argument("--grad", action="store_true", help="time tgp_qehvi_value_grad at 10, 100 and 2048 // q batches instead")
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    if args.grad:
        res = {"qehvi_value_grad": [r for P, n in ((2, 25), (3, 16)) for q in (2, 4, 8) for r in run_grad(P, n, q, args.N, 6, args.S)],
               "acquire": run_acquire()}
    else:
        res = {"qehvi": [run(P, n, q, args.N, 6, args.G, args.S) for P, n in ((2, 25), (3, 16)) for q in (2, 4, 8)]}
    print(json.dumps(res))
