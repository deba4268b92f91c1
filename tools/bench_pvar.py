"""Measurement aid (not bench.py): PredictiveVariance at N = 4096, d = 8, Matern-5/2, for q in (4, 16, 64) --

  call   2048 // q batches through ``trieste_amd.acquisition.predictive_variance.__call__`` (posterior and tail on the device)
         and through ``trieste_amd.extras.predictive_variance.__call__`` (posterior on the device, the [G, q, q] blocks copied
         back, numpy.linalg.slogdet on the host), run alternately on the same model, host clock around the synchronising
         calls; next to them the posterior's device time of the new call (the engine's two events) and one
         ``value_and_gradient`` of the same batches;
  tail   the tail kernel alone on G = 10^4 batches of device-resident covariances (``pvar_moments`` / ``pvar_moments_grad`` on
         CUDA tensors), the engine's two events around the kernel.

WARMUP rounds unrecorded, then REPEATS recorded; median, minimum and maximum are printed as one JSON line per q.

usage: python tools/bench_pvar.py [--N 4096] [--repeats 20] [--warmup 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import trieste_amd.models as M  # noqa: E402
from trieste_amd import engine as E  # noqa: E402
from trieste_amd import extras  # noqa: E402
from trieste_amd.acquisition import PredictiveVariance  # noqa: E402
from trieste_amd.data import Dataset  # noqa: E402
from trieste_amd.space import Box  # noqa: E402


def summary(xs):
    xs = np.asarray(xs)
    return dict(median=float(np.median(xs)), min=float(xs.min()), max=float(xs.max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=4096)
    ap.add_argument("--d", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    space = Box([0.0] * a.d, [1.0] * a.d)
    X = rng.uniform(size=(a.N, a.d))
    data = Dataset(X, (np.sin(3.0 * X.sum(axis=1)) + 0.05 * rng.standard_normal(a.N))[:, None])
    model = M.GaussianProcessRegression(M.build_gpr(data, space, likelihood_variance=1e-3))
    eng = model.engine
    new = PredictiveVariance().prepare_acquisition_function(model)
    grad = PredictiveVariance(differentiable=True).prepare_acquisition_function(model)
    old = extras.PredictiveVariance().prepare_acquisition_function(model)
    for q in (4, 16, 64):
        Xq = rng.uniform(size=(2048 // q, q, a.d))
        t_new, t_old, t_post, t_grad = [], [], [], []
        for r in range(a.warmup + a.repeats):
            t0 = time.perf_counter()
            v_new = new(Xq)
            t1 = time.perf_counter()
            post = eng.last_kernel_ms()[0]
            t2 = time.perf_counter()
            v_old = old(Xq)
            t3 = time.perf_counter()
            grad.value_and_gradient(Xq)
            t4 = time.perf_counter()
            if r >= a.warmup:
                t_new.append((t1 - t0) * 1e3)
                t_post.append(post)
                t_old.append((t3 - t2) * 1e3)
                t_grad.append((t4 - t3) * 1e3)
        G = 10000
        A = rng.standard_normal((G, q, q + 8))
        cov = torch.as_tensor(A @ np.swapaxes(A, 1, 2) / (q + 8)).cuda()
        t_tail, t_tail_grad = [], []
        for r in range(a.warmup + a.repeats):
            E.pvar_moments(eng, cov, 1e-6, with_logdet=True)
            m1 = eng.last_kernel_ms()[0]
            E.pvar_moments_grad(eng, cov, 1e-6)
            m2 = eng.last_kernel_ms()[0]
            if r >= a.warmup:
                t_tail.append(m1)
                t_tail_grad.append(m2)
        print(json.dumps(dict(
            what="pvar", N=a.N, d=a.d, q=q, groups=len(Xq), repeats=a.repeats, warmup=a.warmup,
            new_call_wall_ms=summary(t_new), new_call_posterior_device_ms=summary(t_post), host_composition_wall_ms=summary(t_old),
            speedup_median=float(np.median(t_old) / np.median(t_new)), value_and_gradient_wall_ms=summary(t_grad),
            max_relative_difference=float(np.abs(np.asarray(v_new).reshape(-1) - np.asarray(v_old).reshape(-1)).max() / np.abs(np.asarray(v_old)).max()),
            tail_alone_groups=G, tail_alone_device_ms=summary(t_tail), tail_alone_with_gcov_device_ms=summary(t_tail_grad))), flush=True)


if __name__ == "__main__":
    main()
