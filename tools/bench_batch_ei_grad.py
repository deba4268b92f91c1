"""The analytic batch EI's gradient at the sizes of an L-BFGS-B iteration: N = 2048, d = 6, q in {2, 4, 8}, S in {128, 512},
G in {10, 60, 300} q-batches (development aid; bench.py is the contract).

    python tools/bench_batch_ei_grad.py [--no-ego]

Per (q, S, G), HIP-event milliseconds, one warm-up then the median of 5 (and max - min):
  value_grad     tgp_batch_ei_value_grad, the whole call (events on the engine's stream around it);
  grad tail      bei_grad_tail_kernel alone (tgp_last_kernel_ms after tgp_batch_ei_moments_grad on the same moments);
  forward        tgp_batch_ei, the whole call, and its tail alone (after tgp_batch_ei_moments) -- what the gradient's cost is
                 read against: reverse mode through a chain of this shape should cost a small multiple of the forward pass.
Then one EGO ``acquire`` of a 3-point batch on scaled Branin with and without ``differentiable=True`` on the same model and
seed: seconds and the acquired value.  Prints one line per case and a JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trieste_amd import objectives as O
from trieste_amd.acquisition.function import sobol_points
from trieste_amd.engine import GPEngine, batch_ei, batch_ei_moments, batch_ei_moments_grad, batch_ei_value_grad


def _events(fn, reps=5):
    """Median and spread of the HIP-event time of fn() on the current stream (one warm-up first), and its last result."""
    ms = []
    for rep in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        if rep:
            ms.append(a.elapsed_time(b))
    return statistics.median(ms), max(ms) - min(ms), out


def _kernel_ms(eng, fn, reps=5):
    ms = []
    for rep in range(reps + 1):
        out = fn()
        if rep:
            ms.append(eng.last_kernel_ms()[0])
    return statistics.median(ms), max(ms) - min(ms), out


def run(eng, q, S, G):
    rng = np.random.default_rng(q * 1000 + S + G)
    Xq = torch.as_tensor(rng.uniform(size=(G, q, eng.d))).cuda()
    w1, w2 = (torch.as_tensor(w).cuda() for w in (sobol_points(S, q, 17), sobol_points(S, q - 1, 17)))
    mean, cov = eng.joint_forward(Xq)
    eta = float(mean.min(dim=1).values.median())
    vg, vg_s, (val, grad) = _events(lambda: batch_ei_value_grad(eng, Xq, w1, w2, eta))
    gt, gt_s, (mval, gm, gc) = _kernel_ms(eng, lambda: batch_ei_moments_grad(eng, mean, cov, w1, w2, eta))
    fw, fw_s, fval = _events(lambda: batch_ei(eng, Xq, w1, w2, eta))
    ft, ft_s, _ = _kernel_ms(eng, lambda: batch_ei_moments(eng, mean, cov, w1, w2, eta))
    assert torch.equal(val, mval) and bool(torch.isfinite(grad).all())
    r = {"q": q, "S": S, "G": G, "N": eng.N, "d": eng.d,
         "value_grad_ms": vg, "value_grad_spread": vg_s, "grad_tail_ms": gt, "grad_tail_spread": gt_s,
         "forward_ms": fw, "forward_spread": fw_s, "forward_tail_ms": ft, "forward_tail_spread": ft_s,
         "tail_ratio": gt / ft, "call_ratio": vg / fw,
         "nontrivial_fraction": float((val > 1e-3 * val.max()).double().mean())}
    print(f"q={q} S={S} G={G}: value_grad {vg:.3f} ms (spread {vg_s:.3f}), its tail {gt:.3f} ms (spread {gt_s:.3f}); forward "
          f"{fw:.3f} ms (spread {fw_s:.3f}), its tail {ft:.3f} ms (spread {ft_s:.3f}); tail ratio {gt / ft:.2f}, call ratio "
          f"{vg / fw:.2f}", flush=True)
    return r


def ego_acquire(differentiable, seed=7):
    import trieste_amd
    import trieste_amd.models as M
    from trieste_amd.acquisition import BatchExpectedImprovement, EfficientGlobalOptimization
    from trieste_amd.data import Dataset
    from trieste_amd.space import Box

    trieste_amd.set_seed(seed)
    space = Box([0, 0], [1, 1])
    x = space.sample(8, seed=seed)
    data = Dataset(x, O.scaled_branin(x))
    model = M.GaussianProcessRegression(M.build_gpr(data, space, likelihood_variance=1e-5))
    rule = EfficientGlobalOptimization(BatchExpectedImprovement(100, differentiable=differentiable), num_query_points=3)
    out = []
    for rep in range(2):   # (the first one warms up; the same seed, hence the same candidates and Sobol skip)
        trieste_amd.set_seed(seed)
        rule._acquisition_function = None
        t = time.perf_counter()
        pts = np.asarray(rule.acquire_single(space, model, dataset=data))
        out.append(time.perf_counter() - t)
    value = float(np.asarray(rule.acquisition_function(pts[None]))[0, 0])
    print(f"EGO acquire, 3 points, differentiable={differentiable}: {out[1]:.3f} s, acquired value {value:.6e}", flush=True)
    return {"differentiable": differentiable, "seconds": out[1], "value": value, "points": pts.tolist()}


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=2048)
    ap.add_argument("--no-ego", action="store_true")
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    d = 6
    X, Y = O.synthetic_problem(O.hartmann_6, d, args.N)
    eng = GPEngine(d, "matern52")
    eng.set_hyper(1.0, O.default_lengthscales(d), 1e-2, float(Y.mean()))
    eng.set_data(X, Y)
    eng.use_torch_stream()
    # (300 groups of 8 are more points than a value-and-gradient call takes: the largest count that fits stands in)
    res = {"batch_ei_grad": [run(eng, q, S, min(G, GPEngine.JOINT_SMALL_POINTS // q)) for q in (2, 4, 8) for S in (128, 512)
                             for G in (10, 60, 300)]}
    if not args.no_ego:
        res["ego_acquire"] = [ego_acquire(False), ego_acquire(True)]
    print(json.dumps(res))
