"""Wide inputs (d > 32) at N = 4096: the EI arg-max sweep over 2^20 candidates, `update`, one NLML + gradient and a default
EGO acquire at d = 32 (the narrow form, for comparison), 64 and 128 (development aid; bench.py is the contract).
Prints one line per dimension and a JSON line with the numbers (profiles/r07_wide_inputs.txt)."""
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trieste_amd import objectives as O  # seeded synthetic problems (product side)
from trieste_amd.engine import GPEngine

FP64_PEAK_TFLOPS = 78.6  # MI355X fp64 matrix peak (bench.py)


def best_of(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return min(out)


def run(d, N=4096, M=1 << 20, kind="matern52", noise=1e-2):
    import trieste_amd.models as Mo
    from trieste_amd.acquisition import EfficientGlobalOptimization
    from trieste_amd.data import Dataset
    from trieste_amd.space import Box

    X, Y = O.synthetic_problem(O.ackley, d, N)
    eng = GPEngine(d, kind)
    eng.set_hyper(1.0, O.default_lengthscales(d), noise, float(Y.mean()))
    eng.set_data(X, Y)
    update_ms = best_of(lambda: eng.set_data(X, Y), 3)
    nlml_ms = best_of(lambda: eng.nlml(), 3)
    eta = eng.eta()
    Xq = eng.sample_box(5678, 0, M, 0.0, 1.0)
    eng.use_torch_stream()
    eng.acq_argmax("ei", eta, Xq)
    kms = []
    for _ in range(3):
        eng.acq_argmax("ei", eta, Xq)
        kms.append(eng.last_kernel_ms()[0])
    sweep_ms = min(kms)
    tflops = M * float(N) * N / (sweep_ms * 1e-3) * 1e-12   # algorithmic: N^2 per candidate
    space = Box([0.0] * d, [1.0] * d)
    data = Dataset(X, Y[:, None])
    model = Mo.GaussianProcessRegression(Mo.build_gpr(data, space, likelihood_variance=noise))
    rule = EfficientGlobalOptimization()
    rule.acquire_single(space, model, dataset=data)
    acquire_ms = best_of(lambda: rule.acquire_single(space, model, dataset=data), 3)
    r = {"d": d, "N": N, "M": M, "sweep_kernel_ms": sweep_ms, "cand_per_s": M / sweep_ms * 1e3, "tflops": tflops,
         "frac_fp64_peak": tflops / FP64_PEAK_TFLOPS, "update_ms": update_ms, "nlml_grad_ms": nlml_ms,
         "ego_acquire_ms": acquire_ms}
    print(f"d={d} N={N}: EI arg-max sweep over {M} candidates {sweep_ms:.2f} ms = {r['cand_per_s']:.3e} cand/s, "
          f"{tflops:.1f} TFLOP/s = {r['frac_fp64_peak']:.3f} of fp64 peak; update {update_ms:.1f} ms; "
          f"nlml + gradient {nlml_ms:.2f} ms; default EGO acquire {acquire_ms:.1f} ms", flush=True)
    return r


if __name__ == "__main__":
    print(torch.cuda.get_device_name(0), flush=True)
    dims = [int(a) for a in sys.argv[1:]] or [32, 64, 128]
    print(json.dumps({"wide_inputs": [run(d) for d in dims]}))
