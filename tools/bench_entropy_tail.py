"""`acq_values` for MES and GIBBON at N = 1024, d = 8, M = 1e5 with S = 5 and S = 64 min-value samples: the posterior sweep
plus entropy_tail_kernel (O(S) per candidate).  Every figure is the median of `--calls` calls after two warm-up calls, the
whole set repeated `--repeats` times so that the run-to-run spread is visible next to the figure.  TGP_LIB selects another
build of the library (a parent commit's, for an A/B on one machine).

    python tools/bench_entropy_tail.py [--calls 20] [--repeats 5]
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--N", type=int, default=1024)
    ap.add_argument("--M", type=int, default=100000)
    args = ap.parse_args()
    import torch

    from trieste_amd import _lib
    from trieste_amd.engine import GPEngine

    d = 8
    rng = np.random.default_rng(0)
    X = rng.uniform(size=(args.N, d))
    Y = np.sin(3.0 * X).sum(axis=1) + 0.5 * np.cos(5.0 * X[:, 0] * X[:, 1])
    Y = (Y - Y.mean()) / Y.std()
    eng = GPEngine(d, "matern52")
    eng.set_hyper(1.0, np.full(d, 0.2 * np.sqrt(d)), 1e-3, 0.0)
    eng.set_data(X, Y)
    Xq = torch.as_tensor(rng.uniform(size=(args.M, d))).to("cuda:0")
    eta = eng.eta()
    print(f"library {_lib.LIB_PATH}; N={args.N} M={args.M} d={d}; median of {args.calls} calls, ms")
    for rep in range(args.repeats):
        row = []
        for S in (5, 64):
            eng.set_min_value_samples(eta - 0.6 * rng.uniform(size=S) ** 2)   # as a min-value sampler leaves them: at and below eta
            for acq in ("mes", "gibbon"):
                for _ in range(2):
                    eng.acq_values(acq, 0.0, Xq)
                torch.cuda.synchronize()
                t = []
                for _ in range(args.calls):
                    t0 = time.perf_counter()
                    eng.acq_values(acq, 0.0, Xq)
                    torch.cuda.synchronize()
                    t.append((time.perf_counter() - t0) * 1e3)
                row.append(f"{acq} S={S}: {np.median(t):.4f} (min {min(t):.4f})")
        print(f"repeat {rep}: " + "; ".join(row), flush=True)


if __name__ == "__main__":
    main()
