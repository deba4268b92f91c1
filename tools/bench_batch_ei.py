"""The analytic batch EI (tgp_batch_ei) at N = 2048, d = 6, G = 10^5 q-batches: milliseconds of the posterior part and of
the tail (bei_tail_kernel), q-batches per second, and measured / estimated for the tail (development aid; bench.py is the
contract).  The estimate is the one the kernel was planned with and is NOT a measurement: q^2 (q + 1) S (Phi, Phi^-1)
pairs per q-batch at 130 fp64 VALU instructions of 4.5 cycles each, on 1024 SIMDs at 2.4 GHz.

    python tools/bench_batch_ei.py [--isa <bei kernel assembly .s>] [--G 100000]

Times are HIP-event times as tgp_last_kernel_ms reports them: of the posterior part after tgp_batch_ei, of the tail alone
after tgp_batch_ei_moments on the same moments; one warm-up, then 5 repetitions, median and (max - min).  With --isa the
static VALU instruction count of the sample loop per (Phi, Phi^-1) pair is read from the assembly hipcc leaves with
-save-temps.  Prints one line per (q, S) and a JSON line (profiles/r08_batch_ei.txt)."""
import argparse
import json
import os
import re
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from trieste_amd import objectives as O  # seeded synthetic problems (product side)
from trieste_amd.acquisition.function import sobol_points
from trieste_amd.engine import GPEngine, batch_ei, batch_ei_moments

SIMDS, CLOCK_HZ = 256 * 4, 2.4e9
EST_INSTR_PER_PAIR, EST_CYCLES_PER_INSTR = 130.0, 4.5


def estimated_tail_ms(G, q, S):
    pairs = float(G) * q * q * (q + 1) * S
    return pairs / 64.0 * EST_INSTR_PER_PAIR * EST_CYCLES_PER_INSTR / (SIMDS * CLOCK_HZ) * 1e3


def isa_valu_per_pair(path):
    """{QP: (VALU instructions, fp64 VALU instructions) per pair}: the instructions of the sample loop's blocks (loop
    depth 2) of bei_tail_kernel<QP> over the QP - 1 steps unrolled in it (both sides of the quantile's branch count)."""
    s = open(path).read()
    out = {}
    for qp in (4, 8, 16):
        m = re.search(r"^(_ZN3tgp15bei_tail_kernelILi%d\w+):" % qp, s, re.M)
        if not m:
            continue
        i = s.index("\n" + m.group(1) + ":")
        body = s[i:s.index(".end_amdhsa_kernel", i)].splitlines()
        depth, valu, f64 = 0, 0, 0
        for line in body:
            if line.startswith(".LBB") or line.startswith("; %bb"):
                dm = re.search(r"Depth=(\d+)", line)
                depth = int(dm.group(1)) if dm else 0
            t = line.strip()
            if depth >= 2 and t.startswith("v_"):
                valu += 1
                f64 += "_f64" in t.split()[0]
        out[qp] = (valu / (qp - 1.0), f64 / (qp - 1.0))
    return out


def run(eng, X, q, S, G, reps=5):
    rng = np.random.default_rng(q * 1000 + S)
    Xq = torch.as_tensor(rng.uniform(size=(G, q, eng.d))).cuda()
    w1, w2 = (torch.as_tensor(w).cuda() for w in (sobol_points(S, q, 17), sobol_points(S, q - 1, 17)))
    mean, cov = eng.predict_joint(Xq)
    eta = float(mean.min(dim=1).values.median())
    post, tail = [], []
    for rep in range(reps + 1):   # (the first one warms up)
        a = batch_ei(eng, Xq, w1, w2, eta)
        p = eng.last_kernel_ms()[0]
        b = batch_ei_moments(eng, mean, cov, w1, w2, eta)
        t = eng.last_kernel_ms()[0]
        if rep:
            post.append(p)
            tail.append(t)
    assert torch.equal(a, b)
    frac = float((a > 1e-3 * a.max()).double().mean())
    est = estimated_tail_ms(G, q, S)
    r = {"q": q, "S": S, "G": G, "N": eng.N, "d": eng.d,
         "posterior_ms_median": statistics.median(post), "posterior_ms_spread": max(post) - min(post),
         "tail_ms_median": statistics.median(tail), "tail_ms_spread": max(tail) - min(tail),
         "batches_per_s": G / (statistics.median(post) + statistics.median(tail)) * 1e3,
         "tail_batches_per_s": G / statistics.median(tail) * 1e3,
         "tail_ms_estimated_unmeasured": est, "tail_measured_over_estimated": statistics.median(tail) / est,
         "nontrivial_fraction": frac}
    print(f"q={q} S={S} G={G}: posterior {r['posterior_ms_median']:.2f} ms (spread {r['posterior_ms_spread']:.2f}), tail "
          f"{r['tail_ms_median']:.2f} ms (spread {r['tail_ms_spread']:.2f}) = {r['tail_batches_per_s']:.3e} q-batches/s; "
          f"both {r['batches_per_s']:.3e} q-batches/s; tail estimate (unmeasured) {est:.2f} ms -> measured / estimated "
          f"{r['tail_measured_over_estimated']:.2f}; {100 * frac:.0f} % of the values non-trivial", flush=True)
    return r


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--isa", default=None)
    ap.add_argument("--G", type=int, default=100_000)
    ap.add_argument("--N", type=int, default=2048)
    args = ap.parse_args()
    print(torch.cuda.get_device_name(0), flush=True)
    d = 6
    X, Y = O.synthetic_problem(O.hartmann_6, d, args.N)
    eng = GPEngine(d, "matern52")
    eng.set_hyper(1.0, O.default_lengthscales(d), 1e-2, float(Y.mean()))
    eng.set_data(X, Y)
    eng.use_torch_stream()
    res = {"batch_ei": [run(eng, X, q, S, args.G) for q in (2, 4, 8) for S in (128, 512)]}
    if args.isa:
        res["isa_valu_per_pair"] = {str(k): {"valu": v[0], "valu_f64": v[1]} for k, v in isa_valu_per_pair(args.isa).items()}
        for k, v in res["isa_valu_per_pair"].items():
            print(f"bei_tail_kernel<{k}>: {v['valu']:.0f} VALU instructions per (Phi, Phi^-1) pair in the sample loop, "
                  f"{v['valu_f64']:.0f} of them fp64 (the estimate assumed {EST_INSTR_PER_PAIR:.0f})")
    print(json.dumps(res))
